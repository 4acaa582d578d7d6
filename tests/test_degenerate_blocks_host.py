"""Degenerate macro-atom blocks on the CPU oracle alone (tests/degenerate_blocks.py; the device side is tests/test_degenerate_blocks_gpu.py).

(1) The tables are what they say: every kind, per block and shell; the two giant blocks; the empty block.
(2) The samples hit what they are for: floors on the census (from the tables and the oracle's jump log) and on the packet mix, for the
    "degenerate" family in its four configurations, the giant problem and the chain problem in both modes.  The floors are conditions on the
    sample, none above half of what the oracle measures.
(3) On the error problems the oracle returns the reference's errors, on the same packet with one thread and with many, and that packet's
    last jump ran out of its block (or selected the row of type -3).
(4) A metamorphic property of the reference: rows of probability 0 change nothing but the count of examined rows, and that by exactly
    the number of inserted rows in front of the selections.
"""
import numpy as np
import pytest

import degenerate_blocks as db
import kernel_table_recipes as ktr
from tardis_amd import _abi

CONFIGS = [(False, 0), (False, ktr.N_VPACKETS), (True, 0), (True, ktr.N_VPACKETS)]
MODES = ["macroatom", "downbranch"]
ULP = 2.0 ** -52


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- (1) the tables ---------------------------------------------------------------------------------------------------------------

def check_kinds(op, kinds, base=None):
    """Every block is of the kind the problem says, in every shell (`base`: the probabilities before the kinds were written)."""
    edge, P = op.macro_block_edge_index, op.transition_probabilities
    S = P.shape[1]
    assert np.all(P >= 0.0)
    seen = {k: [] for k in db.KINDS}
    for b, kind in enumerate(kinds):
        kind = db.KINDS[kind]
        blk = P[edge[b]:edge[b + 1]]
        n = len(blk)
        em = op.transition_type[edge[b]:edge[b + 1]] == -1
        seen[kind].append(n)
        total = np.cumsum(blk, axis=0)[-1]  # (the reference's serial sum)
        if kind == "zeros":
            run = max(1, n // 5)
            assert np.all(blk[:run] == 0) and np.all(blk[n - run:] == 0) and np.all((blk[em] > 0).any(axis=0))
            share = (blk == 0).mean(axis=0)
            assert np.all(share >= 2 * run / n) and np.all(share <= 2 * run / n + 0.1), (n, share)
            if n >= 10:
                assert np.all(share > 0.3) and np.all(share < 0.55), (n, share)
            if n >= 60:
                assert len({tuple(np.flatnonzero(blk[:, s] == 0)) for s in range(S)}) > 1, "the same pattern in every shell"
            assert np.all(np.abs(total - 1.0) <= 4 * np.sqrt(n) * ULP + 8 * ULP)
        elif kind == "dyadic_equal":
            u = -np.log2(blk.min())
            assert u == int(u) and u <= 16 and n * 2.0 ** -u <= 0.5
            assert np.all((blk == 2.0 ** -u).sum(axis=0) == n - 1) and np.all(total == 1.0)
            rest = blk.argmax(axis=0)
            assert np.all(em[rest]) and (S < 4 or n < 12 or len(set(rest)) > 1)
            c = np.cumsum(blk, axis=0) * 65536.0
            assert np.all(c == np.floor(c))
        elif kind == "sub_unit":
            small = np.isin(blk, db.SUB_UNIT)
            assert np.all(small.sum(axis=0) == n - 1) and np.all(total == 1.0) and np.all(em[blk.argmax(axis=0)])
            if n > 3 * db.SUB_UNIT_STRETCH:
                assert all((blk == v).any() for v in db.SUB_UNIT)
        elif kind == "quantised":
            q = blk * 2.0 ** 18
            assert np.all(q == np.floor(q)) and np.all(total == 1.0)
        elif kind == "one_row":
            assert np.all((blk == 1.0).sum(axis=0) == 1) and np.all((blk == 0.0).sum(axis=0) == n - 1)
            rows = blk.argmax(axis=0)
            assert np.all(em[rows[1::2]]) and np.all((rows[0::2] == n // 2) | em[rows[0::2]])
        elif kind in db.SCALES:
            for s in range(S):
                f = db.SCALES[kind][s % 2]
                assert abs(total[s] / f - 1.0) < 1e-13
                if base is not None:
                    assert np.array_equal(blk[:, s], base[edge[b]:edge[b + 1], s] * f)
        else:
            assert np.all(blk > 0) and np.all(np.abs(total - 1.0) < 1e-13)
            if base is not None:
                assert np.array_equal(blk, base[edge[b]:edge[b + 1]])
    return seen


def test_the_family_is_what_it_says():
    prob, base = ktr.make_problem(False, 0, "degenerate"), ktr.make_problem(False, 0)
    op = prob.opacity_state
    for f in ("macro_block_edge_index", "transition_type", "destination_level_id", "transition_line_id", "line2macro_level_upper", "line_list_nu", "tau_sobolev"):
        assert np.array_equal(getattr(op, f), getattr(base.opacity_state, f)), f
    seen = check_kinds(op, prob.block_kinds, base.opacity_state.transition_probabilities)
    sizes = np.diff(op.macro_block_edge_index)
    print({k: (len(v), min(v), max(v)) for k, v in seen.items()})
    for k, v in seen.items():  # every kind gets long blocks (more than one window) and short ones
        assert len(v) >= 5 and max(v) > 3 * db.WINDOW and min(v) <= 15, k
    planted = {int(n): db.KINDS[prob.block_kinds[np.flatnonzero(sizes == n)[0]]] for n in (33, 96, 99, 192, 300, 2100)}
    print(planted)
    assert planted == {3 * lines: kind for lines, kind in db.PLANTED.items()}
    assert np.all(np.diff(op.line_list_nu) <= 0)
    full = ktr.make_problem(True, ktr.N_VPACKETS, "degenerate")  # the same tables in every configuration
    assert np.array_equal(full.opacity_state.transition_probabilities, op.transition_probabilities)


@pytest.mark.parametrize("mode", MODES)
def test_the_chain_tables_are_what_they_say(mode):
    prob = db.chain_problem(mode)
    op = prob.opacity_state
    assert op.tau_sobolev.shape == (6000, 4)
    seen = check_kinds(op, prob.block_kinds)
    for k, v in seen.items():
        assert len(v) >= 8 and max(v) > db.WINDOW, k
    if mode == "macroatom":  # the blocks the kinds leave alone or scale hold 2 .. 5 % on their emission rows
        edge, P = op.macro_block_edge_index, op.transition_probabilities
        for b in np.flatnonzero(np.isin(prob.block_kinds, [db.KINDS.index(k) for k in ("continuous", "scaled_up", "barely_off")])):
            blk = P[edge[b]:edge[b + 1]]
            share = blk[op.transition_type[edge[b]:edge[b + 1]] == -1].sum(axis=0) / blk.sum(axis=0)
            assert np.all(share > 0.0199) and np.all(share < 0.0501)


def test_the_giant_tables_are_what_they_say():
    prob = db.giant_problem()
    op = prob.opacity_state
    edge, P, ttype, dest = op.macro_block_edge_index, op.transition_probabilities, op.transition_type, op.destination_level_id
    assert P.shape == (3 * db.GIANT_LINES, 2) and op.tau_sobolev.shape == (db.GIANT_LINES, 2) and np.all(P >= 0)
    sizes = np.diff(edge)
    a, b, e = prob.giant_a, prob.giant_b, prob.empty_block
    assert sizes[a] == 65538 and sizes[b] == 131073 and sizes[e] == 0
    A, B = P[edge[a]:edge[a + 1]], P[edge[b]:edge[b + 1]]
    assert np.all(A[:-1] == 2.0 ** -17) and np.all(A[-1] == 0.5 - 2.0 ** -17) and np.all(np.cumsum(A, axis=0)[-1] == 1.0)
    assert len(A) - 1 == 65537 >= db.HOT_ROW_LIMIT and ttype[edge[a + 1] - 1] == 1
    assert np.all(B[:-1, 0] == 2.0 ** -17) and np.all(B[0::2, 1] == 0) and np.all(B[1::2, 1] == 2.0 ** -16) and np.all(B[-1] == 0)
    assert np.all(np.cumsum(B, axis=0)[-1] == 1.0)
    rest = np.delete(sizes, [a, b, e])
    assert rest.min() >= 3 and rest.max() <= 24 and len(rest) > 50
    # nothing leads to the empty block; internal rows lead to levels with rows, the giant ones among them
    assert not np.any(op.line2macro_level_upper == e) and not np.any(dest[ttype >= 0] == e)
    assert np.all(sizes[dest[ttype >= 0]] > 0) and np.any(dest[ttype >= 0] == a) and np.any(dest[ttype >= 0] == b)
    # with every block on a hot sector the two giant blocks have empty sectors: no interval of theirs is wider than one 16-bit unit, and row 65 537 is past the row limit
    assert np.all(db.hot_sector_entries(prob, a) == 0) and np.all(db.hot_sector_entries(prob, b) <= 1)
    hot = db.hot_blocks(prob, -1)
    assert not hot[a] and not hot[b] and hot.sum() > 10


def test_zero_rows_are_what_they_say():
    base, twin, old_of_new = db.zero_row_problems("macroatom")
    a, b = base.opacity_state, twin.opacity_state
    new = old_of_new < 0
    assert 3000 < new.sum() and np.array_equal(old_of_new[~new], np.arange(len(a.transition_type)))
    assert np.all(b.transition_probabilities[new] == 0) and np.array_equal(b.transition_probabilities[~new], a.transition_probabilities)
    front = np.maximum.accumulate(np.where(new, -1, np.arange(len(new))))  # the row in front of an inserted one
    assert not new[0]
    for f in ("transition_type", "destination_level_id", "transition_line_id"):
        assert np.array_equal(getattr(b, f), getattr(b, f)[front]) and np.array_equal(getattr(b, f)[~new], getattr(a, f)), f
    assert np.array_equal(np.diff(b.macro_block_edge_index) - np.diff(a.macro_block_edge_index),
                          np.add.reduceat(new.astype(np.int64), b.macro_block_edge_index[:-1]))
    runs = np.diff(np.flatnonzero(np.diff(np.concatenate(([0], new, [0]))) != 0))[::2]
    assert set(runs) == set(db.ZERO_ROW_COUNTS)


# ---- (2) the samples ----------------------------------------------------------------------------------------------------------------

FAMILY_FLOORS = {"behind a plateau": 500, "behind leading zeros": 1000, "row >= 32": 1000, "long block": 1500, "saturated tail": 1500, "sum above 1": 400}
FAMILY_HOT = {"hot 1": {"hits": 2000, "misses": 150}, "hot auto": {"hits": 2000, "misses": 150}}
FAMILY_PER_KIND, FAMILY_PER_CLASS = 70, 400
GIANT_FLOORS = {"tie": 8000, "tie run >= 2": 8000, "decided inside a run": 4000, "run crosses a quad": 2000, "run crosses the window": 500,
                "run crosses a sector": 500, "behind a plateau": 800, "behind leading zeros": 800, "row >= 32": 10000, "row >= 65535": 5000,
                "giant": 10000, "fp64 decided": 8000}
GIANT_HOT = {"hot 1": {"hits": 15000, "misses": 15000}, "hot auto": {"hits": 7000, "misses": 500}}
GIANT_MIX = {"no interaction": 200, "last is a line": 2000, "last is electron scattering": 400, "reabsorbed": 1200}
GIANT_PER_BLOCK_AND_SHELL, GIANT_AT_THE_WIDE_ROW = 400, 1800
CHAIN_FLOORS = {"macroatom": {"tie": 300, "tie run >= 2": 150, "tie run >= 8": 20, "decided inside a run": 60, "run crosses a quad": 50,
                              "run crosses the window": 10, "run crosses a sector": 15, "x = 65535": 6, "x = 0": 7, "behind a plateau": 80000,
                              "behind leading zeros": 100000, "row >= 32": 100000, "long block": 150000, "saturated tail": 250000,
                              "sum above 1": 120000},
                "downbranch": {"tie": 270, "tie run >= 2": 140, "tie run >= 8": 15, "decided inside a run": 55, "run crosses a quad": 45,
                               "run crosses the window": 5, "run crosses a sector": 13, "x = 65535": 6, "x = 0": 6, "behind a plateau": 80000,
                               "behind leading zeros": 130000, "row >= 32": 160000, "long block": 220000, "saturated tail": 240000,
                               "sum above 1": 80000}}
CHAIN_HOT = {"macroatom": {"hot 1": {"hits": 400000, "misses": 20000, "end unit": 50}, "hot auto": {"hits": 400000, "misses": 19000, "end unit": 50}},
             "downbranch": {"hot 1": {"hits": 320000, "misses": 15000, "end unit": 35}, "hot auto": {"hits": 310000, "misses": 13000, "end unit": 34}}}
CHAIN_PER_KIND = {"macroatom": 40000, "downbranch": 20000}
CHAIN_MIX = {"macroatom": {"no interaction": 180, "last is a line": 11000, "last is electron scattering": 800, "reabsorbed": 8000},
             "downbranch": {"no interaction": 500, "last is a line": 36000, "last is electron scattering": 2700, "reabsorbed": 26000}}

_samples = {}


def sample(oracle, prob, name):
    """(oracle result, jump log, census) of a problem; computed once."""
    if name not in _samples:
        ref, log = db.jump_log(oracle, prob)
        _samples[name] = (ref, log, db.census(prob, log))
    return _samples[name]


def hold(census, floors, hot, per_kind):
    for k, n in floors.items():
        assert census[k] >= n, (k, census[k])
    for h, d in hot.items():
        assert census[h]["hits"] + census[h]["misses"] == census[h]["jumps"]
        for k, n in d.items():
            assert census[h][k] >= n, (h, k, census[h][k])
    for k in db.KINDS:
        assert census["kind"][k] >= per_kind, (k, census["kind"][k])


@pytest.mark.parametrize("full,n_vpackets", CONFIGS)
def test_the_family_hits_what_it_is_for(oracle, full, n_vpackets):
    prob, ref = ktr.case(oracle, full, n_vpackets, "degenerate")  # (asserts return code 0)
    ref2, log, c = sample(oracle, prob, ("family", full, n_vpackets))
    assert same_bits(ref2.output_nus, ref.output_nus) and ref2.counters["macro_transitions"] == ref.counters["macro_transitions"]
    mix = ktr.sample_mix(ref)
    print(full, n_vpackets, mix, c)
    for what, n in mix.items():
        assert n >= FAMILY_PER_CLASS, what
    hold(c, FAMILY_FLOORS, FAMILY_HOT, FAMILY_PER_KIND)
    assert c["ran out"] == 0 and c["fp64 decided"] >= c["tie"]
    if n_vpackets:
        assert ref.vpacket_log_count > 1000


def test_the_giant_sample_hits_what_it_is_for(oracle):
    prob = db.giant_problem()
    ref, log, c = sample(oracle, prob, "giant")
    cn, mix = ref.counters, ktr.sample_mix(ref)
    print(mix, c, {k: cn[k] for k in ("events", "rng_draws", "macro_transitions")})
    assert ref.return_code == 0 and c["ran out"] == 0
    assert cn["rng_draws"] - 2 * cn["events"] >= 50_000 and cn["macro_transitions"] <= 3_000_000_000
    assert len(log) >= cn["rng_draws"] - 2 * cn["events"]
    assert (ref.output_energies > 0).sum() >= len(ref.output_energies) // 4, "at least a quarter of the packets are emitted"
    for what, n in GIANT_MIX.items():
        assert mix[what] >= n, what
    hold(c, GIANT_FLOORS, GIANT_HOT, 0)
    # the jumps out of the two giant blocks, by block and shell
    edge = prob.opacity_state.macro_block_edge_index
    for b in (prob.giant_a, prob.giant_b):
        for s in (0, 1):
            n = int(((log[:, 1] == edge[b]) & (log[:, 0] == s)).sum())
            print("giant block", b, "shell", s, "jumps", n)
            assert n >= GIANT_PER_BLOCK_AND_SHELL, (b, s, n)
    at_wide_row = int(((log[:, 1] == edge[prob.giant_a]) & (log[:, 2] == 65537)).sum())
    print("selections of row 65537", at_wide_row)
    assert at_wide_row >= GIANT_AT_THE_WIDE_ROW, at_wide_row


@pytest.mark.parametrize("mode", MODES)
def test_the_chain_sample_hits_what_it_is_for(oracle, mode):
    prob = db.chain_problem(mode)
    ref, log, c = sample(oracle, prob, ("chain", mode))
    mix = ktr.sample_mix(ref)
    print(mode, mix, c, ref.counters)
    assert ref.return_code == 0 and c["ran out"] == 0
    assert 200_000 <= c["jumps"] <= 1_000_000
    for what, n in CHAIN_MIX[mode].items():
        assert mix[what] >= n, what
    hold(c, CHAIN_FLOORS[mode], CHAIN_HOT[mode], CHAIN_PER_KIND[mode])
    assert c["x = 65535"] >= 5
    if mode == "macroatom":  # walks are many jumps long
        line_interactions = int(ref.trackers.interactions_count.sum())  # (an upper bound: electron scatterings are in it)
        assert c["jumps"] > 2 * line_interactions


# ---- (3) the errors -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", db.ERROR_KINDS)
def test_the_oracle_raises_the_reference_errors(oracle, what):
    prob = db.error_problem(what)
    want = _abi.ERR_UNSUPPORTED if what == "unsupported_type" else _abi.ERR_MACRO_ATOM
    one = db.oracle_run(oracle, prob, n_threads=1)
    many = db.oracle_run(oracle, prob, n_threads=oracle.max_threads())
    print(what, one.return_code, one.first_error_packet)
    assert one.return_code == many.return_code == one.error_code == want
    assert one.first_error_packet == many.first_error_packet >= 8, "an error on the very first packets says little"
    # the packet's last jump: the block ran out (row -1), or the selected row is of type -3
    ref, log = db.jump_log(oracle, prob, db.first_packets(prob.packet_collection, one.first_error_packet + 1))
    assert ref.first_error_packet == one.first_error_packet and len(log) > 0
    shell, b0, row = (int(v) for v in log[-1, :3])
    op = prob.opacity_state
    if what == "unsupported_type":
        assert row >= 0 and op.transition_type[b0 + row] == -3
    else:
        assert row == -1
        if what == "empty_block":
            assert b0 == op.macro_block_edge_index[-1]
        else:
            assert shell == db.ERROR_SHELL and db.events_of(log)[-1] >= 0.74


# ---- (4) rows of probability 0 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_zero_rows_change_nothing_but_the_count_of_examined_rows(oracle, mode):
    base, twin, old_of_new = db.zero_row_problems(mode)
    a, log, _ = sample(oracle, base, ("chain", mode))
    b = db.oracle_run(oracle, twin)
    assert a.return_code == b.return_code == 0
    assert same_bits(a.output_nus, b.output_nus) and same_bits(a.output_energies, b.output_energies)
    for f in ktr._golden.TRACKER_I64:
        assert np.array_equal(getattr(a.trackers, f), getattr(b.trackers, f)), f
    for f in ktr._golden.TRACKER_F64:
        assert same_bits(getattr(a.trackers, f), getattr(b.trackers, f)), f
    for f in ("j_estimator", "nu_bar_estimator", "j_blue_estimator", "edotlu_estimator"):
        assert same_bits(getattr(a, f), getattr(b, f)), f
    for k in ("rng_draws", "events", "line_visits"):
        assert a.counters[k] == b.counters[k], k
    # the inserted rows in front of every selection, from the jump log
    new_of_old = np.flatnonzero(old_of_new >= 0)
    sel = log[:, 2] >= 0
    assert sel.all()
    in_front = (new_of_old[log[:, 1] + log[:, 2]] - new_of_old[log[:, 1]]) - log[:, 2]
    grown = b.counters["macro_transitions"] - a.counters["macro_transitions"]
    print(mode, "inserted rows", int((old_of_new < 0).sum()), "examined rows grow by", grown)
    assert grown == int(in_front.sum()) > 10000
    assert a.counters["macro_transitions"] == int((log[:, 2] + 1).sum())
