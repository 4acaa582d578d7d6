"""The resident prefix-sum tables of the v-packet screening (tardis_amd/csrc/tau_prefix.hpp) and of the lane sweep's block skip
(tardis_amd/csrc/sweep_skip.hpp), and the two margins argued from them.

  * The tables themselves, read back through op 101 of `tardis_mc_debug_eval`, against exact sums (tests/prefix_tables_ref.py): twelve adversarial rows at
    line counts that give tau_prefix_kernel's threads chunks of 1, 2, 3, 17 and 79 lines and rows that end in the middle of a chunk.  Every entry within
    (2^-53 + 2^-70) P of the exact sum P; the block skip's tables bit for bit what their layout says.
  * The screening's margin on three problems whose v-packets come within 1e-12 of the roulette threshold (tests/test_prefix_tables_host.py shows with
    the oracle alone that they do): a long drift of an inexact term, prefix sums of 7e9 that cancel to 10, and a list so dense that the margin's
    (n + 4) tau_shell term is the larger one.
  * The block skip on tables whose margin M is large, and both on rows that hold +inf or overflow.
"""
import numpy as np
import pytest

import prefix_tables_ref as ptr
import test_sweep_skip_gpu as ssg
from test_prefix_tables_host import reference
from test_vpacket_screening import DECIDED, _run, _same
from tardis_amd import _abi, synthetic

pytestmark = pytest.mark.gpu

SMALLEST = 1  # (neither plan has a floor on the line count: the shortest list set_opacity takes)
LINE_COUNTS = [SMALLEST, 257, 513, 4099, 20003]
_tables = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _propagate(eng, prob):
    eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
    eng.set_packets(prob.packet_collection)
    eng.reset_estimators()
    eng.propagate()
    eng.synchronize()


def device_tables(n_lines):
    """The tables of the adversarial problem of `n_lines` lines, read back once: one lane-sweep call of 4096 packets that builds the block skip's, one call
    of 512 packets with 3 v-packets that builds the screening's."""
    if n_lines in _tables:
        return _tables[n_lines]
    from tardis_amd.engine import Engine
    prob, rows = ptr.table_problem(n_lines, 4096)
    vprob, vrows = ptr.table_problem(n_lines, 512, n_vpackets=3)
    assert np.array_equal(bits(rows), bits(vrows))
    t = dict(rows=rows, nu=np.array(prob.opacity_state.line_list_nu), exact=[ptr.exact_prefix(r) for r in rows])
    with Engine(0) as eng:
        eng.set_option("variant", 3)
        eng.set_option("ls_waves_per_simd", 4)
        eng.set_option("sweep_skip", 1)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        for name in eng.PREFIX_TABLES:  # nothing is built yet
            with pytest.raises(RuntimeError) as ei:
                eng.debug_prefix_table(name)
            assert ei.value.code == _abi.ERR_STATE, name
        _propagate(eng, prob)
        t["skip_on"] = eng.last_sweep_skip()
        for name in ("pn", "ct", "sk_rowsum", "sk_state"):
            t[name] = eng.debug_prefix_table(name)
        with pytest.raises(RuntimeError) as ei:  # (that call screened nothing)
            eng.debug_prefix_table("tau_pfx")
        assert ei.value.code == _abi.ERR_STATE
        eng.set_option("variant", -1)
        eng.set_option("vpacket_screening", 1)
        _propagate(eng, vprob)
        for name in ("tau_pfx", "tau_rowsum"):
            t[name] = eng.debug_prefix_table(name)
        with pytest.raises(RuntimeError) as ei:  # a range that leaves the table
            eng.debug_eval(101, [0, 1], n=ptr.N_TABLE_SHELLS * (n_lines + 1))
        assert ei.value.code == _abi.ERR_INVALID_ARGUMENT
        assert np.array_equal(bits(eng.debug_eval(101, [0, n_lines], n=2)), bits(t["tau_pfx"].reshape(-1)[n_lines:n_lines + 2]))
        eng.set_opacity(vprob.opacity_state)  # a new opacity state: the tables of the old one are gone
        for name in eng.PREFIX_TABLES:
            with pytest.raises(RuntimeError) as ei:
                eng.debug_prefix_table(name)
            assert ei.value.code == _abi.ERR_STATE, name
    _tables[n_lines] = t
    return t


@pytest.mark.parametrize("n_lines", LINE_COUNTS)
def test_every_prefix_sum_is_within_its_bound_of_the_exact_sum(n_lines):
    """|P^ - P| <= (2^-53 + 2^-70) P for every entry of the screening's table, pfx[s][L] and the row sums included (the block skip's prefix sums are
    the same numbers, test_block_skip_tables_are_what_their_layout_says).  Measured on an MI355X: every entry of every row at every line count is the
    correctly rounded sum (profiles/prefix_tables.txt)."""
    t = device_tables(n_lines)
    assert t["tau_pfx"].shape == (ptr.N_TABLE_SHELLS, n_lines + 1)
    worst_all = wrong_all = 0
    for s, name in enumerate(ptr.ROW_NAMES):
        exact = t["exact"][s]
        bad, worst, not_rounded = ptr.check_row(t["tau_pfx"][s], exact)
        sums = [t["tau_rowsum"][s], t["sk_rowsum"][s]]
        bad_sums, worst_sums, not_rounded_sums = ptr.check_row(sums, [exact[n_lines]] * 2)
        print("L %5d row %-22s largest error %.4f x 2^-53 P, not correctly rounded %d of %d; row sums %.4f, %d of 2"
              % (n_lines, name, worst, not_rounded, n_lines + 1, worst_sums, not_rounded_sums))
        assert not bad, (name, bad[:8], [(t["tau_pfx"][s][i], float(exact[i])) for i in bad[:3]])
        assert not bad_sums, (name, sums, float(exact[n_lines]))
        worst_all, wrong_all = max(worst_all, worst, worst_sums), wrong_all + not_rounded + not_rounded_sums
    print("L %5d: largest error %.4f x 2^-53 P, %d entries not correctly rounded" % (n_lines, worst_all, wrong_all))


@pytest.mark.parametrize("n_lines", LINE_COUNTS)
def test_block_skip_tables_are_what_their_layout_says(n_lines):
    t = device_tables(n_lines)
    S, L = ptr.N_TABLE_SHELLS, n_lines
    assert t["skip_on"] == 1
    pfx, pn, ct, nu = t["tau_pfx"], t["pn"], t["ct"], t["nu"]
    # the prefix halves are the screening's table; the frequency halves the interleaved table's slots (-inf from line L - 1 on)
    assert np.array_equal(bits(pn[:, :, 1]), bits(pfx))
    slot = np.full(8 * ((L + 7) // 8) + 8, -np.inf)
    slot[:L - 1] = nu[:L - 1]
    assert np.array_equal(bits(pn[:, :, 0]), bits(np.broadcast_to(slot[:L + 1], (S, L + 1))))
    # coarse entries: {slot of the block's last entry, pfx[s][min(8 b + 8, L)]}, then 16 of slack {-inf, the last row's total}
    rows = (L + 7) // 8
    assert ct.shape == (S * rows + 16, 2) and t["sk_state"][2] == 8 * rows
    b = np.arange(rows)
    want = np.empty((S, rows, 2))
    want[:, :, 0] = slot[8 * b + 7]
    want[:, :, 1] = pfx[:, np.minimum(8 * b + 8, L)]
    assert np.array_equal(bits(ct[:S * rows]), bits(want.reshape(S * rows, 2)))
    assert np.isneginf(want[:, (L - 1) // 8:, 0]).all()  # (the block that holds line L - 1, and whatever lies behind it)
    assert np.isneginf(ct[S * rows:, 0]).all() and np.array_equal(bits(ct[S * rows:, 1]), bits(np.full(16, pfx[S - 1, L])))
    # the margin: ssk::margin of the largest row sum; this table is all finite and non-negative
    assert t["sk_state"][0] == ptr.ssk_margin(L, float(t["sk_rowsum"].max())) and t["sk_state"][1] == 0.0


# ---- the screening's margin, attacked
@pytest.fixture(scope="module")
def engine():
    from tardis_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("name", ptr.SCENARIOS)
def test_screening_decides_no_near_tie_wrongly(engine, oracle, name, variant):
    """At each of the three thresholds -- three different reference runs -- the engine with the screening forced on is the oracle: per-packet outputs,
    v-packet histogram and log, every work counter (_same of tests/test_vpacket_screening.py, the log compared).  One v-packet decided on the wrong
    side shifts its parent's random stream and shows in all of them.

    What each scenario is known to catch (profiles/prefix_tables.txt): a margin without its row-sum term fails `cancellation` on both kernels.  A margin
    without its (n + 4) tau_shell term fails NEITHER `concentrated` nor that scenario enlarged to 4000 lines of 0.01 -- serial sums of equal terms stay
    within a few ulps, far below the worst case the term pays for -- so `concentrated` pins that the margin is large enough there, not that the term is
    needed."""
    prob = ptr.screening_problem(name)
    for thr in ptr.THRESHOLDS:
        ref = reference(oracle, name, thr)
        prob.montecarlo_configuration.VPACKET_TAU_RUSSIAN = thr
        got = _run(engine, prob, variant, 1, flags=DECIDED)
        decided = got.counters["reserved"] >> 40
        print("%s variant %d threshold %.17g: %d v-packets, %d decided on the prefix sums" % (name, variant, thr, ref.counters["vpackets"], decided))
        _same(got, ref, True)
        if name != "concentrated":
            assert decided > 0
        off = _run(engine, prob, variant, 0, flags=DECIDED)
        assert off.counters["reserved"] >> 40 == 0
        _same(off, ref, True)


# ---- the block skip on tables that make its margin large
_skip_cases = {}


def skip_case(oracle, problem, table):
    key = (problem, table)
    if key not in _skip_cases:
        prob, _ = ssg.case(oracle, problem)
        make = ptr.skip_table if table in ptr.SKIP_TABLES else ptr.special_table
        op = ptr.with_tau(prob.opacity_state, make(table, prob.opacity_state.tau_sobolev))
        ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, op, prob.montecarlo_configuration, prob.spectrum_frequency_grid,
                         math_mode=oracle.MATH_PORTABLE, n_threads=oracle.max_threads(), track_last_interaction=True)
        assert ref.return_code == 0
        _skip_cases[key] = (prob, op, ref)
    return _skip_cases[key]


@pytest.mark.parametrize("several", [False, True], ids=["one-launch", "several-launches"])
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("table", ptr.SKIP_TABLES)
@pytest.mark.parametrize("problem", ["a", "b"])
def test_block_skip_on_large_margins(oracle, problem, table, skip, several):
    """Problems (a) and (b) of tests/test_sweep_skip_gpu.py with 200 blue lines of 1e6, 40 lines of 1e4 ... 1e8, one shell times 1e9: M between 7e-4 and
    more than 1, so many interval-mode decisions fall back and g = 8 M is comparable to tau_event."""
    prob, op, ref = skip_case(oracle, problem, table)
    extra = dict(log_capacity=max(256 * ((ssg.N_PACKETS + 63) // 64), int(ref.counters["events"]) // 5), log_chunk_records=257) if several else {}
    res, row, launches, _, on = ssg.run(prob, opacity_state=op, sweep_skip=skip, **extra)
    print(problem, table, "skip", skip, "->", on, "launches", launches, row)
    assert ssg.sixteen_wave_interleaved(row) and on == skip
    assert launches >= 2 or not several
    ssg.same_as_oracle(res, ref)


# ---- non-finite and overflowing rows
@pytest.mark.parametrize("table", ptr.SPECIAL_TABLES)
@pytest.mark.parametrize("problem", ["a", "b"])
def test_lane_sweep_on_rows_that_hold_inf_or_overflow(oracle, problem, table):
    """+inf on one line of one shell; two 1e308 in one row, whose sum overflows: the block skip reports off (its row sums are not finite), the call is
    the oracle's."""
    prob, op, ref = skip_case(oracle, problem, table)
    res, row, _, _, on = ssg.run(prob, opacity_state=op, sweep_skip=1)
    print(problem, table, "->", row, "skip", on)
    assert on == 0
    ssg.same_as_oracle(res, ref)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("table", ptr.SPECIAL_TABLES)
def test_screening_on_rows_that_hold_inf_or_overflow(engine, oracle, table, variant):
    """Downbranch with 3 v-packets and the screening forced: behind the +inf the prefix sums of that row are NaN (inf - inf in the two-sum), behind the
    second 1e308 as well -- every comparison with them fails, the v-packet is left to the line-by-line trace."""
    prob = synthetic.make_problem(seed=42, n_packets=1500, n_shells=30, n_lines=8_000, line_interaction_type="downbranch", n_vpackets=3, log_tau_mean=-1.5)
    prob.montecarlo_configuration.ENABLE_VPACKET_TRACKING = True
    prob.opacity_state = ptr.with_tau(prob.opacity_state, ptr.special_table(table, prob.opacity_state.tau_sobolev))
    ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                     prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=oracle.max_threads(), track_last_interaction=False)
    assert ref.return_code == 0 and np.isfinite(ref.v_packets_energy_hist).all() and (ref.vpacket_energies == 0).sum() > 1000
    got = _run(engine, prob, variant, 1, flags=DECIDED)
    print(table, "variant", variant, "decided on the prefix sums:", got.counters["reserved"] >> 40, "of", ref.counters["vpackets"])
    _same(got, ref, True)
