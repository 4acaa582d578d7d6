"""The macro-atom walks on degenerate transition-probability tables (tests/degenerate_blocks.py; the tables, the samples and the
reference's side are checked in tests/test_degenerate_blocks_host.py).

Where the device departs from the reference's arithmetic: the compact walk decides a jump on 16-bit running sums and asks the
fp64 sums only where an entry equals x = floor(number 65536); saturated entries and the 0xffff padding tie at x = 65535; blocks longer than
one 32-entry window are narrowed by a binary search on the quads' last entries; hot sectors hold six intervals with saturating ends and a
16-bit row number; a number a sector does not decide is parked across passes and launches; the fp64 cross-check walks, the lane kernel and
the group kernel have scans of their own.  Plateaus, tie runs across a quad, a window or a sector, rows past 65 535, sums above and below 1
and empty blocks are what these tables are made of.

At the bars of tests/kernel_table_recipes.py: per-packet results and the fourteen tracker fields bit for bit, estimators within EST_RTOL,
line_visits / events / macro_transitions / rng_draws exactly, j_blue == 0 in the same places.

(1) every row of the three kernel tables on the "degenerate" family; (2) the giant and the chain problems through every walk there is;
(3) the device takes the paths, by its debug counters against the census; (4) carried and parked walks; (5) the errors; (6) rows of
probability 0 change nothing on the device; (7) one engine through three sets of tables.
"""
import time

import numpy as np
import pytest
from numpy.testing import assert_allclose

import degenerate_blocks as db
import kernel_table_recipes as ktr

pytestmark = pytest.mark.gpu

FAMILY = "degenerate"
ROWS = [(t, row) for t in ktr.TABLES for row in ktr.table_rows(t)]
LONG_JUMPS, FP64_DECIDED, HOT_HIT, HOT_MISS = 16384, 32768, 65536, 131072  # debug flags -> counters["reserved"]
T0 = time.perf_counter()
TIMES = {}


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


# ---- (1) every row ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table,row", ROWS, ids=[ktr.row_id(t, row) for t, row in ROWS])
def test_row_on_the_degenerate_family(oracle, table, row):
    k = dict(zip(ktr.FIELDS[table], row))
    t0 = time.perf_counter()
    for rec in ktr.recipes(table, row) or [ktr.recipe(table, row)]:
        prob, ref = ktr.case(oracle, rec.full, rec.n_vpackets, FAMILY)
        got = ktr.run(rec, prob, ref)
        assert got.row == (table, row), (rec.options, got.row)
        res = got.results
        ktr.same_per_packet(res, ref, trackers=bool(k["TRACK"]))
        ktr.same_estimators_and_counters(res, ref)
        assert np.array_equal(res.j_blue_estimator == 0.0, ref.j_blue_estimator == 0.0)  # unvisited lines: exactly zero
        if k["VPK"]:
            ktr.same_vpacket_log(res, got.vpacket_log, ref)
        if k["VLI"]:
            ktr.same_last_interaction_columns(got.vpacket_log, ktr.lane_event_log(oracle, rec.full, rec.n_vpackets, FAMILY),
                                              prob.montecarlo_configuration, rec.n_vpackets)
        if k.get("FT"):
            if table == "lane":
                ktr.same_as_oracle_trace(got.event_log, ktr.oracle_trace(oracle, rec.full, rec.n_vpackets, FAMILY), res)
            else:
                ktr.same_event_log(got.event_log, ktr.lane_event_log(oracle, rec.full, rec.n_vpackets, FAMILY))
    print(ktr.row_id(table, row), "%.2f s" % (time.perf_counter() - t0))


# ---- one call with explicit options ------------------------------------------------------------------------------------------------

_refs = {}


def _problem(name):
    return db.giant_problem() if name == "giant" else db.chain_problem(name)


def _reference(oracle, name, shard=None):
    """(packets, oracle result, jump log) of a problem or of a shard (rank, world) of its packets; computed once."""
    k = (name, shard)
    if k not in _refs:
        prob = _problem(name)
        pc = prob.packet_collection if shard is None else prob.packet_collection.shard(*shard)
        ref, log = db.jump_log(oracle, prob, pc)
        assert ref.return_code == 0
        _refs[k] = (pc, ref, log)
    return _refs[k]


def _call(eng, prob, pc):
    eng.set_geometry(prob.geometry, prob.time_explosion)
    eng.set_opacity(prob.opacity_state)
    eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
    eng.set_packets(pc)
    eng.reset_estimators()
    eng.propagate()
    eng.synchronize()
    return eng.get_results(track_last_interaction=True)


def _run(prob, pc, options):
    """One propagate call on a fresh engine: (results, kernel-table row, launches)."""
    from tardis_amd.engine import Engine
    with Engine(0) as eng:
        eng.set_option("track_last_interaction", 1)
        for name, value in options.items():
            eng.set_option(name, value)
        t0 = time.perf_counter()
        res = _call(eng, prob, pc)
        print(options, "->", eng.last_kernel_key(), "%.2f s" % (time.perf_counter() - t0))
        return res, eng.last_kernel_key(), eng.last_kernel_times()["launches"]


def _same_as_oracle(res, ref):
    ktr.same_per_packet(res, ref, trackers=True)
    ktr.same_estimators_and_counters(res, ref)
    assert np.array_equal(res.j_blue_estimator == 0.0, ref.j_blue_estimator == 0.0)


def _same_per_packet(a, b):
    assert np.array_equal(a.output_nus, b.output_nus) and np.array_equal(a.output_energies, b.output_energies)
    for f in ktr._golden.TRACKER_I64 + ktr._golden.TRACKER_F64:
        assert np.array_equal(getattr(a.trackers, f), getattr(b.trackers, f), equal_nan=True), f


# ---- (2) every walk path -----------------------------------------------------------------------------------------------------------

MIXED_MASS = dict(walk_hot=-1, walk_hot_min_mass=990, walk_hot_min_mass_long=990)  # (of the blocks with rows some are hot, some not: checked below)
PATHS = {
    "compact-hot0": dict(walk_hot=0),
    "compact-hot1": dict(walk_hot=1),
    "compact-auto": dict(walk_hot=-1),
    "compact-mixed-mass": MIXED_MASS,
    "compact-hot0-unpacked": dict(walk_hot=0, walk_sector_packing=0),
    "compact-hot1-unpacked": dict(walk_hot=1, walk_sector_packing=0),
    "fp64-group-scan": dict(debug_flags=ktr.WALK_GROUP_FP64),
    "fp64-lane-search": dict(debug_flags=ktr.WALK_LANE_FP64),
    "variant0": dict(variant=0),
    "variant1": dict(variant=1),
    "variant2": dict(variant=2),
    "variant3": dict(variant=3),
}
# a shard (rank, world) of the giant problem's packets for a path that takes more than about 10 s on all of them.  Measured on an MI355X: the serial
# scans of its 1.3e9 rows take 0.5 s (variant 0) and 0.2 s (flag 8192) on all 6000 packets: no path needs one
GIANT_SHARDS = {}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["giant", "macroatom", "downbranch"])
def test_every_walk_path(oracle, name, path):
    prob = _problem(name)
    pc, ref, _ = _reference(oracle, name, GIANT_SHARDS.get(path) if name == "giant" else None)
    options = PATHS[path]
    if path == "compact-mixed-mass":
        hot = db.hot_blocks(prob, -1, options["walk_hot_min_mass"], options["walk_hot_min_mass_long"])
        with_rows = np.diff(prob.opacity_state.macro_block_edge_index) > 0
        assert 0 < hot.sum() < with_rows.sum() and hot.sum() < db.hot_blocks(prob, -1).sum()
    if path == "compact-hot1" and name == "giant":  # both giant blocks: empty or one-entry sectors, every number is looked up again
        assert np.all(db.hot_sector_entries(prob, prob.giant_a) <= 1) and np.all(db.hot_sector_entries(prob, prob.giant_b) <= 1)
    res, row, _ = _run(prob, pc, options)
    if path.startswith("compact") or path.startswith("fp64"):
        k = dict(zip(ktr.FIELDS["wave"], row[1]))
        assert row[0] == "wave" and k["XWALK"] == int(path.startswith("fp64"))
    else:
        assert row[0] == {"variant0": "lane", "variant1": "group", "variant2": "wave", "variant3": "wave"}[path]
    _same_as_oracle(res, ref)


# ---- (3) the device takes the paths -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["giant", "macroatom"])
def test_the_device_takes_the_paths(oracle, name):
    """The debug counters of the compact walk against the census of the same shard (the first quarter of the packets).

    walk_hot 0: counter 16384 is the census' jumps out of blocks of more than one window; counter 32768, the jumps decided on the fp64
    sums, EQUALS the census' "fp64 decided": the census restates the window predicate exactly -- the binary search on the quads' last
    entries, the four quads read from there, the 0xffff padding that ties at x = 65535 -- and not only the ties among real rows.
    walk_hot 1: hot hits (65536) and hot misses (131072) are the census' hits and misses, and together its jumps out of hot blocks (every
    jump, but for none out of an empty block: there is none here); a number that meets a tie misses every interval, so the fp64-decided
    count is that of walk_hot 0.  walk_hot -1: hits and misses are the census' for the blocks the automatic choice puts on hot sectors.
    With a counter on, the results are those without."""
    prob = _problem(name)
    pc, ref, log = _reference(oracle, name, (0, 4))
    c = db.census(prob, log)
    print(name, {k: v for k, v in c.items() if k != "kind"})
    assert c["ran out"] == 0 and c["fp64 decided"] >= c["tie"] > 50 and c["long block"] > 1000
    got = {}
    for walk_hot, flags in ((0, LONG_JUMPS), (0, FP64_DECIDED), (1, HOT_HIT), (1, HOT_MISS), (1, FP64_DECIDED), (-1, HOT_HIT), (-1, HOT_MISS)):
        res, row, _ = _run(prob, pc, dict(walk_hot=walk_hot, debug_flags=flags))
        _same_as_oracle(res, ref)
        got[(walk_hot, flags)] = int(res.counters["reserved"])
    print(name, "device counters", got)
    assert got[(0, LONG_JUMPS)] == c["long block"]
    assert got[(0, FP64_DECIDED)] == c["fp64 decided"]
    hot = c["hot 1"]
    assert hot["jumps"] == c["jumps"] and hot["hits"] > 1000 and hot["misses"] > 1000
    assert got[(1, HOT_HIT)] == hot["hits"] and got[(1, HOT_MISS)] == hot["misses"]
    assert got[(1, HOT_HIT)] + got[(1, HOT_MISS)] == hot["jumps"]
    # an interval holds no row's 16-bit sum (lo = the sum in front + 1, x < hi) and never x = 65535: every number that meets a tie -- real or
    # padding -- misses its sector and is looked up again in the block's own tables, where it is decided on the fp64 sums as before
    assert got[(1, FP64_DECIDED)] == got[(0, FP64_DECIDED)]
    # the automatic choice of blocks (the mean width of the six intervals over the shells against walk_hot_min_mass): some blocks hot, some not
    auto = c["hot auto"]
    assert 1000 < auto["jumps"] < c["jumps"] and got[(-1, HOT_HIT)] == auto["hits"] and got[(-1, HOT_MISS)] == auto["misses"]


# ---- (4) carried and parked walks ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [2, 3])
def test_parked_numbers_survive_carried_walks_and_launches(oracle, variant):
    """The chain problem in macro-atom mode, every block on a hot sector, walks carried over from pass to pass (walk_min_active 32) and a
    line-visit log so small that the call takes three launches or more: the results are those of the one-launch call and of the oracle,
    bit for bit.  (As test_looked_up_again_numbers_survive_carried_walks_and_epochs of tests/test_walk_hot_sectors.py, on tables whose
    sectors miss on plateaus, tie runs and saturated tails.)"""
    prob = _problem("macroatom")
    pc, ref, _ = _reference(oracle, "macroatom")
    small = int(ref.counters["line_visits"]) // 16
    outs = []
    for cap in (None, small):
        options = dict(variant=variant, walk_hot=1, walk_min_active=32)
        if cap:
            options["log_capacity"] = cap
        res, row, launches = _run(prob, pc, options)
        print("log capacity", cap, "launches", launches)
        assert launches == 1 if cap is None else launches >= 3
        outs.append(res)
    a, b = outs
    _same_per_packet(a, b)
    assert a.counters == b.counters
    _same_as_oracle(a, ref)
    _same_as_oracle(b, ref)


# ---- (5) the errors -----------------------------------------------------------------------------------------------------------------

ERROR_PATHS = {k: PATHS[k] for k in ("compact-hot0", "compact-hot1", "fp64-group-scan", "fp64-lane-search", "variant0", "variant1")}
_error_refs = {}


@pytest.mark.parametrize("path", list(ERROR_PATHS))
@pytest.mark.parametrize("what", db.ERROR_KINDS)
def test_the_errors_are_the_reference_errors(oracle, what, path):
    from tardis_amd.engine import MacroAtomError
    if what not in _error_refs:
        prob = db.error_problem(what)
        _error_refs[what] = (prob, db.oracle_run(oracle, prob, n_threads=oracle.max_threads(), track=False))
    prob, ref = _error_refs[what]
    assert ref.return_code != 0 and ref.first_error_packet >= 8
    with pytest.raises(NotImplementedError if what == "unsupported_type" else MacroAtomError) as ei:
        _run(prob, prob.packet_collection, ERROR_PATHS[path])
    assert ei.value.packet_index == ref.first_error_packet and ei.value.code == ref.return_code


# ---- (6) rows of probability 0 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", [dict(), dict(variant=0)], ids=["wave-automatic", "variant0"])
@pytest.mark.parametrize("mode", ["macroatom", "downbranch"])
def test_zero_rows_change_nothing_on_the_device(oracle, mode, options):
    base, twin, old_of_new = db.zero_row_problems(mode)
    _, ref_a, _ = _reference(oracle, mode)
    if ("twin", mode) not in _refs:
        _refs[("twin", mode)] = db.oracle_run(oracle, twin)
    ref_b = _refs[("twin", mode)]
    a, row_a, _ = _run(base, base.packet_collection, options)
    b, row_b, _ = _run(twin, twin.packet_collection, options)
    assert row_a == row_b and row_a[0] == ("lane" if options else "wave")
    _same_per_packet(a, b)
    for f in ("j_estimator", "nu_bar_estimator", "j_blue_estimator", "edotlu_estimator"):
        assert_allclose(getattr(b, f), getattr(a, f), rtol=ktr.EST_RTOL, atol=0)
    for k in ("rng_draws", "events", "line_visits"):
        assert a.counters[k] == b.counters[k], k
    assert b.counters["macro_transitions"] > a.counters["macro_transitions"]
    _same_as_oracle(a, ref_a)
    _same_as_oracle(b, ref_b)


# ---- (7) rebuilding the tables ------------------------------------------------------------------------------------------------------

def test_one_engine_through_three_sets_of_tables(oracle):
    """set_opacity with the chain tables, then with the family's (another shape: 12 shells x 3000 lines), then the chain tables again on ONE
    engine: the last call is a fresh engine's, bit for bit (stale hot flags, blk_tab or cum16_stride would show), and every call is the
    oracle's."""
    from tardis_amd.engine import Engine
    chain = _problem("macroatom")
    pc, ref, _ = _reference(oracle, "macroatom")
    family, family_ref = ktr.case(oracle, False, 0, FAMILY)
    fresh, _, _ = _run(chain, pc, dict())
    with Engine(0) as eng:
        eng.set_option("track_last_interaction", 1)
        first = _call(eng, chain, pc)
        middle = _call(eng, family, family.packet_collection)
        last = _call(eng, chain, pc)
    _same_as_oracle(middle, family_ref)
    for res in (first, last):
        _same_per_packet(res, fresh)
        assert res.counters == fresh.counters
        _same_as_oracle(res, ref)


def test_zz_time_of_this_file():
    """Printed for the record (run with -s): the file's total and its slowest test."""
    slowest = max(TIMES, key=TIMES.get)
    print("tests/test_degenerate_blocks_gpu.py: %d tests, %.1f s since import; slowest %s %.2f s" % (len(TIMES), time.perf_counter() - T0, slowest, TIMES[slowest]))
