"""The propagation kernels on line lists with coincident and near-coincident lines (tests/coincident_lines.py; the sample and the
reference's side are checked in tests/test_coincident_lines_host.py).

Where the fast kernels depend on how equal or nearly equal frequencies are handled: the lane sweep's "X >= 0 follows
from the sorted list after a run's first entry" -- after an emission into line k the packet restarts at k + 1 within an ulp of nu_k, and
where the lines behind k coincide with it X may be an ulp negative for the whole run; vp_shell_step's four-line window, whose predicate is
constant over a run of equal lines, while the reference adds a line's tau BEFORE it tests the line; the frequency-bucket index, where a run
of equal lines lands in one bucket and a one-frequency list has one key; the last line (MISS_DISTANCE, the -inf slack of nt_t, the clamped
window loads) at the end of a run.

(1) every row of the three kernel tables on the clustered problem family, at the bars of tests/test_kernel_table_gpu.py;
(2) zero-depth twins change nothing, on the device, through explicit option sets;
(3) the degenerate lists; (4) negative optical depths inside runs; (5) the estimator passes with a run across the tile boundary.
"""
import time

import numpy as np
import pytest
from numpy.testing import assert_allclose

import coincident_lines as cl
import kernel_table_recipes as ktr
from test_estimator_pipelines import _same as same_estimator_pipeline

pytestmark = pytest.mark.gpu

FAMILY = "clustered"
ROWS = [(t, row) for t in ktr.TABLES for row in ktr.table_rows(t)]
T0 = time.perf_counter()
TIMES = {}


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


# ---- (1) every row ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table,row", ROWS, ids=[ktr.row_id(t, row) for t, row in ROWS])
def test_row_on_the_clustered_list(oracle, table, row):
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

def _oracle(oracle, prob):
    ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                     prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=True)
    assert ref.return_code == 0
    return ref


def _run(prob, ref, options):
    """One propagate call on a fresh engine: (results, kernel-table row, v-packet log or None, launches)."""
    from tardis_amd.engine import Engine
    vlog = prob.montecarlo_configuration.NUMBER_OF_VPACKETS > 0 and prob.montecarlo_configuration.ENABLE_VPACKET_TRACKING
    with Engine(0) as eng:
        eng.set_option("track_last_interaction", 1)
        for name, value in options.items():
            eng.set_option(name, value)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        row = eng.last_kernel_key()
        launches = eng.last_kernel_times()["launches"]
        res = eng.get_results(track_last_interaction=True, vpacket_log_capacity=int(ref.vpacket_log_count) if vlog else None)
        log = eng.get_vpacket_log() if vlog else None
    return res, row, log, launches


def _same_as_oracle(res, log, ref):
    ktr.same_per_packet(res, ref, trackers=True)
    ktr.same_estimators_and_counters(res, ref)
    assert np.array_equal(res.j_blue_estimator == 0.0, ref.j_blue_estimator == 0.0)
    if log is not None:
        ktr.same_vpacket_log(res, log, ref)


# ---- (2) zero-depth twins ----------------------------------------------------------------------------------------------------------

LANE_SWEEP_SETS = [dict(variant=3, sweep_table=s, ls_waves_per_simd=w) for s in (0, 1, 2) for w in (3, 4)]


def _option_sets(full, n_vpackets):
    if n_vpackets:
        return [dict(variant=v, ls_waves_per_simd=4, vpacket_screening=s) for v in (0, 1, 2, 3) for s in (1, 0)]
    sets = [dict(variant=v, ls_waves_per_simd=4) for v in (0, 1, 2)]
    return sets + (LANE_SWEEP_SETS if not full else [dict(variant=3, ls_waves_per_simd=4)])


def _set_id(o):
    return "-".join(f"{k}{v}" for k, v in o.items())


TWIN_CALLS = [(full, nv, o) for full in (False, True) for nv in (0, ktr.N_VPACKETS) for o in _option_sets(full, nv)]
_twin_inputs, _twin_rows = {}, {}


def _twins(oracle, full, n_vpackets):
    k = (full, n_vpackets)
    if k not in _twin_inputs:
        base, twins, old_of_new = cl.twin_problems(full, n_vpackets)
        _twin_inputs[k] = (base, _oracle(oracle, base), twins, _oracle(oracle, twins), old_of_new)
    return _twin_inputs[k]


def _twin_call(oracle, full, n_vpackets, options):
    """Device without twins and with them, each against its oracle and the two against each other; the rows the calls ran on."""
    k = (full, n_vpackets, _set_id(options))
    if k in _twin_rows:
        return _twin_rows[k]
    base, ref_a, twins, ref_b, old_of_new = _twins(oracle, full, n_vpackets)
    a, row_a, log_a, _ = _run(base, ref_a, options)
    b, row_b, log_b, _ = _run(twins, ref_b, options)
    print(full, n_vpackets, options, "->", row_a, row_b)
    # device with twins against device without: per-packet arrays bit for bit (the line ids through the index map) ...
    assert np.array_equal(a.output_nus, b.output_nus) and np.array_equal(a.output_energies, b.output_energies)
    ta, tb = a.trackers, b.trackers
    for f in ktr._golden.TRACKER_F64:
        assert np.array_equal(getattr(ta, f), getattr(tb, f), equal_nan=True), f
    for f in ("shell_id", "interaction_type", "interactions_count"):
        assert np.array_equal(getattr(ta, f), getattr(tb, f)), f
    line = ta.interaction_type == 2
    for f in ("interaction_line_absorb_id", "interaction_line_emit_id"):
        assert np.array_equal(getattr(ta, f)[line], old_of_new[getattr(tb, f)[line]]), f
        assert np.array_equal(getattr(ta, f)[~line], getattr(tb, f)[~line]), f
    # ... the estimators on the old lines within the summation-order tolerance, the draws exactly
    old = old_of_new >= 0
    assert_allclose(b.j_estimator, a.j_estimator, rtol=ktr.EST_RTOL, atol=0)
    assert_allclose(b.nu_bar_estimator, a.nu_bar_estimator, rtol=ktr.EST_RTOL, atol=0)
    assert_allclose(b.j_blue_estimator[old], a.j_blue_estimator, rtol=ktr.EST_RTOL, atol=0)
    assert_allclose(b.edotlu_estimator[old], a.edotlu_estimator, rtol=ktr.EST_RTOL, atol=0)
    assert a.counters["rng_draws"] == b.counters["rng_draws"] and a.counters["events"] == b.counters["events"]
    if n_vpackets:
        assert_allclose(b.v_packets_energy_hist, a.v_packets_energy_hist, rtol=ktr.EST_RTOL, atol=0)
        for f in ("nus", "energies", "initial_mus", "initial_rs"):
            assert np.array_equal(getattr(log_a, f), getattr(log_b, f)), f
    # each against the oracle
    _same_as_oracle(a, log_a, ref_a)
    _same_as_oracle(b, log_b, ref_b)
    assert row_a == row_b
    _twin_rows[k] = row_a
    return row_a


@pytest.mark.parametrize("full,n_vpackets,options", TWIN_CALLS, ids=[f"full{int(f)}-nv{n}-{_set_id(o)}" for f, n, o in TWIN_CALLS])
def test_zero_depth_twins_change_nothing_on_the_device(oracle, full, n_vpackets, options):
    _twin_call(oracle, full, n_vpackets, options)


def test_the_twin_calls_reach_every_table_and_both_lane_sweep_forms(oracle):
    rows = {_twin_call(oracle, full, nv, o) for full, nv, o in TWIN_CALLS}
    print(sorted(rows))
    assert {t for t, _ in rows} == set(ktr.TABLES)
    wave = [dict(zip(ktr.FIELDS["wave"], key)) for t, key in rows if t == "wave"]
    sweeps = [k for k in wave if k["LS"] and not k["VPK"]]
    assert {k["WPE"] for k in sweeps} == {3, 4}, "ten lines per step (four waves per SIMD) and twelve (three)"
    assert {k["NT"] for k in sweeps} == {0, 1, 2}, "the separate tables, the interleaved table, its twelve-line form"
    assert any(k["LS"] and k["VPK"] for k in wave) and any(not k["LS"] and k["VPK"] for k in wave) and any(k["FULL"] for k in wave)


# ---- (3) the degenerate lists -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("n_vpackets", [0, ktr.N_VPACKETS])
@pytest.mark.parametrize("n_frequencies", [1, 2])
def test_degenerate_lists(oracle, n_frequencies, n_vpackets, full, variant):
    prob = cl.degenerate_problem(n_frequencies, full, n_vpackets)
    ref = _oracle(oracle, prob)
    assert (ref.trackers.interaction_type == 2).sum() > 0
    for options in ([dict(variant=variant, ls_waves_per_simd=w) for w in ((4, 3) if variant == 3 and not full and not n_vpackets else (4,))]):
        res, row, log, _ = _run(prob, ref, options)
        print(n_frequencies, n_vpackets, full, options, "->", row)
        _same_as_oracle(res, log, ref)


# ---- (4) negative optical depths inside runs -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def negative_tau(oracle):
    prob = ktr.make_problem(False, 0, FAMILY)
    _, kind, _ = cl.clustered()
    lines = np.random.default_rng(11).choice(np.flatnonzero(kind != 0), 40, replace=False)
    prob.opacity_state.tau_sobolev[lines, :] *= -0.01
    assert (prob.opacity_state.tau_sobolev < 0).any()
    return prob, _oracle(oracle, prob)


@pytest.mark.parametrize("options", LANE_SWEEP_SETS, ids=[_set_id(o) for o in LANE_SWEEP_SETS])
def test_negative_optical_depths_inside_runs(negative_tau, options):
    prob, ref = negative_tau
    res, row, _, _ = _run(prob, ref, options)
    print(options, "->", row)
    k = dict(zip(ktr.FIELDS["wave"], row[1]))
    assert row[0] == "wave" and k["LS"] == 1 and k["VPK"] == 0
    assert k["NT"] == 0, "a table with a negative optical depth must not be swept on the interleaved table"
    _same_as_oracle(res, None, ref)


# ---- (5) the estimator passes across the tile boundary -------------------------------------------------------------------------------

@pytest.mark.parametrize("accumulate", [1, 3])
def test_estimator_passes_across_the_tile_boundary(oracle, accumulate):
    prob, ref = ktr.case(oracle, False, 0, FAMILY)
    _, _, place = cl.clustered()
    run = np.flatnonzero(place == cl.AT_TILE_BOUNDARY)
    # the run is visited on both sides of line 2048 (not every line of it: an optically thick line shadows the equal lines behind it)
    assert np.any(ref.j_blue_estimator[run[run < ktr.EST_TILE]] != 0) and np.any(ref.j_blue_estimator[run[run >= ktr.EST_TILE]] != 0)
    capacity = int(ref.counters["events"]) // 5
    res, row, _, launches = _run(prob, ref, dict(variant=3, ls_waves_per_simd=4, est_accumulate=accumulate, log_capacity=capacity, log_chunk_records=257))
    print(accumulate, "log capacity", capacity, "launches", launches, row)
    assert row[0] == "wave" and launches >= 3
    same_estimator_pipeline(res, ref)
    _same_as_oracle(res, None, ref)


def test_zz_time_of_this_file():
    """Printed for the record (run with -s): the file's total and its slowest test."""
    slowest = max(TIMES, key=TIMES.get)
    print("tests/test_coincident_lines_gpu.py: %d tests, %.1f s since import; slowest %s %.2f s" % (len(TIMES), time.perf_counter() - T0, slowest, TIMES[slowest]))
