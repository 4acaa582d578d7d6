"""The propagation kernels on degenerate packets, thin shells and extreme scales (tests/edge_kinematics.py; the sample and the reference's
side are checked in tests/test_edge_kinematics_host.py).

Where the fast kernels depend on the packets and the shells every other test leaves alone: distance_boundary's branches on `mu > 0` and
`check >= 0` with mu = +-0, +-1, 2^-1000 and rays grazing r_inner within an ulp; boundary distances of 0, below 0 and of a few ulps in
shells 1e-9 and one ulp wide, where the lane sweep's bound s_xb is 0 or negative and every line goes to the exact
evaluation; the per-lane `fast` predicate with slow lanes (energy 1e-150) beside fast ones in the production instantiations, and a shell
without electrons (chi_e = 0, rcp_chi = inf, d_cont = inf, s_kp = 0); the start-up search at, above and below the ends of the line list
and exactly on a line; beta = 0.5 in the aberration, distance_line_full_relativity and the v-packets' mu_min.

(1) every row of the three kernel tables on the "edges" family, at the bars of tests/test_kernel_table_gpu.py;
(2) the problems at extreme scales through the explicit option sets of tests/test_coincident_lines_gpu.py;
(3) one wave on both sides of the `fast` switch: the production lane sweeps against the oracle and against the all-slow call;
(4) many epochs: suspended lanes carry a boundary distance <= 0 or chi_e = 0 across launches.
"""
import time

import numpy as np
import pytest

import edge_kinematics as ek
import kernel_table_recipes as ktr
import test_coincident_lines_gpu as clg

pytestmark = pytest.mark.gpu

FAMILY = "edges"
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
def test_row_on_the_edges_family(oracle, table, row):
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


# ---- (2) the extreme scales -------------------------------------------------------------------------------------------------------

SCALED_CALLS = [(kind, full, nv, o) for kind in ek.SCALES for full in (False, True) for nv in (0, ktr.N_VPACKETS) for o in clg._option_sets(full, nv)]


@pytest.mark.parametrize("kind,full,n_vpackets,options", SCALED_CALLS,
                         ids=[f"{kind.replace(' ', '_')}-full{int(f)}-nv{n}-{clg._set_id(o)}" for kind, f, n, o in SCALED_CALLS])
def test_scaled_problems(oracle, kind, full, n_vpackets, options):
    prob, ref = ek.scaled_case(oracle, kind, full, n_vpackets)
    assert ref.return_code == 0
    res, row, log, _ = clg._run(prob, ref, options)
    print(kind, full, n_vpackets, options, "->", row)
    clg._same_as_oracle(res, log, ref)
    if kind.startswith("energy"):  # (a uniform factor: the estimators are as far from 0 and inf as the energies, the comparison is not vacuous)
        assert np.isfinite(res.j_estimator).all() and np.all(res.j_estimator != 0)


# ---- (3) one wave, both sides of the switch ---------------------------------------------------------------------------------------

_all_slow = {}


def _slow_call(prob, ref, options):
    k = clg._set_id(options)
    if k not in _all_slow:
        _all_slow[k] = clg._run(prob, ref, dict(options, debug_flags=4))
    return _all_slow[k]


@pytest.mark.parametrize("options", clg.LANE_SWEEP_SETS, ids=[clg._set_id(o) for o in clg.LANE_SWEEP_SETS])
def test_one_wave_on_both_sides_of_the_switch(oracle, options):
    prob, ref = ktr.case(oracle, False, 0, FAMILY)
    e, pk = prob.edges, prob.packet_collection
    # slow lanes beside fast ones: in every wave behind the first, packets of energy 1e-150 between packets of energy 1 / n
    slow = pk.initial_energies < 1e-140
    assert np.array_equal(slow, e.kind == ek.ENERGY_TINY)
    per_wave = np.add.reduceat(slow.astype(np.int64), np.arange(64, ktr.N_PACKETS, 64))
    assert np.all(per_wave >= 1) and np.all(per_wave <= 6)
    res, row, _, _ = clg._run(prob, ref, options)
    print(options, "->", row)
    k = dict(zip(ktr.FIELDS["wave"], row[1]))
    assert row[0] == "wave" and k["LS"] == 1 and k["XWALK"] == 0 and k["VPK"] == 0, "a production lane-sweep row"
    assert k["WPE"] == options["ls_waves_per_simd"]
    clg._same_as_oracle(res, None, ref)
    # ... and the same call with every lane slow (debug flag 4: a cross-check instantiation)
    slow_res, slow_row, _, _ = _slow_call(prob, ref, options)
    assert dict(zip(ktr.FIELDS["wave"], slow_row[1]))["XWALK"] == 1
    ktr.same_per_packet(res, slow_res, trackers=True)  # bit for bit
    for name in ("line_visits", "events", "macro_transitions", "rng_draws"):
        assert res.counters[name] == slow_res.counters[name], name
    ktr.same_estimators_and_counters(res, slow_res)  # (the estimators are sums of atomics: their order differs from call to call)
    assert np.array_equal(res.j_blue_estimator == 0.0, slow_res.j_blue_estimator == 0.0)


# ---- (4) many epochs --------------------------------------------------------------------------------------------------------------

EPOCH_CALLS = [(False, 0, dict(variant=3, ls_waves_per_simd=w, sweep_table=s)) for w, s in ((4, 0), (3, 0), (4, 1), (4, 2))]


@pytest.mark.parametrize("full,n_vpackets,options", EPOCH_CALLS, ids=[f"full{int(f)}-nv{n}-{clg._set_id(o)}" for f, n, o in EPOCH_CALLS])
def test_many_epochs(oracle, full, n_vpackets, options):
    prob, ref = ktr.case(oracle, full, n_vpackets, FAMILY)
    capacity = int(ref.counters["events"]) // 5
    res, row, log, launches = clg._run(prob, ref, dict(options, log_capacity=capacity, log_chunk_records=257))
    print(full, n_vpackets, options, "log capacity", capacity, "launches", launches, row)
    assert row[0] == "wave" and launches >= 3
    clg._same_as_oracle(res, log, ref)


def test_zz_time_of_this_file():
    """Printed for the record (run with -s): the file's total and its slowest test."""
    slowest = max(TIMES, key=TIMES.get)
    print("tests/test_edge_kinematics_gpu.py: %d tests, %.1f s since import; slowest %s %.2f s" % (len(TIMES), time.perf_counter() - T0, slowest, TIMES[slowest]))
