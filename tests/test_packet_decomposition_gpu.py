"""The last-interaction decomposition on the device (tardis_mc_packet_decomposition) against the numpy yardstick
(tests/packet_decomposition_ref.py) on the arrays get_results returns for the same run.

Integer outputs are compared exactly.  A double cell must be within n * 2**-53 of the correctly rounded sum of its n addends, a
cell without addends exactly 0 (the bound is derived in the yardstick's docstring, not measured).  The shapes are small -- 4099
packets, 3000 lines, 5 shells, 37 bins, 7 classes -- but not a multiple of a wave or a workgroup, with every class and shell
populated, frequencies off the grid on both sides, and up to a few hundred addends in a cell."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import packet_decomposition_ref as ref  # noqa: E402
from tardis_amd import spectrum, state as st, synthetic, transport  # noqa: E402

pytestmark = pytest.mark.gpu

S, L, P, B, C = 5, 3000, 4099, 37, 7
MODES = {"scatter": dict(line_interaction_type="scatter"), "downbranch": dict(line_interaction_type="downbranch"),
         "macroatom": dict(line_interaction_type="macroatom", level_sizes="heavy")}


def base_problem(mode="downbranch", **kw):
    args = dict(seed=7, n_packets=P, n_shells=S, n_lines=L, n_bins=B, log_tau_mean=-2.0)
    args.update(MODES[mode])
    args.update(kw)
    return synthetic.make_problem(**args)


def propagate(eng, prob, stream=False, **options):
    """One call the way the wrapper makes it; returns get_results (with the trackers).  Options are set for this call only."""
    for k, v in options.items():
        eng.set_option(k, v)
    try:
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        n = prob.packet_collection.initial_nus.size
        out_nu, out_en, trk = np.full(n, -7.0), np.full(n, -7.0), st.LastInteractionTrackers(n)
        if stream:
            eng.stream_results(out_nu, out_en, trk)
        eng.propagate()
        eng.synchronize()
        return eng.get_results(out_nu, out_en, trackers=trk)
    finally:
        if "variant" in options:
            eng.set_option("variant", -1)


def yardstick(prob, res, cls, n_classes, grid=None, **window):
    return ref.decompose(res.output_nus, res.output_energies, prob.packet_collection.time_of_simulation,
                         prob.spectrum_frequency_grid if grid is None else grid, res.trackers, cls, n_classes,
                         len(prob.geometry.r_inner), **window)


def check(eng, prob, res, cls, n_classes, what, **window):
    # (n_classes None: the engine takes line_class.max() + 1)
    want, n = yardstick(prob, res, cls, int(np.max(cls)) + 1 if n_classes is None else n_classes, **window)
    got = eng.packet_decomposition(prob.packet_collection.time_of_simulation, cls, n_classes, **window)
    ref.assert_matches(got, want, n, what)
    return got, want, n


@pytest.fixture(scope="module")
def engine():
    from tardis_amd.engine import Engine
    with Engine(0) as eng:
        yield eng


@pytest.mark.parametrize("mode", list(MODES))
def test_base_shape(engine, mode):
    prob = base_problem(mode)
    res = propagate(engine, prob)
    cls = np.arange(L) % C
    assert engine.decomposition_path(C, B, S) == "privatised"
    got, want, n = check(engine, prob, res, cls, None, mode)
    assert want["n_line"] > 1000 and want["n_electron_scatter"] > 50 and want["n_no_interaction"] > 100
    assert want["n_selected"] == want["n_line"] + want["n_electron_scatter"] + want["n_no_interaction"] == int((res.output_energies >= 0).sum())
    assert (want["shell_packets"][:C].sum(axis=1) > 0).all() and (want["shell_packets"].sum(axis=0) > 0).all()
    emitted = res.output_energies >= 0
    grid = prob.spectrum_frequency_grid
    assert ((res.output_nus[emitted] < grid[0]) | (res.output_nus[emitted] > grid[-1])).sum() > 10  # frequencies off the grid
    assert max(int(n[k].max()) for k in ref.DOUBLE_KEYS) > 50  # many addends in one cell
    assert engine.last_propagate_ms() > 0.0
    # a second call: the integers again exactly, the doubles again within the bound; nothing resident changed
    again = engine.packet_decomposition(prob.packet_collection.time_of_simulation, cls, C)
    ref.assert_matches(again, want, n, mode + " again")
    res2 = engine.get_results()
    assert np.array_equal(res2.output_nus, res.output_nus) and np.array_equal(res2.trackers.shell_id, res.trackers.shell_id)


def test_direct_path(engine):
    prob = base_problem("downbranch", n_bins=300)
    res = propagate(engine, prob)
    assert engine.decomposition_path(40, 300, S) == "direct" and engine.decomposition_path(C, B, S) == "privatised"
    check(engine, prob, res, np.arange(L) % 40, 40, "direct")
    # an SDEC-like grouping from species ids, classes of very different sizes
    cls, labels = spectrum.species_classes(np.sqrt(np.arange(L)).astype(np.int64) % 31 + 1, np.arange(L) % 3)
    assert engine.decomposition_path(len(labels), 300, S) == "direct"
    check(engine, prob, res, cls, len(labels), "direct species")


def test_degenerate_shape(engine):
    """One shell, one bin: every selected packet on the grid adds to the same few cells; with C = 7 some classes stay empty."""
    prob = synthetic.make_problem(seed=7, n_packets=257, n_shells=1, n_lines=64, n_bins=1, log_tau_mean=-1.0,
                                  line_interaction_type="downbranch", level_sizes="heavy")
    res = propagate(engine, prob)
    got, want, _ = check(engine, prob, res, np.zeros(64, dtype=np.int64), 1, "degenerate C=1")
    assert got["emission"].shape == (1, 1) and got["shell_packets"].shape == (2, 1) and 10 < want["n_line"] < 100
    cls = (np.arange(64) % 3) * 2  # classes 0, 2, 4 of 7
    got, want, _ = check(engine, prob, res, cls, 7, "degenerate C=7")
    assert got["emission"].shape == (7, 1) and not got["shell_packets"][[1, 3, 5, 6]].any() and not got["emission"][[1, 3, 5, 6]].any()
    # n_classes defaults to line_class.max() + 1
    assert engine.packet_decomposition(prob.packet_collection.time_of_simulation, cls)["emission"].shape == (5, 1)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_every_kernel_variant(engine, variant):
    """The lane and group kernels write the last-interaction arrays themselves, the wave kernels through tracker_unpack_kernel."""
    prob = base_problem("downbranch")
    res = propagate(engine, prob, variant=variant)
    assert engine.last_variant() == variant
    check(engine, prob, res, np.arange(L) % C, C, f"variant {variant}")


def test_several_launches_with_streamed_results():
    """A call that runs as several launches, with result streaming armed: part of the tracker was unpacked at a launch boundary,
    the late packets and the rest afterwards -- the arrays on the device must be complete all the same."""
    from tardis_amd.engine import Engine
    prob = base_problem("downbranch")
    with Engine(0) as eng:
        # (the smallest log the wave kernel runs with is one chunk of 256 records per wave: 65 waves here, against 4e4 events)
        res = propagate(eng, prob, stream=True, log_capacity=4096, stream_min_packets=64)
        launches, (streamed, resent) = eng.last_kernel_times()["launches"], eng.streamed_packets()
        print("launches", launches, "streamed", streamed, "resent", resent, "variant", eng.last_variant())
        assert launches > 1 and streamed > 0
        assert not np.any(res.output_nus == -7.0)
        check(eng, prob, res, np.arange(L) % C, C, "several launches")


@pytest.mark.parametrize("kw", [dict(n_vpackets=2), dict(enable_full_relativity=True)], ids=["vpackets", "full-relativity"])
def test_vpackets_and_full_relativity(engine, kw):
    prob = base_problem("macroatom", **kw)
    res = propagate(engine, prob)
    check(engine, prob, res, np.arange(L) % C, C, str(kw))


def test_window_and_edges(engine):
    """The grid's end points are two packets' own frequencies: the first bin is closed on the left, the last one on both sides; the
    packet filter is strict on both sides."""
    prob = base_problem("downbranch")
    res = propagate(engine, prob)
    nus = np.sort(res.output_nus[res.output_energies >= 0])
    a, b = float(nus[len(nus) // 5]), float(nus[4 * len(nus) // 5])
    assert a < b and (nus == a).sum() == 1 and (nus == b).sum() == 1
    prob.spectrum_frequency_grid = np.linspace(a, b, B + 1)
    assert prob.spectrum_frequency_grid[0] == a and prob.spectrum_frequency_grid[-1] == b
    res = propagate(engine, prob)  # (per-packet results do not depend on the grid)
    cls = np.arange(L) % C
    got, want, n = check(engine, prob, res, cls, C, "edges")
    on_grid = int(((nus >= a) & (nus <= b)).sum())
    binned = lambda d: d["emission"].sum(axis=0) + d["no_interaction"] + d["electron_scatter"]  # noqa: E731
    counts = n["emission"].sum(axis=0) + n["no_interaction"] + n["electron_scatter"]
    assert counts.sum() == on_grid and counts[0] >= 1 and counts[-1] >= 1  # both end-point packets have a bin
    assert np.array_equal(binned(got) > 0, counts > 0)
    assert got["n_selected"] == len(nus) > on_grid  # off the grid: no bin, still counted
    got, want, n = check(engine, prob, res, cls, C, "window", nu_start=a, nu_end=b)
    assert got["n_selected"] == on_grid - 2  # the strict filter drops the two end-point packets
    counts_w = n["emission"].sum(axis=0) + n["no_interaction"] + n["electron_scatter"]
    assert counts_w[0] == counts[0] - 1 and counts_w[-1] == counts[-1] - 1


def test_packet_spectrum_is_unchanged(engine):
    """tardis_mc_packet_spectrum shares its bin search with the decomposition now: same values as before, and the three kinds of the
    decomposition add up to its emitted histogram."""
    import math
    prob = base_problem("macroatom")
    res = propagate(engine, prob)
    t, grid = prob.packet_collection.time_of_simulation, prob.spectrum_frequency_grid
    sp = engine.packet_spectrum(t)
    host = spectrum.emitted_luminosity_histogram(res.output_nus, res.output_energies, t, grid)
    np.testing.assert_allclose(sp["montecarlo_emitted_luminosity"], host, rtol=1e-9, atol=0)  # (tests/test_hip_parity.py's tolerance)
    host_r = spectrum.reabsorbed_luminosity_histogram(res.output_nus, res.output_energies, t, grid)
    np.testing.assert_allclose(sp["montecarlo_reabsorbed_luminosity"], host_r, rtol=1e-9, atol=0)
    # the exact per-bin sums of the emitted packets, and their addend counts
    emitted = res.output_energies >= 0
    inside, k = ref.bins_of(res.output_nus[emitted], grid)
    exact, n_bin = ref._cells(np.zeros(len(k), dtype=np.int64), k, (res.output_energies[emitted] / t)[inside], (B,))
    assert ref.within_bound(sp["montecarlo_emitted_luminosity"], exact, n_bin)
    assert math.isclose(sp["emitted_luminosity"], math.fsum(res.output_energies[emitted] / t), rel_tol=1e-12)
    got = engine.packet_decomposition(t, np.arange(L) % C, C)
    total = got["emission"].sum(axis=0) + got["no_interaction"] + got["electron_scatter"]
    # (each of the C + 2 partial sums is within its own n u; adding them up rounds C + 1 times more)
    assert ref.within_bound(total, exact, n_bin + C + 1)
    assert np.array_equal(total == 0, sp["montecarlo_emitted_luminosity"] == 0)


def test_errors():
    from tardis_amd.engine import Engine
    prob = base_problem("downbranch")
    t = prob.packet_collection.time_of_simulation
    cls = np.arange(L) % C
    state, invalid = r"failed \(-7\)", r"failed \(-1\)"
    with Engine(0) as eng:
        with pytest.raises(RuntimeError, match=state):  # nothing propagated
            eng.packet_decomposition(t, np.zeros(0, dtype=np.int64), 1)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        with pytest.raises(RuntimeError, match=state):
            eng.packet_decomposition(t, cls, C)
        res = propagate(eng, prob, track_last_interaction=0)
        with pytest.raises(RuntimeError, match=state):  # the last call ran without the tracker
            eng.packet_decomposition(t, cls, C)
        res = propagate(eng, prob, track_last_interaction=1)
        want, n = yardstick(prob, res, cls, C)
        ref.assert_matches(eng.packet_decomposition(t, cls, C), want, n, "after the untracked call")
        bad = cls.copy()
        bad[L // 2] = C
        with pytest.raises(RuntimeError, match=invalid):  # a class equal to C
            eng.packet_decomposition(t, bad, C)
        bad[L // 2] = -1
        with pytest.raises(RuntimeError, match=invalid):
            eng.packet_decomposition(t, bad, C)
        with pytest.raises(RuntimeError, match=invalid):
            eng.packet_decomposition(t, np.zeros(L, dtype=np.int64), 0)
        with pytest.raises(RuntimeError, match=invalid):
            eng.packet_decomposition(0.0, cls, C)
        ref.assert_matches(eng.packet_decomposition(t, cls, C), want, n, "after the refused calls")
        eng.set_packets(prob.packet_collection)
        with pytest.raises(RuntimeError, match=state):  # the resident packets were replaced
            eng.packet_decomposition(t, cls, C)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        ref.assert_matches(eng.packet_decomposition(t, cls, C), want, n, "after a new propagate")


def test_resident_state_reduces_on_the_device(monkeypatch):
    from tardis_amd.engine import Engine
    cls = np.arange(L) % C
    prob = base_problem("macroatom")
    with Engine(0) as eng:
        host_solver = transport.MCTransportSolverHIP(prob.spectrum_frequency_grid, prob.montecarlo_configuration, "macroatom", engine=eng)
        ts = host_solver.initialize_transport_state(prob.packet_collection, prob.geometry, prob.opacity_state, prob.time_explosion)
        host_solver.run(ts)
        want, n = ref.decompose(ts.output_nu, ts.output_energy, ts.time_of_simulation, prob.spectrum_frequency_grid,
                                ts.tracker_last_interaction, cls, C, S)
        ref.assert_matches(ts.packet_decomposition(prob.spectrum_frequency_grid, cls, C), want, n, "non-resident (host)")
        assert want["n_line"] > 1000

        prob2 = base_problem("macroatom")
        solver = transport.MCTransportSolverHIP(prob2.spectrum_frequency_grid, prob2.montecarlo_configuration, "macroatom", engine=eng,
                                                resident=True)
        ts2 = solver.initialize_transport_state(prob2.packet_collection, prob2.geometry, prob2.opacity_state, prob2.time_explosion)
        solver.run(ts2)
        tracker_downloads = []
        real = Engine.get_results

        def spy(self, *a, **kw):
            if kw.get("track_last_interaction", True):
                tracker_downloads.append(kw)
            return real(self, *a, **kw)
        monkeypatch.setattr(Engine, "get_results", spy)
        generations = (eng.results_generation, eng.packets_generation, eng.estimators_generation)
        got = ts2.packet_decomposition(prob2.spectrum_frequency_grid, cls, C)
        assert not tracker_downloads and ts2._tracker_last_interaction is None
        assert generations == (eng.results_generation, eng.packets_generation, eng.estimators_generation)
        ref.assert_matches(got, want, n, "resident (device)")
        # the trackers are still there to be read, and are the non-resident run's
        assert np.array_equal(ts2.tracker_last_interaction.interaction_line_emit_id, ts.tracker_last_interaction.interaction_line_emit_id)
        assert tracker_downloads
