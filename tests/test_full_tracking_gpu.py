"""Full r-packet tracking on the device (option track_full, Engine.get_event_log, TrackerFull at the boundary)."""
import ctypes as C

import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import oracle
from tardis_amd import state as st, synthetic, transport
from tardis_amd.engine import Engine, EventLogOverflow

import _golden

pytestmark = pytest.mark.gpu

MODES = ["scatter", "downbranch", "macroatom"]
SHAPES = [(m, full, nv) for m in MODES for full in (False, True) for nv in (0, 3)]


def _problem(mode, full, nv, n=600, seed=5):
    return synthetic.make_problem(seed=seed, n_packets=n, n_shells=12, n_lines=3000, line_interaction_type=mode, n_vpackets=nv,
                                  enable_full_relativity=full, n_bins=2000)


def _run(eng, prob, track_full=True, **options):
    """Engine.run with `options` set for the call; a log that outgrows the automatic pool is run again with the capacity it asked for
    (doubled if that is still short: the pool also holds each wave's partly filled last chunk of every launch)."""
    if track_full and "event_log_capacity" not in options:
        cap = 0
        for _ in range(4):
            try:
                return _run(eng, prob, track_full, event_log_capacity=cap, **options)
            except EventLogOverflow as e:
                cap = max(e.rows_needed, 2 * cap)
        raise AssertionError("event log overflow persisted")
    for k, v in options.items():
        eng.set_option(k, v)
    try:
        res = eng.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state,
                      prob.montecarlo_configuration, prob.spectrum_frequency_grid, track_full=track_full)
    finally:
        for k in options:
            eng.set_option(k, {"variant": -1, "event_log_capacity": 0}.get(k, 0))
    return res


def _rows(log):
    return np.stack([getattr(log, f).view(np.int64) for f in st.FullTrackers.F64_FIELDS + st.FullTrackers.I64_FIELDS])


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def _oracle_trace(prob):
    """The oracle's serial trace log: {shell, first line, lines visited, type} per trace_packet, packet by packet."""
    lib = oracle.lib()
    lib.oracle_set_trace_log.restype = None
    lib.oracle_set_trace_log.argtypes = [C.c_void_p, C.c_int64]
    lib.oracle_trace_log_count.restype = C.c_int64
    cap = 2000 * prob.packet_collection.number_of_packets
    buf = np.zeros((cap, 4), dtype=np.int64)
    lib.oracle_set_trace_log(buf.ctypes.data, cap)
    try:
        oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                   prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=False)
        n = int(lib.oracle_trace_log_count())
    finally:
        lib.oracle_set_trace_log(None, 0)
    assert n <= cap
    return buf[:n]


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("mode,full,nv", SHAPES)
def test_rows_follow_the_oracle_and_the_packet(eng, mode, full, nv, variant):
    prob = _problem(mode, full, nv)
    res = _run(eng, prob, variant=variant)
    assert eng.last_variant() == variant
    log = res.full_trackers
    P = prob.packet_collection.number_of_packets
    assert len(log) == P and log.n_rows == res.counters["events"]
    # (1) the oracle's serial trace sequence
    tr = _oracle_trace(prob)
    assert len(tr) == log.n_rows
    assert np.array_equal(log.shell_id, tr[:, 0])
    assert np.array_equal(log.interaction_type, tr[:, 3])
    line = log.interaction_type == 2
    assert np.array_equal(log.line_absorb_id[line], (tr[:, 1] + tr[:, 2] - 1)[line])
    assert np.all(log.line_absorb_id[~line] == -1) and np.all(log.line_emit_id[~line] == -1)
    # (4) continuity and ends
    assert np.array_equal(log.event_id, np.arange(log.n_rows) - np.repeat(log.offsets[:-1], log.counts))
    last = log.offsets[1:] - 1
    inner = np.ones(log.n_rows, bool)
    inner[last] = False
    nxt = np.flatnonzero(inner)
    assert np.array_equal(log.before_nu[nxt + 1], log.after_nu[nxt])
    assert np.array_equal(log.before_energy[nxt + 1], log.after_energy[nxt])
    assert np.all(log.status[inner] == 0) and np.all(log.status[last] != 0)
    assert np.array_equal(log.after_nu[last], res.output_nus)
    assert np.array_equal(log.after_energy[last], np.abs(res.output_energies))
    assert np.array_equal(np.where(log.status[last] == 2, -1, 1) * log.after_energy[last], res.output_energies)
    b = log.interaction_type == 1
    assert np.all(np.abs(log.after_shell_id[b] - log.shell_id[b]) == 1)
    assert np.all(log.after_shell_id[~b] == log.shell_id[~b])
    for f in ("nu", "mu", "energy"):
        assert np.array_equal(getattr(log, "before_" + f)[b], getattr(log, "after_" + f)[b])
    # (3) the projection onto the last interaction is the last-interaction tracker, bit for bit
    t = res.trackers
    inter = (log.interaction_type == 2) | (log.interaction_type == 4)
    idx = np.full(P, -1)
    pid = log.packet_id
    idx[pid[inter]] = np.flatnonzero(inter)  # (the last write per packet wins: rows are in order)
    has = idx >= 0
    assert np.array_equal(has, t.interaction_type != -1)
    k = idx[has]
    for f in ("radius", "before_nu", "before_mu", "before_energy", "after_nu", "after_mu", "after_energy"):
        assert np.array_equal(getattr(log, f)[k], getattr(t, f)[has]), f
    assert np.array_equal(log.shell_id[k], t.shell_id[has])
    assert np.array_equal(log.interaction_type[k], t.interaction_type[has])
    assert np.array_equal(log.line_absorb_id[k], t.interaction_line_absorb_id[has])
    assert np.array_equal(log.line_emit_id[k], t.interaction_line_emit_id[has])
    assert np.array_equal(log.event_id[k] + 1, t.interactions_count[has])


def test_row_count_is_the_oracle_event_count_per_packet(eng):
    prob = _problem("macroatom", False, 0, n=300)
    log = _run(eng, prob).full_trackers
    pc = prob.packet_collection
    for i in (0, 7, 123, 299):
        one = st.PacketCollection(pc.initial_radii[i:i + 1], pc.initial_nus[i:i + 1], pc.initial_mus[i:i + 1],
                                  pc.initial_energies[i:i + 1], pc.packet_seeds[i:i + 1], 1.0)
        ref = oracle.run(one, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                         prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1)
        assert log.counts[i] == ref.counters["events"], i


@pytest.mark.parametrize("name", _golden.CASES)
def test_projection_matches_the_reference_tracker(eng, name):
    prob, g = _golden.load_case(name)
    log = _run(eng, prob).full_trackers
    P = prob.packet_collection.number_of_packets
    inter = (log.interaction_type == 2) | (log.interaction_type == 4)
    idx = np.full(P, -1)
    idx[log.packet_id[inter]] = np.flatnonzero(inter)
    has = idx >= 0
    assert np.array_equal(has, g["trk_interaction_type"] != -1)
    k = idx[has]
    assert np.array_equal(log.shell_id[k], g["trk_shell_id"][has])
    assert np.array_equal(log.interaction_type[k], g["trk_interaction_type"][has])
    assert np.array_equal(log.line_absorb_id[k], g["trk_interaction_line_absorb_id"][has])
    assert np.array_equal(log.line_emit_id[k], g["trk_interaction_line_emit_id"][has])
    assert np.array_equal(log.event_id[k] + 1, g["trk_interactions_count"][has])
    for f in ("radius", "before_nu", "before_mu", "before_energy", "after_mu"):
        assert_allclose(getattr(log, f)[k], g["trk_" + f][has], rtol=1e-13, atol=0, err_msg=f)


@pytest.mark.parametrize("mode,full,nv", SHAPES)
def test_wave_kernel_rows_equal_lane_kernel_rows(eng, mode, full, nv):
    """The tracked wave-owner kernel (variant 2) and the lane kernel (variant 0) write bit-identical logs; explicit requests of
    variants 1, 3 and 4 and the automatic choice run the tracked wave kernel, too."""
    prob = _problem(mode, full, nv, n=3000)
    ref = _run(eng, prob, variant=0).full_trackers
    assert eng.last_variant() == 0
    for v in (-1, 1, 2, 3, 4):
        res = _run(eng, prob, variant=v)
        assert eng.last_variant() == 2, v
        assert np.array_equal(res.full_trackers.offsets, ref.offsets), v
        assert np.array_equal(_rows(res.full_trackers), _rows(ref)), v


@pytest.mark.parametrize("mode,full,nv", [("macroatom", False, 0), ("downbranch", True, 3), ("scatter", False, 0)])
def test_wave_kernel_rows_survive_epochs_and_drain_compaction(eng, mode, full, nv):
    prob = _problem(mode, full, nv, n=20000)
    ref = _run(eng, prob, variant=0).full_trackers
    # a line-visit log far smaller than the call: the call runs as several launches, lanes suspend and resume
    res = _run(eng, prob, variant=2, log_capacity=200000)
    assert eng.last_variant() == 2 and eng.last_kernel_times()["launches"] > 1
    assert np.array_equal(res.full_trackers.offsets, ref.offsets)
    assert np.array_equal(_rows(res.full_trackers), _rows(ref))
    # the drain's live lanes packed into fewer waves
    res = _run(eng, prob, variant=2, drain_compact=16)
    assert eng.last_variant() == 2
    assert np.array_equal(_rows(res.full_trackers), _rows(ref))


@pytest.mark.parametrize("mode,full,nv", [("macroatom", False, 0), ("downbranch", True, 3), ("scatter", False, 3)])
def test_rows_do_not_depend_on_overflow(eng, mode, full, nv):
    prob = _problem(mode, full, nv, n=2000)
    ref = _run(eng, prob).full_trackers
    # a pool far too small: rows dropped, counts exact, and a re-run with the exact capacity gives the same log
    eng.set_option("event_log_capacity", 64)
    try:
        with pytest.raises(EventLogOverflow) as e:
            eng.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state,
                    prob.montecarlo_configuration, prob.spectrum_frequency_grid, track_full=True)
    finally:
        eng.set_option("event_log_capacity", 0)
    assert e.value.rows_needed == ref.n_rows and e.value.dropped > 0
    res = _run(eng, prob, event_log_capacity=e.value.rows_needed)
    assert np.array_equal(res.full_trackers.offsets, ref.offsets)
    assert np.array_equal(_rows(res.full_trackers), _rows(ref))


@pytest.mark.parametrize("mode,full,nv", [("macroatom", False, 0), ("downbranch", True, 3)])
def test_tracking_does_not_disturb_results(eng, mode, full, nv):
    prob = _problem(mode, full, nv, n=2000)
    on = _run(eng, prob, variant=0)
    off = _run(eng, prob, track_full=False, variant=0)
    assert np.array_equal(on.output_nus, off.output_nus) and np.array_equal(on.output_energies, off.output_energies)
    for f in st.LastInteractionTrackers.F64_FIELDS + st.LastInteractionTrackers.I64_FIELDS:
        assert np.array_equal(getattr(on.trackers, f), getattr(off.trackers, f), equal_nan=True), f
    auto = _run(eng, prob, track_full=False)  # (the automatic kernel choice)
    assert_allclose(on.j_estimator, auto.j_estimator, rtol=1e-11)
    assert_allclose(on.j_blue_estimator, auto.j_blue_estimator, rtol=1e-11, atol=1e-300)


@pytest.mark.parametrize("variant", [0, -1])
def test_failed_call_leaves_no_event_log(eng, variant):
    from tardis_amd.engine import MacroAtomError
    # un-normalised transition probabilities (all zero) -> MacroAtomError after some rows of the failing packet were written
    prob = synthetic.make_problem(seed=9, n_packets=64, n_shells=3, n_lines=200, line_interaction_type="downbranch", log_tau_mean=1.0)
    prob.opacity_state.transition_probabilities[:] = 0.0
    with pytest.raises(MacroAtomError):
        _run(eng, prob, variant=variant)
    with pytest.raises(RuntimeError, match="failed"):
        eng.get_event_log()


def test_get_event_log_without_tracking_is_a_state_error(eng):
    prob = _problem("scatter", False, 0, n=64)
    _run(eng, prob, track_full=False)
    with pytest.raises(RuntimeError, match="track_full"):
        eng.get_event_log()


class _TrackerFull:  # the reference's TrackerFull shape: array-valued fields and a count
    def __init__(self):
        self.shell_id = np.zeros(4, dtype=np.int64)
        self.interaction_type = np.zeros(4, dtype=np.int64)
        self.r = np.zeros(4)
        self.before_nu, self.after_nu = np.zeros(4), np.zeros(4)
        self.interactions_count = 0


def test_boundary_fills_full_trackers_and_solver_frame(eng):
    prob = _problem("macroatom", False, 0, n=500)
    trackers = [_TrackerFull() for _ in range(500)]
    cfg = prob.montecarlo_configuration
    transport.montecarlo_transport_with_vpackets(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state,
                                                 cfg, prob.spectrum_frequency_grid, trackers, 0, False, None, engine=eng)
    log = transport.montecarlo_transport_with_vpackets.last_event_log
    for i in (0, 250, 499):
        rows = log.packet(i)
        assert trackers[i].interactions_count == len(rows["event_id"])
        assert np.array_equal(trackers[i].r, rows["radius"])
        assert np.array_equal(trackers[i].shell_id, rows["shell_id"])
        assert np.array_equal(trackers[i].after_nu, rows["after_nu"])
    prob2 = _problem("macroatom", False, 0, n=500)
    solver = transport.MCTransportSolverHIP(prob2.spectrum_frequency_grid, prob2.montecarlo_configuration, line_interaction_type="macroatom",
                                            enable_rpacket_tracking=True, engine=eng)
    ts = solver.initialize_transport_state(prob2.packet_collection, prob2.geometry, prob2.opacity_state, prob2.time_explosion)
    solver.run(ts)
    df = ts.tracker_full_df
    assert df.index.names == ["packet_id", "event_id"] and len(df) == log.n_rows
    assert np.array_equal(df["after_nu"].to_numpy(), log.after_nu)
    last = df.groupby(level=0).tail(1)
    assert np.array_equal(last["after_nu"].to_numpy(), ts.output_nu)
    li = ts.tracker_last_interaction_df
    inter = df[df["interaction_type"].astype(str).isin(["LINE", "ESCATTERING"])].groupby(level=0).tail(1)
    pids = inter.index.get_level_values(0).to_numpy()
    assert np.array_equal(inter["after_mu"].to_numpy(), li["after_mu"].to_numpy()[pids])
    with pytest.raises(NotImplementedError):
        transport.MCTransportSolverHIP(prob2.spectrum_frequency_grid, prob2.montecarlo_configuration, resident=True,
                                       enable_rpacket_tracking=True, engine=eng).run(ts)
