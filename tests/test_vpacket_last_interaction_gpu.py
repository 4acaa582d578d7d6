"""The v-packet log with the spawning r-packet's last interaction (option vpacket_last_interaction), its consolidation on the device
(tardis_mc_get_vpacket_log) and the decomposition of the virtual spectrum (tardis_mc_vpacket_decomposition).

The expected log comes from the full r-packet event log of the same call (tests/vpacket_last_interaction_ref.py), which
tests/test_full_tracking_gpu.py pins to the oracle; the decomposition is held against tests/packet_decomposition_ref.py on the downloaded
v-packet columns: integers exactly, a double cell of n addends within n * 2**-53 relatively (derived there, not measured).

Shapes: those of the real-packet decomposition test -- 5 shells, 3000 lines, 4099 packets (no multiple of a wave), 37 bins -- with three
v-packets per volley and a spawn window narrower than the packet frequencies: about 3e4 entries (8e4 without the window)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import packet_decomposition_ref as dref  # noqa: E402
import vpacket_last_interaction_ref as vref  # noqa: E402
from oracle import oracle  # noqa: E402
from tardis_amd import state as st, synthetic  # noqa: E402
from tardis_amd.engine import Engine, VPacketLogOverflow  # noqa: E402

pytestmark = pytest.mark.gpu

S, L, P, B, C, NV = 5, 3000, 4099, 37, 7, 3
WINDOW = (4.0e14, 1.1e15)  # VPACKET_SPAWN_START / END_FREQUENCY: inside the packets' frequencies on both sides
CASES = {"downbranch": dict(line_interaction_type="downbranch"),
         "macroatom-heavy": dict(line_interaction_type="macroatom", level_sizes="heavy"),
         "full-relativity": dict(line_interaction_type="downbranch", enable_full_relativity=True)}
COLUMNS = ("source_packet", "nus", "energies", "initial_mus", "initial_rs", "last_interaction_in_nu", "last_interaction_in_r",
           "last_interaction_type", "last_interaction_in_id", "last_interaction_out_id", "last_interaction_shell_id")
STATE, INVALID = r"failed \(-7\)", r"failed \(-1\)"


def problem(case="downbranch", **kw):
    args = dict(seed=7, n_packets=P, n_shells=S, n_lines=L, n_bins=B, log_tau_mean=-2.0, n_vpackets=NV, vpacket_spawn_range=WINDOW)
    args.update(CASES[case])
    args.update(kw)
    prob = synthetic.make_problem(**args)
    prob.montecarlo_configuration.ENABLE_VPACKET_TRACKING = True
    return prob


RESET = {"variant": -1, "track_last_interaction": 1, "vpacket_last_interaction": 0, "track_full": 0, "event_log_capacity": 0,
         "vpacket_log_capacity": 0, "log_capacity": 0, "vpk_wide_registers": 1}


def propagate(eng, prob, **options):
    """One call with `options` set for it; returns get_results (with the sorted v-packet arrays of the host path)."""
    opts = dict(vpacket_last_interaction=1)
    opts.update(options)
    for k, v in opts.items():
        eng.set_option(k, v)
    try:
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        return eng.get_results(trackers=st.LastInteractionTrackers(P))
    finally:
        for k in opts:
            if k != "vpacket_last_interaction":  # (get_vpacket_log reads the option: it stays until the next call sets it)
                eng.set_option(k, RESET[k])


def same_columns(a, b):
    assert np.array_equal(a.offsets, b.offsets)
    for f in COLUMNS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and (vref.same_bits(x, y) if x.dtype == np.float64 else np.array_equal(x, y)), f


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def tracked(eng):
    """case -> (problem, get_results, the consolidated log, the event log) of ONE call with track_full, v-packet tracking and the
    option on; computed once per case and shared."""
    cache = {}

    def get(case):
        if case not in cache:
            prob = problem(case)
            res = propagate(eng, prob, track_full=1, event_log_capacity=64 * P)
            cache[case] = (prob, res, eng.get_vpacket_log(), eng.get_event_log())
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_yardstick(eng, tracked, case):
    prob, res, vlog, events = tracked(case)
    want = vref.expected_from_event_log(events, WINDOW[0], WINDOW[1], NV)
    # the conditions of the test: the window skips volleys of both kinds, every kind of entry is there -- and the oracle agrees on
    # the number of entries
    orc = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                     prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE)
    n = len(want["source_packet"])
    print(case, "entries", n, {k: want[k] for k in ("launch_volleys", "launch_skipped", "interaction_volleys", "interaction_skipped")})
    assert orc.return_code == 0 and orc.vpacket_log_count == n == res.vpacket_log_count
    assert want["interaction_skipped"] >= 0.05 * (want["interaction_skipped"] + want["interaction_volleys"])
    assert want["launch_skipped"] >= 0.05 * P
    for t in (-1, 2, 4):
        assert (want["last_interaction_type"] == t).sum() > 100, t
    # the log
    assert len(vlog.nus) == n
    assert np.array_equal(vlog.offsets, want["offsets"]) and np.array_equal(vlog.source_packet, want["source_packet"])
    for f in vref.INT_FIELDS:
        assert getattr(vlog, f).dtype == np.int64 and np.array_equal(getattr(vlog, f), want[f]), f
    assert vref.same_bits(vlog.last_interaction_in_nu, want["last_interaction_in_nu"])
    assert vref.same_bits(vlog.last_interaction_in_r, want["last_interaction_in_r"])
    some = vlog.last_interaction_type != -1
    assert np.array_equal(vlog.last_interaction_in_r[some].view(np.int64), vlog.initial_rs[some].view(np.int64))
    # the four old columns: those of get_results from the same call (and the oracle's)
    for f in ("nus", "energies", "initial_mus", "initial_rs"):
        assert np.array_equal(getattr(vlog, f), getattr(res, "vpacket_" + f)[:n]), f
        assert np.array_equal(getattr(vlog, f), getattr(orc, "vpacket_" + f)), f


@pytest.mark.parametrize("variant,wide", [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (2, 2), (3, 2), (4, 2)])
def test_across_kernels(eng, tracked, variant, wide):
    """Per-packet results do not depend on the kernel: the same run without track_full on every variant."""
    prob, _, ref_log, _ = tracked("downbranch")
    propagate(eng, prob, variant=variant, vpk_wide_registers=wide)
    assert eng.last_variant() == variant
    same_columns(eng.get_vpacket_log(), ref_log)


def test_across_launches(tracked):
    prob, _, ref_log, _ = tracked("downbranch")
    with Engine(0) as e:
        # (the smallest log the wave kernel runs with is one chunk of 256 records per wave, tests/test_packet_decomposition_gpu.py)
        propagate(e, prob, variant=2, log_capacity=4096)
        launches = e.last_kernel_times()["launches"]
        print("launches", launches, "variant", e.last_variant())
        assert launches >= 3 and e.last_variant() >= 2
        same_columns(e.get_vpacket_log(), ref_log)


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_final_trackers(tracked, case):
    """Every packet whose last tracker row spawned a volley: its last NV entries are its final last-interaction tracker."""
    _, res, vlog, _ = tracked(case)
    t = res.trackers
    spawned = (t.interaction_type != -1) & ~((res.output_nus < WINDOW[0]) | (res.output_nus > WINDOW[1]))  # (after_nu of that row = output_nu)
    assert spawned.sum() > 500
    last = vlog.offsets[1:][spawned] - 1
    assert np.all(np.diff(vlog.offsets)[spawned] >= NV)
    for back in range(NV):
        k = last - back
        assert np.array_equal(vlog.source_packet[k], np.flatnonzero(spawned))
        assert np.array_equal(vlog.last_interaction_type[k], t.interaction_type[spawned])
        assert np.array_equal(vlog.last_interaction_in_id[k], t.interaction_line_absorb_id[spawned])
        assert np.array_equal(vlog.last_interaction_out_id[k], t.interaction_line_emit_id[spawned])
        assert np.array_equal(vlog.last_interaction_shell_id[k], t.shell_id[spawned])
        assert vref.same_bits(vlog.last_interaction_in_nu[k], t.before_nu[spawned])
        assert vref.same_bits(vlog.last_interaction_in_r[k], t.radius[spawned])


class _Columns:  # the v-packet columns under the names packet_decomposition_ref.decompose reads
    def __init__(self, vlog):
        self.interaction_type, self.before_nu, self.shell_id = vlog.last_interaction_type, vlog.last_interaction_in_nu, vlog.last_interaction_shell_id
        self.interaction_line_emit_id, self.interaction_line_absorb_id = vlog.last_interaction_out_id, vlog.last_interaction_in_id


def check_decomposition(e, prob, vlog, cls, n_classes, what, **window):
    t = prob.packet_collection.time_of_simulation
    want, n = dref.decompose(vlog.nus, vlog.energies, t, prob.spectrum_frequency_grid, _Columns(vlog), cls, n_classes, S, **window)
    got = e.vpacket_decomposition(t, cls, n_classes, **window)
    dref.assert_matches(got, want, n, what)
    return got, want, n


@pytest.mark.parametrize("case", ["downbranch", "macroatom-heavy"])
def test_decomposition_privatised_and_window(tracked, case):
    prob, _, vlog, _ = tracked(case)
    cls = np.arange(L) % C
    with Engine(0) as e:
        res = propagate(e, prob)
        assert e.decomposition_path(C, B, S) == "privatised"
        # (no get_vpacket_log before it: the call consolidates the log itself)
        got, want, n = check_decomposition(e, prob, vlog, cls, C, case)
        assert e.last_propagate_ms() > 0.0
        assert want["n_selected"] == len(vlog.nus) and want["n_line"] > 1000 and want["n_electron_scatter"] > 100 and want["n_no_interaction"] > 100
        assert (vlog.energies == 0.0).sum() > 0 and not (vlog.energies < 0).any()
        # the invariant: the same non-negative addends as the v-packet histogram, in another order
        t = prob.packet_collection.time_of_simulation
        total = math.fsum(got["emission"].ravel()) + math.fsum(got["electron_scatter"]) + math.fsum(got["no_interaction"])
        hist = math.fsum(res.v_packets_energy_hist) / t
        grid = prob.spectrum_frequency_grid
        on_grid = int(((vlog.nus >= grid[0]) & (vlog.nus <= grid[-1])).sum())
        print(case, "sum of cells", total, "v-hist / t", hist, "v-packets on the grid", on_grid)
        assert 0 < on_grid and abs(total - hist) <= on_grid * 2.0 ** -52 * hist
        # a strict window between two v-packets' own frequencies
        nus = np.sort(vlog.nus)
        a, b = float(nus[len(nus) // 4]), float(nus[3 * len(nus) // 4])
        gw, ww, _ = check_decomposition(e, prob, vlog, cls, C, case + " window", nu_start=a, nu_end=b)
        assert 0 < gw["n_selected"] == int(((vlog.nus > a) & (vlog.nus < b)).sum()) < want["n_selected"]
        same_columns(e.get_vpacket_log(), vlog)  # nothing resident changed


def test_decomposition_direct_path(tracked):
    prob = problem("downbranch", n_bins=300)
    with Engine(0) as e:
        propagate(e, prob)
        vlog = e.get_vpacket_log()
        assert e.decomposition_path(40, 300, S) == "direct"  # (2 * 40 + 2) * 300 * 8 bytes: past 64 KiB
        check_decomposition(e, prob, vlog, np.arange(L) % 40, 40, "direct")
        same_columns(vlog, tracked("downbranch")[2])  # (per-packet results do not depend on the grid)


def test_overflow(tracked):
    prob, _, ref_log, _ = tracked("downbranch")
    count = len(ref_log.nus)
    cls = np.arange(L) % C
    t = prob.packet_collection.time_of_simulation
    with Engine(0) as e:
        propagate(e, prob, vpacket_log_capacity=count // 2)
        from tardis_amd import _abi
        import ctypes
        log = _abi.TardisMcVpacketLog()
        nus = np.full(count, -7.0)
        log.capacity, log.nus = count, _abi._dp(nus)
        assert e._L.tardis_mc_get_vpacket_log(e._h, ctypes.byref(log)) == 0
        assert log.count == count and np.all(nus == -7.0)  # the count, and no column
        with pytest.raises(VPacketLogOverflow) as err:
            e.get_vpacket_log()
        assert err.value.entries_needed == count
        with pytest.raises(RuntimeError, match=STATE):
            e.vpacket_decomposition(t, cls, C)
        propagate(e, prob, vpacket_log_capacity=count)
        same_columns(e.get_vpacket_log(), ref_log)
        check_decomposition(e, prob, ref_log, cls, C, "after the overflow")


def test_errors(tracked):
    prob, res_on, ref_log, _ = tracked("downbranch")
    cls = np.arange(L) % C
    t = prob.packet_collection.time_of_simulation
    with Engine(0) as e:
        with pytest.raises(RuntimeError, match=STATE):  # nothing propagated
            e.get_vpacket_log()
        # the option without a tracker: refused before anything is launched
        with pytest.raises(RuntimeError, match=INVALID):
            propagate(e, prob, track_last_interaction=0)
        with pytest.raises(RuntimeError, match=STATE):
            e.get_vpacket_log()
        # the option off: the six columns are refused, the others work; get_results is what it is with the option on
        res_off = propagate(e, prob, vpacket_last_interaction=0)
        from tardis_amd import _abi
        import ctypes
        n = len(ref_log.nus)
        log = _abi.TardisMcVpacketLog()
        col = np.zeros(n, dtype=np.int64)
        log.capacity, log.last_interaction_type = n, _abi._ip(col)
        assert e._L.tardis_mc_get_vpacket_log(e._h, ctypes.byref(log)) == _abi.ERR_STATE
        plain = e.get_vpacket_log()
        assert np.array_equal(plain.offsets, ref_log.offsets) and np.array_equal(plain.source_packet, ref_log.source_packet)
        for f in ("nus", "energies", "initial_mus", "initial_rs"):
            assert np.array_equal(getattr(plain, f), getattr(ref_log, f)), f
            assert np.array_equal(getattr(res_off, "vpacket_" + f)[:n], getattr(res_on, "vpacket_" + f)[:n]), f  # (the arrays are sized for the capacity)
        assert np.all(plain.last_interaction_type == -99) and np.all(plain.last_interaction_in_nu == -99.0)  # the reference's placeholders
        assert res_off.vpacket_log_count == res_on.vpacket_log_count == n
        assert np.array_equal(res_off.output_nus, res_on.output_nus) and np.array_equal(res_off.output_energies, res_on.output_energies)
        # (the histogram is summed with atomics, in an order that differs from call to call: a bin of at most n non-negative addends is within
        # (n - 1) 2^-53 of its exact sum either way)
        np.testing.assert_allclose(res_off.v_packets_energy_hist, res_on.v_packets_energy_hist, rtol=n * 2.0 ** -52, atol=0.0)
        with pytest.raises(RuntimeError, match=STATE):  # no last-interaction columns
            e.vpacket_decomposition(t, cls, C)
        # the argument checks of packet_decomposition
        propagate(e, prob)
        bad = cls.copy()
        bad[L // 2] = C
        with pytest.raises(RuntimeError, match=INVALID):
            e.vpacket_decomposition(t, bad, C)
        with pytest.raises(RuntimeError, match=INVALID):
            e.vpacket_decomposition(0.0, cls, C)
        check_decomposition(e, prob, ref_log, cls, C, "after the refused calls")
        # the resident packets were replaced
        e.set_packets(prob.packet_collection)
        with pytest.raises(RuntimeError, match=STATE):
            e.get_vpacket_log()
        with pytest.raises(RuntimeError, match=STATE):
            e.vpacket_decomposition(t, cls, C)


def test_wrapper_fills_the_collection(tracked):
    from tardis_amd import transport
    prob, _, ref_log, _ = tracked("downbranch")
    with Engine(0) as e:
        args = (prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                prob.spectrum_frequency_grid)
        _, vt, _, _ = transport.montecarlo_transport_with_vpackets(*args, st.LastInteractionTrackers(P), NV, engine=e,
                                                                   track_vpacket_last_interaction=True)
        same_columns(vt, ref_log)
        assert e.options["vpacket_last_interaction"] == 0
        _, vt0, _, _ = transport.montecarlo_transport_with_vpackets(*args, st.LastInteractionTrackers(P), NV, engine=e)
        assert np.array_equal(vt0.nus, ref_log.nus) and np.all(vt0.last_interaction_type == -99) and np.all(vt0.last_interaction_in_r == -99.0)
        ts = transport.MonteCarloTransportState(prob.packet_collection, prob.geometry, prob.opacity_state, prob.time_explosion)
        ts.vpacket_tracker = vt
        cls = np.arange(L) % C
        want, n = dref.decompose(vt.nus, vt.energies, ts.time_of_simulation, prob.spectrum_frequency_grid, _Columns(vt), cls, C, S)
        dref.assert_matches(ts.vpacket_decomposition(prob.spectrum_frequency_grid, cls, C), want, n, "state")
