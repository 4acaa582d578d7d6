"""The context's resources and validity flags on the device: tardis_mc_destroy gives back what the context allocated, and a table of
which entry point invalidates which resident product (the transport side's counterpart of LADDER in tests/test_nlte_collision_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tardis_amd import _abi, synthetic
from tardis_amd.engine import Engine

pytestmark = pytest.mark.gpu

OK, STATE = 0, _abi.ERR_STATE
EVENT_ROW_BYTES = 96            # sizeof(mc::EventRow), csrc/event_log.hpp
POOL_ROWS = 4 << 20             # option event_log_capacity of the cycles below
POOL_BYTES = POOL_ROWS * EVENT_ROW_BYTES  # 384 MiB: the least setup_event_log allocates for the row pool of one cycle


def _problem(n_vpackets, n_packets=600):
    return synthetic.make_problem(seed=5, n_packets=n_packets, n_shells=12, n_lines=3000, line_interaction_type="macroatom",
                                  n_vpackets=n_vpackets, n_bins=2000)


def _free_device_memory(eng):
    """hipMemGetInfo of the HIP runtime the engine's library is linked against: looked up through the library's own handle, which
    resolves the symbols of its dependencies too, so that no second runtime is loaded."""
    hip = eng._L
    free, total = C.c_size_t(0), C.c_size_t(0)
    eng.synchronize()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def _tracked_cycle(prob):
    with Engine(0) as eng:
        eng.set_option("event_log_capacity", POOL_ROWS)
        res = eng.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                      prob.spectrum_frequency_grid, track_full=True)
        assert res.full_trackers is not None and len(res.full_trackers.offsets) == 601


def test_destroy_returns_the_event_log():
    """Five create / run with track_full / destroy cycles, each with a row pool of 4 Mi rows x 96 B = 384 MiB: the free device memory
    after the first (warm-up) cycle and after the fifth.  A library that leaves the event log behind at destroy loses at least four
    pools (1536 MiB); one that frees it loses none.  The bound of ONE pool is not a tolerance of the library: other processes may
    allocate on the same card between the two readings, and that is all the margin is for."""
    prob = _problem(n_vpackets=0)
    with Engine(0) as probe:  # (keeps the runtime initialised while the cycles come and go; allocates nothing)
        _tracked_cycle(prob)
        before = _free_device_memory(probe)
        for _ in range(4):
            _tracked_cycle(prob)
        after = _free_device_memory(probe)
    lost = before - after
    print(f"free device memory: {before} B after the warm-up cycle, {after} B after four more: lost {lost} B ({lost / 2**20:.1f} MiB)")
    assert lost < POOL_BYTES, f"{lost / 2**20:.1f} MiB of device memory lost over four cycles"


# -- what each call invalidates
def _same_packets(eng, prob):
    eng.set_packets(prob.packet_collection)


def _other_packets(eng, prob):
    eng.set_packets(_problem(3, n_packets=601).packet_collection)


def _blackbody_same_count(eng, prob):
    eng.create_blackbody_packets(600, float(prob.geometry.r_inner[0]), 10000.0)


def _propagate_untracked(eng, prob):
    for name in ("track_full", "track_last_interaction", "vpacket_last_interaction"):
        eng.set_option(name, 0)
    cfg = prob.montecarlo_configuration
    cfg.ENABLE_VPACKET_TRACKING = False
    try:
        eng.set_config(cfg, prob.spectrum_frequency_grid)
    finally:
        cfg.ENABLE_VPACKET_TRACKING = True
    eng.propagate()
    eng.synchronize()


#              call                                             event log, packet decomposition, v-packet log, v-packet decomposition, source function
TABLE = [
    ("set_geometry", lambda eng, p: eng.set_geometry(p.geometry, p.time_explosion), (OK, OK, OK, OK, STATE)),
    ("set_opacity", lambda eng, p: eng.set_opacity(p.opacity_state), (OK, OK, OK, OK, STATE)),
    ("set_config", lambda eng, p: eng.set_config(p.montecarlo_configuration, p.spectrum_frequency_grid), (OK, OK, STATE, STATE, OK)),
    ("set_packets-same-count", _same_packets, (OK, STATE, STATE, STATE, OK)),
    ("set_packets-other-count", _other_packets, (STATE, STATE, STATE, STATE, OK)),
    ("create_blackbody_packets-same-count", _blackbody_same_count, (OK, STATE, STATE, STATE, OK)),
    ("reset_estimators", lambda eng, p: eng.reset_estimators(), (OK, OK, OK, OK, STATE)),
    ("propagate-untracked", _propagate_untracked, (STATE, STATE, STATE, STATE, STATE)),
]


def _code(call):
    try:
        call()
    except RuntimeError as e:
        return e.code
    return OK


@pytest.fixture(scope="module")
def tracked_problem():
    prob = _problem(n_vpackets=3)
    prob.montecarlo_configuration.ENABLE_VPACKET_TRACKING = True
    return prob


@pytest.mark.parametrize("name,call,expect", TABLE, ids=[row[0] for row in TABLE])
def test_what_each_call_invalidates(tracked_problem, name, call, expect):
    """After a propagate with every tracker on and a source_function, the five getters work; one call later each of them either still
    works or refuses with ERR_STATE -- per row, which.  (The lazily rebuilt tables -- screening prefix sums, sweep table, exp(-tau) --
    have no getter: the parity tests that propagate or integrate after a set_opacity / update_opacity are their check.)"""
    prob = tracked_problem
    t = prob.packet_collection.time_of_simulation
    cls = np.arange(3000) % 5
    with Engine(0) as eng:
        for option in ("track_full", "track_last_interaction", "vpacket_last_interaction"):
            eng.set_option(option, 1)
        eng.set_option("event_log_capacity", 1 << 18)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        eng.source_function(t, prob.geometry.volume, want_arrays=False)
        getters = (eng.get_event_log, lambda: eng.packet_decomposition(t, cls, 5), eng.get_vpacket_log,
                   lambda: eng.vpacket_decomposition(t, cls, 5), lambda: eng.interpolated_source(7))
        assert tuple(_code(g) for g in getters) == (OK, OK, OK, OK, OK)
        call(eng, prob)
        got = tuple(_code(g) for g in getters)
        print(name, got)
        assert got == expect
