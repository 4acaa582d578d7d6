"""Recipes for the tables of compiled propagation kernels (LANE_KERNELS, GROUP_KERNELS, WAVE_KERNELS of csrc/tardis_mc_hip.hip).

A propagate call computes a key from the configuration and the options and looks its kernel up.  `recipe(table, key)` is the inverse for the
one problem family of tests/test_kernel_table_gpu.py: the configuration (full relativity, v-packets, v-packet tracking) and the complete option
set with which a call lands on the row `key` of `table`.  `selected_row(recipe)` is the forward direction -- plan_propagate
(csrc/propagate_plan.hpp), launch_lane, run_group_kernel and choose_wave_kernel (csrc/tardis_mc_hip.hip) written out for this family -- and every
recipe is checked against it before it is handed out, so a row no call can reach has no recipe.  What the library really launched is
Engine.last_kernel_key(); the GPU test holds the two together.

A NEW ROW OF A KERNEL TABLE NEEDS A RECIPE HERE: tests/test_kernel_table_host.py fails until `recipe` returns one for it.

The module also builds the problem family, runs a recipe and holds the comparisons with the CPU oracle (the bars of tests/test_hip_parity.py).
Further families of the same shape (`register_family`; tests/coincident_lines.py registers "clustered") run through the same recipes.
"""
import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np
from numpy.testing import assert_allclose

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _golden  # noqa: E402
import vpacket_last_interaction_ref as vref  # noqa: E402
from tardis_amd import _lib, synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

TABLES = Engine.KERNEL_TABLES
FIELDS = Engine.KERNEL_KEY_FIELDS
EST_RTOL = 1e-11  # (tests/test_hip_parity.py: atomics change the summation order of the estimators)

# every option that feeds a key; a recipe sets each of them
OPTIONS = ("variant", "group_size", "track_last_interaction", "track_full", "vpacket_last_interaction", "table_offsets", "vpk_wide_registers",
           "ls_waves_per_simd", "sweep_table", "log_by_shell", "est_pipeline", "debug_flags")
# debug flags: the macro-atom walks on the fp64 running sums (the XWALK instantiations): the cooperative group scan | the per-lane search
WALK_GROUP_FP64, WALK_LANE_FP64 = 8192, 128
# ... and every flag that needs a cross-check instantiation of the wave kernel (plan::DBG_WAVE_CROSS_CHECK)
CROSS_CHECK = 128 | 8192 | 1048576 | (1 | 2 | 4 | 16 | 32 | 16384 | 32768 | 65536 | 131072 | 524288 | 2097152 | 4194304 | 8388608 | 16777216 | 134217728 | 268435456)

# the problem family: macro-atom, heavy-tailed blocks; 6037 packets = 94 full waves and one of 21 lanes, no multiple of 8, 16 or 64
N_PACKETS, N_SHELLS, N_LINES, N_VPACKETS = 6037, 12, 3000, 3
EST_TILE, PART_LOCAL_BUCKETS = 2048, 1024  # (csrc/estimator_log.hpp, csrc/estimator_partition.hpp)

Recipe = namedtuple("Recipe", "full n_vpackets vpacket_tracking options")


def table_rows(table):
    """The rows of `table` as the library reports them (needs no GPU)."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return Engine.kernel_table(table)


def row_id(table, key):
    return table + "-" + "-".join(str(v) for v in key)


# ---- the forward direction: which row a call of the problem family runs on ------------------------------------------------------------

def selected_row(rec):
    """(table, key) of the row a propagate call with this recipe looks up, or ("error", text) where the library refuses the call."""
    o = rec.options
    assert set(o) == set(OPTIONS), set(o) ^ set(OPTIONS)
    assert o["ls_waves_per_simd"] in (3, 4), "0 lets the lane-sweep tuner choose (and time calls)"
    full, vpk = bool(rec.full), rec.n_vpackets > 0
    track, ft = bool(o["track_last_interaction"]), bool(o["track_full"])
    vli = bool(o["vpacket_last_interaction"]) and rec.vpacket_tracking and vpk  # (vlog_li_call)
    flags = o["debug_flags"]
    if vli and not track and not ft:
        return "error", "the option vpacket_last_interaction needs a tracker"
    # plan_propagate for sorted lines, monotone probabilities, survival probability 0, at most 32 v-packets, compact walk tables, small tables
    variant = o["variant"]
    assert variant in (0, 1, 2, 3, 4)
    wave_auto = 3 if (not full and not vpk) else 2
    if variant == 4 and not vpk:
        variant = wave_auto
    if ft:
        variant = 2 if (variant != 0 and not (flags & CROSS_CHECK)) else 0
    cooperative = variant != 0
    is_wave = variant in (2, 3, 4)
    w64 = False
    if cooperative and o["table_offsets"] == 1:
        if variant == 4:
            return "error", "variant 4 (the volley queue) has no 64-bit table offsets"
        if is_wave and (flags & CROSS_CHECK):
            return "error", "the cross-check instantiations of the wave kernel have no 64-bit table offsets"
        w64 = True
    if not cooperative:  # launch_lane
        return "lane", (int(full), int(vpk), int(track), int(ft), int(vli))
    gs = o["group_size"] if o["group_size"] in (4, 8, 16) else 0
    if variant == 1:  # run_group_kernel (N_LINES <= 100000)
        g = 8 if gs == 8 else (16 if gs == 16 else (8 if not vpk else 16))
        return "group", (int(full), int(track), g, 256, 4, int(vpk), int(w64), int(vli))
    # choose_wave_kernel (line_interaction_type != 0, the compact walk tables exist)
    ls = variant == 3 and not full
    wpe = 3 if vpk else 4
    xwalk = bool(flags & CROSS_CHECK)  # (the fp64 walks instead of the compact tables, the long instantiations, the counter flags)
    if w64 and xwalk:
        return "error", "the fp64 macro-atom walks have no 64-bit table offsets"
    gw = gs if gs else 8
    width = 16 if ls else gw
    if vpk and not xwalk and not w64 and not ft and (ls or gw in (8, 16)):
        assert o["vpk_wide_registers"] in (0, 2), "1 depends on the LDS of the shape"
        if o["vpk_wide_registers"] == 2:
            wpe = 2
    nt, ls3 = 0, False
    if ls and not vpk and not xwalk:
        ls3 = o["ls_waves_per_simd"] == 3
        if ls3:
            wpe = 3
        if not w64 and o["sweep_table"] != 0:  # (tables without a negative optical depth)
            nt = 2 if (o["sweep_table"] == 2 and not ls3) else 1
    tiles = max((N_LINES + EST_TILE - 1) // EST_TILE, 1)
    partition = o["est_pipeline"] == 1 and tiles <= PART_LOCAL_BUCKETS and N_SHELLS <= PART_LOCAL_BUCKETS
    sl = (ls and not vpk and not xwalk and not w64 and variant != 4 and partition and o["log_by_shell"] != 0 and N_SHELLS <= 64 and
          ((not ls3 and nt == 1) or (ls3 and nt == 0)))
    if ft:
        track, width = True, 16
    if w64 and width == 4:
        width = 8
    return "wave", (int(full), int(track), width, int(vpk), int(ls), int(xwalk), wpe, nt, int(sl), int(ft), int(w64), int(vli))


# ---- the inverse: the recipes of a row --------------------------------------------------------------------------------------------

def _candidate(table, key):
    k = dict(zip(FIELDS[table], key))
    o = dict(variant=TABLES.index(table), group_size=16, track_last_interaction=k["TRACK"], track_full=0, vpacket_last_interaction=k["VLI"],
             table_offsets=0, vpk_wide_registers=0, ls_waves_per_simd=4, sweep_table=0, log_by_shell=0, est_pipeline=1, debug_flags=0)
    if table == "lane":
        o["track_full"] = k["FT"]
    elif table == "group":
        o.update(group_size=k["G"], table_offsets=k["WIDE"])
    else:
        production_ls = k["LS"] and not k["VPK"] and not k["XWALK"]
        o.update(variant=3 if k["LS"] else 2, group_size=k["G"], track_full=k["FT"], table_offsets=k["WIDE"],
                 vpk_wide_registers=2 if k["WPE"] == 2 else 0, ls_waves_per_simd=3 if (production_ls and k["WPE"] == 3) else 4,
                 sweep_table=k["NT"], log_by_shell=k["SL"], debug_flags=WALK_GROUP_FP64 if k["XWALK"] else 0)
    n_v = N_VPACKETS if k["VPK"] else 0
    return Recipe(bool(k["FULL"]), n_v, n_v > 0, o)


def recipes(table, key):
    """Every recipe of the row: one, or two for an XWALK row (the instantiation is the same, the walk compiled into it that runs differs:
    debug flag 8192, then 128).  Empty when no configuration and option set of the family reaches the row."""
    key = tuple(int(v) for v in key)
    if len(key) != len(FIELDS[table]):
        return []
    first = _candidate(table, key)
    out = [first]
    if table == "wave" and dict(zip(FIELDS[table], key))["XWALK"]:
        out.append(first._replace(options=dict(first.options, debug_flags=WALK_LANE_FP64)))
    return [r for r in out if selected_row(r) == (table, key)]


def recipe(table, key):
    found = recipes(table, key)
    if not found:
        raise KeyError(f"no recipe reaches the row {row_id(table, key)}: write one in tests/kernel_table_recipes.py, or delete the row")
    return found[0]


def recipe_id(rec):
    """A recipe as a hashable value (two rows must not share one)."""
    return (rec.full, rec.n_vpackets, rec.vpacket_tracking, tuple(sorted(rec.options.items())))


# ---- the problem family and its oracle runs -------------------------------------------------------------------------------------

_families = {"base": lambda prob: prob}


def register_family(name, transform):
    """A further problem family: `transform` changes the base problem of a configuration in place and returns it.  The shape (packets,
    shells, lines, v-packets) stays, so the recipes hold for every family (tests/coincident_lines.py: the clustered line list)."""
    _families[name] = transform


def make_problem(full, n_vpackets, family="base"):
    prob = synthetic.make_problem(seed=41, n_packets=N_PACKETS, n_shells=N_SHELLS, n_lines=N_LINES, line_interaction_type="macroatom",
                                  level_sizes="heavy", n_bins=2000, n_vpackets=n_vpackets, enable_full_relativity=bool(full))
    prob.montecarlo_configuration.ENABLE_VPACKET_TRACKING = n_vpackets > 0
    return _families[family](prob)


_cases, _traces, _lane_logs = {}, {}, {}


def case(oracle, full, n_vpackets, family="base"):
    """(problem, oracle result) of a configuration: MATH_PORTABLE, tracked, one thread (the v-packet log in packet order); computed once."""
    k = (bool(full), int(n_vpackets), family)
    if k not in _cases:
        prob = make_problem(*k)
        ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                         prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=True)
        assert ref.return_code == 0
        _cases[k] = (prob, ref)
    return _cases[k]


def sample_mix(ref):
    """The four classes of packets the sample must hold, from the oracle result alone."""
    t = ref.trackers
    return {"no interaction": int((t.interactions_count == 0).sum()), "last is a line": int((t.interaction_type == 2).sum()),
            "last is electron scattering": int((t.interaction_type == 4).sum()), "reabsorbed": int((ref.output_energies < 0).sum())}


def oracle_trace(oracle, full, n_vpackets, family="base"):
    """The oracle's serial trace log of a configuration: {shell, first line, lines visited, type} per trace_packet, packet by packet
    (as _oracle_trace of tests/test_full_tracking_gpu.py; one row per event)."""
    k = (bool(full), int(n_vpackets), family)
    if k not in _traces:
        prob, ref = case(oracle, *k)
        lib = oracle.lib()
        lib.oracle_set_trace_log.restype = None
        lib.oracle_set_trace_log.argtypes = [C.c_void_p, C.c_int64]
        lib.oracle_trace_log_count.restype = C.c_int64
        cap = int(ref.counters["events"]) + 64
        buf = np.zeros((cap, 4), dtype=np.int64)
        lib.oracle_set_trace_log(buf.ctypes.data, cap)
        try:
            oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                       prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=False)
            n = int(lib.oracle_trace_log_count())
        finally:
            lib.oracle_set_trace_log(None, 0)
        assert n == ref.counters["events"]
        _traces[k] = buf[:n]
    return _traces[k]


# ---- one call on a fresh engine ---------------------------------------------------------------------------------------------------

Run = namedtuple("Run", "results row vpacket_log event_log")


def run(rec, prob, ref):
    """One propagate call of `rec` on a fresh engine.  `ref` (the oracle's result) only sizes the logs: the event log for the oracle's
    event count, the v-packet log arrays for its entries."""
    o = rec.options
    with Engine(0) as eng:
        for name in OPTIONS:
            eng.set_option(name, o[name])
        if o["track_full"]:
            eng.set_option("event_log_capacity", int(ref.counters["events"]))
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        row = eng.last_kernel_key()
        res = eng.get_results(track_last_interaction=bool(o["track_last_interaction"]),
                              vpacket_log_capacity=int(ref.vpacket_log_count) if rec.vpacket_tracking else None)
        vlog = eng.get_vpacket_log() if rec.vpacket_tracking else None
        events = eng.get_event_log() if o["track_full"] else None
    return Run(res, row, vlog, events)


def lane_event_log(oracle, full, n_vpackets, family="base"):
    """The lane kernel's full r-packet log of a configuration (the row lane FULL, VPK, 1, 1, 0), held against the oracle's trace: the
    yardstick of the wave kernel's FT rows and, through tests/vpacket_last_interaction_ref.py, of the VLI rows.  Computed once."""
    k = (bool(full), int(n_vpackets), family)
    if k not in _lane_logs:
        prob, ref = case(oracle, *k)
        key = (int(k[0]), int(k[1] > 0), 1, 1, 0)
        got = run(recipe("lane", key), prob, ref)
        assert got.row == ("lane", key)
        same_as_oracle_trace(got.event_log, oracle_trace(oracle, *k), got.results)
        _lane_logs[k] = got.event_log
    return _lane_logs[k]


# ---- the comparisons --------------------------------------------------------------------------------------------------------------

def same_per_packet(got, ref, trackers):
    """output_nus, output_energies and, with `trackers`, the 14 tracker fields: bit for bit."""
    assert np.array_equal(got.output_nus, ref.output_nus)
    assert np.array_equal(got.output_energies, ref.output_energies)
    if trackers:
        assert len(_golden.TRACKER_I64 + _golden.TRACKER_F64) == 14
        for f in _golden.TRACKER_I64:
            assert np.array_equal(getattr(got.trackers, f), getattr(ref.trackers, f)), f
        for f in _golden.TRACKER_F64:
            assert np.array_equal(getattr(got.trackers, f), getattr(ref.trackers, f), equal_nan=True), f


def same_estimators_and_counters(got, ref):
    assert_allclose(got.j_estimator, ref.j_estimator, rtol=EST_RTOL, atol=0)
    assert_allclose(got.nu_bar_estimator, ref.nu_bar_estimator, rtol=EST_RTOL, atol=0)
    assert_allclose(got.j_blue_estimator, ref.j_blue_estimator, rtol=EST_RTOL, atol=0)
    assert_allclose(got.edotlu_estimator, ref.edotlu_estimator, rtol=EST_RTOL, atol=0)
    for k in ("line_visits", "events", "macro_transitions", "rng_draws"):
        assert got.counters[k] == ref.counters[k], k


def same_vpacket_log(got, vlog, ref):
    """The v-packet log columns bit for bit (the consolidated log is in packet order, then spawn order: the serial oracle's order), the
    v-packet histogram within the summation-order tolerance, the v-packet counters exactly."""
    n = int(ref.vpacket_log_count)
    assert n > 0 and got.vpacket_log_count == n and len(vlog.nus) == n and vlog.offsets[-1] == n
    for f in ("nus", "energies", "initial_mus", "initial_rs"):
        assert np.array_equal(getattr(vlog, f), getattr(ref, "vpacket_" + f)), f
    assert_allclose(got.v_packets_energy_hist, ref.v_packets_energy_hist, rtol=EST_RTOL, atol=0)
    for k in ("vpacket_line_visits", "vpackets"):
        assert got.counters[k] == ref.counters[k], k


def same_last_interaction_columns(vlog, events, cfg, n_vpackets):
    """The last-interaction columns of the v-packet log against tests/vpacket_last_interaction_ref.py on a full event log of the same
    problem (as test_against_the_yardstick of tests/test_vpacket_last_interaction_gpu.py)."""
    want = vref.expected_from_event_log(events, cfg.VPACKET_SPAWN_START_FREQUENCY, cfg.VPACKET_SPAWN_END_FREQUENCY, n_vpackets)
    assert len(vlog.nus) == len(want["source_packet"])
    for t in (-1, 2, 4):
        assert (want["last_interaction_type"] == t).sum() > 100, t
    assert np.array_equal(vlog.offsets, want["offsets"]) and np.array_equal(vlog.source_packet, want["source_packet"])
    for f in vref.INT_FIELDS:
        assert getattr(vlog, f).dtype == np.int64 and np.array_equal(getattr(vlog, f), want[f]), f
    assert vref.same_bits(vlog.last_interaction_in_nu, want["last_interaction_in_nu"])
    assert vref.same_bits(vlog.last_interaction_in_r, want["last_interaction_in_r"])
    some = vlog.last_interaction_type != -1
    assert np.array_equal(vlog.last_interaction_in_r[some].view(np.int64), vlog.initial_rs[some].view(np.int64))


def same_as_oracle_trace(log, tr, res):
    """Offsets and event rows of a full r-packet log against the oracle's serial trace and the call's own per-packet results (parts (1)
    and (4) of test_rows_follow_the_oracle_and_the_packet, tests/test_full_tracking_gpu.py)."""
    assert len(log) == N_PACKETS and log.n_rows == res.counters["events"] == len(tr)
    assert log.offsets[0] == 0 and log.offsets[-1] == log.n_rows and np.all(np.diff(log.offsets) >= 1)
    assert np.array_equal(log.shell_id, tr[:, 0])
    assert np.array_equal(log.interaction_type, tr[:, 3])
    line = log.interaction_type == 2
    assert np.array_equal(log.line_absorb_id[line], (tr[:, 1] + tr[:, 2] - 1)[line])
    assert np.all(log.line_absorb_id[~line] == -1) and np.all(log.line_emit_id[~line] == -1)
    assert np.array_equal(log.event_id, np.arange(log.n_rows) - np.repeat(log.offsets[:-1], log.counts))
    last = log.offsets[1:] - 1
    inner = np.ones(log.n_rows, bool)
    inner[last] = False
    nxt = np.flatnonzero(inner)
    assert np.array_equal(log.before_nu[nxt + 1], log.after_nu[nxt])
    assert np.array_equal(log.before_energy[nxt + 1], log.after_energy[nxt])
    assert np.all(log.status[inner] == 0) and np.all(log.status[last] != 0)
    assert np.array_equal(log.after_nu[last], res.output_nus)
    assert np.array_equal(np.where(log.status[last] == 2, -1, 1) * log.after_energy[last], res.output_energies)


def event_rows(log):
    from tardis_amd import state as st
    return np.stack([getattr(log, f).view(np.int64) for f in st.FullTrackers.F64_FIELDS + st.FullTrackers.I64_FIELDS])


def same_event_log(log, want):
    """Offsets and event rows of two full r-packet logs: bit for bit (test_wave_kernel_rows_equal_lane_kernel_rows)."""
    assert np.array_equal(log.offsets, want.offsets)
    assert np.array_equal(event_rows(log), event_rows(want))
