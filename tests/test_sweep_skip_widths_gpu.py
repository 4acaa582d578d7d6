"""The block skip at its two step widths (tardis_amd/csrc/sweep_skip.hpp, propagate_wave.hpp: eight loads per step in the sixteen-wave lane-sweep
instantiation, ten in the twelve-wave one) against the CPU oracle: per-packet outputs (and the last-interaction trackers where tracked) bit for bit,
line_visits / events / macro_transitions / rng_draws exactly.  The algorithm at these widths is checked on the host in
tests/test_sweep_skip_widths_host.py; here it is the kernel's glue -- the advance after a full coarse step, the loads behind a short row, the
suspension of a lane in coarse or interval mode -- at the smallest shapes at which each can go wrong.

The line lists are DENSE: L lines 2.5e-5 apart in relative frequency, 1e-5 in the longest (a shell of the 4-shell grid shifts a packet's comoving
frequency by up to 0.75 %, i.e. across up to 300 and 750 lines), the packets start just blueward of the list, anywhere in it, or redward of it (nothing left to pass), and the optical
depths are small, so that a trace runs over many lines, off the end of a short list, and -- after a line interaction, which re-emits at a line of the
list -- starts again anywhere in it, on its last line and in its last block included.
    L = 5, 13            shorter than one coarse step at either width: the step's loads run into the next row / the slack behind the table
    L = 57, 121          no multiple of 8
    L = 56, 57, 72, 73   a row of exactly 7 and 9 blocks (the coarse entries of a full step of eight and ten loads), and one line more
    L = 4003             (the suspension test) a list that covers a packet's whole way through the grid: every trace passes lines, a third more than 56
    L = 400              a fifth of its 84 000 traces (the ones of a packet still inside the list) run past 56, past 80 and mostly past 160 lines: two and
                         three coarse steps, the advance from the last cleared block
Every shape runs at ls_waves_per_simd 3 and 4, tracked and untracked, with the skip on (1) and with every interval-mode decision counted as ambiguous
(2: debug flag 536870912, WaveCold::sweep_skip = 2 -- every skipped trace falls back); each call must have run on the intended row of the kernel table
and report the skip.  Then a log so small that lanes are suspended in the middle of coarse and interval mode, and the options switched between the
calls of one context."""
import ctypes as C

import numpy as np
import pytest

import kernel_table_recipes as ktr
from tardis_amd import synthetic

pytestmark = pytest.mark.gpu

FALLBACK = 536870912
# L -> (packets, mean of log10 tau, relative distance of neighbouring lines)
SHAPES = {5: (2000, -1.5, 2.5e-5), 13: (2000, -3.5, 2.5e-5), 56: (3000, -4.5, 2.5e-5), 57: (3000, -4.5, 2.5e-5), 72: (3000, -4.5, 2.5e-5),
          73: (3000, -4.5, 2.5e-5), 121: (4000, -5.0, 2.5e-5), 400: (20000, -6.5, 1.0e-5)}
ONE_LAUNCH = list(SHAPES)
# The suspension test.  The smallest log the engine takes holds four records per packet, and a trace that passes no line logs none: a list that covers a packet's
# whole way through the grid (4 %), and thirty times the electron density -- 92 000 traces of 4096 packets, 54 000 of them with a record, 28 000 past 56 lines.
SUSPENDED, DENSE_ELECTRONS = 4003, 3e10
SHAPES[SUSPENDED] = (4096, -6.0, 1.0e-5)
_cases = {}


def dense_problem(n_lines, electron_density_0=1e9):
    n_packets, log_tau, SPACING = SHAPES[n_lines]
    prob = synthetic.make_problem(seed=9, n_packets=n_packets, n_shells=4, n_lines=n_lines, line_interaction_type="macroatom", log_tau_mean=log_tau, n_bins=2000,
                                  electron_density_0=electron_density_0)
    rng = np.random.default_rng(1000 + n_lines)
    nu_hi = 1.0e15
    nu = nu_hi * (1.0 - SPACING * (np.arange(n_lines) + rng.uniform(0.0, 0.5, n_lines)))  # strictly descending
    assert np.all(np.diff(nu) < 0)
    prob.opacity_state.line_list_nu[:] = nu
    pc = prob.packet_collection
    # comoving frequencies from 0.3 % blueward of the first line to just redward of the last one
    beta = float(prob.geometry.v_inner[0]) / 2.99792458e10
    comov = rng.uniform(nu[-1] * (1.0 - 2 * SPACING), nu_hi * 1.003, n_packets)
    pc.initial_nus[:] = comov / (1.0 - beta * pc.initial_mus)
    return prob


def trace_log(oracle, prob, n_events):
    """First line and lines visited of every trace, from the oracle's serial trace log (as kernel_table_recipes.oracle_trace)."""
    lib = oracle.lib()
    lib.oracle_set_trace_log.restype = None
    lib.oracle_set_trace_log.argtypes = [C.c_void_p, C.c_int64]
    lib.oracle_trace_log_count.restype = C.c_int64
    buf = np.zeros((n_events + 64, 4), dtype=np.int64)
    lib.oracle_set_trace_log(buf.ctypes.data, len(buf))
    try:
        oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                   prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=False)
        n = int(lib.oracle_trace_log_count())
    finally:
        lib.oracle_set_trace_log(None, 0)
    assert n == n_events
    return buf[:n, 1], buf[:n, 2]


def case(oracle, n_lines, electron_density_0=1e9):
    key = (n_lines, electron_density_0)
    if key not in _cases:
        prob = dense_problem(n_lines, electron_density_0)
        ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                         prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=oracle.max_threads(), track_last_interaction=True)
        assert ref.return_code == 0
        per_trace = ref.counters["line_visits"] / max(ref.counters["events"], 1)
        print("L", n_lines, "events", ref.counters["events"], "line visits per trace %.1f" % per_trace, "macro transitions", ref.counters["macro_transitions"])
        assert ref.counters["macro_transitions"] > 100  # (line interactions: traces that start inside the list)
        start, visited = trace_log(oracle, prob, int(ref.counters["events"]))
        last_block = (start >= ((n_lines - 1) & ~7)) & (start < n_lines)
        print("   traces that start in the last block", int(last_block.sum()), "on the last line", int((start == n_lines - 1).sum()),
              "past 56 lines", int((visited > 56).sum()), "past 80 lines", int((visited > 80).sum()))
        assert (start == n_lines - 1).sum() > 100
        if ((n_lines - 1) & 7) and n_lines in ONE_LAUNCH:  # (the last block holds more than the last line)
            assert (last_block & (start < n_lines - 1)).sum() > 100
        if n_lines == SUSPENDED:
            assert (visited >= 2).sum() > 50000 and (visited > 56).sum() > 20000 and (visited > 80).sum() > 20000
        if n_lines == 400:
            # (a packet that has passed the list goes on with one-line traces from its last line: of the 84 000 traces a fifth are long, and those are long
            # enough for a second and third coarse step at either width -- 7 and 9 blocks the first, 6 and 8 every further one)
            assert (visited > 56).sum() > 15000 and (visited > 80).sum() > 15000 and (visited > 160).sum() > 5000
        _cases[key] = (prob, ref)
    return _cases[key]


def intended_row(wpe, track):
    #                FULL TRACK  G  VPK LS XWALK WPE NT SL FT WIDE VLI
    return ("wave", (0, int(track), 16, 0, 1, 0, wpe, 1, 0, 0, 0, 0))


def set_up(eng, prob, wpe, track, skip):
    eng.set_option("variant", 3)
    eng.set_option("ls_waves_per_simd", wpe)
    eng.set_option("track_last_interaction", int(track))
    eng.set_option("sweep_skip", 1 if skip else 0)
    eng.set_option("debug_flags", FALLBACK if skip == 2 else 0)
    eng.set_packets(prob.packet_collection)
    eng.reset_estimators()


def call(eng, ref, wpe, track, skip):
    eng.propagate()
    eng.synchronize()
    assert eng.last_kernel_key() == intended_row(wpe, track), eng.last_kernel_key()
    assert eng.last_sweep_skip() == (1 if skip else 0)
    res = eng.get_results(track_last_interaction=bool(track))
    ktr.same_per_packet(res, ref, trackers=bool(track))  # bit for bit
    for k in ("line_visits", "events", "macro_transitions", "rng_draws"):
        assert res.counters[k] == ref.counters[k], k
    return res


def run(prob, ref, wpe, track, skip, **options):
    from tardis_amd.engine import Engine
    with Engine(0) as eng:
        for k, v in options.items():
            eng.set_option(k, v)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        set_up(eng, prob, wpe, track, skip)
        res = call(eng, ref, wpe, track, skip)
        return res, eng.last_kernel_times()["launches"]


@pytest.mark.parametrize("skip", [1, 2])
@pytest.mark.parametrize("track", [0, 1], ids=["untracked", "tracked"])
@pytest.mark.parametrize("wpe", [3, 4])
@pytest.mark.parametrize("n_lines", ONE_LAUNCH)
def test_one_launch(oracle, n_lines, wpe, track, skip):
    prob, ref = case(oracle, n_lines)
    res, _ = run(prob, ref, wpe, track, skip)
    ktr.same_estimators_and_counters(res, ref)


@pytest.mark.parametrize("skip", [1, 2])
@pytest.mark.parametrize("track", [0, 1], ids=["untracked", "tracked"])
@pytest.mark.parametrize("wpe", [3, 4])
@pytest.mark.parametrize("n_lines", [SUSPENDED])
def test_lanes_suspended_in_the_middle_of_a_trace(oracle, n_lines, wpe, track, skip):
    """A log of a third of the call's records: every wave is suspended, lanes in coarse and in interval mode start their trace again in the next epoch."""
    prob, ref = case(oracle, n_lines, DENSE_ELECTRONS)
    n = SHAPES[n_lines][0]
    capacity = max(256 * ((n + 63) // 64), int(ref.counters["events"]) // 5)
    res, launches = run(prob, ref, wpe, track, skip, log_capacity=capacity, log_chunk_records=257)
    print(n_lines, wpe, track, skip, "log capacity", capacity, "launches", launches)
    assert launches >= 2
    ktr.same_estimators_and_counters(res, ref)


@pytest.mark.parametrize("n_lines", [73, 400])
def test_options_switched_between_calls_of_one_context(oracle, n_lines):
    from tardis_amd.engine import Engine
    prob, ref = case(oracle, n_lines)
    with Engine(0) as eng:
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        for wpe, track, skip in ((4, 1, 0), (3, 1, 1), (4, 0, 1), (3, 0, 0), (3, 1, 2), (4, 1, 1), (4, 1, 2), (3, 0, 1)):
            set_up(eng, prob, wpe, track, skip)
            res = call(eng, ref, wpe, track, skip)
            ktr.same_estimators_and_counters(res, ref)
