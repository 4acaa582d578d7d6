"""The block skip of the sixteen-wave lane sweeps (option `sweep_skip`, include/tardis_mc.h; tardis_amd/csrc/sweep_skip.hpp; the algorithm itself is
checked on the host in tests/test_sweep_skip_host.py) against the CPU oracle: per-packet outputs and last-interaction trackers bit for bit, all work
counters exactly, J / nu_bar and the line estimators at the usual bars.

Four problems whose traces are long enough to leave their first block of 8 lines, (a) and (b) with traces beyond one coarse step, (b) with a row that is
no multiple of 8, (c) with many traces that end in electron scattering (which fall back to the line-by-line sweep), (d) downbranch on 20 shells.  Each
runs with the skip off and on; in one launch and in several (a small line-visit log: lanes are suspended in the middle of a trace, in coarse and in
interval mode, and start it again); through the packed drain; with every interval-mode decision counted as ambiguous (debug flag 536870912: every skipped
trace falls back); and on a table with one negative optical depth, where the skip must report off."""
import numpy as np
import pytest

import kernel_table_recipes as ktr
from tardis_amd import state as st, synthetic

pytestmark = pytest.mark.gpu

N_PACKETS = 4096
FALLBACK = 536870912
PROBLEMS = {
    "a": dict(seed=3, n_packets=N_PACKETS, n_shells=4, n_lines=20_000, line_interaction_type="macroatom", level_sizes="heavy"),
    "b": dict(seed=3, n_packets=N_PACKETS, n_shells=4, n_lines=20_003, line_interaction_type="macroatom", level_sizes="heavy"),
    "c": dict(seed=3, n_packets=N_PACKETS, n_shells=3, n_lines=4_000, line_interaction_type="macroatom", level_sizes="heavy"),
    "d": dict(seed=3, n_packets=N_PACKETS, n_shells=20, n_lines=30_000, line_interaction_type="downbranch"),
}
_cases = {}


def case(oracle, name):
    if name not in _cases:
        prob = synthetic.make_problem(**PROBLEMS[name])
        ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                         prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=oracle.max_threads(), track_last_interaction=True)
        assert ref.return_code == 0
        print(name, "line visits per trace: %.1f" % (ref.counters["line_visits"] / max(ref.counters["events"], 1)))
        _cases[name] = (prob, ref)
    return _cases[name]


def run(prob, opacity_state=None, **options):
    from tardis_amd.engine import Engine
    with Engine(0) as eng:
        eng.set_option("variant", 3)
        eng.set_option("ls_waves_per_simd", 4)
        for k, v in options.items():
            eng.set_option(k, v)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state if opacity_state is None else opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        res = eng.get_results(track_last_interaction=True)
        return res, eng.last_kernel_key(), eng.last_kernel_times()["launches"], eng.last_compactions(), eng.last_sweep_skip()


def same_as_oracle(res, ref):
    ktr.same_per_packet(res, ref, trackers=True)   # bit for bit
    ktr.same_estimators_and_counters(res, ref)     # estimators to 1e-11, line_visits / events / macro_transitions / rng_draws exactly
    assert np.array_equal(res.j_blue_estimator == 0.0, ref.j_blue_estimator == 0.0)


def sixteen_wave_interleaved(row):
    k = dict(zip(ktr.FIELDS["wave"], row[1]))
    return row[0] == "wave" and k["LS"] == 1 and k["VPK"] == 0 and k["XWALK"] == 0 and k["WPE"] == 4 and k["NT"] == 1 and k["SL"] == 0


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_one_launch(oracle, name, skip):
    prob, ref = case(oracle, name)
    res, row, launches, _, on = run(prob, sweep_skip=skip)
    print(name, skip, "->", row, "launches", launches, "skip", on)
    assert sixteen_wave_interleaved(row), row
    assert on == skip
    same_as_oracle(res, ref)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_automatic_is_on(oracle, name):
    prob, ref = case(oracle, name)
    res, row, _, _, on = run(prob)
    assert sixteen_wave_interleaved(row) and on == 1
    same_as_oracle(res, ref)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_several_launches(oracle, name, skip):
    """A small log: the waves suspend again and again, with lanes in the middle of a trace."""
    prob, ref = case(oracle, name)
    capacity = max(256 * ((N_PACKETS + 63) // 64), int(ref.counters["events"]) // 5)
    res, row, launches, _, on = run(prob, sweep_skip=skip, log_capacity=capacity, log_chunk_records=257)
    print(name, skip, "log capacity", capacity, "launches", launches, row)
    assert sixteen_wave_interleaved(row) and on == skip
    assert launches >= 2  # (every wave was suspended at least once)
    same_as_oracle(res, ref)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_packed_drain(oracle, name, skip):
    prob, ref = case(oracle, name)
    res, row, launches, packed, on = run(prob, sweep_skip=skip, drain_compact=16)
    print(name, skip, "launches", launches, "packed", packed, row)
    assert sixteen_wave_interleaved(row) and on == skip
    assert packed >= 1 and launches >= 2
    same_as_oracle(res, ref)


@pytest.mark.parametrize("several", [False, True], ids=["one-launch", "several-launches"])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_every_skipped_trace_falls_back(oracle, name, several):
    prob, ref = case(oracle, name)
    extra = dict(log_capacity=max(256 * ((N_PACKETS + 63) // 64), int(ref.counters["events"]) // 5), log_chunk_records=257) if several else {}
    res, row, launches, _, on = run(prob, sweep_skip=1, debug_flags=FALLBACK, **extra)
    assert sixteen_wave_interleaved(row) and on == 1, row
    same_as_oracle(res, ref)


def test_option_turned_on_between_calls_of_one_context(oracle):
    """The interleaved table of the first call was built without room for the skip's tables: the second call builds it again, elsewhere."""
    from tardis_amd.engine import Engine
    prob, ref = case(oracle, "a")
    with Engine(0) as eng:
        eng.set_option("variant", 3)
        eng.set_option("ls_waves_per_simd", 4)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        for skip in (0, 1, 0, 1):
            eng.set_option("sweep_skip", skip)
            eng.set_packets(prob.packet_collection)
            eng.reset_estimators()
            eng.propagate()
            eng.synchronize()
            assert eng.last_sweep_skip() == skip
            same_as_oracle(eng.get_results(track_last_interaction=True), ref)
        # a call of another kernel reports off, not what the call before it ran with
        eng.set_option("variant", 0)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        assert eng.last_variant() == 0 and eng.last_sweep_skip() == 0


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_a_negative_optical_depth_turns_the_skip_off(oracle, name):
    prob, _ = case(oracle, name)
    op = prob.opacity_state
    tau = np.array(op.tau_sobolev, dtype=np.float64, copy=True)
    tau[tau.shape[0] // 2, 1] = -1e-3
    op2 = st.OpacityState(op.electron_density, op.t_electrons, op.line_list_nu, tau, op.transition_probabilities, op.line2macro_level_upper,
                          op.macro_block_edge_index, op.transition_type, op.destination_level_id, op.transition_line_id)
    ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, op2, prob.montecarlo_configuration, prob.spectrum_frequency_grid,
                     math_mode=oracle.MATH_PORTABLE, n_threads=oracle.max_threads(), track_last_interaction=True)
    res, row, _, _, on = run(prob, opacity_state=op2, sweep_skip=1)
    print(name, "->", row, "skip", on)
    assert on == 0
    same_as_oracle(res, ref)
