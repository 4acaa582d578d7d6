"""64-bit table offsets of the cooperative kernels (option table_offsets, Engine.last_table_offsets): tables whose shell-major
rows reach 2^28 entries run on variants 1-3, bit-identical to the oracle and to the 32-bit kernels.

The tables over the limit sit just above 2^28 entries (2.7e8 - 2.9e8): they exercise the host's choice and the WIDE instantiations at
those sizes, not an offset at or above 2^32 (below that the 32-bit arithmetic would still be exact -- 2^28 is the host's margin); a
table of 2^32 entries is 32 GiB per array, beyond what a test builds on the host."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import oracle
from tardis_amd import synthetic
from tardis_amd.engine import Engine, EventLogOverflow

import _golden

pytestmark = pytest.mark.gpu

EST_RTOL = 1e-11
LIMIT = 1 << 28
GOLDEN = ["macroatom_heavy_nv0", "downbranch_nv0", "macroatom_heavy_fullrel_nv2", "downbranch_fullrel", "macroatom_nv3_log", "scatter_nv0"]


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


def _run(eng, prob, track_full=False, **options):
    for k, v in options.items():
        eng.set_option(k, v)
    try:
        return eng.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state,
                       prob.montecarlo_configuration, prob.spectrum_frequency_grid, track_full=track_full)
    finally:
        for k in options:
            eng.set_option(k, -1 if k in ("variant", "table_offsets") else 0)


def _oracle(prob):
    return oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                      prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=oracle.max_threads(),
                      track_last_interaction=False)


def _same_packets(a, b):
    assert np.array_equal(a.output_nus, b.output_nus)
    assert np.array_equal(a.output_energies, b.output_energies)


def _close_estimators(a, b, lines=True):
    assert_allclose(a.j_estimator, b.j_estimator, rtol=EST_RTOL)
    assert_allclose(a.nu_bar_estimator, b.nu_bar_estimator, rtol=EST_RTOL)
    if lines:
        assert_allclose(a.j_blue_estimator, b.j_blue_estimator, rtol=EST_RTOL)
        assert_allclose(a.edotlu_estimator, b.edotlu_estimator, rtol=EST_RTOL)


@pytest.mark.parametrize("variant", [-1, 1, 2, 3])
@pytest.mark.parametrize("name", GOLDEN)
def test_forced_wide_offsets_reproduce_the_goldens(eng, name, variant):
    prob, g = _golden.load_case(name)
    narrow = _run(eng, prob, variant=variant, table_offsets=0)
    narrow_variant = eng.last_variant()
    assert eng.last_table_offsets() == (32 if narrow_variant else 64)
    wide = _run(eng, prob, variant=variant, table_offsets=1)
    assert eng.last_table_offsets() == 64
    assert eng.last_variant() == narrow_variant  # (the same kernel, in its WIDE form -- not a fall-back to variant 0)
    assert np.array_equal(wide.output_nus, g["output_nus"]) and np.array_equal(wide.output_energies, g["output_energies"])
    _same_packets(wide, narrow)
    _close_estimators(wide, narrow)
    assert_allclose(wide.v_packets_energy_hist, narrow.v_packets_energy_hist, rtol=EST_RTOL, atol=0)


_PROBLEMS = {}


def _big(mode, n_shells, n_lines, n_packets, n_vpackets=0):
    key = (mode, n_shells, n_lines, n_packets, n_vpackets)
    if key not in _PROBLEMS:
        _PROBLEMS.clear()  # (one large problem in host memory at a time)
        _PROBLEMS[key] = synthetic.make_problem(seed=3, n_packets=n_packets, n_shells=n_shells, n_lines=n_lines, line_interaction_type=mode,
                                                n_vpackets=n_vpackets, n_bins=2000, shell_independent_probabilities=True,
                                                level_sizes="heavy" if mode == "macroatom" else "uniform")
    return _PROBLEMS[key]


def _shape(prob):
    op = prob.opacity_state
    S, L, T = len(prob.geometry.r_inner), len(op.line_list_nu), len(op.transition_probabilities)
    return S * L, S * T


# (macroatom, transitions over the limit, lines below it) and downbranch with the lines over it: est_pipeline 1 at 4.8e5 lines, the
# index sort + gather (est_pipeline 0: more than 1024 tiles of 2048 lines per shell) at 2.1e6
BIG = [("macroatom", 190, 500_000, "trans"), ("downbranch", 560, 480_000, "lines"), ("downbranch", 128, 2_100_000, "lines")]


@pytest.mark.parametrize("mode,S,L,over", BIG)
def test_tables_over_the_32_bit_limit_run_on_the_cooperative_kernels(eng, mode, S, L, over):
    prob = _big(mode, S, L, 20_000)
    sl, st_ = _shape(prob)
    assert (st_ >= LIMIT and sl < LIMIT) if over == "trans" else sl >= LIMIT
    got = _run(eng, prob)
    assert eng.last_variant() in (2, 3) and eng.last_table_offsets() == 64
    ref = _oracle(prob)
    _same_packets(got, ref)
    _close_estimators(got, ref, lines=False)
    lane = _run(eng, prob, variant=0)
    _same_packets(lane, ref)
    _close_estimators(got, lane)


def test_explicit_opt_out_still_fails_on_a_wide_table(eng):
    prob = _big("macroatom", 190, 500_000, 20_000)
    with pytest.raises(RuntimeError, match="2\\^28"):
        _run(eng, prob, table_offsets=0)


def test_vpackets_on_a_wide_table(eng):
    prob = _big("macroatom", 190, 500_000, 2_000, n_vpackets=10)
    ref = _oracle(prob)
    for variant in (-1, 1, 2):
        got = _run(eng, prob, variant=variant)
        assert eng.last_table_offsets() == 64 and (variant < 0 or eng.last_variant() == variant)
        _same_packets(got, ref)
        _close_estimators(got, ref, lines=False)
        assert_allclose(got.v_packets_energy_hist, ref.v_packets_energy_hist, rtol=EST_RTOL, atol=0)


def test_full_tracking_on_a_wide_table(eng):
    prob = _big("macroatom", 190, 500_000, 2_000)

    def rows(variant):
        cap = 0
        for _ in range(4):
            try:
                res = _run(eng, prob, track_full=True, variant=variant, event_log_capacity=cap)
                return res, eng.last_table_offsets(), eng.last_variant()
            except EventLogOverflow as e:
                cap = max(e.rows_needed, 2 * cap)
        raise AssertionError("event log overflow persisted")

    wide, bits, var = rows(-1)
    assert bits == 64 and var == 2
    lane, _, _ = rows(0)
    _same_packets(wide, lane)
    a, b = wide.full_trackers, lane.full_trackers
    assert np.array_equal(a.offsets, b.offsets)
    for f in a.F64_FIELDS + a.I64_FIELDS:
        assert np.array_equal(getattr(a, f).view(np.int64), getattr(b, f).view(np.int64)), f


def test_small_tables_keep_32_bit_offsets(eng):
    prob, _ = _golden.load_case("macroatom_heavy_nv0")
    _run(eng, prob)
    assert eng.last_variant() in (1, 2, 3) and eng.last_table_offsets() == 32
