"""CPU side of the prefix-sum tables (tests/prefix_tables_ref.py; the device side is tests/test_prefix_tables_gpu.py).

  * The yardstick itself: exact sums by `fractions.Fraction`, against `math.fsum`.
  * The serial two-sum prefix of the block skip's host shim (tests/test_sweep_skip_host.py), held to the same exact sums and the same bound as the
    device's chunked one.
  * The planted-threshold check of tests/test_sweep_skip_host.py on three tables that make the margin M large.
  * With the oracle alone, that the attacks on the screening's margin exist: the runs at the three roulette thresholds 10 (1 - 1e-13), 10, 10 (1 + 1e-13)
    are pairwise different (near-ties lie on both sides), the blue optical depths of the cancellation scenario change nothing in the reference, and on
    the concentrated list (n + 4) tau_shell exceeds the row sum for many crossings.
"""
import ctypes as C
import math
from collections import Counter

import numpy as np
import pytest

import prefix_tables_ref as ptr
import test_sweep_skip_host as base

ACCESSORS = r"""
extern "C" const double *prefix_sums() { return T.pfx.data(); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    L = base.load_shim(tmp_path_factory.mktemp("prefix_tables"), base.SHIM + ACCESSORS)
    L.prefix_sums.restype = C.POINTER(C.c_double)
    return L


@pytest.mark.parametrize("n_lines", [1, 257, 4099])
def test_exact_sums_are_what_fsum_rounds(n_lines):
    _, rows = ptr.table_problem(n_lines, n_packets=1)
    assert rows.shape == (ptr.N_TABLE_SHELLS, n_lines)
    for name, row in zip(ptr.ROW_NAMES, rows):
        exact = ptr.exact_prefix(row)
        assert len(exact) == n_lines + 1 and exact[0] == 0
        for i in (1, n_lines // 2, n_lines):
            assert float(exact[i]) == math.fsum(row[:i]), (name, i)
    # the checker sees a lost low word: plain double accumulation of the tenths
    row = rows[ptr.ROW_NAMES.index("tenths")]
    if n_lines == 4099:
        bad, worst, not_rounded = ptr.check_row(np.concatenate(([0.0], np.cumsum(row))), ptr.exact_prefix(row))
        assert bad and worst > 2.0 and not_rounded >= len(bad)


def test_the_shim_s_serial_prefix_meets_the_device_s_bound(shim):
    """The host restatement of the block skip builds its prefix sums with one serial two-sum per row; the device with two-sums per chunk and a scan of the
    chunk totals.  Both are held to the exact sums, within (2^-53 + 2^-70) P."""
    n_lines = 4099
    _, rows = ptr.table_problem(n_lines, n_packets=1)
    rows = np.ascontiguousarray(rows[[ptr.ROW_NAMES.index(r) for r in ("lognormal", "tenths", "single-one-at-the-end", "one-1e250")]])
    assert rows.shape[0] == base.N_SHELLS
    nu = np.ascontiguousarray(np.linspace(2e15, 1e14, n_lines))
    shim.build_tables(nu.ctypes.data, rows.ctypes.data, base.N_SHELLS, n_lines, 1.0)
    pfx = np.ctypeslib.as_array(shim.prefix_sums(), shape=(base.N_SHELLS, n_lines + 1)).copy()
    for s in range(base.N_SHELLS):
        bad, worst, _ = ptr.check_row(pfx[s], ptr.exact_prefix(rows[s]))
        assert not bad and worst <= 1.0 + 2.0 ** -17, (s, bad[:5], worst)


@pytest.mark.parametrize("name", ptr.SKIP_TABLES)
def test_block_skip_equals_the_reference_loop_on_large_margins(shim, name):
    """test_block_skip_equals_the_reference_loop of tests/test_sweep_skip_host.py, its planted thresholds included, on tables whose margin is not small:
    many interval-mode fall-backs, g = 8 M comparable to tau_event or beyond it."""
    n_lines, n = 20003, 6000
    geo, nu_line, tau_t = base.tables(n_lines)
    tau_t = np.ascontiguousarray(ptr.skip_table(name, tau_t.T).T)
    m = shim.build_tables(nu_line.ctypes.data, tau_t.ctypes.data, base.N_SHELLS, n_lines, 1.0)
    rowsums = np.ctypeslib.as_array(shim.prefix_sums(), shape=(base.N_SHELLS, n_lines + 1))[:, n_lines]
    assert m == ptr.ssk_margin(n_lines, float(rowsums.max()))
    g = 8.0 * m
    rng = np.random.default_rng(n_lines)
    tr = base.make_traces(rng, geo, nu_line, n)
    stats = Counter()
    planted = 0
    for k in range(n):
        ref, info = base.check(shim, tr, k, g, stats)
        if k % 4 == 0:
            for ulps in (-3, -1, 0, 1, 3):
                te = float(ref[3]) * (1.0 + ulps * 2.0 ** -52)
                if te > 1e-6:
                    base.check(shim, tr, k, g, stats, te)
                    planted += 1
            kp = shim.kprime(float(tr[4][k]), float(tr[2][k]), tr[7])
            for j in (0, 1, 9):
                thr = shim.block_threshold(int(tr[0][k]), int(tr[1][k]), j, float(tr[3][k]), kp)
                for ulps in (-2, 0, 2):
                    te = thr * (1.0 + ulps * 2.0 ** -52)
                    if te > 1e-6:
                        base.check(shim, tr, k, g, stats, te)
                        planted += 1
    print(name, "margin", m, "planted", planted, dict(stats))
    for code in (1, 2, 3, 9, 10):
        assert stats["code%d" % code] > 0, code
    assert stats["interval"] > 0 and stats["fallback_margin"] > 0


# ---- the attacks on the screening's margin exist (oracle alone)
_refs = {}


def reference(oracle, name, threshold, prob=None):
    """The oracle's run of scenario `name` at roulette threshold `threshold` (shared with tests/test_prefix_tables_gpu.py; never modified)."""
    key = (name, threshold)
    if key not in _refs:
        prob = ptr.screening_problem(name) if prob is None else prob
        prob.montecarlo_configuration.VPACKET_TAU_RUSSIAN = threshold
        ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                         prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=False)  # (one thread: the estimators' summation order is fixed)
        assert ref.return_code == 0
        _refs[key] = ref
    return _refs[key]


def same_run(a, b):
    return (a.counters == b.counters and a.vpacket_log_count == b.vpacket_log_count and np.array_equal(a.output_nus, b.output_nus)
            and np.array_equal(a.output_energies, b.output_energies) and np.array_equal(a.vpacket_energies, b.vpacket_energies)
            and np.array_equal(a.vpacket_nus, b.vpacket_nus) and np.array_equal(a.v_packets_energy_hist, b.v_packets_energy_hist)
            and np.array_equal(a.j_blue_estimator, b.j_blue_estimator) and np.array_equal(a.j_estimator, b.j_estimator))


@pytest.mark.parametrize("name", ptr.SCENARIOS)
def test_near_ties_lie_on_both_sides_of_the_threshold(oracle, name):
    below, at, above = (reference(oracle, name, thr) for thr in ptr.THRESHOLDS)
    for r in (below, at, above):
        print(name, {k: r.counters[k] for k in ("vpackets", "vpacket_line_visits", "rng_draws")}, "log", r.vpacket_log_count)
    assert not same_run(below, at) and not same_run(at, above) and not same_run(below, above)
    for a, b in ((below, at), (at, above), (below, above)):
        assert a.counters["vpacket_line_visits"] != b.counters["vpacket_line_visits"]  # (what _same of tests/test_vpacket_screening.py would see)


def test_blue_optical_depths_do_not_change_the_reference(oracle):
    """Scatter mode: nothing is ever emitted into the lines bluer than every packet, so their optical depths are never read -- while every prefix sum a
    v-packet reads carries them (row sums of 7e9 in place of 3e3)."""
    prob = ptr.screening_problem("cancellation")
    blue = ptr.blue_lines(prob)
    assert blue.sum() > 1000 and not blue[int(blue.sum()):].any()  # (the head of the list)
    tau = prob.opacity_state.tau_sobolev
    assert (tau[blue] >= 1e6).all() and (tau[~blue] == 0.1).all() and tau[:, 0].sum() > 1e9
    for thr in ptr.THRESHOLDS:
        plain, planted = reference(oracle, "drift", thr), reference(oracle, "cancellation", thr, prob)
        assert same_run(plain, planted), thr
        assert not planted.j_blue_estimator[blue].any()


def test_concentrated_list_makes_the_n_term_the_larger_one():
    """(n + 4) tau_shell of the margin against its row-sum term, for v-packets leaving the inner boundary across the band: from the line list and the
    geometry alone (n lines per crossing, tau_shell = 0.02 n without electron scattering)."""
    prob = ptr.screening_problem("concentrated")
    op = prob.opacity_state
    rowsum = float(op.tau_sobolev[:, 0].sum())
    assert rowsum == 40.0 and (op.tau_sobolev == 0.02).all()
    larger = crossings = 0
    for nu in np.linspace(0.95e15, 1.07e15, 25):
        for mu in np.linspace(0.0, 1.0, 9):
            for n in ptr.lines_per_crossing(prob.geometry, op.line_list_nu, nu, mu):
                crossings += n > 0
                larger += (n + 4) * (0.02 * n) > rowsum
    print("crossings with lines", crossings, "of which (n + 4) tau_shell > row sum", larger)
    assert larger >= 100
