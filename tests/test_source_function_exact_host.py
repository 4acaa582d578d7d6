"""The exact reference of the source function's level solve (tests/source_function_exact.py) checked on itself, the condition of its
bound, the record of what the former max-norm stop rule accepted, and what tardis_mc_debug_set_line_estimators refuses without a device.

The condition: a plain serial fp64 iteration x <- e + Q^T x, run until x no longer changes, stays within w B_k of the exact C_k on every
case the GPU tests use (w = (r + n + 3) 2^-53).  The GPU tests allow the device twice that plus 1e-14 C_k."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import source_function_exact as sfx  # noqa: E402
import source_function_ref as ref  # noqa: E402
from tardis_amd import _abi, _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_in_the_library_the_loader_the_header_and_the_engine():
    from tardis_amd.engine import Engine
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    name = "tardis_mc_debug_set_line_estimators"
    assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    assert re.search(r"\bint %s\(TardisMcContext \*ctx, const double \*j_blue, const double \*edotlu\);" % name, header)
    assert callable(getattr(Engine, "debug_set_line_estimators", None))
    # the header states the stop rule the tests hold the device to
    assert "changed no level" in header and "1e-14 max|C|" not in header


def test_entry_point_refuses_what_needs_no_device():
    L = _lib.lib()
    a = np.zeros(4)
    assert L.tardis_mc_debug_set_line_estimators(None, a.ctypes.data, a.ctypes.data) == _abi.ERR_INVALID_ARGUMENT


# ---- the reference on itself ----------------------------------------------------------------------------------------------------------

def test_exact_solvers_agree_with_one_another():
    """One cyclic system three ways: Gaussian elimination in Fractions is exact (its residual is 0), mpmath agrees with it to 1e-30, and the
    substitution of an acyclic system is the finite series sum of (Q^T)^j e."""
    rng = np.random.default_rng(1)
    K = 6
    src, dst = np.repeat(np.arange(K), 2), rng.integers(0, K, 2 * K)
    dst[::2] = (np.arange(K) + 1) % K
    q = rng.uniform(0.1, 0.45, 2 * K)
    rhs = [Fraction(float(v)) for v in rng.uniform(0, 1, K)]
    stats = {}
    x = sfx.solve_exact(K, src, dst, q, rhs, stats)
    assert stats == {"cyclic, Fractions": 1}
    for k in range(K):
        assert x[k] == rhs[k] + sum(Fraction(float(q[t])) * x[int(src[t])] for t in range(2 * K) if dst[t] == k)
    old, sfx.EXACT_CYCLIC = sfx.EXACT_CYCLIC, 0
    try:
        stats = {}
        y = sfx.solve_exact(K, src, dst, q, rhs, stats)
    finally:
        sfx.EXACT_CYCLIC = old
    assert stats == {"cyclic, mpmath": 1}
    assert all(abs(a - b) <= Fraction(1, 10 ** 30) * a for a, b in zip(x, y))
    # acyclic: 3 -> 2 -> 0, 3 -> 0 twice (duplicate rows add), level 1 alone
    x = sfx.solve_exact(4, [3, 2, 3, 3], [2, 0, 0, 0], [0.5, 0.25, 0.125, 0.125], [Fraction(1), Fraction(2), Fraction(4), Fraction(8)])
    assert x == [Fraction(1) + Fraction(1, 4) * 8 + Fraction(1, 4) * 8, Fraction(2), Fraction(8), Fraction(8)]


def test_menus_put_every_row_length_on_its_path():
    for G, shape in sfx.SHAPES.items():
        for case, lengths in ((sfx.row_sum_case(G), sfx.row_sum_case(G).lines_of_level), (sfx.acyclic_case(G), sfx.acyclic_case(G).in_lengths())):
            got, is_long = sfx.row_paths(lengths)
            assert got == G and len(lengths) == shape["K"]
            have = set(lengths.tolist())
            assert {0, 1, G - 1, G, G + 1, 32 * G, 32 * G + 1} <= have
            per_wave = 64 // G
            waves = np.arange(len(lengths)) // per_wave
            assert np.bincount(waves[is_long]).max() >= 2           # two long rows meet in one wave
            assert is_long[-1] and len(lengths) % per_wave != 0      # a long row in the last, partly filled wave
            assert len(lengths) % (256 // G) != 0 and len(lengths) > 256 // G
    assert sfx.row_sum_case(0).K == 1
    # the acyclic tables: jumps never close a circle, some level has no incoming row, some no line, and the estimators span 30 decades
    for G in sfx.SHAPES:
        case = sfx.acyclic_case(G)
        assert sfx.exact(case)["how"].keys() <= {"acyclic"}
        assert (case.in_lengths() == 0).any() and (case.lines_of_level == 0).any()
        assert case.edotlu.max() / case.edotlu.min() > 1e25
    assert set(sfx.exact(sfx.stop_rule_case("1e-6, 0.99", 63, 2))["how"]) == {"cyclic, Fractions"}
    assert set(sfx.exact(sfx.mixed_case())["how"]) == {"cyclic, mpmath"}


def test_close_restatement_matches_the_make_source_function_restatement():
    """close_bitwise against tests/source_function_ref.py (libm's exp there: a few ulp)."""
    case = sfx.mixed_case()
    C = np.array([[float(v) for v in row] for row in sfx.exact(case)["C"]]).T
    mine = sfx.close_bitwise(case, C)
    theirs = ref.make_source_function(case.op, case.j_blue, case.edotlu, case.t_sim, case.volume, case.time_explosion, solver="dense")
    for key in ("att_S_ul", "Jred_lu", "Jblue_lu"):
        np.testing.assert_allclose(mine[key], theirs[key], rtol=1e-12, atol=0)
    np.testing.assert_allclose(C, theirs["e_dot_u"], rtol=1e-11)


# ---- the condition of the bound ---------------------------------------------------------------------------------------------------------

def _condition(case):
    x, its = sfx.serial_fixed_point(case)
    ratio, where = sfx.worst_ratio(case, x, sfx.level_bound(case, factor=1, truncation=0.0))
    print(case.name, "serial iterations", its, "worst |x - C| / (w B)", ratio, "at", where)
    assert ratio <= 1.0, (case.name, ratio, where)


@pytest.mark.parametrize("G", list(sfx.SHAPES))
def test_condition_on_the_acyclic_tables(G):
    _condition(sfx.acyclic_case(G))


def test_condition_on_the_well_mixed_table():
    _condition(sfx.mixed_case())


@pytest.mark.parametrize("table", list(sfx.STOP_TABLES))
@pytest.mark.parametrize("position,shell", [(0, 0), (63, 2), (64, 4), (255, 0), (256, 2), (sfx.STOP_K - 1, 4)])
def test_condition_on_the_stop_rule_tables(table, position, shell):
    _condition(sfx.stop_rule_case(table, position, shell))


@pytest.mark.parametrize("G", [0] + list(sfx.SHAPES))
def test_serial_row_sums_meet_the_row_sum_bound(G):
    case = sfx.row_sum_case(G)
    ratio, where = sfx.worst_ratio(case, sfx.serial_level_sums(case), sfx.sum_bound(case), want="e")
    assert ratio <= 1.0, (ratio, where)


# ---- what the former rule accepted --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,p,iterations,weak_error,max_norm_error", [
    (1e-6, 0.99, 1824, 1.1e-8, 4.6e-13),
    (1e-8, 0.999, 13664, 1.2e-6, 4.9e-12),
    (1.0, 0.9999, 237232, 5e-11, 5e-11),
])
def test_former_max_norm_rule_stops_short_of_a_weak_block(scale, p, iterations, weak_error, max_norm_error):
    """max|dx| <= 1e-14 max|x|, checked every 16 iterations from x = e, on a strong two-level block beside a weak one: the iteration count
    and the errors of the issue that replaced the rule, independent of any device.  The first two stop within the default bound of 20 000
    iterations with the weak levels wrong in the 8th and 6th digit; the third shows the 1e-12 max-norm bound was no property of the rule."""
    QT, e, exact = sfx.two_block_system(scale, p)
    x, it = sfx.former_rule(QT, e)
    assert it == iterations
    rel = max(float(abs(Fraction(float(x[k])) - exact[k]) / exact[k]) for k in (2, 3))
    top = max(float(abs(Fraction(float(x[k])) - exact[k])) for k in range(4)) / float(max(exact))
    print(scale, p, it, rel, top)
    assert 0.8 * weak_error <= rel <= 1.25 * weak_error
    assert 0.8 * max_norm_error <= top <= 1.25 * max_norm_error
    # the rule that replaced it -- go on until nothing changes -- meets the bound of the module on the same systems
    y = e.copy()
    for _ in range(2_000_000):
        y_new = e + QT @ y
        same = np.array_equal(y_new, y)
        y = y_new
        if same:
            break
    B = sfx.solve_exact(4, [0, 1, 2, 3], [1, 0, 3, 2], [0.3, 0.2, p, p], exact)
    for k in range(4):
        assert abs(Fraction(float(y[k])) - exact[k]) <= Fraction((1 + 0 + 3) * sfx.U) * B[k]


def test_fixed_point_of_the_restatement_runs_the_new_rule():
    QT, e, exact = sfx.two_block_system(1e-6, 0.99)
    from scipy import sparse as sp
    x, it = ref.fixed_point(sp.csr_matrix(QT.T), e, max_iterations=100000)
    assert it > 1824
    for k in range(4):
        assert abs(Fraction(float(x[k])) - exact[k]) <= Fraction(8 * sfx.U) * exact[k] / Fraction(1 - 0.99)
