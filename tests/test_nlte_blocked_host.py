"""The blocked form of the NLTE solve without a GPU: the NumPy restatement of the BLOCKED order (tests/nlte_blocked_ref.py) gives the bits
of the unblocked yardstick (nlte_excitation_ref.lu_solve), in x and in the swap steps, on random dense systems whose rows are swapped
at nearly every step and on the rate matrices of a 261-level species; the re-association that sums an entry's products first does not.
Also the ABI pieces of the form."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nlte_blocked_ref as bref  # noqa: E402
import nlte_excitation_ref as nref  # noqa: E402
import opacity_update_ref as oref  # noqa: E402
from tardis_amd import _abi, _lib  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 31, 32, 33, 64, 65, 97, 261)
# species of 22 and 261 levels (261 = 8 x 32 + 5: nine panels, the last one ragged)
LONG_COUNTS = (1, 1, 1, 1, 2, 261, 22, 2, 1, 3, 4, 1)
LONG_SPECIES = (6, 5)


def test_the_header_and_the_restatement_share_the_panel_width():
    src = open(os.path.join(ROOT, "tardis_amd", "csrc", "nlte_plan.hpp")).read()
    assert int(re.search(r"constexpr int PANEL_COLUMNS = (\d+);", src).group(1)) == bref.PANEL_COLUMNS


@pytest.mark.parametrize("n", SIZES)
def test_blocked_order_gives_the_bits_of_the_unblocked_order_on_dense_systems(n):
    ms, bs = bref.random_systems(n, 2 if n == 261 else 4, seed=7)
    for m, b in zip(ms, bs):
        want, want_swaps = nref.lu_solve(m, b)
        got, got_swaps = bref.blocked_lu_solve(m, b)
        assert got_swaps == want_swaps and np.array_equal(got, want)
        assert n < 31 or len(want_swaps) > n // 2  # rows swapped at more than half of the steps


def test_summing_the_products_first_changes_the_bits():
    """The comparison above is not vacuous: the one re-association the kernels must not make is visible in the bits."""
    differ = 0
    for n in (33, 65, 97):
        ms, bs = bref.random_systems(n, 4, seed=7)
        for m, b in zip(ms, bs):
            want, _ = nref.lu_solve(m, b)
            wrong, _ = bref.blocked_lu_solve(m, b, summed_first=True)
            assert np.allclose(wrong, want, rtol=1e-6, atol=1e-9)  # the same solution to rounding
            differ += not np.array_equal(wrong, want)
    assert differ >= 1


def test_a_narrow_panel_and_a_panel_wider_than_the_matrix():
    ms, bs = bref.random_systems(65, 2, seed=11)
    for m, b in zip(ms, bs):
        want = nref.lu_solve(m, b)
        for nb in (1, 5, 64, 65, 200):
            got = bref.blocked_lu_solve(m, b, nb=nb)
            assert got[1] == want[1] and np.array_equal(got[0], want[0])


def test_failures_name_the_step_of_the_unblocked_order():
    ms, bs = bref.random_systems(65, 1, seed=3)
    m = ms[0].copy()
    m[:, 40] = 0.0
    for solve in (nref.lu_solve, bref.blocked_lu_solve):
        with pytest.raises(nref.NlteSolveError) as e:
            solve(m, bs[0])
        assert e.value.step == 40
    m = ms[0].copy()
    m[50, 3] = np.nan
    steps = []
    for solve in (nref.lu_solve, bref.blocked_lu_solve):
        with pytest.raises(nref.NlteSolveError) as e:
            solve(m, bs[0])
        steps.append(e.value.step)
    assert steps[0] == steps[1] == 3  # NaN ranks above everything: it is the pivot of its column


def test_the_rate_matrices_of_a_261_level_species(oracle):
    prob, ld, pd, nd = nref.model(2, counts=LONG_COUNTS, species=LONG_SPECIES)
    j = oref.j_blues_dilute_blackbody(np.asarray(prob.opacity_state.line_list_nu, dtype=np.float64), pd.t_radiative, pd.dilution_factor)
    sizes, panels = set(), set()
    for pos, s, k0, n, m in nref.species_systems(pd, ld, nd, j, None):
        b = np.zeros(n)
        b[0] = 1.0
        want, want_swaps = nref.lu_solve(m, b)
        got, got_swaps = bref.blocked_lu_solve(m, b)
        assert got_swaps == want_swaps and np.array_equal(got, want)
        sizes.add(n)
        if n == 261:
            panels |= {k // bref.PANEL_COLUMNS for k in want_swaps}
    assert sizes == {22, 261} and len(panels) >= 3


def test_symbols_in_the_library_the_loader_and_the_header():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    for name in ("tardis_mc_nlte_solve_form", "tardis_mc_debug_nlte_solve"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
        assert re.search(r"\bint %s\(" % name, header)
    assert "nlte_blocked_levels" in header and "never summed first" in header
    assert _abi.NLTE_FORMS == ("lds", "global", "blocked")
    assert Engine.nlte_solve_form(141) == "lds" and Engine.nlte_solve_form(1) == "lds"
    assert [Engine.nlte_solve_path(n) for n in (141, 142, 1071)] == ["lds", "global", "global"]
    assert hasattr(Engine, "debug_nlte_solve")
