"""The host side of the mean opacities (tardis_mc_mean_opacity): the bin layout of tardis_mc_mean_opacity_bins against the padded-array
spelling, its refusals, the rule of tardis_mc_mean_opacity_path, the serial restatement (tests/mean_opacity_ref.py) against a plain NumPy
spelling and on inputs with known answers, and estimate_v_inner.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mean_opacity_ref as ref  # noqa: E402
from tardis_amd import _abi, _lib  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402
from tardis_amd.transport import estimate_v_inner  # noqa: E402


def descending_list(n_lines, seed=5):
    rng = np.random.default_rng(seed)
    return np.sort(rng.uniform(1.5e14, 6e15, n_lines))[::-1].copy()


def padded_array_spelling(nu_desc, m):
    asc = nu_desc[::-1]
    extra = m - len(asc) % m
    nu_p = np.hstack([np.arange(1, extra + 2, dtype=np.float64), asc])
    return nu_p[:-m:m], nu_p[m::m]


@pytest.mark.parametrize("n_lines,m", [(160, 10), (161, 10), (169, 10), (7, 10), (7, 7), (7, 1), (10, 3), (1601, 17), (1, 1), (1, 4), (48, 16),
                                       (49, 16), (63, 16)])
def test_bin_layout_equals_the_padded_array_spelling(n_lines, m):
    assert n_lines % m in (0, 1, m - 1) or n_lines < m or m == 1 or (n_lines, m) == (1601, 17)
    nu = descending_list(n_lines)
    low, high = padded_array_spelling(nu, m)
    n_bins, first = Engine.mean_opacity_bins(nu, m)
    assert (n_bins, first) == (len(low), -1)
    e, n_ref = ref.layout(n_lines, m)
    assert 1 <= e <= m and n_ref == n_bins and n_bins * m == n_lines + e
    got_low, got_dnu = ref.bin_edges(nu, m)
    assert np.array_equal(got_low, low) and np.array_equal(got_dnu, high - low)
    assert low[0] == 1.0 and high[-1] == nu[0]
    p = ref.padded(nu, m)
    assert np.array_equal(p[:e + 1], np.arange(1, e + 2)) and np.array_equal(p[e + 1:], nu[::-1])


def test_refusals_of_the_layout_carry_their_message():
    nu = descending_list(160)
    for m in (0, -3):
        assert Engine.mean_opacity_bins(nu, m) == (_abi.ERR_INVALID_ARGUMENT, -1)
        assert "bin_size %d, it must be at least 1" % m in Engine.mean_opacity_bins_error()
    # the pads must lie below the list: e = 10 at L = 160, m = 10, so the pads reach 11 Hz
    low = nu.copy()
    low[-1] = 11.0
    assert Engine.mean_opacity_bins(low, 10) == (_abi.ERR_INVALID_ARGUMENT, -1)
    assert "does not lie above the 11 pads" in Engine.mean_opacity_bins_error()
    low[-1] = np.nextafter(11.0, 12.0)
    assert Engine.mean_opacity_bins(low, 10) == (16 + 1, -1)
    assert Engine.mean_opacity_bins(np.empty(0), 10)[0] == _abi.ERR_INVALID_ARGUMENT
    assert "no line list" in Engine.mean_opacity_bins_error()


def test_duplicate_lines_on_two_consecutive_edges_are_refused_elsewhere_accepted():
    L, m = 160, 3
    e, n_bins = ref.layout(L, m)
    assert e == 2
    asc = descending_list(L)[::-1].copy()
    # four equal lines at ascending 30 .. 33 are padded members 33 .. 36: both edges of bin 11
    dup = asc.copy()
    dup[30:34] = dup[30]
    low, high = padded_array_spelling(dup[::-1].copy(), m)
    assert np.flatnonzero(high - low == 0.0).tolist() == [11]
    assert Engine.mean_opacity_bins(dup[::-1].copy(), m) == (_abi.ERR_INVALID_ARGUMENT, 11)
    msg = Engine.mean_opacity_bins_error()
    assert "bin 11 of %d has width 0 at bin_size 3" % n_bins in msg
    # the first of two degenerate bins is the one named
    dup2 = dup.copy()
    dup2[60:64] = dup2[60]
    assert Engine.mean_opacity_bins(dup2[::-1].copy(), m) == (_abi.ERR_INVALID_ARGUMENT, 11)
    # one line further the run covers one edge only; and at m = 4 no two edges
    off = asc.copy()
    off[31:35] = off[31]
    assert Engine.mean_opacity_bins(off[::-1].copy(), m) == (n_bins, -1)
    assert Engine.mean_opacity_bins(dup[::-1].copy(), 4)[1] == -1
    # m = 1: every pair of equal neighbours is a bin of width 0
    pair = asc.copy()
    pair[100] = pair[99]
    assert Engine.mean_opacity_bins(pair[::-1].copy(), 1) == (_abi.ERR_INVALID_ARGUMENT, 100 + 1)
    assert Engine.mean_opacity_bins(pair[::-1].copy(), 2) == (ref.layout(L, 2)[1], -1)


def test_reduction_form_rule():
    lib = _lib.lib()
    assert [lib.tardis_mc_mean_opacity_path(n) for n in (0, 1, 15)] == [0, 0, 0]
    assert [lib.tardis_mc_mean_opacity_path(n) for n in (16, 17, 1024, 10**7)] == [1, 1, 1, 1]
    assert Engine.mean_opacity_path(15) == "lane" and Engine.mean_opacity_path(16) == "row"


def test_symbols_are_listed():
    for name in ("tardis_mc_mean_opacity", "tardis_mc_mean_opacity_bins", "tardis_mc_last_mean_opacity_ms", "tardis_mc_mean_opacity_path"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)


def ulp_distance(a, b):
    return np.abs(np.asarray(a).view(np.int64) - np.asarray(b).view(np.int64))


@pytest.mark.parametrize("sigma", [ref.SIGMA_THOMSON, 1e-200])
def test_all_tau_zero_gives_thomson_opacity(oracle, sigma):
    geo, op, t_exp, t_rad = ref.model(1, 3, 160, plants=False, cold_shell=True)
    op.tau_sobolev[:] = 0.0
    out = ref.reference(geo, op, t_exp, t_rad, 10, sigma)
    kthom = op.electron_density * sigma
    assert np.array_equal(out["kappa_expansion"], np.zeros((17, 3)))
    assert np.array_equal(out["kappa_planck"], kthom)
    # rn = sum ud (1 / kthom), rd = sum ud: 1 / (rn / rd) is kthom up to the roundings of the two sums, the quotient and the reciprocals
    assert ulp_distance(out["kappa_rosseland"], kthom).max() <= 4
    dr = geo.r_outer - geo.r_inner
    assert out["tau_planck"][2] == kthom[2] * dr[2] and out["tau_planck"][0] == (kthom[2] * dr[2] + kthom[1] * dr[1]) + kthom[0] * dr[0]


MODELS = [(seed, S, L, m) for seed in (1, 2, 3) for S, L in ((3, 160), (20, 1601)) for m in (3, 10, 17)]


def test_restatement_against_plain_numpy(oracle):
    """Measured: the largest relative deviation of the four vectors over these models, 8.5e-15, is written in the docstring of
    mean_opacity_ref.py and in the header; ten times that figure is asserted, and no looser than 1e-10.  A single bin of the expansion
    opacity has no relative bound -- 1.0 - exp(-tau) of thin lines cancels, and the two exp differ by up to an ulp of 1.0 each from the
    true value -- so it is held to that: m members times 2**-52, scaled as kexp is, plus the same relative figure."""
    worst = 0.0
    for seed, S, L, m in MODELS:
        geo, op, t_exp, t_rad = ref.model(seed, S, L, plants=True, cold_shell=False)
        op.tau_sobolev[op.tau_sobolev < 0.0] = 0.25  # (the plain spelling has no trouble with it; a negative kexp next to kthom cancels, which is no rounding test)
        args = (op.line_list_nu, op.tau_sobolev, op.electron_density, geo.r_inner, geo.r_outer, t_exp, t_rad, m)
        got, plain = ref.mean_opacity(*args), ref.numpy_spelling(*args)
        assert np.array_equal(got["bins_low"], plain["bins_low"]) and np.array_equal(got["delta_nu"], plain["delta_nu"])
        for name in ("kappa_planck", "kappa_rosseland", "tau_planck", "tau_rosseland"):
            assert np.all(np.isfinite(got[name])) and np.all(plain[name] > 0.0), name
            worst = max(worst, np.max(np.abs(got[name] - plain[name]) / plain[name]))
        kexp, kexp_plain = got["kappa_expansion"], plain["kappa_expansion"]
        bound = ((got["bins_low"] / got["delta_nu"]) / (t_exp * ref.C_LIGHT))[:, None] * (m * 2.0**-52) + 10 * 8.5e-15 * np.abs(kexp_plain)
        assert np.all(np.isfinite(kexp)) and np.all(np.abs(kexp - kexp_plain) <= bound)
    print("mean opacity restatement vs plain NumPy: largest relative deviation of the four vectors %.3g" % worst)  # (pytest -s shows it)
    assert worst <= 10 * 8.5e-15 <= 1e-10


def test_cold_shell_bins_contribute_zero(oracle):
    geo, op, t_exp, t_rad = ref.model(2, 3, 160)
    assert t_rad[2] == 300.0
    out = ref.reference(geo, op, t_exp, t_rad, 3)
    with np.errstate(over="ignore"):
        E = np.exp(ref.H_PLANCK * out["bins_low"] / (ref.K_BOLTZMANN * 300.0))
    assert 0 < np.isinf(E).sum() < len(E)
    for name in ("kappa_planck", "kappa_rosseland", "tau_planck", "tau_rosseland", "kappa_expansion"):
        assert np.all(np.isfinite(out[name])), name
    # the overflowing bins are out of the sums: the shell's means are those of the list cut below them
    keep = int(np.flatnonzero(np.isinf(E))[0])
    cut = ref.mean_opacity(op.line_list_nu[-(keep * 3 - ref.layout(160, 3)[0]):], op.tau_sobolev[-(keep * 3 - ref.layout(160, 3)[0]):],
                           op.electron_density, geo.r_inner, geo.r_outer, t_exp, t_rad, 3)
    assert len(cut["bins_low"]) == keep and np.array_equal(cut["bins_low"], out["bins_low"][:keep])
    assert cut["kappa_planck"][2] == out["kappa_planck"][2] and cut["kappa_rosseland"][2] == out["kappa_rosseland"][2]
    assert (op.tau_sobolev < 0).sum() == 1 and (op.tau_sobolev == 0).sum() > 3 and (op.tau_sobolev == 1e8).sum() > 3


def test_reversing_the_shells_reverses_both_kappa(oracle):
    geo, op, t_exp, t_rad = ref.model(3, 20, 1601)
    a = ref.mean_opacity(op.line_list_nu, op.tau_sobolev, op.electron_density, geo.r_inner, geo.r_outer, t_exp, t_rad, 10)
    b = ref.mean_opacity(op.line_list_nu, op.tau_sobolev[:, ::-1], op.electron_density[::-1], geo.r_inner, geo.r_outer, t_exp, t_rad[::-1], 10)
    for name in ("kappa_planck", "kappa_rosseland"):
        assert np.array_equal(a[name][::-1], b[name]), name
    assert np.array_equal(a["kappa_expansion"][:, ::-1], b["kappa_expansion"])
    assert not np.array_equal(a["tau_planck"][::-1], b["tau_planck"])


def test_estimate_v_inner_on_a_hand_made_profile():
    v = np.array([1.0e9, 1.2e9, 1.4e9, 1.6e9])
    tau = np.exp(np.array([2.0, 1.0, 0.0, -1.0]))  # ln tau falls by one per shell
    x = np.log(tau)[::-1]
    y = v[::-1]
    for target, hi in ((np.exp(0.5), 2), (1.0, 1), (2.0 / 3.0, 1), (np.exp(-3.0), 1), (np.exp(5.0), 3)):  # (x = -1, 0, 1, 2)
        xn = np.log(target)
        assert hi == int(np.clip(np.searchsorted(x, xn, side="left"), 1, 3))
        want = (y[hi] - y[hi - 1]) / (x[hi] - x[hi - 1]) * (xn - x[hi - 1]) + y[hi - 1]
        assert estimate_v_inner(tau, v, target) == want
    assert abs(estimate_v_inner(tau, v, np.exp(0.5)) - 1.3e9) < 1.0
    assert abs(estimate_v_inner(tau, v, np.exp(-3.0)) - 2.0e9) < 10.0  # extrapolated outward
    assert estimate_v_inner(tau, v) == estimate_v_inner(tau, v, 2.0 / 3.0)
    # shells without a positive finite depth are left out
    holes = np.array([np.inf, np.e, 1.0, 0.0, np.nan, -1.0])
    vv = np.array([9.0, 1.0, 2.0, 8.0, 7.0, 6.0])
    assert estimate_v_inner(holes, vv, np.exp(0.5)) == (1.0 - 2.0) / (1.0 - 0.0) * (0.5 - 0.0) + 2.0
    with pytest.raises(ValueError, match="at least two shells"):
        estimate_v_inner(np.array([1.0, 0.0, np.nan]), np.array([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError):
        estimate_v_inner(np.array([1.0, 2.0]), np.array([1.0, 2.0, 3.0]))
