"""The yardstick of the device mean opacities (tardis_mc_mean_opacity): a serial NumPy restatement of the definition in
include/tardis_mc.h -- the expansion opacity in frequency bins of m lines, its Planck and Rosseland means with electron scattering, and
the optical depths summed from the surface inward -- every product, quotient and sum a rounding of its own.  exp is the transport's own
(oracle.exp_array(x, 1), which tests/test_hip_parity.py pins the device's mcm::exp to); every sum is serial from 0.0
(np.add.accumulate behind a row of zeros -- np.sum is pairwise along a contiguous axis and is wrong here).

``numpy_spelling`` is the plain spelling the restatement is compared with (libm exp, **-1, **2, nu**3, np.sum, np.cumsum): it agrees
to rounding, not bitwise.  Largest relative deviation of the four vectors measured on the models of tests/test_mean_opacity_host.py
(seeds 1-3, S = 3 and 20, L = 160 and 1601, m = 3, 10, 17): 8.5e-15, in kappa_rosseland and tau_rosseland (kappa_planck 7.0e-16);
test_restatement_against_plain_numpy asserts ten times that.  A single bin of the expansion opacity has no such bound: 1.0 - exp(-tau) of
thin lines cancels, and there the two exp decide (measured: 1.1e-10 of a bin whose lines have tau ~ 1e-6).

The problem builders are here too: ``model`` plants the cells the kernels can go wrong on."""
import numpy as np

from oracle import oracle

C_LIGHT, H_PLANCK, K_BOLTZMANN = 2.99792458e10, 6.62606957e-27, 1.3806488e-16  # tardis/constants.py (CODATA 2010, cgs)
SIGMA_THOMSON = 6.652458734e-25


def exp(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.asarray(oracle.exp_array(x.ravel(), 1)).reshape(x.shape)


def serial_sum(a, axis=0):
    """((0.0 + a[0]) + a[1]) + ... along ``axis``."""
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, 0)
    return np.add.accumulate(np.concatenate([np.zeros((1,) + a.shape[1:]), a]), axis=0)[-1]


def layout(n_lines, bin_size):
    """(e, n_bins) of L lines in bins of m."""
    e = bin_size - n_lines % bin_size
    return e, (n_lines + e) // bin_size


def padded(line_list_nu, bin_size):
    """p[0 .. L + e]: the pads 1.0 .. e + 1.0 Hz, then the list in ascending order."""
    nu = np.asarray(line_list_nu, dtype=np.float64)
    e, _ = layout(len(nu), bin_size)
    p = np.empty(len(nu) + e + 1)
    for j in range(e + 1):
        p[j] = j + 1
    p[e + 1:] = nu[::-1]
    return p


def bin_edges(line_list_nu, bin_size):
    """(low, dnu) [n_bins]."""
    p = padded(line_list_nu, bin_size)
    _, n_bins = layout(len(line_list_nu), bin_size)
    b = np.arange(n_bins)
    low, high = p[b * bin_size], p[(b + 1) * bin_size]
    return low, high - low


def mean_opacity(line_list_nu, tau_sobolev, electron_density, r_inner, r_outer, time_explosion, t_radiative, bin_size,
                 sigma_thomson=SIGMA_THOMSON, exp=exp):
    """The outputs of tardis_mc_mean_opacity: kappa_planck, kappa_rosseland, tau_planck, tau_rosseland [S], kappa_expansion [n_bins, S],
    bins_low, delta_nu [n_bins].  ``exp``: np.exp for the cost of the host pass with libm (tools/time_mean_opacity.py); not the yardstick."""
    nu = np.asarray(line_list_nu, dtype=np.float64)
    tau = np.asarray(tau_sobolev, dtype=np.float64)
    t = np.asarray(t_radiative, dtype=np.float64)
    n_e = np.asarray(electron_density, dtype=np.float64)
    L, S = tau.shape
    m = int(bin_size)
    e, n_bins = layout(L, m)
    low, dnu = bin_edges(nu, m)
    q = np.concatenate([np.zeros((e + 1, S)), tau[::-1]])  # q[j][s], 0 <= j <= L + e
    terms = (1.0 - exp(-q[1:])).reshape(n_bins, m, S)      # members b m + 1 .. (b+1) m of bin b
    x = serial_sum(terms, axis=1)
    ct = time_explosion * C_LIGHT
    kexp = ((low / dnu) / ct)[:, None] * x
    planck_coef = 2 * H_PLANCK / (C_LIGHT * C_LIGHT)
    beta = 1 / (K_BOLTZMANN * t)
    with np.errstate(all="ignore"):
        E = exp((H_PLANCK * low)[:, None] * beta[None, :])
        Em1 = E - 1
        B = (planck_coef * (low * low * low))[:, None] / Em1
        cn = C_LIGHT / low
        U = (((B * E) * B) * (cn * cn)[:, None]) / ((2 * K_BOLTZMANN) * (t * t))[None, :]
        bd, ud = B * dnu[:, None], U * dnu[:, None]
        kthom = n_e * sigma_thomson
        off = ~np.isfinite(E) | (Em1 == 0.0)
        pn = serial_sum(np.where(off, 0.0, bd * kexp))
        pd = serial_sum(np.where(off, 0.0, bd))
        rn = serial_sum(np.where(off, 0.0, ud * (1.0 / (kthom[None, :] + kexp))))
        rd = serial_sum(np.where(off, 0.0, ud))
        kappa_planck = kthom + pn / pd
        kappa_rosseland = 1.0 / (rn / rd)
    dr = np.asarray(r_outer, dtype=np.float64) - np.asarray(r_inner, dtype=np.float64)

    def inward(kappa):
        d = kappa * dr
        out = np.empty(S)
        out[S - 1] = d[S - 1]
        for s in range(S - 2, -1, -1):
            out[s] = out[s + 1] + d[s]
        return out

    return {"kappa_planck": kappa_planck, "kappa_rosseland": kappa_rosseland, "tau_planck": inward(kappa_planck),
            "tau_rosseland": inward(kappa_rosseland), "kappa_expansion": kexp, "bins_low": low, "delta_nu": dnu}


def numpy_spelling(line_list_nu, tau_sobolev, electron_density, r_inner, r_outer, time_explosion, t_radiative, bin_size,
                   sigma_thomson=SIGMA_THOMSON):
    """The same quantities spelt the plain way: padded arrays, strided slices, libm exp, ** and NumPy's own reductions."""
    nu = np.asarray(line_list_nu, dtype=np.float64)[::-1]
    tau = np.asarray(tau_sobolev, dtype=np.float64)[::-1]
    t = np.asarray(t_radiative, dtype=np.float64)
    L, S = tau.shape
    m = int(bin_size)
    extra = m - L % m
    nu_p = np.hstack([np.arange(1, extra + 2, dtype=np.float64), nu])
    tau_p = np.vstack([np.zeros((extra + 1, S)), tau])
    low, high = nu_p[:-m:m], nu_p[m::m]
    dnu = high - low
    x = (1 - np.exp(-tau_p[1:])).reshape(len(low), m, S).sum(axis=1)
    kexp = (low / dnu)[:, None] / (time_explosion * C_LIGHT) * x
    E = np.exp(H_PLANCK * low[:, None] / (K_BOLTZMANN * t[None, :]))
    B = 2 * H_PLANCK * low[:, None] ** 3 / C_LIGHT**2 / (E - 1)
    U = B**2 * E * (C_LIGHT / low[:, None]) ** 2 / (2 * K_BOLTZMANN * t[None, :] ** 2)
    kthom = np.asarray(electron_density, dtype=np.float64) * sigma_thomson
    kappa_planck = kthom + (B * dnu[:, None] * kexp).sum(axis=0) / (B * dnu[:, None]).sum(axis=0)
    kappa_rosseland = ((U * dnu[:, None] * (kthom[None, :] + kexp) ** -1).sum(axis=0) / (U * dnu[:, None]).sum(axis=0)) ** -1
    dr = np.asarray(r_outer, dtype=np.float64) - np.asarray(r_inner, dtype=np.float64)
    return {"kappa_planck": kappa_planck, "kappa_rosseland": kappa_rosseland,
            "tau_planck": np.cumsum((kappa_planck * dr)[::-1])[::-1], "tau_rosseland": np.cumsum((kappa_rosseland * dr)[::-1])[::-1],
            "kappa_expansion": kexp, "bins_low": low.copy(), "delta_nu": dnu}


def model(seed, n_shells, n_lines, plants=True, cold_shell=True, duplicate_run=0, duplicate_at=0):
    """A geometry, an opacity state (scatter mode: no macro-atom tables) and radiation temperatures, for the mean opacities.

    ``plants``: cells of exactly 0.0 (a whole line, and scattered cells), of 1e-20 and of 1e8, and one negative cell (-0.5).
    ``cold_shell``: the outermost shell at 300 K, where exp(h nu / (k_B t)) overflows in the bluest bins (above ~4e15 Hz).
    ``duplicate_run`` k > 1: lines duplicate_at .. duplicate_at + k - 1 of the ASCENDING list share one frequency.
    Returns (geometry, opacity_state, time_explosion, t_radiative)."""
    from tardis_amd import synthetic

    rng = np.random.default_rng(seed)
    geo = synthetic.make_geometry(n_shells)
    op = synthetic.make_opacity_state(seed, geo, n_lines, "scatter", log_tau_mean=-1.0)
    L, S = op.tau_sobolev.shape
    if duplicate_run > 1:
        asc = op.line_list_nu[::-1].copy()
        asc[duplicate_at:duplicate_at + duplicate_run] = asc[duplicate_at]
        op.line_list_nu = np.ascontiguousarray(asc[::-1])
    if plants:
        tau = op.tau_sobolev
        tau[rng.integers(0, L)] = 0.0
        cells = rng.integers(0, L * S, max(3, L * S // 10))
        kind = rng.integers(0, 3, len(cells))
        flat = tau.reshape(-1)
        flat[cells[kind == 0]] = 0.0
        flat[cells[kind == 1]] = 1e-20
        flat[cells[kind == 2]] = 1e8
        flat[rng.integers(0, L * S)] = -0.5
    t_rad = np.linspace(12000.0, 7000.0, S) if S > 1 else np.array([10000.0])
    if cold_shell:
        t_rad[S - 1] = 300.0
    return geo, op, geo.time_explosion, t_rad


def reference(geo, op, t_exp, t_rad, bin_size, sigma_thomson=SIGMA_THOMSON):
    return mean_opacity(op.line_list_nu, op.tau_sobolev, op.electron_density, geo.r_inner, geo.r_outer, t_exp, t_rad, bin_size, sigma_thomson)
