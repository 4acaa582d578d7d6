"""NumPy restatement of the reference's ``interpolate_shells`` (FormalIntegralSolver / interpolate_integrator_quantities in
tardis/spectrum/formal_integral/): the integrator's grid, linear interpolation with extrapolation clipped at zero for the source
function, nearest-shell values for tau_sobolev and the electron density.  Every expression is written out in the order scipy's
interp1d evaluates it, so that the result is scipy's bit for bit (tests/test_formal_interpolate_host.py) and the device can be
held to equality (tests/test_formal_interpolate_gpu.py).  Test infrastructure only."""
import numpy as np


def grid(r_inner, r_outer, n_points):
    """The grid of ``interpolate_shells = n_points`` and the interpolation maps: dict of r_inner, r_outer [S'], the old and new
    midpoints x [S], xn [S'], and the source shells lo, hi, near [S']."""
    r_inner, r_outer = np.asarray(r_inner, dtype=np.float64), np.asarray(r_outer, dtype=np.float64)
    S = len(r_inner)
    x = (r_inner + r_outer) / 2.0
    r = np.linspace(r_inner[0], r_outer[-1], int(n_points))
    r_inner_i, r_outer_i = r[:-1], r[1:]
    xn = (r_inner_i + r_outer_i) / 2.0
    hi = np.clip(np.searchsorted(x, xn, side="left"), 1, S - 1)
    near = np.searchsorted((x[1:] + x[:-1]) / 2.0, xn, side="left")
    return {"r_inner": r_inner_i.copy(), "r_outer": r_outer_i.copy(), "x": x, "xn": xn, "lo": hi - 1, "hi": hi, "near": near}


def linear_unclipped(y, g):
    """y [S, ...] -> [S', ...]: interp1d(x, y, axis=0, fill_value="extrapolate")(xn), before the clip."""
    y = np.asarray(y, dtype=np.float64)
    lo, hi, x, xn = g["lo"], g["hi"], g["x"], g["xn"]
    shape = (-1,) + (1,) * (y.ndim - 1)
    slope = (y[hi] - y[lo]) / (x[hi] - x[lo]).reshape(shape)
    return slope * (xn - x[lo]).reshape(shape) + y[lo]


def linear_clipped(y, g):
    return np.maximum(linear_unclipped(y, g), 0.0)


def nearest(y, g):
    """y [S, ...] -> [S', ...]: interp1d(x, y, axis=0, kind="nearest", fill_value="extrapolate")(xn)."""
    return np.asarray(y)[g["near"]]


def interpolate_source(r_inner, r_outer, n_points, tau_sobolev, electron_density, att_S_ul, Jred_lu, Jblue_lu, e_dot_u=None):
    """The eight arrays of Engine.interpolated_source: tau_sobolev [L, S] (as the opacity state holds it), electron_density [S],
    att_S_ul / Jred_lu / Jblue_lu [S * L] flat shell-major, e_dot_u [levels, S] or None."""
    g = grid(r_inner, r_outer, n_points)
    S = len(g["x"])
    out = {"r_inner": g["r_inner"], "r_outer": g["r_outer"], "electron_density": nearest(electron_density, g),
           "tau_sobolev": nearest(np.asarray(tau_sobolev).T, g).ravel()}
    for key, y in (("att_S_ul", att_S_ul), ("Jred_lu", Jred_lu), ("Jblue_lu", Jblue_lu)):
        out[key] = linear_clipped(np.asarray(y).reshape(S, -1), g).ravel()
    out["e_dot_u"] = None if e_dot_u is None else np.ascontiguousarray(linear_clipped(np.asarray(e_dot_u).T, g).T)
    return out
