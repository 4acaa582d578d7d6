"""TEST INFRASTRUCTURE: an independent restatement of the reference's formal integral at higher precision, hand-derived closed
forms for one-shell models, and the edge model the host and GPU tests share.

reference() follows the structure of numba_formal_integral (tardis/spectrum/formal_integral/formal_integral_numba.py:375-560, with
populate_z :52-118, line_search :132-166 and base.py:13-16,105-120), not the C oracle: the intersection points of a ray are a dict
keyed by their index, the lines of a segment come from np.searchsorted on the negated line list, and the table positions are
(shell, line) pairs put together where they are used.

What decides which ray is followed is evaluated in float64 with exactly the reference's expressions -- p = p_idx * r_max / (N - 1),
z = 1 +- sqrt(r^2 - p^2) * C_INV * (1 / t), nu * z, t / C_INV * (1 - nu_line / nu): single correctly rounded IEEE operations, the
same on every side (in long double a ray could fall on the other side of a line on a tie, and another ray would be compared).
What accumulates is np.longdouble (x87 extended, 64-bit mantissa): exp(-tau), the black body (through expm1: same function, no
cancellation), the I += escat; I *= e; I += att recurrence, I * p and the trapezoid sum.

Out-of-range rule: Jblue_lu / Jred_lu read as 0 where the flat index is outside [0, S * L) -- the project's contract (the
reference would read past the end there)."""
import functools
import math

import numpy as np

C_INV = 3.33564e-11
KB_CGS = 1.3806488e-16
H_CGS = 6.62606957e-27
SIGMA_THOMSON = 6.652458734e-25
LD = np.longdouble
EPS = 2.0 ** -53  # half an ulp of a float64 in [1, 2): the unit of the derived bounds


def impact_parameter(p_idx, r_max, N):
    return float(p_idx) * float(r_max) / float(N - 1)


def _intersection(radius, p, inv_t):
    if radius > p:
        return math.sqrt(radius * radius - p * p) * C_INV * inv_t
    return 0.0


def intersection_points(r_inner, r_outer, time_explosion, p):
    """{index along the ray: (z, shell)}, float64.  A core ray (p <= r_inner[0]) leaves through every shell once; any other ray
    enters through the shells it reaches from the outermost inwards (z > 1) and leaves through them again (z < 1).  A shell
    whose intersection evaluates to 0 (p >= r_outer, the tangent ray included) is not reached."""
    inv_t = 1 / float(time_explosion)
    S = len(r_outer)
    ip = [_intersection(float(r), p, inv_t) for r in r_outer]
    if p <= float(r_inner[0]):
        return {i: (1 - ip[i], i) for i in range(S)}
    reached = [i for i in range(S) if ip[i] != 0]
    pts = {}
    for i in reversed(reached):
        pts[len(pts)] = (1 + ip[i], i)
    for i in reached:
        pts[len(pts)] = (1 - ip[i], i)
    return pts


def black_body(nu, t):
    """B_nu(T) of base.py:110-120 in long double, with expm1 for exp(x) - 1."""
    nu = np.asarray(nu, dtype=np.float64).astype(LD)
    x = LD(H_CGS) * nu / (LD(KB_CGS) * LD(t))
    return LD(2) * LD(H_CGS) * LD(C_INV) * LD(C_INV) * nu * nu * nu / np.expm1(x)


def reference(r_inner, r_outer, time_explosion, line_list_nu, tau_sobolev, electron_density, inner_temperature, frequencies,
              att_S_ul, Jred_lu, Jblue_lu, N):
    """(L_nu [n_nu], I_nu_p [n_nu, N], K_nu_p [n_nu, N]): luminosity densities and intensities (np.longdouble) and the number of
    resonances each ray crossed (int64)."""
    r_inner, r_outer = np.asarray(r_inner, dtype=np.float64), np.asarray(r_outer, dtype=np.float64)
    lines = np.asarray(line_list_nu, dtype=np.float64)
    tau = np.asarray(tau_sobolev, dtype=np.float64)
    freqs = np.asarray(frequencies, dtype=np.float64).ravel()
    L, S = tau.shape
    assert lines.shape == (L,) and len(r_inner) == S == len(r_outer) and N >= 2
    total = S * L
    t = float(time_explosion)
    neg_lines = -lines  # ascending: searchsorted(-x, "left") counts the lines with nu_line > x
    exp_tau = np.exp(-tau.T.astype(LD)).ravel()  # shell-major
    att = np.asarray(att_S_ul, dtype=np.float64).ravel().astype(LD)
    jred = np.asarray(Jred_lu, dtype=np.float64).ravel().astype(LD)
    jblue = np.asarray(Jblue_lu, dtype=np.float64).ravel().astype(LD)
    assert att.size == total and jred.size == total and jblue.size == total
    opacity = np.asarray(electron_density, dtype=np.float64).astype(LD) * LD(SIGMA_THOMSON)
    zero = LD(0)
    r_max = float(r_outer[-1])
    rays = [(p_idx, impact_parameter(p_idx, r_max, N)) for p_idx in range(1, N)]
    rays = [(p_idx, p, intersection_points(r_inner, r_outer, t, p)) for p_idx, p in rays]

    def table(a, flat):
        return a[flat] if 0 <= flat < total else zero

    I_nu_p = np.zeros((freqs.size, N), dtype=LD)
    K_nu_p = np.zeros((freqs.size, N), dtype=np.int64)
    for nu_idx, nu in enumerate(freqs.tolist()):
        with np.errstate(all="ignore"):
            line_end = t / C_INV * (1.0 - lines / nu)  # float64, per line
        for p_idx, p, pts in rays:
            if not pts:
                continue  # the ray touches no shell: 0
            zs = [pts[k][0] for k in range(len(pts))]
            shells = [pts[k][1] for k in range(len(pts))]
            I = black_body(nu * zs[0], inner_temperature) if p <= float(r_inner[0]) else zero
            bounds = np.searchsorted(neg_lines, [-(nu * z) for z in zs], side="left").tolist()
            start = LD(t / C_INV * (1.0 - zs[0]))
            line = red = bounds[0]
            first = True
            escat = zero
            crossed = 0
            for seg in range(len(pts) - 1):
                row = shells[seg] * L
                stop = max(bounds[seg + 1], line)
                for line in range(line, stop):
                    end = LD(line_end[line])
                    jb = table(jblue, row + line)
                    if first:
                        escat += (end - start) * opacity[shells[seg]] * (jb - I)
                        first = False
                    else:
                        escat += (end - start) * opacity[shells[seg]] * (LD(0.5) * (table(jred, row + red) + jb) - I)
                        red += 1
                    I += escat
                    I *= exp_tau[row + line]
                    I += att[row + line]
                    escat = zero
                    start = end
                    crossed += 1
                line = stop
                # electron scattering up to the shell boundary (added to I at the next resonance only)
                end = LD(t / C_INV * (1.0 - (nu * zs[seg + 1]) / nu))
                avg = LD(0.5) * (table(jred, row + red) + table(jblue, row + line))
                escat += (end - start) * opacity[shells[seg]] * (avg - I)
                start = end
            I_nu_p[nu_idx, p_idx] = I * LD(p)
            K_nu_p[nu_idx, p_idx] = crossed
    dx = LD(r_max) / LD(N)
    L_nu = LD(8) * LD(np.pi) ** 2 * (dx * (I_nu_p[:, 1:] + I_nu_p[:, :-1]) / LD(2)).sum(axis=1)
    return L_nu, I_nu_p, K_nu_p


def ray_bound(K):
    """The derived relative bound of a float64 evaluation of a ray with every term non-negative (electron_density == 0) against
    reference(): (4 K + 64) * 2^-53.  Per crossed line one exp, one product and one sum, each within an ulp, plus one ulp of
    slack; 64 for the black body, whose argument h nu / k T <= 8 carries about 4 roundings amplified by that factor, plus about
    12 further roundings."""
    return (4.0 * np.asarray(K, dtype=np.float64) + 64.0) * EPS


# ---- closed forms ---------------------------------------------------------------------------------------------------------

CLOSED_N = 9
CLOSED_T_INNER = 1.0e4
CLOSED_T_EXP = 1123200.0


def closed_form_model(n_lines, seed=0):
    """One shell r_inner = r_max / 2, r_outer = r_max = 2^51, n_e > 0, one or two lines, N = 9 (p_idx = 4 lands on r_inner), 65
    frequencies across the line(s).  The same keys as edge_model()."""
    assert n_lines in (1, 2)
    rng = np.random.default_rng(100 + seed)
    r_max = 2.0 ** 51
    lines = np.array([1.2e15, 1.19e15][:n_lines])
    tau = np.array([[0.7], [1.9]][:n_lines])
    bb = np.asarray(black_body(lines, CLOSED_T_INNER), dtype=np.float64)
    m = dict(r_inner=np.array([r_max / 2]), r_outer=np.array([r_max]), time_explosion=CLOSED_T_EXP, line_list_nu=lines,
             tau_sobolev=tau, electron_density=np.array([2.0e9]), inner_temperature=CLOSED_T_INNER,
             frequencies=np.linspace(lines[-1] * 0.9, lines[0] * 1.1, 65),
             att_S_ul=bb * 0.125 * rng.uniform(0.2, 1.2, n_lines) * (1 - np.exp(-tau[:, 0])),
             Jred_lu=bb * 0.125 * rng.uniform(0.5, 1.5, n_lines), Jblue_lu=bb * 0.125 * rng.uniform(0.5, 1.5, n_lines))
    return m


def closed_form_one_shell(m, N=CLOSED_N):
    """I_nu_p [n_nu, N] (long double) of a one-shell model with one or two lines, and the mask of the rays that cross a line.

    Derivation.  With one shell a core ray (p <= r_inner) has the single intersection point z0 = 1 - sqrt(r_max^2 - p^2) / (c t):
    there is no segment, so nothing is crossed and nothing scatters,  I = B_nu(nu z0) p.
    A ray outside the core has two points, z0 = 1 + s and z1 = 1 - s with s = sqrt(r_max^2 - p^2) / (c t), and one segment from
    the comoving frequency nu z0 down to nu z1.  It starts with I = 0 at d0 = c t (1 - z0).  A line is crossed iff
    nu z1 < nu_line <= nu z0, at d = c t (1 - nu_line / nu).
      First crossed line a:   I1 = (d_a - d0) n_e sigma_T (Jblue[a] - 0) e^-tau_a + att[a]
      (the scattering integral of the stretch before the line, with the blue-wing mean intensity of that line, is attenuated
      by the line and the line's own emission is added.)
      Second crossed line b:  I2 = (I1 + (d_b - d_a) n_e sigma_T (0.5 (Jred[a] + Jblue[b]) - I1)) e^-tau_b + att[b]
      (between two lines the mean intensity is the average of the red wing of the line behind and the blue wing of the line
      ahead: the red-wing position lags the blue one by one line.)
    The scattering of the stretch after the last line never reaches I.  The ray at p = r_max touches no shell: 0.  Every ray is
    multiplied by p; p_idx = 0 is 0."""
    lines, freqs = m["line_list_nu"], m["frequencies"]
    assert len(m["r_outer"]) == 1 and len(lines) in (1, 2)
    r_in, r_max, t = float(m["r_inner"][0]), float(m["r_outer"][0]), float(m["time_explosion"])
    op = LD(float(m["electron_density"][0])) * LD(SIGMA_THOMSON)
    e = np.exp(-m["tau_sobolev"][:, 0].astype(LD))
    att, jr, jb = (np.asarray(m[k], dtype=np.float64).astype(LD) for k in ("att_S_ul", "Jred_lu", "Jblue_lu"))
    I = np.zeros((len(freqs), N), dtype=LD)
    crossing = np.zeros((len(freqs), N), dtype=bool)
    for p_idx in range(1, N):
        p = impact_parameter(p_idx, r_max, N)
        if not r_max > p:
            continue
        s = math.sqrt(r_max * r_max - p * p) * C_INV * (1 / t)
        for k, nu in enumerate(freqs.tolist()):
            if p <= r_in:
                I[k, p_idx] = black_body(nu * (1 - s), m["inner_temperature"]) * LD(p)
                continue
            z0, z1 = 1 + s, 1 - s
            hit = [a for a in range(len(lines)) if nu * z1 < lines[a] <= nu * z0]
            if not hit:
                continue
            d0 = LD(t / C_INV * (1.0 - z0))
            d = [LD(t / C_INV * (1.0 - float(lines[a]) / nu)) for a in hit]
            a = hit[0]
            val = (d[0] - d0) * op * jb[a] * e[a] + att[a]
            if len(hit) == 2:
                b = hit[1]
                val = (val + (d[1] - d[0]) * op * (LD(0.5) * (jr[a] + jb[b]) - val)) * e[b] + att[b]
            I[k, p_idx] = val * LD(p)
            crossing[k, p_idx] = True
    return I, crossing


def closed_form_luminosity(I, r_max):
    """8 pi^2 times the trapezoid sum of the reference, dx = r_max / N, in long double."""
    N = I.shape[1]
    return LD(8) * LD(np.pi) ** 2 * (LD(r_max) / LD(N) * (I[:, 1:] + I[:, :-1]) / LD(2)).sum(axis=1)


# ---- the edge model -------------------------------------------------------------------------------------------------------

EDGE_N = (2, 3, 9, 17, 33)
EDGE_SEED = 11
TAU_ZERO_LINE, TAU_OPAQUE_LINE = 7, 11


def recipe_frequencies(line_list_nu, r_max, time_explosion):
    """The 129 frequencies of the edge model for a line list: one from which every line is out of reach bluewards (every ray
    starts behind the last line), one from which every line is out of reach redwards (nothing is crossed), and 127 evenly spaced
    from 0.9 nu[-1] to 1.1 nu[0]."""
    nu = np.asarray(line_list_nu, dtype=np.float64)
    z_max = 1 + float(r_max) / float(time_explosion) * C_INV
    return np.concatenate([[nu[-1] / z_max * 0.99, nu[0] * z_max * 1.01], np.linspace(0.9 * nu[-1], 1.1 * nu[0], 127)])


def edge_model(L, seed=EDGE_SEED, electrons=True):
    """Four shells whose radii are exact multiples of r_max / 8 = 2^48, so that for N = 9, 17, 33 impact parameters fall ON
    r_inner[0] and ON r_outer[0..2] (tangent rays); L lines with a duplicated pair and a triple, one transparent and one opaque
    line; 129 frequencies that include both out-of-reach ones.  ``electrons=False``: the variant with no electron scattering."""
    rng = np.random.default_rng(seed)
    S = 4
    r_max = 2.0 ** 51
    r_inner = r_max * np.array([4.0, 5.0, 6.0, 7.0]) / 8
    r_outer = r_max * np.array([5.0, 6.0, 7.0, 8.0]) / 8
    t, T = 1123200.0, 1.0e4
    nu = np.sort(rng.uniform(1.0e15, 1.3e15, L))[::-1].copy()
    nu[5] = nu[4]
    nu[19] = nu[20] = nu[18]
    assert (np.diff(nu) <= 0).all()
    tau = 10.0 ** rng.uniform(-3.0, 3.0 if L < 1000 else 1.0, (L, S))
    tau[TAU_ZERO_LINE] = 0.0
    tau[TAU_OPAQUE_LINE] = 800.0
    n_e = np.array([1.0e9, 0.0, 3.0e8, 1.0e8]) if electrons else np.zeros(S)
    bb = np.asarray(black_body(nu, T), dtype=np.float64)
    w = 0.5 * (r_inner[0] / r_outer) ** 2
    jblue = (bb[None, :] * w[:, None] * rng.uniform(0.5, 1.5, (S, L))).ravel()
    jred = (bb[None, :] * w[:, None] * rng.uniform(0.5, 1.5, (S, L))).ravel()
    att = (bb[None, :] * w[:, None] * rng.uniform(0.2, 1.2, (S, L)) * (1 - np.exp(-tau.T))).ravel()
    return dict(r_inner=r_inner, r_outer=r_outer, time_explosion=t, line_list_nu=nu, tau_sobolev=tau, electron_density=n_e,
                inner_temperature=T, frequencies=recipe_frequencies(nu, r_max, t), att_S_ul=att, Jred_lu=jred, Jblue_lu=jblue)


ARGS = ("r_inner", "r_outer", "time_explosion", "line_list_nu", "tau_sobolev", "electron_density", "inner_temperature",
        "frequencies", "att_S_ul", "Jred_lu", "Jblue_lu")


def call(fn, m, N, **replace):
    """fn(*the model's arrays in the order reference() and the oracle take them, N)."""
    m = dict(m, **replace)
    return fn(*(m[k] for k in ARGS), N)


# every (L, N, electrons) the edge tests run
EDGE_CASES = [(37, N, e) for N in EDGE_N for e in (True, False)] + [(2000, 17, True), (2000, 17, False)]


@functools.lru_cache(maxsize=None)
def edge_reference(L, N, electrons=True):
    """(model, (L_nu, I_nu_p, K_nu_p)) of an edge case, computed once per process; treat as read-only."""
    m = edge_model(L, EDGE_SEED, electrons)
    out = call(reference, m, N)
    for a in out:
        a.setflags(write=False)
    return m, out


def max_rel(a, b):
    """max |a - b| / |b| over b != 0 (long double)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    nz = b != 0
    return float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0
