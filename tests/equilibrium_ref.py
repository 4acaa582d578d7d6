"""The outside anchor of the device plasma chain: a consistent atom, and mpmath references (40 digits) written from the physics and
the CODATA 2010 constants, not from the operation order of include/tardis_mc.h.  The NumPy restatements under tests/*_ref.py pin the
device bit for bit, but they were written from the same paragraphs as the kernels: a convention both share (g_l / g_u the wrong way
round, the ion in place of the upper ion, beta_rad for beta_e, a wrong literal) passes them.  In strict thermodynamic equilibrium --
W = 1, link_t_rad_t_electron = 1, a Planckian J, line frequencies that equal the level-energy differences -- every stage has a closed
form, and away from it every table is a quadrature that mpmath evaluates.

THE ATOM (atom()).  Two elements, ions of (6, 17, 1) and (70, 5, 2, 1) levels; closed shells keep one level.  Level energies rise from
0 with gaps of at least MIN_GAP_EV; weights 2J + 1.  Lines run between two levels of one ion: the ladder (k, k + 1) and random other
pairs, so every ion of three or more levels has cycles; nu = (E_u - E_l) / h, the line list is these nu sorted descending, f_lu is
log-uniform over four decades.  NlteData (A_ul, B_ul, B_lu) is computed from those nu, NlteCollisionData takes delta_e and g_ratio from
the same levels.  Continuum blocks are hydrogenic, x = x0 (nu0 / nu)^3 on geometric grids from the threshold (chi - E_k) / h, on levels
of charge 0, 1 and 2.  The OpacityState is hand-built around that line list with the scatter-mode dummies for the macro-atom topology.
S = 5 shells, t_rad 5000 .. 25000 K.  assert_conditions() asserts, on the CPU, what the bounds below need of it.

THE CONSTANTS are those of tardis/constants.py (CODATA 2010, cgs) as decimal strings; e = 4.80320451e-10 esu, the nine digits
include/tardis_mc.h states for FF_OPAC_CONST (1.602176565e-19 C times c / 10 is 4.8032045057e-10).  The atom's sobolev_coefficient and
Einstein coefficients are formed with the same e.  C0_FF = 1.426e-27 (FreeFreeCoolingRate) and 1.55e13 (Seaton) are literature
literals with a Gaunt factor inside, not functions of CODATA: they are taken as given; c0_ff_hydrogenic() shows that the first is the
physical constant (2^5 pi e^6 / (3 h m_e c^3)) sqrt(2 pi k_B / (3 m_e)) times a Gaunt factor within 1e-3 of 1.

THE BOUNDS.  u = 2^-53 is the relative error of one rounding; a decimal constant's double is one more.  The transport's exp is correctly
rounded on normal results (profiles/portable_math.txt), so exp(a') with a' = a (1 + r u) is exp(a) (1 + (|a| r + 1) u).  Every bound below
is such a count, first order in u, with generous integer slack; every one is asserted < CAP_TABLES = 1e-12 by assert_conditions(),
which is a condition on the atom, not a measurement.
  a = (h nu) beta or E beta with beta = 1 / (k_B T) carries r = 4 (k_B, the product, the quotient, the product; h one more: 5).
  exp_err(a) = (5 |a| + 1) u                                                            exp of such an argument
  lbf_err    = exp_err(X_E) + 2 u                                                       g exp(-E / kT)
  z_err      = lbf_err + n_max u                                                        a serial sum of n positive terms
  g_e: x = ((2 pi m_e) / beta) / (h h), g_e = x sqrt(x): 12 roundings in x, 1.5 x 12 + 2 = 20 u
  saha_err   = 2 z_err + 20 u + exp_err(X_chi) + 4 u                                    (Z_up / Z) (2 g_e exp(-chi / kT))
  ion-ratio  = saha_err + 8 u          n_up n_e / n_i on the device's tables: pe = phi / n_e, the running product, n_0 cp, twice
  boltzmann  = 2 lbf_err + 6 u         n_k / n_0 inside an ion: (lbf / Z) n_ion, twice, and the quotient
  sum        = (I_e + 6) u             the ions of an element add up to its density: 1 + sum cp, the quotient, the products
  phi_ik     = saha_err + lbf_err + z_err + 4 u
  planck_err(a) = (5 a + 8 + 2 / a) u                  2 h nu^3 / c^2 / (exp(a) - 1): the subtraction magnifies exp's error by 1 / (1 - e^-a)
                                                       <= 1 + 1 / a, hence the 1 / a term; a >= A_MIN is a condition on the atom
  point_err  = planck_err + exp_err + 12 u             the three integrands: y_sp has no Planck factor, y_st both
  trapezoid  = (n + 2) 2^-52 + point_err               relative to the sum of the terms' magnitudes; the integrands are positive,
                                                       so that is the integral itself
  milne      = 3 trapezoid + 3 phi_ik + 12 u           gamma_corr n_i - alpha_sp n_up n_e with alpha = T phi_ik, relative to gamma n_i (the
                                                       difference cancels)
  chi_bf     = exp_err(A_MAX) + ion-ratio + 8 u        (n_i - n_lte bfp) x, relative to n_i x (the difference cancels)
  coll_ion   = exp_err(A_MAX) + 12 u                   Seaton's closed form
  chi_ff     = exp_err(a) / a' + 24 u  with a' = min(a, 1): 1 - exp(-a) cancels below a = 1; sum over the ions adds I u
  cool_ff    = (I + 10) u
  sef        = 2 lbf_err + 8 u                         1 - (g_l n_u) / (g_u n_l) against 1 - exp(-h nu / kT), relative to 1: the
                                                       minuend's magnitude (the difference cancels for a line between close levels)
  tau        = sef (absolute in units of tau / sef) + 8 u ;  j_blues = planck_err(a_line) + 4 u
  beta       = tau's error relative to tau itself, that is the tau bound over sef (|tau beta' / beta| <= 1; this is why the lines' gaps
               are at least MIN_GAP_EV), + 4 u, and per branch: tau > 1e3: exp(-tau) < 1e-434, nothing; 1e-4 <= tau: 2^-54 / tau
               (exp(-tau) rounds by at most 2^-54 absolute and the subtraction adds one rounding, counted in the 4 u); tau < 1e-4: the
               truncation tau^2 / 6 of 1 - tau / 2.  So a thin line with tau above 2.4e-6 misses the cap: the atom has no thin line.
The NLTE solve has no tight bound (the matrices' condition numbers reach 1e9 and more): the device is held to 4 x the restatement's
own measured distance from Boltzmann, per species, and that bound is asserted < CAP_NLTE = 1e-10."""
import os
import sys
from types import SimpleNamespace

import mpmath
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tardis_amd import state as st, synthetic  # noqa: E402

mp = mpmath.mp.clone()  # (a context of its own: nothing else's precision changes)
mp.dps = 40

CODATA = {"k_B": "1.3806488e-16", "h": "6.62606957e-27", "m_e": "9.10938291e-28", "c": "2.99792458e10", "e": "4.80320451e-10",
          "eV": "1.602176565e-12"}
K_B, H, M_E, C, E_ESU = (mp.mpf(CODATA[k]) for k in ("k_B", "h", "m_e", "c", "e"))
PI = mp.pi
C0_FF = mp.mpf("1.426e-27")
SEATON = mp.mpf("1.55e13")
F64 = {k: float(v) for k, v in CODATA.items()}
EV = F64["eV"]
SOBOLEV_COEFFICIENT = np.pi * F64["e"] ** 2 / (F64["m_e"] * F64["c"])
EINSTEIN_COEFFICIENT = 4.0 * np.pi ** 2 * F64["e"] ** 2 / (F64["h"] * F64["m_e"] * F64["c"])

U = 2.0 ** -53
CAP_TABLES, CAP_NLTE = 1e-12, 1e-10
ION_ZERO = 1e-20

LEVELS = ((6, 17, 1), (70, 5, 2, 1))
CHI_EV = ((4.0, 6.0, 0.0), (12.0, 5.0, 6.5, 0.0))
T_RAD = np.array([5000.0, 9000.0, 13000.0, 19000.0, 25000.0])
W_EQUILIBRIUM = np.ones(5)
W_DILUTE = np.array([0.5, 0.35, 0.2, 0.1, 0.05])
LINK_TWO_TEMPERATURE = 0.9
DENSITY = 1e17 * np.array([1.0, 0.6, 0.4, 0.25, 0.15])
ABUNDANCE = np.array([0.3, 0.7])
TIME_EXPLOSION = 40 * 86400.0
MIN_GAP_EV = 0.11  # 0.05 k_B T at 25000 K: no line's 1 - exp(-h nu / kT) lies below 0.048 (beta's bound)
A_MIN, A_MAX = 0.1, 30.0  # h nu / kT of every continuum point
# continua: (ion, local level, block length); charges 0 (ions 0, 3), 1 (ions 1, 4) and 2 (ion 5); lengths that are no multiple of a
# row or a wave, and 65 / 129 for the quadrature's convergence
CONTINUA = ((0, 0, 17), (0, 3, 2), (0, 5, 33), (1, 0, 65), (1, 9, 3), (1, 16, 16), (3, 40, 129), (3, 55, 9), (3, 69, 64), (4, 0, 12),
            (4, 4, 5), (5, 0, 40), (5, 1, 7))
SPAN = 1.7
NLTE_SPECIES = (2, 5, 1, 3)  # the ions of 1, 2, 17 and 70 levels
COLLISION_FRACTIONS = (0.0, 1.0, 0.4, 1.0)


def _levels(rng, n, top_ev):
    """n energies [erg] from 0 to ``top_ev``, ascending, every gap at least MIN_GAP_EV."""
    if n == 1:
        return np.zeros(1)
    gaps = rng.random(n - 1) ** 2 + 0.05
    gaps = MIN_GAP_EV + gaps * ((top_ev - (n - 1) * MIN_GAP_EV) / gaps.sum())
    return np.concatenate(([0.0], np.cumsum(gaps))) * EV


def atom(link=1.0, seed=7):
    """The model: a namespace of pd (PlasmaData, with ``link``), ld (LineData), nd (NlteData), col (NlteCollisionData), cd
    (ContinuumData), op (OpacityState), geometry, time_explosion, cfg, grid, t_rad, and ion (the ion of every level)."""
    rng = np.random.default_rng(seed)
    counts = np.array([n for e in LEVELS for n in e])
    chi = np.array([c for e in CHI_EV for c in e]) * EV
    I, K, S = len(counts), int(counts.sum()), len(T_RAD)
    ion_level_edge = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    element_ion_edge = np.concatenate(([0], np.cumsum([len(e) for e in LEVELS]))).astype(np.int64)
    ion_charge = np.concatenate([np.arange(len(e), dtype=np.float64) for e in LEVELS])
    level_energy = np.concatenate([_levels(rng, n, 0.9 * c / EV if c > 0 else 1.0) for n, c in zip(counts, chi)])
    level_g = 2.0 * rng.integers(0, 6, K) + 1.0
    meta = np.zeros(K, dtype=np.int32)
    meta[ion_level_edge[:-1]] = 1
    meta[ion_level_edge[:-1][counts > 3] + 1] = 1
    ion = np.repeat(np.arange(I), counts)
    # lines
    lower, upper = [], []
    for a, n in zip(ion_level_edge[:-1], counts):
        pairs = {(k, k + 1) for k in range(n - 1)}
        if n >= 3:
            want = len(pairs) + min(n * (n - 1) // 2 - (n - 1), 2 * n)
            while len(pairs) < want:
                p, q = sorted(rng.integers(0, n, 2))
                if p != q:
                    pairs.add((int(p), int(q)))
        for p, q in sorted(pairs):
            lower.append(a + p)
            upper.append(a + q)
    lower, upper = np.array(lower, dtype=np.int64), np.array(upper, dtype=np.int64)
    nu = (level_energy[upper] - level_energy[lower]) / F64["h"]
    order = np.argsort(-nu, kind="stable")
    lower, upper, nu = lower[order], upper[order], nu[order]
    L = len(nu)
    f_lu = 10.0 ** rng.uniform(-4.0, 0.0, L)
    zeros = np.zeros(1, dtype=np.int64)
    n_e0 = 0.5 * DENSITY
    op = st.OpacityState(n_e0, link * T_RAD, nu, np.zeros((L, S)), np.zeros((1, S)), zeros, zeros, zeros, zeros, zeros)
    ld = synthetic.LineData(f_lu, F64["c"] / nu, level_g[lower], level_g[upper], lower, upper, K, None, float(SOBOLEV_COEFFICIENT),
                            np.zeros((K, S)), n_e0.copy(), T_RAD.copy(), W_EQUILIBRIUM.copy())
    zeta_t = np.arange(2000.0, 40001.0, 2000.0)
    centre, width = rng.uniform(5000.0, 30000.0, I), rng.uniform(4000.0, 15000.0, I)
    zeta = 0.05 + 0.9 / (1.0 + np.exp((zeta_t[None, :] - centre[:, None]) / width[:, None]))
    pd = synthetic.PlasmaData(level_energy, level_g, meta, ion_level_edge, element_ion_edge, ion_charge, chi, zeta_t, zeta,
                              ABUNDANCE[:, None] * DENSITY[None, :], float(synthetic.CHI_0_CA_II), float(link), np.array([20, 26]), T_RAD.copy(),
                              W_EQUILIBRIUM.copy())
    # NLTE data: every line of a species' ion, in line-list order
    ids, line_edge = [], [0]
    for i in NLTE_SPECIES:
        own = np.flatnonzero(ion[lower] == i)
        ids.append(own)
        line_edge.append(line_edge[-1] + len(own))
    line_id = np.concatenate(ids).astype(np.int64)
    b_lu = EINSTEIN_COEFFICIENT * f_lu[line_id] / nu[line_id]
    b_ul = b_lu * ld.g_lower[line_id] / ld.g_upper[line_id]
    a_ul = (2.0 * F64["h"] * nu[line_id] ** 3 / F64["c"] ** 2) * b_ul
    nd = synthetic.NlteData(np.array(NLTE_SPECIES, dtype=np.int64), np.array(line_edge, dtype=np.int64), line_id, a_ul, b_ul, b_lu)
    # collisions: c n_e among the radiative rates (the median A_ul over the median electron density)
    col = synthetic.make_nlte_collision_data(seed, pd, nd, pair_fraction=COLLISION_FRACTIONS, magnitude=float(np.median(a_ul) / np.median(n_e0)),
                                             t_min=4000.0, t_max=30000.0)
    # continua
    level = np.array([ion_level_edge[i] + k for i, k, _ in CONTINUA], dtype=np.int64)
    lengths = np.array([n for _, _, n in CONTINUA], dtype=np.int64)
    c_nu, c_x = [], []
    for k, n in zip(level, lengths):
        nu_i = (chi[ion[k]] - level_energy[k]) / F64["h"]
        grid = nu_i * np.geomspace(1.0, SPAN, int(n))
        grid[0] = nu_i
        x0 = 6.3e-18 * 10.0 ** rng.normal(0.0, 0.3)
        c_nu.append(grid)
        c_x.append(x0 * (nu_i / grid) ** 3)
    cd = synthetic.ContinuumData(level, np.concatenate(([0], np.cumsum(lengths))).astype(np.int64), np.concatenate(c_nu), np.concatenate(c_x))
    cfg = st.MonteCarloConfiguration()
    cfg.LINE_INTERACTION_TYPE = st.LINE_INTERACTION_TYPES["scatter"]
    geometry = synthetic.make_geometry(S, time_explosion=TIME_EXPLOSION)
    return SimpleNamespace(pd=pd, ld=ld, nd=nd, col=col, cd=cd, op=op, geometry=geometry, time_explosion=TIME_EXPLOSION, cfg=cfg,
                           grid=synthetic.make_spectrum_grid(100), t_rad=T_RAD.copy(), ion=ion, nu=nu, n_e0=n_e0)


# ---- mpmath references --------------------------------------------------------------------------------------------------------------------

def mpf(a):
    """A float64 array as an object array of mpf, exactly."""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = mp.mpf(float(a[idx]))
    return out


def rel(got, want, scale=None):
    """max |got - want| / |scale| (scale None: want), got float64, want and scale mpf arrays; as a float."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=object)
    scale = want if scale is None else np.broadcast_to(np.asarray(scale, dtype=object), want.shape)
    assert got.shape == want.shape, (got.shape, want.shape)
    worst = mp.mpf(0)
    for idx in np.ndindex(want.shape):
        assert np.isfinite(got[idx]) and scale[idx] != 0, idx
        worst = max(worst, abs((mp.mpf(float(got[idx])) - want[idx]) / scale[idx]))
    return float(worst)


def boltzmann(pd, t):
    """g_k exp(-E_k / (k_B T_s)) [K, S]."""
    e, g = mpf(pd.level_energy), mpf(pd.level_g)
    return np.array([[g[k] * mp.exp(-e[k] / (K_B * mp.mpf(float(ts)))) for ts in t] for k in range(len(e))], dtype=object)


def partition(pd, lbf):
    edge = pd.ion_level_edge
    return np.array([[mp.fsum(lbf[a:b, s]) for s in range(lbf.shape[1])] for a, b in zip(edge[:-1], edge[1:])], dtype=object)


def last_ions(pd):
    last = np.zeros(len(pd.ion_charge), dtype=bool)
    last[np.asarray(pd.element_ion_edge[1:]) - 1] = True
    return last


def saha(pd, t, z=None):
    """n_{i+1} n_e / n_i = (2 Z_{i+1} / Z_i) (2 pi m_e k_B T / h^2)^(3/2) exp(-chi_i / (k_B T)) [I, S]; None for an element's last ion."""
    z = partition(pd, boltzmann(pd, t)) if z is None else z
    chi, last = mpf(pd.ionization_energy), last_ions(pd)
    out = np.full(z.shape, None, dtype=object)
    for i in range(len(chi)):
        if last[i]:
            continue
        for s, ts in enumerate(t):
            kt = K_B * mp.mpf(float(ts))
            out[i, s] = (2 * z[i + 1, s] / z[i, s]) * (2 * PI * M_E * kt / H ** 2) ** mp.mpf("1.5") * mp.exp(-chi[i] / kt)
    return out


def planck(nu, t):
    """B_nu(T) = (2 h nu^3 / c^2) / (exp(h nu / (k_B T)) - 1), scalars of mpf."""
    return (2 * H * nu ** 3 / C ** 2) / mp.expm1(H * nu / (K_B * t))


def phi_ik(pd, cd, t_e):
    """n_k / (n_up n_e) in LTE at t_e [NC, S]: the level's share of its ion over the Saha factor."""
    lbf = boltzmann(pd, t_e)
    z = partition(pd, lbf)
    sf = saha(pd, t_e, z)
    ion = np.repeat(np.arange(len(pd.ion_charge)), np.diff(pd.ion_level_edge))
    return np.array([[(lbf[k, s] / z[ion[k], s]) / sf[ion[k], s] for s in range(len(t_e))] for k in cd.level], dtype=object)


def integrands(cd, t_rad, w, t_e):
    """y_sp = (8 pi x nu^2 / c^2) exp(-h nu / k T_e), y_g = 4 pi W B_nu(T_rad) x / (h nu), y_st = y_g exp(-h nu / k T_e): [NP, S] each."""
    nu, x = mpf(cd.nu), mpf(cd.x_sect)
    y_sp, y_g, y_st = (np.empty((len(nu), len(t_rad)), dtype=object) for _ in range(3))
    for s in range(len(t_rad)):
        tr, te, ws = mp.mpf(float(t_rad[s])), mp.mpf(float(t_e[s])), mp.mpf(float(w[s]))
        for p in range(len(nu)):
            bf = mp.exp(-H * nu[p] / (K_B * te))
            y_sp[p, s] = 8 * PI * x[p] * nu[p] ** 2 / C ** 2 * bf
            y_g[p, s] = 4 * PI * ws * planck(nu[p], tr) * x[p] / (H * nu[p])
            y_st[p, s] = y_g[p, s] * bf
    return y_sp, y_g, y_st


def trapezoid(nu, y):
    """The exact trapezoid sum of y [n, ...] on the grid nu [n] (mpf arrays): sum (nu[j+1] - nu[j]) (y[j+1] + y[j]) / 2."""
    return sum((nu[j + 1] - nu[j]) * (y[j + 1] + y[j]) / 2 for j in range(len(nu) - 1))


def block_trapezoids(cd, y):
    nu, edge = mpf(cd.nu), cd.block_edge
    return np.array([trapezoid(nu[a:b], y[a:b]) for a, b in zip(edge[:-1], edge[1:])], dtype=object)


def spontaneous_closed(x0, nu0, nu1, t_e):
    """The integral of (8 pi x nu^2 / c^2) exp(-h nu / k T) over [nu0, nu1] for x = x0 (nu0 / nu)^3:
    (8 pi x0 nu0^3 / c^2) [E1(u0) - E1(u1)], u = h nu / (k T)."""
    x0, nu0, nu1, kt = mp.mpf(x0), mp.mpf(nu0), mp.mpf(nu1), K_B * mp.mpf(t_e)
    return 8 * PI * x0 * nu0 ** 3 / C ** 2 * (mp.e1(H * nu0 / kt) - mp.e1(H * nu1 / kt))


def photoionisation_quad(x0, nu0, nu1, t_rad, w):
    """The integral of 4 pi W B_nu(T) x / (h nu) over [nu0, nu1] for x = x0 (nu0 / nu)^3, by mp.quad."""
    x0, nu0, nu1, t = mp.mpf(x0), mp.mpf(nu0), mp.mpf(nu1), mp.mpf(t_rad)
    return mp.quad(lambda v: 4 * PI * mp.mpf(w) * planck(v, t) * x0 * (nu0 / v) ** 3 / (H * v), [nu0, nu1])


def seaton(pd, cd, t_e):
    """CollIonRateCoeffSeaton [NC, S]: 1.55e13 gbar x_threshold exp(-u0) / (u0 sqrt(T_e)), gbar 0.1 / 0.2 / 0.3 by the ion's charge."""
    ion = np.repeat(np.arange(len(pd.ion_charge)), np.diff(pd.ion_level_edge))
    nu, x = mpf(cd.nu), mpf(cd.x_sect)
    out = np.empty((len(cd.level), len(t_e)), dtype=object)
    for c, k in enumerate(cd.level):
        gbar = {0.0: mp.mpf("0.1"), 1.0: mp.mpf("0.2")}.get(float(pd.ion_charge[ion[k]]), mp.mpf("0.3"))
        a = int(cd.block_edge[c])
        for s, te in enumerate(t_e):
            u0 = H * nu[a] / (K_B * mp.mpf(float(te)))
            out[c, s] = SEATON * gbar * x[a] * mp.exp(-u0) / (u0 * mp.sqrt(mp.mpf(float(te))))
    return out


def ff_opacity_constant():
    """sqrt(2 pi / (3 m_e k_B)) 4 e^6 / (3 m_e h c)."""
    return mp.sqrt(2 * PI / (3 * M_E * K_B)) * 4 * E_ESU ** 6 / (3 * M_E * H * C)


def charge_sum(pd, n_ion):
    """sum over the ions of n_ion Z^2 [S], on float64 populations, exactly."""
    n, z = mpf(n_ion), mpf(pd.ion_charge)
    return np.array([mp.fsum(n[i, s] * z[i] ** 2 for i in range(len(z))) for s in range(n.shape[1])], dtype=object)


def chi_ff(pd, n_ion, n_e, t_e, nu, shell):
    """The free-free opacity at (nu[q], shell[q]): FF n_e sum(n_ion Z^2) / (sqrt(T_e) nu^3) (1 - exp(-h nu / k T_e))."""
    q2, ne, ff = charge_sum(pd, n_ion), mpf(n_e), ff_opacity_constant()
    out = []
    for v, s in zip(nu, shell):
        v, te = mp.mpf(float(v)), mp.mpf(float(t_e[s]))
        out.append(ff * ne[s] * q2[s] / (mp.sqrt(te) * v ** 3) * (-mp.expm1(-H * v / (K_B * te))))
    return np.array(out, dtype=object)


def cool_rate_ff(pd, n_ion, n_e, t_e):
    q2, ne = charge_sum(pd, n_ion), mpf(n_e)
    return np.array([C0_FF * ne[s] * mp.sqrt(mp.mpf(float(t_e[s]))) * q2[s] for s in range(len(t_e))], dtype=object)


def c0_ff_hydrogenic():
    """The free-free emission constant with a Gaunt factor of 1: (2^5 pi e^6 / (3 h m_e c^3)) sqrt(2 pi k_B / (3 m_e))."""
    return 32 * PI * E_ESU ** 6 / (3 * H * M_E * C ** 3) * mp.sqrt(2 * PI * K_B / (3 * M_E))


def opacity_tables(m, n, t_rad, w):
    """The closed forms of the opacity update on the populations n [K, S] (float64, taken exactly): stimulated_emission_factor of
    strict equilibrium 1 - exp(-h nu / k T), tau_sobolev = (pi e^2 / (m_e c)) f lambda t n_l (1 - exp(-h nu / k T)),
    beta_sobolev = (1 - exp(-tau)) / tau and j_blues = W B_nu(T_rad): [L, S] each."""
    ld = m.ld
    nu, f, n_l = mpf(m.nu), mpf(ld.f_lu), mpf(n)[np.asarray(ld.level_lower)]
    coef = PI * E_ESU ** 2 / (M_E * C)
    L, S = len(nu), len(t_rad)
    sef, tau, beta, j = (np.empty((L, S), dtype=object) for _ in range(4))
    for s in range(S):
        t = mp.mpf(float(t_rad[s]))
        for l in range(L):
            sef[l, s] = -mp.expm1(-H * nu[l] / (K_B * t))
            tau[l, s] = coef * f[l] * (C / nu[l]) * mp.mpf(m.time_explosion) * n_l[l, s] * sef[l, s]
            beta[l, s] = -mp.expm1(-tau[l, s]) / tau[l, s]
            j[l, s] = mp.mpf(float(w[s])) * planck(nu[l], t)
    return {"stimulated_emission_factor": sef, "tau_sobolev": tau, "beta_sobolev": beta, "j_blues": j}


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------

def exp_err(a):
    return (5.0 * abs(a) + 1.0) * U


def planck_err(a_min, a_max):
    return (5.0 * a_max + 8.0 + 2.0 / a_min) * U


def bounds(m):
    """Every derived bound of the module docstring for the atom ``m`` (relative errors, floats)."""
    pd, cd = m.pd, m.cd
    kt_min = F64["k_B"] * (min(1.0, pd.link_t_rad_t_electron) * T_RAD.min())
    x_e, x_chi = float(np.max(pd.level_energy)) / kt_min, float(np.max(pd.ionization_energy)) / kt_min
    n_max, n_ions = int(np.max(np.diff(pd.ion_level_edge))), len(pd.ion_charge)
    n_block = int(np.max(np.diff(cd.block_edge)))
    a_line = F64["h"] * m.nu / F64["k_B"]
    a_line_min, a_line_max = float(a_line.min() / T_RAD.max()), float(a_line.max() / T_RAD.min())
    lbf = exp_err(x_e) + 2 * U
    z = lbf + n_max * U
    sf = 2 * z + 20 * U + exp_err(x_chi) + 4 * U
    phi = sf + lbf + z + 4 * U
    point = planck_err(A_MIN, A_MAX) + exp_err(A_MAX) + 12 * U
    trap = (n_block + 2) * 2 * U + point
    sef = 2 * lbf + 8 * U
    return {"boltzmann": 2 * lbf + 6 * U, "saha": sf + 8 * U, "sum": (n_ions + 6) * U, "phi_ik": phi, "phi_identity": sf + 8 * U + 12 * U,
            "trapezoid": trap, "milne": 3 * trap + 3 * phi + 12 * U, "chi_bf": exp_err(A_MAX) + sf + 16 * U,
            "coll_ion": exp_err(A_MAX) + 12 * U, "coll_balance": sf + 24 * U, "cool_rate_ff": (n_ions + 10) * U, "sef": sef, "tau": sef + 8 * U,
            "j_blues": planck_err(a_line_min, a_line_max) + 4 * U, "lbf": lbf}


def chi_ff_bound(m, nu, t_e):
    """Per query: exp_err(a) / min(a, 1) + (24 + I) u."""
    a = F64["h"] * np.asarray(nu) / (F64["k_B"] * np.asarray(t_e))
    return (5.0 * a + 1.0) * U / np.minimum(a, 1.0) + (24 + len(m.pd.ion_charge)) * U


def beta_bound(m, tau, sef):
    """Per entry of beta_sobolev, for tau and the stimulated-emission factor [L, S] (float64): the tau bound over sef plus the branch's
    own term."""
    tau, sef = np.asarray(tau, dtype=np.float64), np.asarray(sef, dtype=np.float64)
    own = np.where(tau > 1e3, 0.0, np.where(tau < 1e-4, tau * tau / 6.0, 2.0 ** -54 / np.maximum(tau, 1e-300)))
    return bounds(m)["tau"] / sef + 4 * U + own


def assert_conditions(m, sol, tables):
    """What the bounds need of the atom, on the CPU: ``sol`` the restatement's lte / lte plasma of the equilibrium arm, ``tables`` its
    opacity tables."""
    tau, sef = tables["tau_sobolev"], tables["stimulated_emission_factor"]
    pd, cd, ld = m.pd, m.cd, m.ld
    counts = np.diff(pd.ion_level_edge)
    assert tuple(counts) == tuple(n for e in LEVELS for n in e) and len(pd.element_ion_edge) == 3 and len(T_RAD) == 5
    assert T_RAD.min() == 5000.0 and T_RAD.max() == 25000.0
    for a, b in zip(pd.ion_level_edge[:-1], pd.ion_level_edge[1:]):
        e = pd.level_energy[a:b]
        assert e[0] == 0.0 and np.all(np.diff(e) >= 0.999 * MIN_GAP_EV * EV), (a, b)
    assert np.all(counts[np.asarray(pd.element_ion_edge[1:]) - 1] == 1)                      # closed shells keep one level
    assert np.all(pd.level_g % 2 == 1) and np.all(pd.level_g >= 1)                           # 2J + 1
    ion_l, ion_u = m.ion[ld.level_lower], m.ion[ld.level_upper]
    assert np.array_equal(ion_l, ion_u) and np.all(ld.level_lower < ld.level_upper)          # lines inside one ion
    assert np.all(np.diff(m.nu) < 0) and np.array_equal(m.nu, m.op.line_list_nu)             # descending, no duplicates
    assert np.array_equal(m.nu, (pd.level_energy[ld.level_upper] - pd.level_energy[ld.level_lower]) / F64["h"])
    assert np.array_equal(ld.wavelength_cm, F64["c"] / m.nu)
    for i, n in enumerate(counts):                                                           # a ladder and, from three levels on, cycles
        own = int(np.sum(ion_l == i))
        assert own == (0 if n == 1 else n - 1 if n == 2 else n - 1 + min(n * (n - 1) // 2 - (n - 1), 2 * n)), i
    assert len(set(zip(ld.level_lower.tolist(), ld.level_upper.tolist()))) == len(m.nu)
    f = np.log10(ld.f_lu)
    assert f.min() >= -4.0 and f.max() <= 0.0 and f.max() - f.min() > 3.5
    assert tuple(counts[np.asarray(m.nd.species_ion)]) == (1, 2, 17, 70)
    assert np.array_equal(np.diff(m.nd.species_line_edge), [np.sum(ion_l == i) for i in m.nd.species_ion])
    pairs = np.diff(m.col.species_pair_edge)
    assert pairs[0] == 0 and pairs[1] == 1 and 0 < pairs[2] < 136 and pairs[3] == 2415
    t_e = pd.link_t_rad_t_electron * T_RAD
    assert m.col.collision_temperatures[0] <= LINK_TWO_TEMPERATURE * T_RAD.min() and m.col.collision_temperatures[-1] >= T_RAD.max()
    # continua: hydrogenic, thresholds (chi - E_k) / h, charges 0, 1 and 2, h nu / kT inside [A_MIN, A_MAX] at t_rad and at t_e
    assert set(pd.ion_charge[m.ion[cd.level]]) == {0.0, 1.0, 2.0}
    for c, k in enumerate(cd.level):
        a, b = int(cd.block_edge[c]), int(cd.block_edge[c + 1])
        assert cd.nu[a] == (pd.ionization_energy[m.ion[k]] - pd.level_energy[k]) / F64["h"] and np.all(np.diff(cd.nu[a:b]) > 0)
        assert np.allclose(cd.x_sect[a:b], cd.x_sect[a] * (cd.nu[a] / cd.nu[a:b]) ** 3, rtol=1e-14, atol=0)
    for t in (T_RAD, t_e, LINK_TWO_TEMPERATURE * T_RAD):
        a = F64["h"] * cd.nu[:, None] / (F64["k_B"] * t[None, :])
        assert A_MIN <= a.min() and a.max() <= A_MAX, (a.min(), a.max())
    # no Saha factor underflows, every ion above the cut, every level populated
    assert np.all(sol["ion_number_density"] > 1e3 * ION_ZERO) and np.all(sol["level_number_density"] > 0)
    assert np.all(np.nan_to_num(sol["phi"], nan=1.0) > 1e-200)
    # every derived bound below the cap; beta's needs the optical depths
    for name, value in bounds(m).items():
        assert 0 < value < CAP_TABLES, (name, value)
    bb = beta_bound(m, tau, sef)
    assert sef.min() > 0.04 and bb.max() < CAP_TABLES, (float(bb.max()), float(np.min(tau)), float(sef.min()))
    assert (tau > 1e3).any() and ((tau >= 1e-4) & (tau <= 1e3)).any()


# ---- the identities, on whatever tables they are given (the restatement's on the CPU, the device's on the GPU) ------------------------------
# Every function returns {name: (measured, bound)}: the worst relative figure and the derived bound it is held to.

def plasma_figures(m, plasma, t_rad):
    """Saha between neighbouring ions on the tables' own n_e, Boltzmann inside every ion, and the ions of an element against its
    density."""
    pd, b = m.pd, bounds(m)
    n, n_ion, n_e = mpf(plasma["level_number_density"]), mpf(plasma["ion_number_density"]), mpf(plasma["electron_density"])
    lbf = boltzmann(pd, t_rad)
    sf, last = saha(pd, t_rad), last_ions(pd)
    S = len(t_rad)
    got = np.array([[n_ion[i + 1, s] * n_e[s] / n_ion[i, s] for s in range(S)] for i in range(len(last)) if not last[i]], dtype=object)
    worst_saha = max(abs(g / w - 1) for g, w in zip(got.ravel(), sf[~last].ravel()))
    edge = pd.ion_level_edge
    worst_b = mp.mpf(0)
    for a, e in zip(edge[:-1], edge[1:]):
        for k in range(a + 1, e):
            for s in range(S):
                worst_b = max(worst_b, abs((n[k, s] / n[a, s]) / (lbf[k, s] / lbf[a, s]) - 1))
    worst_sum = mp.mpf(0)
    for e, (a, c) in enumerate(zip(pd.element_ion_edge[:-1], pd.element_ion_edge[1:])):
        for s in range(S):
            worst_sum = max(worst_sum, abs(mp.fsum(n_ion[a:c, s]) / mp.mpf(float(pd.number_density[e, s])) - 1))
    return {"saha": (float(worst_saha), b["saha"]), "boltzmann": (float(worst_b), b["boltzmann"]), "sum": (float(worst_sum), b["sum"])}


def nlte_distances(m, x, level_boltzmann_factor, t_rad):
    """Per NLTE species (in the data set's order): the largest |x / x_Boltzmann - 1| with x_Boltzmann = lbf / Z, and the largest
    |lbf_replaced / lbf - 1| of the species' rows; [NS] each."""
    pd = m.pd
    lbf = boltzmann(pd, t_rad)
    z = partition(pd, lbf)
    x, got_lbf = mpf(x), mpf(level_boltzmann_factor)
    d_x, d_lbf, row = [], [], 0
    for i in m.nd.species_ion:
        a, b = int(pd.ion_level_edge[i]), int(pd.ion_level_edge[i + 1])
        wx = wl = mp.mpf(0)
        for k in range(a, b):
            for s in range(len(t_rad)):
                wx = max(wx, abs(x[row + k - a, s] / (lbf[k, s] / z[i, s]) - 1))
                wl = max(wl, abs(got_lbf[k, s] / lbf[k, s] - 1))
        row += b - a
        d_x.append(float(wx))
        d_lbf.append(float(wl))
    return np.array(d_x), np.array(d_lbf)


def continuum_identity_figures(m, plasma, rates, opacity, t_rad):
    """The equilibrium identities of the continuum stage on the tables' own populations: phi_ik n_up n_e = n_i; gamma_corr n_i =
    alpha_sp n_up n_e (Milne), relative to gamma n_i; coll_ion n_i = coll_recomb n_up n_e; chi_bf = n_i x (1 - exp(-h nu / kT)),
    relative to n_i x."""
    pd, cd, b = m.pd, m.cd, bounds(m)
    n, n_ion, n_e = mpf(plasma["level_number_density"]), mpf(plasma["ion_number_density"]), mpf(plasma["electron_density"])
    r = {k: mpf(v) for k, v in rates.items()}
    chi_bf, nu, x = mpf(opacity["chi_bf"]), mpf(cd.nu), mpf(cd.x_sect)
    w = dict.fromkeys(("phi_identity", "milne", "coll_balance", "chi_bf"), mp.mpf(0))
    for c, k in enumerate(cd.level):
        i = int(m.ion[k])
        for s in range(len(t_rad)):
            n_i, up = n[k, s], n_ion[i + 1, s] * n_e[s]
            w["phi_identity"] = max(w["phi_identity"], abs(r["phi_ik"][c, s] * up / n_i - 1))
            w["milne"] = max(w["milne"], abs(r["gamma_corr"][c, s] * n_i - r["alpha_sp"][c, s] * up) / (r["gamma"][c, s] * n_i))
            w["coll_balance"] = max(w["coll_balance"], abs(r["coll_ion"][c, s] * n_i / (r["coll_recomb"][c, s] * up) - 1))
            kt = K_B * mp.mpf(float(t_rad[s]))
            for p in range(int(cd.block_edge[c]), int(cd.block_edge[c + 1])):
                w["chi_bf"] = max(w["chi_bf"], abs(chi_bf[p, s] / (n_i * x[p]) + mp.expm1(-H * nu[p] / kt)))
    return {k: (float(v), b[k]) for k, v in w.items()}


def opacity_figures(m, n, tables, t_rad, w):
    """stimulated_emission_factor (relative to 1), tau_sobolev (relative to tau / sef), j_blues, and beta_sobolev in units of its
    per-entry bound, against the closed forms on the populations n."""
    want, b = opacity_tables(m, n, t_rad, w), bounds(m)
    out = {"sef": (rel(tables["stimulated_emission_factor"], want["stimulated_emission_factor"], mp.mpf(1)), b["sef"]),
           "tau": (rel(tables["tau_sobolev"], want["tau_sobolev"], want["tau_sobolev"] / want["stimulated_emission_factor"]), b["tau"]),
           "j_blues": (rel(tables["j_blues"], want["j_blues"]), b["j_blues"])}
    got, wb, per = np.asarray(tables["beta_sobolev"]), want["beta_sobolev"], beta_bound(m, tables["tau_sobolev"], tables["stimulated_emission_factor"])
    worst = max(float(abs(mp.mpf(float(got[idx])) / wb[idx] - 1)) / per[idx] for idx in np.ndindex(got.shape))
    out["beta / its bound"] = (worst, 1.0)
    return out


def two_temperature_figures(m, rates, t_rad, w):
    """alpha_sp / phi_ik, gamma and alpha_stim / phi_ik against the exact trapezoid on the same grid, phi_ik and coll_ion against their
    closed forms, at t_e = link t_rad."""
    pd, cd, b = m.pd, m.cd, bounds(m)
    t_e = pd.link_t_rad_t_electron * np.asarray(t_rad)
    y_sp, y_g, y_st = integrands(cd, t_rad, w, t_e)
    r = {k: mpf(v) for k, v in rates.items()}
    # (the quotient of two of the device's tables, formed exactly here: its bound is the trapezoid's plus nothing)
    return {"alpha_sp / phi_ik": (float(np.max(np.abs(r["alpha_sp"] / r["phi_ik"] / block_trapezoids(cd, y_sp) - 1))), b["trapezoid"] + 2 * U),
            "gamma": (float(np.max(np.abs(r["gamma"] / block_trapezoids(cd, y_g) - 1))), b["trapezoid"]),
            "alpha_stim / phi_ik": (float(np.max(np.abs(r["alpha_stim"] / r["phi_ik"] / block_trapezoids(cd, y_st) - 1))), b["trapezoid"] + 2 * U),
            "phi_ik": (rel(rates["phi_ik"], phi_ik(pd, cd, t_e)), b["phi_ik"]),
            "coll_ion": (rel(rates["coll_ion"], seaton(pd, cd, t_e)), b["coll_ion"])}


def free_free_query(m):
    """The frequencies and shells of the chi_ff check: per shell a block's first, an interior and its last point, one frequency below
    every threshold and one above every block."""
    cd, S = m.cd, len(T_RAD)
    a, b = int(cd.block_edge[3]), int(cd.block_edge[4])
    nu = np.array([cd.nu[a], cd.nu[(a + b) // 2], cd.nu[b - 1], 0.5 * cd.nu.min(), 2.0 * cd.nu.max()])
    return np.tile(nu, S), np.repeat(np.arange(S), len(nu))


def free_free_figures(m, plasma, t_e, nu, shell, got_chi_ff, got_cool_rate_ff):
    """chi_ff of the batch query in units of its per-query bound, and cool_rate_ff, on the tables' own n_ion and n_e."""
    want = chi_ff(m.pd, plasma["ion_number_density"], plasma["electron_density"], t_e, nu, shell)
    per = chi_ff_bound(m, nu, np.asarray(t_e)[shell])
    worst = max(float(abs(mp.mpf(float(g)) / wv - 1)) / p for g, wv, p in zip(got_chi_ff, want, per))
    return {"chi_ff / its bound": (worst, 1.0),
            "cool_rate_ff": (rel(got_cool_rate_ff, cool_rate_ff(m.pd, plasma["ion_number_density"], plasma["electron_density"], t_e)), bounds(m)["cool_rate_ff"])}


def assert_figures(figures, report=None, prefix=""):
    """Print every figure beside its bound, then assert it (and the bound's cap)."""
    for name, (measured, bound) in figures.items():
        line = "%-44s measured %.3e   bound %.3e" % (prefix + name, measured, bound)
        print(line)
        if report is not None:
            report.append(line)
    for name, (measured, bound) in figures.items():
        assert bound == 1.0 or bound < CAP_TABLES, (name, bound)
        assert measured <= bound, (prefix + name, measured, bound)


# ---- the restatements on the atom, computed once and never written to ------------------------------------------------------------------------

NLTE_CONFIGS = ("first", "second", "collisions", "collisions, second")


class Restatement:
    """The NumPy restatements (tests/*_ref.py) on an atom: the measurements the GPU margins rest on.  Needs the oracle built."""

    def __init__(self, m, w, ionization="lte", excitation="lte"):
        self.m, self.w, self.modes = m, np.asarray(w, dtype=np.float64), (ionization, excitation)
        self._cache = {}

    def _once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def j_blues(self):
        import opacity_update_ref as oref
        return self._once("j", lambda: oref.j_blues_dilute_blackbody(self.m.nu, self.m.t_rad, self.w))

    def tables(self, sol):
        import opacity_update_ref as oref
        return oref.update(self.m.ld, self.m.op, self.m.time_explosion, sol["level_number_density"], j_blues=self.j_blues())

    def plasma(self, modes=None):
        """(solved plasma, opacity tables) without NLTE species."""
        import plasma_update_ref as ref
        modes = self.modes if modes is None else modes

        def make():
            sol = ref.solve(self.m.pd, self.m.t_rad, self.w, *modes)
            return sol, self.tables(sol)
        return self._once(("plasma",) + tuple(modes), make)

    def continuum(self):
        """(continuum_ref.stage, cooling_ref.stage) on plasma()."""
        import continuum_ref as cref
        import cooling_ref as kref

        def make():
            sol = self.plasma()[0]
            out = cref.stage(self.m.pd, self.m.cd, sol, self.m.t_rad, self.w)
            return out, kref.stage(self.m.pd, self.m.cd, sol, out, self.m.time_explosion)
        return self._once("continuum", make)

    def nlte(self, config):
        """(solved plasma, opacity tables) of an update with the NLTE species installed: "first" after set_opacity (beta of ones),
        "second" on the first's beta_sobolev; "collisions" with the collision data and the opacity state's n_e, "collisions, second" on
        that update's beta_sobolev and solved n_e."""
        import nlte_collision_ref as ccref
        import nlte_excitation_ref as nref
        m = self.m

        def make():
            if config == "first":
                sol = nref.solve(m.pd, m.ld, m.nd, m.t_rad, self.w, self.j_blues(), None, *self.modes)
            elif config == "second":
                sol = nref.solve(m.pd, m.ld, m.nd, m.t_rad, self.w, self.j_blues(), self.nlte("first")[1]["beta_sobolev"], *self.modes)
            elif config == "collisions":
                sol = ccref.solve(m.pd, m.ld, m.nd, m.col, m.t_rad, self.w, self.j_blues(), None, m.n_e0, *self.modes)
            else:
                before = self.nlte("collisions")
                sol = ccref.solve(m.pd, m.ld, m.nd, m.col, m.t_rad, self.w, self.j_blues(), before[1]["beta_sobolev"], before[0]["electron_density"],
                                  *self.modes)
            return sol, self.tables(sol)
        return self._once(("nlte", config), make)

    def nlte_distances(self, config):
        sol = self.nlte(config)[0]
        return nlte_distances(self.m, sol["relative_populations"], sol["level_boltzmann_factor"], self.m.t_rad)
