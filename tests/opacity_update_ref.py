"""The yardstick of the device opacity update (tardis_mc_update_opacity): a NumPy restatement of the legacy plasma's
StimulatedEmissionFactor, TauSobolev, BetaSobolev, JBluesDiluteBlackBody and calculate_transition_probabilities in their operation
order, every product and sum a rounding of its own.  exp is the transport's own (oracle.exp_array(x, 1), which tests/test_hip_parity.py
pins the device's mcm::exp to); a block's norm is the serial left-to-right sum (np.add.accumulate -- np.sum is pairwise and is wrong
here)."""
import numpy as np

from oracle import oracle

C_LIGHT, H_PLANCK, K_BOLTZMANN = 2.99792458e10, 6.62606957e-27, 1.3806488e-16  # tardis/constants.py (CODATA 2010, cgs)


def exp(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.asarray(oracle.exp_array(x.ravel(), 1)).reshape(x.shape)


def stimulated_emission_factor(n, level_lower, level_upper, g_lower, g_upper):
    n_l, n_u = n[level_lower], n[level_upper]  # [L, S]
    with np.errstate(divide="ignore", invalid="ignore"):
        sef = 1.0 - (g_lower[:, None] * n_u) / (g_upper[:, None] * n_l)
    sef = np.where(n_l == 0.0, 0.0, sef)
    return np.where(sef < 0.0, 0.0, sef)


def tau_sobolev(sobolev_coefficient, f_lu, wavelength_cm, time_explosion, n_l, sef):
    return ((((sobolev_coefficient * f_lu) * wavelength_cm) * time_explosion)[:, None] * n_l) * sef


def beta_sobolev(tau):
    thick, thin = tau > 1e3, tau < 1e-4
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = (1.0 - exp(-tau)) / tau
        return np.where(thick, 1.0 / tau, np.where(thin, 1.0 - 0.5 * tau, mid))


def j_blues_dilute_blackbody(nu, t_rad, w):
    beta_rad = 1 / (K_BOLTZMANN * np.asarray(t_rad, dtype=np.float64))
    planck_coef = 2 * H_PLANCK / (C_LIGHT * C_LIGHT)
    return w[None, :] * ((planck_coef * (nu * nu * nu))[:, None] / (exp((H_PLANCK * nu)[:, None] * beta_rad[None, :]) - 1))


def transition_probabilities(coef, transition_type, transition_line_id, block_edge, beta, sef, j):
    p = coef[:, None] * beta[transition_line_id]
    up = transition_type == 1
    p[up] = p[up] * (sef[transition_line_id[up]] * j[transition_line_id[up]])
    out = np.zeros_like(p)
    for a, b in zip(block_edge[:-1], block_edge[1:]):
        if b <= a:
            continue
        norm = np.add.accumulate(p[a:b], axis=0)[-1]  # serial, row by row
        with np.errstate(divide="ignore", invalid="ignore"):
            out[a:b] = np.where(norm != 0.0, p[a:b] / norm, 0.0)
    return out


def update(line_data, opacity_state, time_explosion, level_number_density, t_rad=None, w=None, j_blues=None):
    """The five tables of one update: {"tau_sobolev", "beta_sobolev", "stimulated_emission_factor", "j_blues": [L, S],
    "transition_probabilities": [T, S] or None without coefficients}.  j_blues None: the dilute black body of (t_rad, w)."""
    ld, n = line_data, np.asarray(level_number_density, dtype=np.float64)
    lo, up = np.asarray(ld.level_lower), np.asarray(ld.level_upper)
    sef = stimulated_emission_factor(n, lo, up, np.asarray(ld.g_lower, dtype=np.float64), np.asarray(ld.g_upper, dtype=np.float64))
    tau = tau_sobolev(ld.sobolev_coefficient, np.asarray(ld.f_lu), np.asarray(ld.wavelength_cm), time_explosion, n[lo], sef)
    beta = beta_sobolev(tau)
    if j_blues is None:
        j_blues = j_blues_dilute_blackbody(np.asarray(opacity_state.line_list_nu, dtype=np.float64), np.asarray(t_rad, dtype=np.float64),
                                           np.asarray(w, dtype=np.float64))
    prob = None
    if ld.transition_probability_coef is not None:
        prob = transition_probabilities(np.asarray(ld.transition_probability_coef, dtype=np.float64), np.asarray(opacity_state.transition_type),
                                        np.asarray(opacity_state.transition_line_id), np.asarray(opacity_state.macro_block_edge_index),
                                        beta, sef, np.asarray(j_blues, dtype=np.float64))
    return {"tau_sobolev": tau, "beta_sobolev": beta, "stimulated_emission_factor": sef, "j_blues": np.asarray(j_blues),
            "transition_probabilities": prob}


def planted_model(seed=11):
    """L = 200 lines, S = 3 shells, with every edge the arithmetic has: a zero-length block, a block whose norm is zero in exactly one
    shell, n_l == 0 cells, inverted populations, tau exactly 1e3 and 1e-4, tau = 0.  Returns (line_data, opacity_state, time_explosion,
    populations, t_rad, w, facts) -- facts names where each plant sits."""
    from tardis_amd import state as st, synthetic
    rng = np.random.default_rng(seed)
    L, S, K = 200, 3, 24
    t_exp = 13 * 86400.0
    lam = np.sort(np.exp(rng.uniform(np.log(500.0), np.log(20000.0), L)))
    nu = C_LIGHT / (lam * 1e-8)
    wave = C_LIGHT / nu
    f_lu = 10.0 ** rng.uniform(-3, 0, L)
    lower = rng.integers(0, K // 2, L).astype(np.int64)
    upper = rng.integers(K // 2, K, L).astype(np.int64)
    g = 2.0 * rng.integers(0, 5, K) + 1.0
    n = 10.0 ** rng.uniform(-2, 6, (K, S))
    n[K // 2:] *= 1e-3
    # plants on the populations.  Level 0 is empty in shell 1 (n_l == 0); level 1 is empty everywhere (its lines: tau = 0, beta = 1);
    # level K - 1 outnumbers every lower level in shell 2 (inverted: sef clamps to 0, tau = 0)
    n[0, 1] = 0.0
    n[1, :] = 0.0
    n[K - 1, 2] = 1e12
    # exact optical depths: lines 0 and 1 run between level 2 and level K - 2, which is empty (sef = 1 exactly), with f_lu (and the last
    # bits of the wavelength) searched so that the product chain lands on the bound exactly
    n[K - 2, :] = 0.0
    lower[:2], upper[:2] = 2, K - 2
    n[2, :] = [1.0, 2.0, 4.0]  # (shell 0 sits on the bound; the others at twice and four times it)
    coef_s = float(synthetic.SOBOLEV_COEFFICIENT)

    def chain(f, w_):
        return ((coef_s * f) * w_) * t_exp

    def solve(target, w0):
        # the chain of three roundings does not reach every double: the wavelength is moved by a few ulps as well
        w_ = w0
        for _ in range(4096):
            f = target / (coef_s * w_ * t_exp)
            for _ in range(64):
                v = chain(f, w_)
                if v == target:
                    return f, w_
                f = np.nextafter(f, np.inf if v < target else -np.inf)
            w_ = np.nextafter(w_, np.inf)
        raise AssertionError("no pair of doubles reaches the target")

    f_lu[0], wave[0] = solve(1e3, wave[0])   # tau = 1e3 in shell 0 (2e3, 4e3 in the others: thick branch)
    f_lu[1], wave[1] = solve(1e-4, wave[1])  # tau = 1e-4 in shell 0
    # macro-atom topology: blocks of 1-12 lines x 3 rows (emission, down, up), line ids assigned in order; block 3 has zero length
    sizes = []
    left = L
    while left > 0:
        gsz = int(min(left, rng.integers(1, 13)))
        sizes.append(gsz)
        left -= gsz
    sizes.insert(3, 0)
    n_blocks = len(sizes)
    T = 3 * L
    ttype, dest, tline = np.empty(T, np.int64), np.empty(T, np.int64), np.empty(T, np.int64)
    edge = np.empty(n_blocks + 1, np.int64)
    l2m = np.empty(L, np.int64)
    row = line = 0
    for b, gsz in enumerate(sizes):
        edge[b] = row
        ids = np.arange(line, line + gsz)
        l2m[ids] = b
        for tt in (-1, 0, 1):
            ttype[row:row + gsz] = tt
            dest[row:row + gsz] = -99 if tt == -1 else rng.integers(0, n_blocks, gsz)
            tline[row:row + gsz] = ids
            row += gsz
        line += gsz
    edge[n_blocks] = T
    coef = rng.random(T) + 0.05
    coef[ttype == 1] *= 1e4
    # a block whose norm is zero in exactly one shell: block 5 keeps only its type-1 rows (the other coefficients are 0), and its lines
    # all start from level 0, empty in shell 1 alone: sef = 0 there, so every p of the block is 0 in shell 1 and positive elsewhere
    zb = 5
    a, b = edge[zb], edge[zb + 1]
    assert b > a
    rows = np.arange(a, b)
    coef[rows[ttype[rows] != 1]] = 0.0
    zl = np.unique(tline[rows])
    assert zl.min() >= 2
    lower[zl] = 0
    upper[zl] = K // 2  # (sparsely populated: not inverted in shells 0 and 2)
    n[K // 2, :] = 1e-6
    n[0, 0], n[0, 2] = 1e3, 1e3
    ne = 1e9 * np.array([1.0, 0.6, 0.3])
    op = st.OpacityState(ne, np.full(S, 9000.0), nu, np.zeros((L, S)), np.zeros((T, S)), l2m, edge, ttype, dest, tline)
    ld = synthetic.LineData(f_lu, wave, g[lower], g[upper], lower, upper, K, coef, coef_s, n, ne, np.array([10000.0, 9500.0, 9000.0]),
                            np.array([0.4, 0.3, 0.2]))
    facts = {"zero_length_block": 3, "zero_norm_block": zb, "zero_norm_shell": 1, "exact_lines": (0, 1), "empty_level": 1,
             "inverted_level": K - 1, "inverted_shell": 2}
    return ld, op, t_exp, n, ld.t_radiative, ld.dilution_factor, facts
