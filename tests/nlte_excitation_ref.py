"""The yardstick of the NLTE excitation stage of tardis_mc_update_plasma: a NumPy restatement of the contract in include/tardis_mc.h
(LevelBoltzmannFactorNLTE._calculate_general / _main_nlte_calculation without collision data) -- the rates of a species' lines, the rate
matrix with the destination as the row, the diagonal from the serial column sums, the row of ones, and M x = b by unblocked LU with
partial pivoting written as whole-array steps per k.  NumPy does not fuse separate ufuncs, so every product, quotient and difference is
rounded on its own and every entry sees its updates in the order of k: this IS the serial order.  Around it the stages of
tests/plasma_update_ref.py, imported and not edited: Boltzmann factors -> NLTE overwrite -> partition functions, phi, the electron-density
iteration and the populations."""
import numpy as np

import plasma_update_ref as ref


class NlteSolveError(RuntimeError):
    def __init__(self, what, step):
        super().__init__(f"{what} (step {step})")
        self.step = step


def rate_matrix(n, lower, upper, r_ul, r_lu):
    """[n, n]: M[l][u] = r_ul, M[u][l] = r_lu, the diagonal minus the serial sum of its column, the first row ones."""
    m = np.zeros((n, n))
    m[lower, upper] = r_ul
    m[upper, lower] = r_lu
    diagonal = -ref.serial_sum(m)  # (the diagonal is still 0.0, as in the reference; adding 0.0 changes nothing)
    m[np.arange(n), np.arange(n)] = diagonal
    m[0, :] = 1.0
    return m


def lu_solve(m, b):
    """x, and the steps at which two rows were swapped.  m and b are not modified."""
    m, b = np.array(m, dtype=np.float64), np.array(b, dtype=np.float64)
    n = len(b)
    swaps = []
    for k in range(n):
        p = k + int(np.argmax(np.abs(m[k:, k])))  # the lowest row with the largest magnitude
        if p != k:
            m[[k, p]] = m[[p, k]]
            b[[k, p]] = b[[p, k]]
            swaps.append(k)
        pivot = m[k, k]
        if pivot == 0.0 or not np.isfinite(pivot):
            raise NlteSolveError("zero or non-finite pivot", k)
        with np.errstate(all="ignore"):
            l = m[k + 1:, k] / pivot
            m[k + 1:, k + 1:] = m[k + 1:, k + 1:] - l[:, None] * m[k, k + 1:][None, :]
            b[k + 1:] = b[k + 1:] - l * b[k]
    x = np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n - 1, -1, -1):
            x[j] = b[j] / m[j, j]
            b[:j] = b[:j] - m[:j, j] * x[j]
    if not np.all(np.isfinite(x)):
        raise NlteSolveError("a population that is not finite", n)
    if x[0] == 0.0:
        raise NlteSolveError("x[0] == 0", n)
    return x, swaps


def species_systems(pd, ld, nd, j_blues, beta_sobolev):
    """Per species and shell the system (M, b): yields (position, shell, k0, n, M).  j_blues [L, S]: the mean intensities of the update
    (ignored with coronal_approximation); beta_sobolev [L, S] of the previous update, or None (ones; also with classical_nebular)."""
    edge = np.asarray(pd.ion_level_edge, dtype=np.int64)
    lower_all, upper_all = np.asarray(ld.level_lower, dtype=np.int64), np.asarray(ld.level_upper, dtype=np.int64)
    S = np.shape(j_blues)[1]
    for pos, ion in enumerate(np.asarray(nd.species_ion, dtype=np.int64)):
        k0, n = int(edge[ion]), int(edge[ion + 1] - edge[ion])
        a, b = int(nd.species_line_edge[pos]), int(nd.species_line_edge[pos + 1])
        lines = np.asarray(nd.line_id[a:b], dtype=np.int64)
        lower, upper = lower_all[lines] - k0, upper_all[lines] - k0
        j = np.zeros((len(lines), S)) if nd.coronal_approximation else np.asarray(j_blues, dtype=np.float64)[lines]
        beta = np.ones((len(lines), S)) if beta_sobolev is None or nd.classical_nebular else np.asarray(beta_sobolev, dtype=np.float64)[lines]
        r_ul = (np.asarray(nd.A_ul[a:b])[:, None] + np.asarray(nd.B_ul[a:b])[:, None] * j) * beta
        r_lu = (np.asarray(nd.B_lu[a:b])[:, None] * j) * beta
        for s in range(S):
            yield pos, s, k0, n, rate_matrix(n, lower, upper, r_ul[:, s], r_lu[:, s])


def lapack_solve(m, b):
    """What the legacy plasma calls: numpy.linalg.solve (to rounding, not bitwise; tools/time_nlte_excitation.py times it)."""
    return np.linalg.solve(m, b), []


def nlte_boltzmann_factors(pd, ld, nd, lbf, j_blues, beta_sobolev=None, solver=lu_solve):
    """The Boltzmann factors with the NLTE species' rows replaced ([K, S], a copy), x [sum of n, S] and {(position, shell): swap steps}."""
    lbf = np.array(lbf, dtype=np.float64)
    edge = np.asarray(pd.ion_level_edge, dtype=np.int64)
    sizes = np.diff(edge)[np.asarray(nd.species_ion, dtype=np.int64)]
    x0 = np.concatenate(([0], np.cumsum(sizes)))
    x_all = np.zeros((int(x0[-1]), lbf.shape[1]))
    swaps = {}
    for pos, s, k0, n, m in species_systems(pd, ld, nd, j_blues, beta_sobolev):
        b = np.zeros(n)
        b[0] = 1.0
        try:
            x, swaps[(pos, s)] = solver(m, b)
        except NlteSolveError as e:
            e.species, e.shell = pos, s
            raise
        x_all[x0[pos]:x0[pos + 1], s] = x
        lbf[k0:k0 + n, s] = (x * pd.level_g[k0]) / x[0]
    return lbf, x_all, swaps


def solve(pd, ld, nd, t_rad, w, j_blues, beta_sobolev=None, ionization="nebular", excitation="dilute-lte", max_iterations=1000, guard=1e-9,
          solver=lu_solve):
    """tests/plasma_update_ref.solve with the NLTE stage between the Boltzmann factors and the partition functions; nd None: without.
    Adds "relative_populations" and "swaps" to its dict."""
    t_rad, w = np.asarray(t_rad, dtype=np.float64), np.asarray(w, dtype=np.float64)
    lbf = ref.boltzmann_factors(pd, t_rad, w, excitation)
    x_all, swaps = None, {}
    if nd is not None:
        lbf, x_all, swaps = nlte_boltzmann_factors(pd, ld, nd, lbf, j_blues, beta_sobolev, solver)
    z = ref.partition_functions(pd, lbf)
    phi = ref.phi_values(pd, z, t_rad, w, ionization)
    charge = np.asarray(pd.ion_charge, dtype=np.float64)[:, None]
    n_e = ref.serial_sum(pd.number_density)
    iterations, deltas = 0, []
    while True:
        if iterations >= max_iterations:
            raise ref.PlasmaIonizationError("the electron density has not converged")
        n_ion = ref.ion_populations(pd, phi, n_e)
        new = ref.serial_sum(n_ion * charge)
        if np.any(np.isnan(new)):
            raise ref.PlasmaIonizationError("the electron density became NaN")
        iterations += 1
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = np.abs(new - n_e) / n_e
        deltas.append(delta)
        assert np.all(np.abs(delta - ref.THRESHOLD) > guard), (iterations, delta)
        if np.all(delta < ref.THRESHOLD):
            break
        n_e = 0.5 * (new + n_e)
    ion = ref.level_ion(pd)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = (lbf / z[ion]) * n_ion[ion]
    return {"level_number_density": n, "ion_number_density": n_ion, "partition_function": z, "phi": phi, "electron_density": n_e,
            "iterations": iterations, "deltas": deltas, "level_boltzmann_factor": lbf, "relative_populations": x_all, "swaps": swaps}


SPECIES_LEVELS = (1, 2, 17, 70)
COUNTS = (12, 30, 2, 1, 45, 70, 40, 17, 1, 50, 31, 1)
SPECIES = (2, 5, 3, 7)
# the boundary of the LDS form: 141 levels are the most a workgroup's LDS holds (more than 64 KiB of it), 142 take the global form
BOUNDARY_COUNTS = (1, 1, 1, 1, 2, 141, 142, 2, 1, 3, 4, 1)
BOUNDARY_SPECIES = (6, 5)


def model(n_shells, seed=13, n_lines=2000, counts=COUNTS, species=SPECIES):
    """The test model: K = 300 levels on 12 ions of 3 elements (``counts`` levels each), L = 2000 lines each inside one ion,
    ``n_shells`` shells.  By default the NLTE species are the ions of 2, 70, 1 and 17 levels (in that order of the data set, which is
    not the level order); the ion of 40 levels between the 70 and the 17 in level order is not NLTE.  Returns (problem, line_data,
    plasma_data, nlte_data)."""
    from tardis_amd import synthetic
    K = 300
    prob = synthetic.make_problem(seed=seed, n_packets=20_000, n_shells=n_shells, n_lines=n_lines, line_interaction_type="macroatom", log_tau_mean=-2.0)
    ld = synthetic.make_line_data(seed, prob.opacity_state, n_levels=K, time_explosion=prob.time_explosion)
    rng = np.random.default_rng(seed)
    ev = synthetic.EV
    chi_ev = [6.113, 11.872, 50.913, 0.0, 7.902, 16.199, 30.651, 54.91, 0.0, 13.618, 35.121, 0.0]
    element_ion_edge = np.array([0, 4, 9, 12], dtype=np.int64)
    ion_charge = np.array([0, 1, 2, 3, 0, 1, 2, 3, 4, 0, 1, 2], dtype=np.float64)
    counts = np.array(counts)
    assert counts.sum() == K and len(counts) == 12
    ion_level_edge = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    chi = np.array(chi_ev) * ev
    level_energy, meta = np.zeros(K), np.zeros(K, dtype=np.int32)
    for i in range(12):
        a, b = ion_level_edge[i], ion_level_edge[i + 1]
        top = chi[i] if chi[i] > 0 else 40.0 * ev
        level_energy[a + 1:b] = np.sort(0.05 * top + 0.9 * top * rng.random(b - a - 1) ** 0.7)
        meta[a:a + 3] = 1
    meta[ion_level_edge[1:] - 1] = np.where(counts > 3, 0, 1)
    level_g = 2.0 * rng.integers(0, 6, K) + 1.0
    zeta_t = np.arange(2000.0, 40001.0, 2000.0)
    centre, width = rng.uniform(5000.0, 30000.0, 12), rng.uniform(4000.0, 15000.0, 12)
    zeta = 0.05 + 0.9 / (1.0 + np.exp((zeta_t[None, :] - centre[:, None]) / width[:, None]))
    zeta[[2, 10]] = 1.0
    s = np.arange(n_shells)
    t_rad, w = 11000.0 - 230.0 * s, 0.4 / (1.0 + 0.3 * s)
    number_density = np.array([0.05, 0.6, 0.35])[:, None] * (1e9 * (1.0 + 0.15 * s) ** -7.0)[None, :]
    pd = synthetic.PlasmaData(level_energy, level_g, meta, ion_level_edge, element_ion_edge, ion_charge, chi, zeta_t, zeta, number_density,
                              float(synthetic.CHI_0_CA_II), 0.9, np.array([20, 26, 8]), t_rad, w)
    ld = synthetic.lines_within_ions(seed, ld, pd)
    return prob, ld, pd, synthetic.make_nlte_data(seed, ld, pd, species=list(species))
