"""The yardstick of the two switches of the nebular ionisation stage of tardis_mc_update_plasma (tardis_mc_set_ionization_options):
helium_treatment "recomb-nlte" and delta_treatment, as include/tardis_mc.h spells them out -- a NumPy restatement on top of
tests/plasma_update_ref.py, whose exp, serial sums, Boltzmann factors, partition functions, zeta and ion populations it reuses unchanged.

delta_treatment replaces RadiationFieldCorrection's delta by one number for every ion and shell.  The helium treatment sits INSIDE the
electron-density iteration: every pass renormalises the relative helium level populations hp with the pass's n_e and writes the three
helium ion rows over the ones the ordinary Saha chain gave, after the 1e-20 cut and before the new n_e is summed; the level populations
of helium are those of the last pass, not (lbf / Z) N.  With neither option solve() performs the operations of plasma_update_ref.solve
in its order and returns its bits."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plasma_update_ref as ref  # noqa: E402

exp, serial_sum, level_ion = ref.exp, ref.serial_sum, ref.level_ion
boltzmann_factors, partition_functions, zeta_values, ion_populations = ref.boltzmann_factors, ref.partition_functions, ref.zeta_values, ref.ion_populations
K_BOLTZMANN, H_PLANCK, M_ELECTRON, THRESHOLD = ref.K_BOLTZMANN, ref.H_PLANCK, ref.M_ELECTRON, ref.THRESHOLD
EV = 1.602176565e-12  # erg, CODATA 2010 (tardis_amd.synthetic.EV)


def helium_element_of(pd):
    """The row of element_ion_edge whose atomic_number is 2; ValueError when there is none."""
    rows = np.flatnonzero(np.asarray(pd.atomic_number) == 2)
    if len(rows) == 0:
        raise ValueError("the plasma data hold no element with atomic_number 2")
    return int(rows[0])


def delta_values(pd, t_rad, w, delta_treatment=None):
    """[I, S]: RadiationFieldCorrection with departure_coefficient 1 / W, or delta_treatment everywhere."""
    chi = np.asarray(pd.ionization_energy, dtype=np.float64)[:, None]
    if delta_treatment is not None:
        return np.full((len(chi), len(t_rad)), float(delta_treatment))
    beta_rad = 1 / (K_BOLTZMANN * t_rad)
    t_e = pd.link_t_rad_t_electron * t_rad
    beta_e = 1 / (K_BOLTZMANN * t_e)
    fa = t_e / (((1 / w) * w) * t_rad)
    with np.errstate(over="ignore", invalid="ignore"):
        above = fa[None, :] * exp(chi * (beta_rad - beta_e)[None, :])
        below = (1 - exp(chi * beta_rad[None, :] - (beta_rad * pd.chi_0)[None, :])) + fa[None, :] * exp(chi * beta_rad[None, :] - (beta_e * pd.chi_0)[None, :])
    return np.where(chi >= pd.chi_0, above, below)


def g_electron(t_rad):
    beta_rad = 1 / (K_BOLTZMANN * t_rad)
    x = ((2 * np.pi * M_ELECTRON) / beta_rad) / (H_PLANCK * H_PLANCK)
    return x * np.sqrt(x)


def phi_values(pd, z, t_rad, w, ionization, delta_treatment=None):
    """plasma_update_ref.phi_values with the delta of delta_values; [I, S], the rows of the elements' last ions NaN."""
    chi = np.asarray(pd.ionization_energy, dtype=np.float64)[:, None]
    beta_rad = 1 / (K_BOLTZMANN * t_rad)
    t_e = pd.link_t_rad_t_electron * t_rad
    g_e = g_electron(t_rad)
    last = np.zeros(len(chi), dtype=bool)
    last[np.asarray(pd.element_ion_edge[1:]) - 1] = True
    ratio = np.full(z.shape, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio[:-1] = z[1:] / z[:-1]
        phi = ratio * ((2 * g_e)[None, :] * exp(chi * (-beta_rad)[None, :]))
        if ionization == "nebular":
            zeta = zeta_values(pd, t_rad)
            delta = delta_values(pd, t_rad, w, delta_treatment)
            phi = ((phi * w[None, :]) * ((zeta * delta) + w[None, :] * (1 - zeta))) * np.sqrt(t_e / t_rad)[None, :]
        elif ionization != "lte":
            raise ValueError(ionization)
    phi[last] = np.nan
    return phi


def helium_relative(pd, lbf, t_rad, w, helium_element, delta_treatment=None):
    """hp [K_He, S]: the populations of the helium levels relative to the He II ground level, before the electron density enters."""
    a = int(pd.element_ion_edge[helium_element])
    edge = np.asarray(pd.ion_level_edge)
    k0, k1, k2, k3 = (int(edge[a + j]) for j in range(4))
    g = np.asarray(pd.level_g, dtype=np.float64)
    chi = np.asarray(pd.ionization_energy, dtype=np.float64)
    g1, g2 = g[k1], g[k2]
    beta_rad = 1 / (K_BOLTZMANN * t_rad)
    t_e = pd.link_t_rad_t_electron * t_rad
    g_e = g_electron(t_rad)
    hp = np.empty((k3 - k0, len(t_rad)))
    with np.errstate(over="ignore", invalid="ignore"):
        hp[0] = 0.0
        hp[1:k1 - k0] = (((lbf[k0 + 1:k1] * (1 / (2 * g1))) * (1 / g_e)[None, :]) * (1 / (w * w))[None, :]) * exp(chi[a] * beta_rad)[None, :]
        hp[k1 - k0] = 1.0
        hp[k1 - k0 + 1:k2 - k0] = lbf[k1 + 1:k2] * (1 / g1)
        zeta = zeta_values(pd, t_rad)[a + 1]
        delta = delta_values(pd, t_rad, w, delta_treatment)[a + 1]
        hp[k2 - k0] = (((((2 * (g2 / g1)) * g_e) * exp(chi[a + 1] * (-beta_rad))) * w) * ((delta * zeta) + w * (1 - zeta))) * np.sqrt(t_e / t_rad)
    return hp


def helium_pass(pd, hp, n_e, helium_element):
    """One pass's helium: (v [K_He, S], the three ion rows [3, S])."""
    a = int(pd.element_ion_edge[helium_element])
    edge = np.asarray(pd.ion_level_edge)
    n1, n2 = int(edge[a + 1] - edge[a]), int(edge[a + 2] - edge[a])
    u = hp.copy()
    u[:n1] = hp[:n1] * n_e[None, :]
    total = serial_sum(u)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        f = np.asarray(pd.number_density, dtype=np.float64)[helium_element] / total
        v = u * f[None, :]
    return v, np.stack((serial_sum(v[:n1]), serial_sum(v[n1:n2]), v[n2]))


def check_helium(pd, helium_element):
    """What tardis_mc_check_ionization_options refuses, as a ValueError."""
    E = len(pd.element_ion_edge) - 1
    if not 0 <= helium_element < E:
        raise ValueError("helium_element outside the elements")
    a, b = int(pd.element_ion_edge[helium_element]), int(pd.element_ion_edge[helium_element + 1])
    if b - a != 3 or list(np.asarray(pd.ion_charge)[a:b]) != [0, 1, 2] or pd.ion_level_edge[b] - pd.ion_level_edge[b - 1] != 1:
        raise ValueError("the helium element needs the ions He I, He II, He III, the last with one level")


def solve(pd, t_rad, w, helium_element=None, delta_treatment=None, ionization="nebular", excitation="dilute-lte", max_iterations=1000, guard=1e-9):
    """plasma_update_ref.solve with the two options.  helium_element: None for no helium treatment, else the element row that is helium
    (recomb-nlte); delta_treatment: None for RadiationFieldCorrection, else the number.  Returns the fields of plasma_update_ref.solve
    and, with helium, "helium_relative" (hp) and "helium_population" (the v of the last pass), [K_He, S] each (None without).  Asserts,
    like its model, that no delta of any pass lies within ``guard`` of the 5 % threshold."""
    t_rad, w = np.asarray(t_rad, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if helium_element is not None:
        if ionization != "nebular":
            raise ValueError("helium_treatment recomb-nlte needs ionization nebular")
        check_helium(pd, helium_element)
    lbf = boltzmann_factors(pd, t_rad, w, excitation)
    z = partition_functions(pd, lbf)
    phi = phi_values(pd, z, t_rad, w, ionization, delta_treatment)
    hp = v = None
    if helium_element is not None:
        hp = helium_relative(pd, lbf, t_rad, w, helium_element, delta_treatment)
        a = int(pd.element_ion_edge[helium_element])
    charge = np.asarray(pd.ion_charge, dtype=np.float64)[:, None]
    n_e = serial_sum(pd.number_density)
    iterations, deltas = 0, []
    while True:
        if iterations >= max_iterations:
            raise ref.PlasmaIonizationError("the electron density has not converged")
        n_ion = ion_populations(pd, phi, n_e)
        if hp is not None:
            v, n_ion[a:a + 3] = helium_pass(pd, hp, n_e, helium_element)
        new = serial_sum(n_ion * charge)
        if np.any(np.isnan(new)):
            raise ref.PlasmaIonizationError("the electron density became NaN")
        iterations += 1
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = np.abs(new - n_e) / n_e
        deltas.append(delta)
        assert np.all(np.abs(delta - THRESHOLD) > guard), (iterations, delta)
        if np.all(delta < THRESHOLD):
            break
        n_e = 0.5 * (new + n_e)
    ion = level_ion(pd)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = (lbf / z[ion]) * n_ion[ion]
    if hp is not None:
        k0 = int(pd.ion_level_edge[a])
        n[k0:k0 + len(v)] = v
    return {"level_number_density": n, "ion_number_density": n_ion, "partition_function": z, "phi": phi, "electron_density": n_e,
            "iterations": iterations, "deltas": deltas, "level_boltzmann_factor": lbf, "helium_relative": hp, "helium_population": v}


def planted_helium_model():
    """plasma_update_ref.planted_model(5) with its third element (ions 9, 10, 11 of 20 / 14 / 1 levels) relabelled as helium: the
    ionisation energies of He I and He II, excited levels between 0.78 and 0.98 of them.  S = 4, K = 300, L = 400.  Returns
    (plasma_data, line_data, problem, t_rad, w, facts); facts gains "helium_element" and "helium_ions"."""
    pd, ld, prob, t_rad, w, facts = ref.planted_model(5)
    assert list(np.diff(pd.ion_level_edge)[9:12]) == [20, 14, 1]
    pd.ionization_energy = pd.ionization_energy.copy()
    pd.level_energy = pd.level_energy.copy()
    pd.atomic_number = np.array(pd.atomic_number).copy()
    pd.ionization_energy[9], pd.ionization_energy[10] = 24.587 * EV, 54.418 * EV
    rng = np.random.default_rng(6)
    for i in (9, 10):
        a, b = int(pd.ion_level_edge[i]), int(pd.ion_level_edge[i + 1])
        top = pd.ionization_energy[i]
        pd.level_energy[a + 1:b] = np.sort(0.78 * top + 0.2 * top * rng.random(b - a - 1))
    pd.atomic_number[2] = 2
    facts = dict(facts, helium_element=2, helium_ions=(9, 10, 11))
    return pd, ld, prob, t_rad, w, facts
