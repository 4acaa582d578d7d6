"""The device plasma chain (tardis_mc_update_plasma and what it leaves resident) held to thermodynamic equilibrium and to mpmath
quadratures (tests/equilibrium_ref.py), not to its NumPy restatement: a convention the kernel and the restatement share passes every
bit-for-bit test and fails here.

Equilibrium arm (W = 1, link_t_rad_t_electron = 1, j_blues_mode 0, line frequencies that are level-energy differences): nebular /
dilute-LTE IS lte / lte; the populations are Saha-Boltzmann; the NLTE rate equations return Boltzmann populations in the LDS, the global
and the blocked form, on the first update's beta_sobolev and with collisional rates; photo-ionisation balances recombination (Milne) and
chi_bf is n_i x (1 - exp(-h nu / kT)); the opacity tables are their closed forms.  Two-temperature arm (link = 0.9, W 0.5 .. 0.05, where
a t_e / t_rad swap shows): the rate tables against the exact trapezoid on the same grid, phi_ik and coll_ion against closed forms,
chi_ff of the batch query and cool_rate_ff from the physical constants.  Power: the identities fail by far more than 1e-3 at W = 0.5
and at link = 0.9.

Every table is held to the bound derived in tests/equilibrium_ref.py (all below 1e-12; tests/test_equilibrium_host.py asserts the
restatement inside the same bounds and prints its figures, profiles/equilibrium.txt has both).  The NLTE solve is held to 4 x the
restatement's own measured distance from Boltzmann, per species and configuration (below 1e-10)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import equilibrium_ref as eq  # noqa: E402
from tardis_amd import synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

PLASMA = ("level_number_density", "ion_number_density", "partition_function", "electron_density")
ALL = dict(tau_sobolev=True, transition_probabilities=False, beta_sobolev=True, stimulated_emission_factor=True, j_blues=True)
TABLES = ("tau_sobolev", "beta_sobolev", "stimulated_emission_factor", "j_blues")
# options nlte_lds_levels / nlte_blocked_levels: the rule (every species of the atom in LDS); every species on a slab of HBM, one
# workgroup each; every species blocked
FORMS = {"lds": (-1, -1), "global": (0, 1 << 20), "blocked": (0, 0)}
W1 = eq.W_EQUILIBRIUM


class World:
    def __init__(self):
        self.m = eq.atom()
        self.eq = eq.Restatement(self.m, W1)
        self.m2 = eq.atom(link=eq.LINK_TWO_TEMPERATURE)
        sol, tables = self.eq.plasma()
        eq.assert_conditions(self.m, sol, tables)
        eq.assert_conditions(self.m2, sol, tables)


@pytest.fixture(scope="module")
def world(oracle):
    return World()


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as eng:
        yield eng


def stage(eng, m, continuum=True, form="lds"):
    eng.set_option("nlte_lds_levels", FORMS[form][0])
    eng.set_option("nlte_blocked_levels", FORMS[form][1])
    eng.set_geometry(m.geometry, m.time_explosion)
    eng.set_opacity(m.op)
    eng.set_config(m.cfg, m.grid)
    eng.set_line_data(m.ld)
    eng.set_plasma_data(m.pd)
    if continuum:
        eng.set_continuum_data(m.cd)


def test_nebular_dilute_lte_at_w_1_is_lte_lte(engine, world):
    m = world.m
    stage(engine, m)
    got = {}
    for modes in (("lte", "lte"), ("nebular", "dilute-lte")):
        engine.update_plasma(m.t_rad, W1, *modes)
        got[modes] = (engine.get_plasma(), engine.get_opacity(**ALL), engine.get_continuum_rates(), engine.get_continuum_opacity())
    a, b = got.values()
    assert a[0]["iterations"] == b[0]["iterations"] > 1
    for name in PLASMA:
        assert np.array_equal(a[0][name], b[0][name]), name
    for x, y in zip(a[1:], b[1:]):
        for name in x:
            assert np.array_equal(x[name], y[name]), name


def test_the_populations_are_saha_boltzmann(engine, world):
    m = world.m
    stage(engine, m, continuum=False)
    engine.update_plasma(m.t_rad, W1, "lte", "lte")
    got = engine.get_plasma()
    assert np.all(got["ion_number_density"] > 1e3 * eq.ION_ZERO)
    eq.assert_figures(eq.plasma_figures(m, got, m.t_rad), prefix="device  ")


def _assert_boltzmann(m, eng, want, label, plain_lbf=None):
    """The device's x and replaced Boltzmann factors within 4 x the restatement's distances ``want`` = (d_x, d_lbf), per species."""
    got = eng.get_nlte()
    d_x, d_lbf = eq.nlte_distances(m, got["relative_populations"], got["level_boltzmann_factor"], m.t_rad)
    for sp in range(len(d_x)):
        print("device  NLTE %-28s species %d   x %.3e (bound %.3e)   lbf %.3e (bound %.3e)" % (label, sp, d_x[sp], 4 * want[0][sp], d_lbf[sp], 4 * want[1][sp]))
    assert 4 * max(want[0].max(), want[1].max()) < eq.CAP_NLTE
    assert np.all(d_x <= 4 * want[0]) and np.all(d_lbf <= 4 * want[1]), (label, d_x, d_lbf, want)
    x = got["relative_populations"]
    assert np.all(x > 0) and x.shape[0] == 1 + 2 + 17 + 70
    if plain_lbf is not None:  # against the device's own plain factors: the two distances add
        for sp, i in enumerate(m.nd.species_ion):
            a, b = int(m.pd.ion_level_edge[i]), int(m.pd.ion_level_edge[i + 1])
            worst = float(np.max(np.abs(got["level_boltzmann_factor"][a:b] / plain_lbf[a:b] - 1)))
            assert worst <= 4 * want[1][sp] + eq.bounds(m)["lbf"] + eq.U, (label, sp, worst)
        other = np.ones(len(plain_lbf), dtype=bool)
        for i in m.nd.species_ion:
            other[int(m.pd.ion_level_edge[i]):int(m.pd.ion_level_edge[i + 1])] = False
        assert np.array_equal(got["level_boltzmann_factor"][other], plain_lbf[other])


@pytest.mark.parametrize("form", list(FORMS))
def test_nlte_returns_boltzmann(engine, world, form):
    """Species of 1, 2, 17 and 70 levels: x is normalised Boltzmann and the replaced factors are those of the lte arm -- after
    set_opacity, on that update's beta_sobolev (down to 1e-17: the escape probabilities multiply both directions), and with the
    collisional rates installed (on the opacity state's n_e, then on the solved one)."""
    m, r = world.m, world.eq
    # the lte arm's own factors: only the one-level species installed, every other row is g exp(-E / kT) as the device forms it
    stage(engine, m, continuum=False, form=form)
    one = synthetic.NlteData(m.nd.species_ion[:1], np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0), np.zeros(0))
    engine.set_nlte_data(one)
    engine.update_plasma(m.t_rad, W1, "lte", "lte")
    plain_lbf = engine.get_nlte()["level_boltzmann_factor"]
    assert eq.rel(plain_lbf, eq.boltzmann(m.pd, m.t_rad)) <= eq.bounds(m)["lbf"]
    plain = engine.get_plasma()
    for collisions in (False, True):
        stage(engine, m, continuum=False, form=form)
        engine.set_nlte_data(m.nd)
        if collisions:
            engine.set_nlte_collision_data(m.col)
        for config in (eq.NLTE_CONFIGS[2:] if collisions else eq.NLTE_CONFIGS[:2]):
            engine.update_plasma(m.t_rad, W1, "lte", "lte")
            _assert_boltzmann(m, engine, r.nlte_distances(config), "%s, %s" % (form, config), plain_lbf)
            got = engine.get_plasma()
            assert np.max(np.abs(got["level_number_density"] / plain["level_number_density"] - 1)) < eq.CAP_NLTE
        assert engine.get_opacity(**ALL)["beta_sobolev"].min() < 1e-6
        if collisions:
            c = engine.get_nlte_collision_rates()
            assert c["c_ul"].shape == (len(m.col.delta_e), len(m.t_rad)) and (c["c_ul"] > 0).mean() > 0.8


def test_continuum_identities(engine, world):
    m = world.m
    stage(engine, m)
    engine.update_plasma(m.t_rad, W1, "lte", "lte")
    opacity = engine.get_continuum_opacity()
    assert opacity["n_negative_chi_bf"] == 0 and opacity["n_negative_gamma_corr"] == 0
    eq.assert_figures(eq.continuum_identity_figures(m, engine.get_plasma(), engine.get_continuum_rates(), opacity, m.t_rad), prefix="device  ")


def test_opacity_tables_are_their_closed_forms(engine, world):
    m = world.m
    stage(engine, m, continuum=False)
    engine.update_plasma(m.t_rad, W1, "lte", "lte")
    tables = engine.get_opacity(**ALL)
    assert (tables["tau_sobolev"] > 1e3).any() and (tables["tau_sobolev"] < 1e3).any()
    eq.assert_figures(eq.opacity_figures(m, engine.get_plasma()["level_number_density"], tables, m.t_rad, W1), prefix="device  ")


def test_two_temperature_tables(engine, world):
    """link = 0.9, W from 0.5 down to 0.05, nebular / dilute-LTE: the stage's quadratures and closed forms at t_e = 0.9 t_rad."""
    m = world.m2
    stage(engine, m)
    engine.update_plasma(m.t_rad, eq.W_DILUTE)
    rates, opacity, plasma = engine.get_continuum_rates(), engine.get_continuum_opacity(), engine.get_plasma()
    assert opacity["n_negative_chi_bf"] == 0 and opacity["n_negative_gamma_corr"] == 0
    assert np.array_equal(opacity["t_electrons"], 0.9 * m.t_rad)
    eq.assert_figures(eq.two_temperature_figures(m, rates, m.t_rad, eq.W_DILUTE), prefix="device  two-temperature  ")
    nu, shell = eq.free_free_query(m)
    q = engine.continuum_opacity(nu, shell)
    assert np.all(q["n_current"][:3] >= 1) and q["n_current"][3] == 0 and q["n_current"][4] == 0
    eq.assert_figures(eq.free_free_figures(m, plasma, opacity["t_electrons"], nu, shell, q["chi_ff"], engine.get_cooling_rates()["cool_rate_ff"]),
                      prefix="device  two-temperature  ")
    # power: away from equilibrium Milne's identity fails
    f = eq.continuum_identity_figures(m, plasma, rates, opacity, m.t_rad)
    print("device  power  Milne residual at link = 0.9: %.3e" % f["milne"][0])
    assert f["milne"][0] > 1e-3


def test_a_diluted_field_departs_from_boltzmann(engine, world):
    """Power: at W = 0.5 the same NLTE identity fails by far more than 1e-3 for every species that has a line."""
    m = world.m
    stage(engine, m, continuum=False)
    engine.set_nlte_data(m.nd)
    engine.update_plasma(m.t_rad, np.full(len(m.t_rad), 0.5), "lte", "lte")
    got = engine.get_nlte()
    d_x, _ = eq.nlte_distances(m, got["relative_populations"], got["level_boltzmann_factor"], m.t_rad)
    print("device  power  NLTE x against Boltzmann at W = 0.5:", d_x)
    assert d_x[0] == 0.0 and np.all(d_x[1:] > 1e-3)
