"""The plasma chain held to thermodynamic equilibrium, on the CPU (tests/equilibrium_ref.py): the atom's conditions; every identity of
tests/test_equilibrium_gpu.py run on the NumPy restatements, the worst figure of each printed beside its derived bound -- these are the
measurements the GPU margins rest on (profiles/equilibrium.txt; `python tests/test_equilibrium_host.py` prints them) --; and the pure
mathematics of the quadrature test: the exact trapezoid sum against the closed integral.

mpmath is the reference; the restatements are code under test here exactly as the device is on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import equilibrium_ref as eq  # noqa: E402

mp = eq.mp
REPORT = []


class World:
    def __init__(self):
        self.m = eq.atom()
        self.eq = eq.Restatement(self.m, eq.W_EQUILIBRIUM)
        self.m2 = eq.atom(link=eq.LINK_TWO_TEMPERATURE)
        self.two = eq.Restatement(self.m2, eq.W_DILUTE, "nebular", "dilute-lte")


@pytest.fixture(scope="module")
def world(oracle):
    return World()


def test_the_atom_meets_its_conditions(world):
    sol, tables = world.eq.plasma()
    eq.assert_conditions(world.m, sol, tables)
    eq.assert_conditions(world.m2, sol, tables)  # (the same levels, lines and continua at link 0.9: the bounds at the lower t_e)
    assert world.m2.pd.link_t_rad_t_electron == 0.9 and world.m.pd.link_t_rad_t_electron == 1.0
    assert np.array_equal(world.m.nu, world.m2.nu) and np.array_equal(world.m.cd.nu, world.m2.cd.nu)
    # the two-temperature arm: W from 0.5 down to 0.05, no clamp, no ion below the cut
    assert eq.W_DILUTE[0] == 0.5 and eq.W_DILUTE[-1] == 0.05 and np.all(np.diff(eq.W_DILUTE) < 0)
    assert np.all(world.two.plasma()[0]["ion_number_density"] > 1e3 * eq.ION_ZERO)


def test_the_constants():
    import continuum_ref as cref
    import cooling_ref as kref
    from tardis_amd import synthetic
    # FF_OPAC_CONST from the physical constants: the literal is the double next to it (14 roundings in ff_opac_const())
    assert abs(eq.ff_opacity_constant() / mp.mpf(cref.FF_OPAC_CONST) - 1) < 14 * eq.U
    assert mp.mpf(kref.C0_FF) == mp.mpf(float(eq.C0_FF)) and abs(eq.C0_FF / eq.c0_ff_hydrogenic() - 1) < 1e-3
    # pi e^2 / (m_e c): the atom's coefficient to rounding; the synthetic models' own (e truncated to 4.80320450e-10) to 5e-9
    want = eq.PI * eq.E_ESU ** 2 / (eq.M_E * eq.C)
    assert abs(mp.mpf(float(eq.SOBOLEV_COEFFICIENT)) / want - 1) < 8 * eq.U
    assert abs(mp.mpf(float(synthetic.SOBOLEV_COEFFICIENT)) / want - 1) < 5e-9
    for name, value in (("k_B", cref.K_BOLTZMANN), ("h", cref.H_PLANCK), ("m_e", cref.M_ELECTRON), ("c", cref.C_LIGHT)):
        assert value == eq.F64[name], name


def test_equilibrium_populations(world):
    """Nebular / dilute-LTE at W = 1 IS lte / lte, and lte / lte is Saha-Boltzmann."""
    lte, neb = world.eq.plasma()[0], world.eq.plasma(("nebular", "dilute-lte"))[0]
    assert lte["iterations"] == neb["iterations"]
    for name in ("level_number_density", "ion_number_density", "partition_function", "electron_density"):
        assert np.array_equal(lte[name], neb[name]), name
    eq.assert_figures(eq.plasma_figures(world.m, lte, world.m.t_rad), REPORT, "restatement  ")


@pytest.mark.parametrize("config", eq.NLTE_CONFIGS)
def test_nlte_returns_boltzmann(world, config):
    """The rate equations return Boltzmann populations whatever the beta_sobolev, with and without collisions.  No derived bound: the
    restatement's own distance is the measurement, 4 x it the device's bound, and that must stay below CAP_NLTE."""
    d_x, d_lbf = world.eq.nlte_distances(config)
    for sp, n in enumerate((1, 2, 17, 70)):
        line = "restatement  NLTE %-20s %2d levels   x %.3e   lbf %.3e   device bounds %.3e, %.3e" % (config, n, d_x[sp], d_lbf[sp], 4 * d_x[sp], 4 * d_lbf[sp])
        print(line)
        REPORT.append(line)
    assert d_x[0] == 0.0 and d_lbf[0] == 0.0
    assert 4 * max(d_x.max(), d_lbf.max()) < eq.CAP_NLTE
    sol, tables = world.eq.nlte(config)
    if config.endswith("second"):  # the escape probabilities the second update found are far from 1
        first = world.eq.nlte(config.replace(", second", "") if "," in config else "first")[1]
        assert first["beta_sobolev"].min() < 1e-6 and not np.array_equal(sol["relative_populations"], world.eq.nlte("first")[0]["relative_populations"])
    if config == "collisions":    # ... and the collisional terms are in the matrices
        assert not np.array_equal(sol["relative_populations"], world.eq.nlte("first")[0]["relative_populations"])
        assert np.all(sol["c_lu"][~np.isnan(world.m.col.C_ul[:, :1]).ravel()] >= 0) and (sol["c_ul"] > 0).mean() > 0.8
    # the populations of the NLTE update are those of the plain one, to the same bound
    plain = world.eq.plasma()[0]["level_number_density"]
    assert np.max(np.abs(sol["level_number_density"] / plain - 1)) < eq.CAP_NLTE


def test_continuum_identities(world):
    out = world.eq.continuum()[0]
    assert out["n_negative_chi_bf"] == 0 and out["n_negative_gamma_corr"] == 0
    eq.assert_figures(eq.continuum_identity_figures(world.m, world.eq.plasma()[0], out, out, world.m.t_rad), REPORT, "restatement  ")


def test_opacity_tables(world):
    sol, tables = world.eq.plasma()
    eq.assert_figures(eq.opacity_figures(world.m, sol["level_number_density"], tables, world.m.t_rad, eq.W_EQUILIBRIUM), REPORT, "restatement  ")


def test_two_temperature_tables(world):
    m, r = world.m2, world.two
    out, cool = r.continuum()
    assert out["n_negative_chi_bf"] == 0 and out["n_negative_gamma_corr"] == 0
    eq.assert_figures(eq.two_temperature_figures(m, out, m.t_rad, eq.W_DILUTE), REPORT, "restatement  two-temperature  ")
    import continuum_ref as cref
    nu, shell = eq.free_free_query(m)
    q = cref.query(m.cd, out, nu, shell)
    assert np.all(q["n_current"][:3] >= 1) and q["n_current"][3] == 0 and q["n_current"][4] == 0
    eq.assert_figures(eq.free_free_figures(m, r.plasma()[0], out["t_electrons"], nu, shell, q["chi_ff"], cool["cool_rate_ff"]), REPORT,
                      "restatement  two-temperature  ")
    assert np.array_equal(out["t_electrons"], 0.9 * m.t_rad)


def test_the_identities_see_a_departure(world):
    """Power: at W = 0.5 the NLTE populations miss Boltzmann, at link = 0.9 Milne's identity fails, by far more than 1e-3."""
    import nlte_excitation_ref as nref
    import opacity_update_ref as oref
    m = world.m
    w = np.full(len(m.t_rad), 0.5)
    sol = nref.solve(m.pd, m.ld, m.nd, m.t_rad, w, oref.j_blues_dilute_blackbody(m.nu, m.t_rad, w), None, "lte", "lte")
    d_x, _ = eq.nlte_distances(m, sol["relative_populations"], sol["level_boltzmann_factor"], m.t_rad)
    assert d_x[0] == 0.0 and np.all(d_x[1:] > 1e-3), d_x
    f = eq.continuum_identity_figures(world.m2, world.two.plasma()[0], world.two.continuum()[0], world.two.continuum()[0], world.m2.t_rad)
    assert f["milne"][0] > 1e-3, f
    for line in ("restatement  power  NLTE x against Boltzmann at W = 0.5: %s" % np.array2string(d_x, precision=3),
                 "restatement  power  Milne residual at link = 0.9, W 0.5 .. 0.05: %.3e" % f["milne"][0]):
        print(line)
        REPORT.append(line)


# ---- the pure mathematics of the quadrature ---------------------------------------------------------------------------------------------

def _grid(nu0, n):
    return nu0 * np.geomspace(1.0, eq.SPAN, n)


@pytest.mark.parametrize("u0", [0.5, 3.0, 10.0])
def test_the_exact_trapezoid_converges_to_the_closed_integral(u0):
    """On hydrogenic blocks of n and 2 n - 1 points (n = 65, 129, 257; geometric grids in fp64, the sums in mpmath) the error of the
    trapezoid against the closed integral falls by 4 within 5 %: (8 pi x0 nu0^3 / c^2) [E1(u0) - E1(u1)] for the spontaneous-recombination
    integrand, mp.quad for the photo-ionisation integrand.  u0 <= 10: in the hundreds the ratio falls to 2.9 (the integrand then decays
    across a handful of intervals)."""
    t, x0, w = 11000.0, 6.3e-18, 0.5
    nu0 = u0 * eq.F64["k_B"] * t / eq.F64["h"]

    def errors(n):
        g = _grid(nu0, n)
        cd = eq.synthetic.ContinuumData(np.array([0]), np.array([0, n]), g, x0 * (g[0] / g) ** 3)
        y_sp, y_g, _ = eq.integrands(cd, [t], [w], [t])
        nu = eq.mpf(g)
        # (x_sect on the grid is x0 (nu0 / nu)^3 rounded: three roundings, 1e-16 relative, far below the quadrature's error)
        return (abs(eq.trapezoid(nu, y_sp[:, 0]) / eq.spontaneous_closed(x0, g[0], g[-1], t) - 1),
                abs(eq.trapezoid(nu, y_g[:, 0]) / eq.photoionisation_quad(x0, g[0], g[-1], t, w) - 1))

    e = {n: errors(n) for n in (65, 129, 257, 513)}
    for n in (65, 129, 257):
        for which, name in enumerate(("spontaneous recombination", "photo-ionisation")):
            ratio = float(e[n][which] / e[2 * n - 1][which])
            line = "quadrature  u0 = %4.1f  %-26s n = %3d: error %.3e, over the error at 2 n - 1: %.4f" % (u0, name, n, float(e[n][which]), ratio)
            print(line)
            REPORT.append(line)
            assert abs(ratio / 4 - 1) < 0.05, (u0, n, name, ratio)


if __name__ == "__main__":
    from oracle import oracle as _o
    _o.build()
    w = World()
    test_the_atom_meets_its_conditions(w)
    test_the_constants()
    test_equilibrium_populations(w)
    for c in eq.NLTE_CONFIGS:
        test_nlte_returns_boltzmann(w, c)
    test_continuum_identities(w)
    test_opacity_tables(w)
    test_two_temperature_tables(w)
    test_the_identities_see_a_departure(w)
    for u in (0.5, 3.0, 10.0):
        test_the_exact_trapezoid_converges_to_the_closed_integral(u)
