"""The long-double restatement of the formal integral (tests/formal_integral_ref.py) against what is known, and the C oracle
against the restatement where nothing else is known.  No GPU.

  a. reference() reproduces the three golden vectors the reference itself produced (tests/golden/formal_*.npz) at rtol 1e-13,
     the bar tests/test_formal_integral.py gives the oracle; measured 4.5e-15 / 5.7e-16 / 2.8e-15.
  b. the oracle equals reference() at rtol 1e-13 on every input of the edge model (impact parameters ON r_inner[0] and ON
     r_outer[0..2], duplicate lines, tau = 0 and tau = 800, frequencies from which no line is in reach), and every ray of the
     variants without electron scattering meets the derived bound (4 K + 64) 2^-53 (formal_integral_ref.ray_bound).
  c. reference() and the oracle equal the closed forms of a one-shell model with one and with two lines at rtol 1e-14."""
import os
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import formal_integral_ref as ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def oracle_call(m, N, **replace):
    from oracle import formal
    return ref.call(formal.formal_integral, m, N, **replace)


@pytest.mark.parametrize("name", ["formal_small", "formal_thick", "formal_one_shell"])
def test_reference_reproduces_the_goldens(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    lum, inten, K = ref.call(ref.reference, g, int(g["n_impact_parameters"]))
    print(name, "max relative deviation: I", ref.max_rel(inten, g["intensities_nu_p"]), "L", ref.max_rel(lum, g["luminosity_densities"]),
          "resonances", int(K.sum()))
    assert np.array_equal(inten == 0, g["intensities_nu_p"] == 0)
    assert np.array_equal(lum == 0, g["luminosity_densities"] == 0)
    assert_allclose(inten.astype(np.float64), g["intensities_nu_p"], rtol=1e-13, atol=0)
    assert_allclose(lum.astype(np.float64), g["luminosity_densities"], rtol=1e-13, atol=0)
    assert ref.max_rel(inten, g["intensities_nu_p"]) <= 1e-13 and ref.max_rel(lum, g["luminosity_densities"]) <= 1e-13
    assert K.sum() > 0


def test_the_edge_model_has_its_edges():
    for L in (37, 2000):
        m = ref.edge_model(L)
        nu, r_in, r_out = m["line_list_nu"], m["r_inner"], m["r_outer"]
        assert nu[5] == nu[4] and nu[18] == nu[19] == nu[20] and (np.diff(nu) <= 0).all()
        assert (m["tau_sobolev"][ref.TAU_ZERO_LINE] == 0).all() and np.exp(-m["tau_sobolev"][ref.TAU_OPAQUE_LINE]).max() == 0
        assert len(m["frequencies"]) == 129
        # h nu / k T <= 8 for every comoving frequency a black body is evaluated at (ray_bound assumes it)
        z_max = 1 + r_out[-1] / m["time_explosion"] * ref.C_INV
        assert ref.H_CGS * m["frequencies"].max() * z_max / (ref.KB_CGS * m["inner_temperature"]) <= 8
        assert (ref.edge_model(L, electrons=False)["electron_density"] == 0).all() and (m["electron_density"] > 0).sum() == 3
        for N in (9, 17, 33):
            p = np.array([ref.impact_parameter(k, r_out[-1], N) for k in range(N)])
            assert (p == r_in[0]).sum() == 1  # a ray ON the photosphere
            for s in range(3):
                assert (p == r_out[s]).sum() == 1  # tangent rays
            assert p[-1] == r_out[-1]
    # the tangent ray skips the shell it touches: two points fewer than the ray just inside it
    m = ref.edge_model(37)
    tangent = ref.intersection_points(m["r_inner"], m["r_outer"], m["time_explosion"], float(m["r_outer"][0]))
    inside = ref.intersection_points(m["r_inner"], m["r_outer"], m["time_explosion"], np.nextafter(m["r_outer"][0], 0))
    assert len(tangent) == 6 and len(inside) == 8 and tangent[0][1] == 3 and tangent[2][1] == tangent[3][1] == 1
    on_core = ref.intersection_points(m["r_inner"], m["r_outer"], m["time_explosion"], float(m["r_inner"][0]))
    assert len(on_core) == 4 and [on_core[k][1] for k in range(4)] == [0, 1, 2, 3]


@pytest.mark.parametrize("L,N,electrons", ref.EDGE_CASES, ids=[f"L{L}-N{N}-{'ne' if e else 'ne0'}" for L, N, e in ref.EDGE_CASES])
def test_oracle_against_the_reference_on_the_edges(L, N, electrons):
    m, (lum, inten, K) = ref.edge_reference(L, N, electrons)
    lum_o, inten_o = oracle_call(m, N)
    nz = inten != 0
    print(f"L {L} N {N} electrons {electrons}: resonances {int(K.sum())} non-zero rays {int(nz.sum())} longest ray K = {int(K.max())}; "
          f"oracle max relative deviation I {ref.max_rel(inten_o, inten):.3g} L {ref.max_rel(lum_o, lum):.3g}")
    assert np.isfinite(inten_o).all() and np.isfinite(lum_o).all() and (inten_o >= 0).all() and (lum_o >= 0).all()
    assert np.array_equal(inten_o == 0, ~nz) and np.array_equal(lum_o == 0, lum == 0)
    assert (inten[:, 0] == 0).all() and (inten[:, -1] == 0).all()
    if N == 2:
        assert not nz.any() and (lum == 0).all() and K.sum() == 0
        return
    assert ref.max_rel(inten_o, inten) <= 1e-13 and ref.max_rel(lum_o, lum) <= 1e-13
    # the frequency from which every line is blueward starts every ray behind the last line; from the other nothing is in reach
    assert K[0].sum() == 0 and K[1].sum() == 0 and (inten[0] != 0).any() and (inten[1] != 0).any()
    core = [k for k in range(N) if ref.impact_parameter(k, m["r_outer"][-1], N) <= m["r_inner"][0]]
    assert core[0] == 0 and nz[:, core[1:]].all()  # every core ray but p = 0 carries light at every frequency
    assert ((K == 0) & nz).any()  # a ray that crosses nothing and still carries the photosphere's black body
    if N >= 9:
        assert nz[:, (N - 1) // 2].all() and nz[:, (N - 1) // 2 + 1:].any()  # the ray ON r_inner[0] is a core ray; tangent rays carry light
    if L == 2000:
        assert K.max() >= 500
    if not electrons:
        err = np.abs(inten_o.astype(ref.LD) - inten)[nz] / inten[nz]
        worst = np.argmax(err / ref.ray_bound(K[nz]))
        print(f"  worst ray against (4K + 64) 2^-53: {float(err[worst]) / ref.EPS:.1f} x 2^-53 at K = {int(K[nz][worst])}")
        assert (err <= ref.ray_bound(K[nz])).all()


@pytest.mark.parametrize("n_lines", [1, 2])
def test_closed_forms(n_lines):
    m = ref.closed_form_model(n_lines)
    N = ref.CLOSED_N
    want, crossing = ref.closed_form_one_shell(m)
    want_lum = ref.closed_form_luminosity(want, m["r_outer"][0])
    # the model is what the derivation assumes, and every kind of ray is there
    assert ref.impact_parameter(4, m["r_outer"][0], N) == m["r_inner"][0]
    assert crossing[:, 5:8].any() and (~crossing[:, 5:8]).any() and (want[:, 1:5] != 0).all() and (want[:, 8] == 0).all()
    lum, inten, K = ref.call(ref.reference, m, N)
    assert np.array_equal(K > 0, crossing) and K.max() == n_lines
    if n_lines == 2:
        assert (K == 1).any()  # rays that reach one of the two lines only, from either side
    lum_o, inten_o = oracle_call(m, N)
    for who, got_i, got_l in (("reference", inten, lum), ("oracle", inten_o, lum_o)):
        print(n_lines, "line(s):", who, "max relative deviation from the closed form: I", ref.max_rel(got_i, want), "L", ref.max_rel(got_l, want_lum),
              "crossing rays", int(crossing.sum()))
        assert np.array_equal(got_i == 0, want == 0), who
        assert ref.max_rel(got_i, want) <= 1e-14 and ref.max_rel(got_l, want_lum) <= 1e-14, who
