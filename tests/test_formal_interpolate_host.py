"""interpolate_shells on the resident source function (tardis_mc_formal_integral_interpolated / tardis_mc_interpolated_source):
what can be checked without a GPU -- the library, the Python wrappers and the header carry the new entry points, and the NumPy
restatement of the interpolation that the device is held to (tests/formal_interpolate_ref.py) is scipy's interp1d bit for bit."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import formal_interpolate_ref as ref  # noqa: E402
from tardis_amd import _lib, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tardis_mc_formal_integral_interpolated", "tardis_mc_interpolated_source")
CASES = [(20, 81), (20, 8), (20, 11), (2, 30), (3, 2)]  # (resident shells, interpolate_shells)


def test_library_exports_the_new_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name


def test_engine_and_integrator_carry_the_new_methods():
    from tardis_amd.engine import Engine
    from tardis_amd.formal_integral import FormalIntegratorHIP
    for name in ("formal_integral_interpolated", "interpolated_source"):
        assert callable(getattr(Engine, name, None)), name
    sig = inspect.signature(Engine.formal_integral_interpolated)
    assert list(sig.parameters)[1:] == ["interpolate_shells", "inner_temperature", "frequencies", "n_impact_parameters",
                                        "want_intensities"]
    assert sig.parameters["n_impact_parameters"].default == 1000 and sig.parameters["want_intensities"].default is False
    assert inspect.signature(FormalIntegratorHIP.integrated_spectrum).parameters["interpolate_shells"].default == 0


def test_header_names_both_functions():
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
    assert "#define TARDIS_MC_ABI_VERSION 2 " in header


@pytest.mark.parametrize("S,n", CASES)
def test_restatement_is_scipy_bit_for_bit(S, n):
    """Random non-negative tables with about 30 % exact zeros, 257 columns: the restatement equals interp1d(...,
    fill_value="extrapolate") followed by .clip(0.0), and kind="nearest", with array_equal."""
    from scipy.interpolate import interp1d
    geo = synthetic.make_geometry(n_shells=S)
    g = ref.grid(geo.r_inner, geo.r_outer, n)
    rng = np.random.default_rng(100 * S + n)
    y = rng.random((S, 257)) * 10.0 ** rng.uniform(-12, 0, (1, 257))
    y[rng.random(y.shape) < 0.3] = 0.0
    assert 0.2 < (y == 0).mean() < 0.4
    x, xn = g["x"], g["xn"]
    assert len(xn) == n - 1 and g["r_inner"][0] == geo.r_inner[0] and g["r_outer"][-1] == geo.r_outer[-1]
    want = interp1d(x, y, axis=0, fill_value="extrapolate")(xn).clip(0.0)
    got = ref.linear_clipped(y, g)
    assert got.shape == (n - 1, 257) and np.array_equal(got, want)
    assert (got >= 0).all()
    want_near = interp1d(x, y, axis=0, kind="nearest", fill_value="extrapolate")(xn)
    assert np.array_equal(ref.nearest(y, g), want_near)
    n_e = rng.random(S) + 1.0
    assert np.array_equal(ref.nearest(n_e, g), interp1d(x, n_e, kind="nearest", fill_value="extrapolate")(xn))
    # one column, as e_dot_u's levels and 1-d callers pass it
    assert np.array_equal(ref.linear_clipped(y[:, 3], g), interp1d(x, y[:, 3], fill_value="extrapolate")(xn).clip(0.0))
    # what each case is there for
    raw = ref.linear_unclipped(y, g)
    if (S, n) == (20, 81):   # refine: points outside the nodes at both ends, values clipped there and inside the grid
        assert xn[0] < x[0] and xn[-1] > x[-1]
        inside = (xn >= x[0]) & (xn <= x[-1])
        assert (raw[~inside] < 0).any() and (raw < 0).sum() > 0
        assert len(np.unique(g["near"])) == S
    elif (S, n) == (20, 8):  # coarsen: fewer shells than the model has
        assert n - 1 < S and (np.diff(g["lo"]) > 1).any()
    elif (S, n) == (20, 11):  # every new midpoint lies on an old shell edge, half way between two nodes: the tie rule decides
        edges = geo.r_outer[0::2][:n - 1]
        assert np.allclose(xn, edges, rtol=1e-14, atol=0)
        assert (np.abs(g["near"] - (2 * np.arange(n - 1) + 0.5)) == 0.5).all()  # (one of the two shells that share the edge)
    elif (S, n) == (2, 30):  # two nodes: one interval serves every point, most of them extrapolated
        assert (g["lo"] == 0).all() and (g["hi"] == 1).all() and ((xn < x[0]) | (xn > x[1])).sum() > 10
    elif (S, n) == (3, 2):   # one output shell
        assert got.shape[0] == 1 and len(g["near"]) == 1


def test_interpolate_source_layouts():
    """The eight arrays in the layouts Engine.interpolated_source returns them."""
    S, L, K, n = 5, 7, 3, 9
    geo = synthetic.make_geometry(n_shells=S)
    rng = np.random.default_rng(1)
    tau, n_e = rng.random((L, S)), rng.random(S)
    att, jred, jblue, e = rng.random(S * L), rng.random(S * L), rng.random(S * L), rng.random((K, S))
    out = ref.interpolate_source(geo.r_inner, geo.r_outer, n, tau, n_e, att, jred, jblue, e)
    g = ref.grid(geo.r_inner, geo.r_outer, n)
    assert out["tau_sobolev"].shape == ((n - 1) * L,) and out["att_S_ul"].shape == ((n - 1) * L,) and out["e_dot_u"].shape == (K, n - 1)
    j = 4
    assert np.array_equal(out["tau_sobolev"].reshape(n - 1, L)[j], tau[:, g["near"][j]])
    assert out["electron_density"][j] == n_e[g["near"][j]]
    assert np.array_equal(out["e_dot_u"][1], ref.linear_clipped(e[1], g))
    assert np.array_equal(out["Jred_lu"].reshape(n - 1, L)[:, 2], ref.linear_clipped(jred.reshape(S, L)[:, 2], g))
