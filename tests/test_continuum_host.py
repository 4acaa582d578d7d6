"""The host side of the continuum stage, without a GPU: every refusal of tardis_mc_check_continuum_data, the header's prototypes, the
restatement's serial trapezoid against numpy's, its spontaneous-recombination integral against the closed form in E1, the free-free
constant, and the query restatement on a hand-made table (tests/continuum_ref.py is the yardstick of tests/test_continuum_gpu.py)."""
import copy
import math
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import continuum_ref as cref  # noqa: E402
import plasma_update_ref as ref  # noqa: E402
from tardis_amd import _abi, _lib, synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
trapz = getattr(np, "trapezoid", None) or np.trapz


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def planted(oracle):
    pd, ld, prob, t_rad, w, cd, facts = cref.planted_continuum_model()
    arms = {}
    for arm in ("nebular", "lte"):
        sol = ref.solve(pd, t_rad, w, *(("lte", "lte") if arm == "lte" else ()))
        arms[arm] = (sol, cref.stage(pd, cd, sol, t_rad, w))
    return SimpleNamespace(pd=pd, cd=cd, t_rad=t_rad, w=w, facts=facts, arms=arms)


def test_the_planted_model_exercises_every_arm(planted):
    cref.assert_planted_facts(planted.pd, planted.cd, planted.arms["nebular"], planted.arms["lte"], planted.facts)


def mutated(cd, **fields):
    out = copy.copy(cd)
    for name, (index, value) in fields.items():
        a = np.array(getattr(cd, name)).copy()
        a[index] = value
        setattr(out, name, a)
    return out


# (field, index, value, what the message must name); level 51 is the only level of ion 3, the last ion of element 0
REFUSALS = [
    ("block_edge", 0, 1, "block_edge must run from 0"),
    ("block_edge", -1, 95, "block_edge must run from 0"),
    ("block_edge", 1, 1, "block 0 has 1 points"),
    ("block_edge", 2, 3, "block 1 has 1 points"),
    ("level", 0, -1, "level[0] = -1 lies outside"),
    ("level", 11, 300, "level[11] = 300 lies outside"),
    ("level", 3, 12, "level[3] = 12 does not ascend"),
    ("level", 4, 51, "level[4] = 51 belongs to ion 3, the last ion of its element"),
    ("level", 11, 299, "level[11] = 299 belongs to ion 11, the last ion of its element"),
    ("nu", 7, np.nan, "nu[7]"),
    ("nu", 7, np.inf, "nu[7]"),
    ("nu", 0, 0.0, "nu[0] = 0 is not finite and positive"),
    ("nu", 0, -1e15, "nu[0]"),
    ("x_sect", 40, -1e-18, "x_sect[40]"),
    ("x_sect", 129, np.nan, "x_sect[129]"),
    ("x_sect", 5, np.inf, "x_sect[5]"),
]


@pytest.mark.parametrize("field,index,value,word", REFUSALS)
def test_every_refusal_of_the_check(lib, planted, field, index, value, word):
    assert Engine.check_continuum_data(planted.cd, planted.pd) == (0, "")
    rc, msg = Engine.check_continuum_data(mutated(planted.cd, **{field: (index, value)}), planted.pd)
    assert rc == _abi.ERR_INVALID_ARGUMENT and word in msg, msg


def test_refusals_that_are_not_one_element_of_an_array(lib, planted):
    cd, pd = planted.cd, planted.pd
    # a nu that does not ascend inside its block: the third point of block 2 set to the second
    a = int(cd.block_edge[2])
    rc, msg = Engine.check_continuum_data(mutated(cd, nu=(a + 2, cd.nu[a + 1])), pd)
    assert rc == _abi.ERR_INVALID_ARGUMENT and f"nu[{a + 2}]" in msg and "ascend strictly inside block 2" in msg
    ion_edge = np.ascontiguousarray(pd.ion_level_edge, dtype=np.int64)
    elem_edge = np.ascontiguousarray(pd.element_ion_edge, dtype=np.int64)
    m = _abi.marshal_continuum_data(cd)
    args = (int(ion_edge[-1]), len(ion_edge) - 1, ion_edge.ctypes.data, elem_edge.ctypes.data)
    assert lib.tardis_mc_check_continuum_data(m.ref(), *args) == 0
    for name in ("level", "block_edge", "nu", "x_sect"):    # a missing pointer
        s = _abi.TardisMcContinuumData.from_buffer_copy(m.struct)
        setattr(s, name, None)
        assert lib.tardis_mc_check_continuum_data(_abi.C.byref(s), *args) == _abi.ERR_INVALID_ARGUMENT
        assert "pointer is missing" in lib.tardis_mc_last_error(None).decode()
    assert lib.tardis_mc_check_continuum_data(None, *args) == _abi.ERR_INVALID_ARGUMENT
    assert lib.tardis_mc_check_continuum_data(m.ref(), args[0], args[1], None, args[3]) == _abi.ERR_INVALID_ARGUMENT
    s = _abi.TardisMcContinuumData.from_buffer_copy(m.struct)
    s.n_continua = 0                                          # NC < 1
    assert lib.tardis_mc_check_continuum_data(_abi.C.byref(s), *args) == _abi.ERR_INVALID_ARGUMENT
    assert "n_continua = 0" in lib.tardis_mc_last_error(None).decode()
    bad = elem_edge.copy()
    bad[-1] += 1                                              # an element table that does not end at n_ions
    assert lib.tardis_mc_check_continuum_data(m.ref(), args[0], args[1], args[2], bad.ctypes.data) == _abi.ERR_INVALID_ARGUMENT
    assert "element_ion_edge" in lib.tardis_mc_last_error(None).decode()


def test_the_header_carries_the_prototypes_and_the_abi_version():
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    assert "#define TARDIS_MC_ABI_VERSION 2 " in header and _abi.ABI_VERSION == 2
    flat = re.sub(r"\s+", " ", header)
    for proto in ("int tardis_mc_set_continuum_data(TardisMcContext *ctx, const TardisMcContinuumData *data);",
                  "int tardis_mc_check_continuum_data(const TardisMcContinuumData *data, int64_t n_levels, int64_t n_ions, const int64_t *ion_level_edge, "
                  "const int64_t *element_ion_edge);",
                  "int tardis_mc_get_continuum_rates(TardisMcContext *ctx, double *phi_ik, double *alpha_sp, double *gamma, double *alpha_stim, "
                  "double *gamma_corr, double *coll_ion, double *coll_recomb);",
                  "int tardis_mc_get_continuum_opacity(TardisMcContext *ctx, double *chi_bf, double *ff_opacity_factor, double *t_electrons, "
                  "int64_t *n_negative_chi_bf, int64_t *n_negative_gamma_corr);",
                  "int tardis_mc_last_continuum_ms(TardisMcContext *ctx, double *out_thermal_ms, double *out_points_ms, double *out_rates_ms, "
                  "double *out_opacity_ms);",
                  "int tardis_mc_continuum_opacity(TardisMcContext *ctx, const TardisMcContinuumQuery *query);",
                  "typedef struct TardisMcContinuumData {", "typedef struct TardisMcContinuumQuery {"):
        assert proto in flat, proto
    # the three decisions that differ from the reference are stated where a caller reads them
    for words in ("n_i == 0.0: gamma_corr = gamma", "raises a PlasmaException", "indexes [-1]"):
        assert words in flat, words
    assert _abi.C.sizeof(_abi.TardisMcContinuumData) == 6 * 8 and _abi.C.sizeof(_abi.TardisMcContinuumQuery) == 8 * 8


def test_the_free_free_constant_is_one_literal_everywhere():
    literal = "3.6923492443190485e+08"
    assert float(literal) == cref.FF_OPAC_CONST == cref.ff_opac_const() and len(literal.split("e")[0].replace(".", "")) == 17
    assert abs(cref.FF_OPAC_CONST - 3.69e8) < 1e6
    for path in ("include/tardis_mc.h", "tardis_amd/csrc/continuum_opacity.hpp", "tests/continuum_ref.py"):
        assert literal in open(os.path.join(ROOT, path)).read(), path


def test_the_serial_trapezoid_agrees_with_numpy(planted, oracle):
    """Reordering a sum of n non-negative terms moves it by at most n 2^-52 of its value (each partial sum carries at most 2^-53 relative
    error per addition, and no term cancels): the serial sum against numpy's pairwise one, per block and shell."""
    models = [(planted.cd, planted.t_rad, planted.w, planted.pd.link_t_rad_t_electron)]
    prob = synthetic.make_problem(seed=1, n_packets=10, n_shells=7, n_lines=900, line_interaction_type="macroatom")
    ld = synthetic.make_line_data(1, prob.opacity_state, n_levels=400, time_explosion=prob.time_explosion)
    pd = synthetic.make_plasma_data(1, ld, 7)
    models.append((synthetic.make_continuum_data(1, pd, 9, lengths=(2, 3, 16, 17, 64, 65, 257, 40, 5)), np.linspace(14000.0, 5000.0, 7), np.full(7, 0.3), 0.9))
    for cd, t_rad, w, link in models:
        _, _, y_sp, y_g, y_st = cref.integrands(cd, np.asarray(t_rad, dtype=np.float64), np.asarray(w, dtype=np.float64), link)
        for y in (y_sp, y_g, y_st):
            assert np.all(y >= 0.0)
            for a, b in zip(cd.block_edge[:-1], cd.block_edge[1:]):
                mine, theirs = cref.trapezoid(cd.nu[a:b], y[a:b]), trapz(y[a:b], cd.nu[a:b], axis=0)
                assert np.all(np.abs(mine - theirs) <= (b - a) * 2.0 ** -52 * np.abs(theirs)), (a, b)


def expint_e1(u):
    """E1(u) = -gamma - ln u - sum_{k >= 1} (-u)^k / (k k!), 60 terms: for u <= 5 the terms stay below 5.3 in magnitude and the 61st is
    below 1e-40, so the value carries at most 60 * 5.3 * 2^-53 < 4e-14 of absolute error."""
    total, term = 0.0, 1.0
    for k in range(1, 61):
        term = term * (-u) / k
        total += term / k
    return -0.5772156649015329 - math.log(u) - total


def test_spontaneous_recombination_against_the_closed_form(oracle):
    """x_sect = a nu^-3 and W = 0: alpha_sp / phi_ik = T(y_sp) -> (8 pi a / c^2) (E1(h nu_i beta_e) - E1(h nu_max beta_e)), the second term
    the part of the integral above the last grid point.  The composite trapezoid rule on a uniform grid of spacing d is off by at most
    (d^2 / 12) max|y''| (nu_max - nu_i); y = C exp(-b nu) / nu has y'' = C exp(-b nu) (b^2 / nu + 2 b / nu^2 + 2 / nu^3), positive and
    falling, so its maximum is at nu_i.  To that bound come the series' 4e-14 per E1 and n 2^-52 of the sum for its roundings."""
    t_rad, link, a = np.array([10000.0]), 0.9, 3.0e27
    b = cref.H_PLANCK / (cref.K_BOLTZMANN * (link * t_rad[0]))
    nu_i, n = 1.0 / b, 4001                                   # u = h nu beta_e runs from 1 to 5
    d = 4.0 * nu_i / (n - 1)
    nu = nu_i + d * np.arange(n)
    cd = SimpleNamespace(nu=nu, x_sect=a / (nu * nu * nu), block_edge=np.array([0, n]))
    _, j, y_sp, y_g, y_st = cref.integrands(cd, t_rad, np.zeros(1), link)
    assert not j.any() and not y_g.any() and not y_st.any()  # W = 0: no field
    got = cref.trapezoid(nu, y_sp)[0]
    coef = 8.0 * np.pi * a / (cref.C_LIGHT * cref.C_LIGHT)
    exact = coef * (expint_e1(b * nu_i) - expint_e1(b * nu[-1]))
    second = coef * math.exp(-b * nu_i) * (b * b / nu_i + 2.0 * b / nu_i**2 + 2.0 / nu_i**3)
    spacing = float(np.max(np.diff(nu)))
    bound = spacing * spacing / 12.0 * second * (nu[-1] - nu_i) + coef * 2 * 4e-14 + n * 2.0 ** -52 * exact
    assert bound < 5e-6 * exact                              # the bound is a tight one: a few parts in a million
    assert 0.0 <= got - exact <= bound, (got, exact, bound)  # (y'' > 0: the trapezoid rule overestimates)


def test_the_query_restatement_on_a_hand_made_table(oracle):
    """Two overlapping blocks, one shell, integers times 1e15 Hz: every product, sum and quotient below is exact."""
    e = 1e15
    cd = SimpleNamespace(block_edge=np.array([0, 3, 5]), nu=np.array([1 * e, 2 * e, 4 * e, 3 * e, 5 * e]), x_sect=np.array([8.0, 4.0, 1.0, 6.0, 2.0]))
    out = {"chi_bf": np.array([[10.0], [20.0], [40.0], [3.0], [7.0]]), "ff_opacity_factor": np.array([2.0]), "t_electrons": np.array([1.0e4])}
    #        nu      n_current  block 0 (chi, x)   block 1 (chi, x)
    table = [(0.5 * e, 0, (0.0, 0.0), (0.0, 0.0)),       # below every threshold
             (1.0 * e, 1, (10.0, 8.0), (0.0, 0.0)),      # block 0's first point: the clip at 1 -> the first interval, its low end
             (1.5 * e, 1, (15.0, 6.0), (0.0, 0.0)),      # between points
             (2.0 * e, 1, (20.0, 4.0), (0.0, 0.0)),      # an interior grid point: side="left" -> the interval below it, its high end
             (3.0 * e, 2, (30.0, 2.5), (3.0, 6.0)),      # inside block 0, block 1's first point
             (4.0 * e, 2, (40.0, 1.0), (5.0, 4.0)),      # block 0's last point, the middle of block 1
             (4.5 * e, 1, (0.0, 0.0), (6.0, 3.0)),       # past block 0
             (5.0 * e, 1, (0.0, 0.0), (7.0, 2.0)),       # block 1's last point
             (6.0 * e, 0, (0.0, 0.0), (0.0, 0.0))]       # above every block
    nu = np.array([row[0] for row in table])
    got = cref.query(cd, out, nu, 0)
    assert got["n_current"].tolist() == [row[1] for row in table]
    assert got["chi_bf_each"].tolist() == [[row[2][0], row[3][0]] for row in table]
    assert got["x_sect_each"].tolist() == [[row[2][1], row[3][1]] for row in table]
    assert got["chi_bf_tot"].tolist() == [row[2][0] + row[3][0] for row in table]
    # chi_ff with the C library's exp: the transport's exp is within a few ulp of it, and 1 - exp(-x) at x >= 2.4 keeps that relative size
    beta_e = 1.0 / (cref.K_BOLTZMANN * 1.0e4)
    want = np.array([cref.FF_OPAC_CONST * 2.0 / v**3 * (1.0 - math.exp(-cref.H_PLANCK * v * beta_e)) for v in nu])
    assert np.all(np.abs(got["chi_ff"] - want) <= 1e-14 * want) and np.all(np.diff(got["chi_ff"]) < 0)
