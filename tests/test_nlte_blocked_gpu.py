"""The blocked form of the NLTE solve on the device (nlte_assemble / nlte_panel / nlte_trailing / nlte_backsolve kernels behind options
nlte_lds_levels and nlte_blocked_levels, and tardis_mc_debug_nlte_solve) against the unblocked NumPy yardstick
(tests/nlte_excitation_ref.py, tests/nlte_collision_ref.py): the plasma, x, the Boltzmann factors and every opacity table bit for bit --
on the small model with every species blocked (one level and fewer levels than a panel has columns included), at the LDS boundary, on
a species of 261 levels (nine panels, the last ragged; several strips and row blocks), along a chain of updates, with collisional
rates, through a singular species and back, and on random dense systems whose rows are swapped at nearly every step.  Every comparison
is array_equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nlte_blocked_ref as bref  # noqa: E402
import nlte_excitation_ref as nref  # noqa: E402
import test_nlte_collision_gpu as cg  # noqa: E402
import test_nlte_excitation_gpu as xg  # noqa: E402
from test_nlte_blocked_host import LONG_COUNTS, LONG_SPECIES, SIZES  # noqa: E402
from test_nlte_blocked_plan import shim  # noqa: E402,F401
from tardis_amd import _abi, synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

NB = bref.PANEL_COLUMNS


def stage(eng, m, lds_levels, blocked_levels, stage_of=xg.stage, **kw):
    stage_of(eng, m, **kw)
    eng.set_option("nlte_lds_levels", lds_levels)
    eng.set_option("nlte_blocked_levels", blocked_levels)


@pytest.fixture(scope="module")
def small(oracle):
    return {3: xg.Model(3), 20: xg.Model(20)}


@pytest.fixture(scope="module")
def long_model(oracle):
    m = xg.Model(2, counts=LONG_COUNTS, species=LONG_SPECIES)
    m.solved()
    return m


@pytest.mark.parametrize("shells", [3, 20])
def test_the_small_model_with_every_species_blocked_then_a_split_then_the_rule(small, shells):
    m = small[shells]
    want = m.solved()
    with Engine(0) as eng:
        for lds_levels, blocked_levels in ((0, 0), (0, 18), (-1, -1)):  # 1, 2, 17, 70 blocked | 70 blocked, the others one workgroup | LDS
            stage(eng, m, lds_levels, blocked_levels)
            eng.update_plasma(m.t_rad, m.w)
            xg.assert_equal(eng, want)
            assert eng.last_nlte_ms()["solve_ms"] > 0


def test_the_lds_boundary_blocked(oracle):
    m = xg.Model(3, counts=nref.BOUNDARY_COUNTS, species=nref.BOUNDARY_SPECIES)
    first = m.solved()
    with Engine(0) as eng:
        stage(eng, m, 0, 0)
        eng.update_plasma(m.t_rad, m.w)
        xg.assert_equal(eng, first)


def test_261_levels_nine_panels(long_model):
    m = long_model
    sol = m.solved()[0]
    steps = {k for (pos, s), ks in sol["swaps"].items() if pos == 1 for k in ks}  # species 1 of the data set: the ion of 261 levels
    assert sol["relative_populations"].shape == (22 + 261, 2) and np.all(sol["relative_populations"] > 0)
    assert len({k // NB for k in steps}) >= 3  # swaps in three different panels: the swap tables of several trailing launches are used
    with Engine(0) as eng:
        for lds_levels, blocked_levels in ((0, 0), (-1, -1)):
            stage(eng, m, lds_levels, blocked_levels)
            eng.update_plasma(m.t_rad, m.w)
            xg.assert_equal(eng, m.solved())
        # two calls give identical bits
        a = eng.get_nlte()
        stage(eng, m, 0, 0)
        eng.update_plasma(m.t_rad, m.w)
        b = eng.get_nlte()
        assert all(np.array_equal(a[k], b[k]) for k in xg.NLTE)


def test_a_chain_of_updates_on_261_levels(long_model):
    """Two mode pairs, each with the dilute and the detailed j, every update on the beta of the one before it."""
    m = long_model
    with Engine(0) as eng:
        stage(eng, m, 0, 0)
        xg.propagate(eng, m.prob)
        t, vol = m.prob.packet_collection.time_of_simulation, m.prob.geometry.volume
        rf = eng.radiation_field(t, vol, 1e-10, False)
        beta = None
        for ionization, excitation in (("nebular", "dilute-lte"), ("lte", "lte")):
            for j_mode, j in ((0, m.j0), (1, rf["j_blues"])):
                eng.update_plasma(m.t_rad, m.w, ionization, excitation, j_mode, time_of_simulation=t, volume=vol, w_epsilon=1e-10)
                want = m.reference(m.nd, j, beta, ionization, excitation)
                xg.assert_equal(eng, want)
                beta = want[1]["beta_sobolev"]


def test_collisional_rates_with_every_species_blocked(oracle):
    models = {name: cg.Model(entry) for name, entry in cg.cref.test_models().items()}
    with Engine(0) as eng:
        m = models["four"]
        stage(eng, m, 0, 0, stage_of=cg.stage)
        eng.update_plasma(m.t_rad, m.w)
        cg.assert_equal(eng, m.first())
        eng.update_plasma(m.t_rad, m.w)
        cg.assert_equal(eng, m.second())
        m = models["boundary"]
        stage(eng, m, 0, 0, stage_of=cg.stage)
        eng.update_plasma(m.t_rad, m.w)
        cg.assert_equal(eng, m.first())


def test_a_singular_species_in_the_blocked_form_fails_and_leaves_the_state(small):
    m = small[3]
    bad = synthetic.make_nlte_data(13, m.ld, m.pd, species=[2, 5, 3, 7], untouched_level=(3, 9))  # level 9 of the 17: no line
    with pytest.raises(nref.NlteSolveError) as e:
        nref.solve(m.pd, m.ld, bad, m.t_rad, m.w, m.j0)
    assert e.value.species == 3 and e.value.shell == 0 and e.value.step == 16
    with Engine(0) as eng:
        stage(eng, m, 0, 0)
        eng.update_plasma(m.t_rad, m.w)
        before, plasma = eng.get_opacity(**xg.ALL), eng.get_plasma()
        ran_before = xg.propagate(eng, m.prob)
        eng.set_nlte_data(bad)
        err = xg._error(lambda: eng.update_plasma(m.t_rad * 1.1, m.w))
        assert err.code == _abi.ERR_STATE and "species 3" in str(err) and "shell 0" in str(err) and "step 16" in str(err)
        after = eng.get_opacity(**xg.ALL)
        assert all(np.array_equal(after[k], before[k]) for k in xg.TABLES)
        assert xg._error(eng.get_plasma).code == _abi.ERR_STATE and xg._error(eng.get_nlte).code == _abi.ERR_STATE
        ran_after = xg.propagate(eng, m.prob)
        assert np.array_equal(ran_after.output_nus, ran_before.output_nus) and np.array_equal(ran_after.output_energies, ran_before.output_energies)
        eng.set_nlte_data(m.nd)
        eng.update_plasma(m.t_rad, m.w)
        xg.assert_equal(eng, m.reference(m.nd, m.j0, before["beta_sobolev"]))
        assert plasma["iterations"] > 0


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as eng:
        yield eng


@pytest.mark.parametrize("n", SIZES)
def test_debug_nlte_solve_on_random_dense_systems(engine, n):
    ms, bs = bref.random_systems(n, 2 if n == 261 else 4, seed=7)
    want = [nref.lu_solve(m, b) for m, b in zip(ms, bs)]
    assert n < 31 or all(len(swaps) > n // 2 for _, swaps in want)  # the reference swaps at more than half of the steps
    x, status = engine.debug_nlte_solve(ms, bs)
    assert status.tolist() == [0] * len(ms)
    for got, (ref_x, _) in zip(x, want):
        assert np.array_equal(got, ref_x), int((got != ref_x).sum())
    again, status = engine.debug_nlte_solve(ms, bs)
    assert status.tolist() == [0] * len(ms) and np.array_equal(again, x)  # two calls give identical bits


def test_debug_nlte_solve_status_words(engine):
    """n = 65 beside a good system: an all-zero column 40 (status 41); a NaN at (50, 3) (the step at which the reference raises); and
    x[0] == 0 by construction -- row and column 0 are e_0 and b[0] = 0, so nothing ever reaches b[0] and x[0] = 0.0 / 1.0."""
    n = 65
    ms, bs = bref.random_systems(n, 4, seed=3)
    ms[1][:, 40] = 0.0
    ms[2][50, 3] = np.nan
    ms[3][0, :], ms[3][:, 0], ms[3][0, 0], bs[3][0] = 0.0, 0.0, 1.0, 0.0
    want = []
    for m, b in zip(ms, bs):
        try:
            nref.lu_solve(m, b)
            want.append(0)
        except nref.NlteSolveError as e:
            want.append({"zero or non-finite pivot": 1 + e.step, "x[0] == 0": n + 1, "a population that is not finite": n + 2}[str(e).split(" (step")[0]])
    assert want == [0, 41, 4, n + 1]
    x, status = engine.debug_nlte_solve(ms, bs)
    assert status.tolist() == want
    assert np.array_equal(x[0], nref.lu_solve(ms[0], bs[0])[0])


def test_solve_form_agrees_with_the_plan(shim):  # noqa: F811
    rule = shim.constants["BLOCKED_FORM_LEVELS"]
    for n in (141, 142, rule - 1, rule, rule + 1):
        assert Engine.nlte_solve_form(n) == _abi.NLTE_FORMS[shim.form_shim(n, -1, -1)], n
    assert Engine.nlte_solve_form(141) == "lds" and Engine.nlte_solve_path(1071) == "global"
