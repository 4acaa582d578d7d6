"""NLTE excitation inside the device plasma update (tardis_mc_set_nlte_data / tardis_mc_update_plasma / tardis_mc_get_nlte) against the
NumPy restatement of the contract (tests/nlte_excitation_ref.py): the level Boltzmann factors, the solutions x, the plasma and every
opacity table bit for bit -- in all four mode pairs and both j modes, with the matrices in LDS, in HBM and split between the two, over
two consecutive updates (the second on the first's beta_sobolev), with coronal_approximation and classical_nebular, through a singular
species and back, without the data again, and through the resident solver.  Every comparison is array_equal.

Model (nlte_excitation_ref.model): 300 levels on 12 ions, 2000 lines each inside one ion, S = 3 and S = 20; the NLTE species have 2, 70,
1 and 17 levels (70: more than a wave's lanes, no multiple of 16, rows swapped late in the elimination), and the ion of 40 levels
between the 70 and the 17 is not NLTE."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nlte_excitation_ref as nref  # noqa: E402
import opacity_update_ref as oref  # noqa: E402
import plasma_update_ref as ref  # noqa: E402
from tardis_amd import _abi, state as st, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [(i, e) for i in ("nebular", "lte") for e in ("dilute-lte", "lte")]
PLASMA = ("level_number_density", "ion_number_density", "partition_function", "electron_density")
NLTE = ("level_boltzmann_factor", "relative_populations")
TABLES = ("tau_sobolev", "beta_sobolev", "stimulated_emission_factor", "j_blues", "transition_probabilities")
ALL = dict(tau_sobolev=True, transition_probabilities=True, beta_sobolev=True, stimulated_emission_factor=True, j_blues=True)


class Model:
    def __init__(self, n_shells, **kw):
        self.prob, self.ld, self.pd, self.nd = nref.model(n_shells, **kw)
        self.t_rad, self.w = self.pd.t_radiative, self.pd.dilution_factor
        self.nu = np.asarray(self.prob.opacity_state.line_list_nu, dtype=np.float64)
        self.j0 = oref.j_blues_dilute_blackbody(self.nu, self.t_rad, self.w)
        self._solved = {}

    def solved(self, ionization="nebular", excitation="dilute-lte"):
        """The reference of a first update (beta of ones) in j mode 0, computed once and never written to: (plasma, tables)."""
        key = (ionization, excitation)
        if key not in self._solved:
            self._solved[key] = self.reference(self.nd, self.j0, None, ionization, excitation)
        return self._solved[key]

    def reference(self, nd, j, beta, ionization="nebular", excitation="dilute-lte", t_rad=None, w=None):
        t_rad, w = self.t_rad if t_rad is None else t_rad, self.w if w is None else w
        sol = nref.solve(self.pd, self.ld, nd, t_rad, w, j, beta, ionization, excitation)
        return sol, oref.update(self.ld, self.prob.opacity_state, self.prob.time_explosion, sol["level_number_density"], j_blues=j)


@pytest.fixture(scope="module")
def models(oracle):
    return {3: Model(3), 20: Model(20)}


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as eng:
        yield eng


def stage(eng, m, nd="own"):
    eng.set_option("nlte_lds_levels", -1)
    eng.set_geometry(m.prob.geometry, m.prob.time_explosion)
    eng.set_opacity(m.prob.opacity_state)
    eng.set_config(m.prob.montecarlo_configuration, m.prob.spectrum_frequency_grid)
    eng.set_line_data(m.ld)
    eng.set_plasma_data(m.pd)
    nd = m.nd if isinstance(nd, str) else nd
    if nd is not None:
        eng.set_nlte_data(nd)


def propagate(eng, prob):
    eng.set_packets(prob.packet_collection)
    eng.reset_estimators()
    eng.propagate()
    eng.synchronize()
    return eng.get_results()


def assert_equal(eng, want, nlte=True):
    sol, tables = want
    got = eng.get_plasma()
    assert got["iterations"] == sol["iterations"]
    if nlte:
        n = eng.get_nlte()
        for name in NLTE:
            assert n[name].shape == sol[name].shape, name
            assert np.array_equal(n[name], sol[name]), (name, int((n[name] != sol[name]).sum()))
    for name in PLASMA:
        assert np.array_equal(got[name], sol[name]), (name, int((got[name] != sol[name]).sum()))
    t = eng.get_opacity(**ALL)
    for name in TABLES:
        assert np.array_equal(t[name], tables[name]), (name, int((t[name] != tables[name]).sum()))


def _error(call):
    with pytest.raises((RuntimeError, NotImplementedError)) as e:
        call()
    return e.value


@pytest.mark.parametrize("ionization,excitation", MODES)
@pytest.mark.parametrize("shells", [3, 20])
def test_first_update_equals_the_restatement(engine, models, shells, ionization, excitation):
    m = models[shells]
    want = m.solved(ionization, excitation)
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w, ionization, excitation)
    assert_equal(engine, want)
    x = engine.get_nlte()["relative_populations"]
    assert x.shape == (sum(nref.SPECIES_LEVELS), shells) and np.all(x > 0)
    # the species of one level: x = [1], lbf = g_0
    one = int(m.pd.ion_level_edge[3])
    assert np.all(x[72] == 1.0) and np.all(engine.get_nlte()["level_boltzmann_factor"][one] == m.pd.level_g[one])
    ms = engine.last_nlte_ms()
    assert ms["assemble_ms"] > 0 and ms["solve_ms"] > 0 and engine.last_plasma_update_ms()["partition_ms"] > 0
    # the rows of a solve were swapped late in the elimination: a kernel whose pivoting is wrong cannot pass
    assert any(k > 10 for steps in want[0]["swaps"].values() for k in steps)


@pytest.mark.parametrize("shells", [3, 20])
def test_detailed_j_blues(engine, models, shells):
    m = models[shells]
    stage(engine, m)
    res = propagate(engine, m.prob)
    assert np.count_nonzero(res.j_blue_estimator) > 1000
    t, vol = m.prob.packet_collection.time_of_simulation, m.prob.geometry.volume
    rf = engine.radiation_field(t, vol, 1e-10, False)
    assert not np.array_equal(rf["t_radiative"], m.t_rad)
    beta = None  # (the first update after a set_opacity; each later one runs on the beta of the one before)
    for ionization, excitation in MODES:
        engine.update_plasma(m.t_rad, m.w, ionization, excitation, 1, time_of_simulation=t, volume=vol, w_epsilon=1e-10)
        want = m.reference(m.nd, rf["j_blues"], beta, ionization, excitation)
        assert_equal(engine, want)
        beta = want[1]["beta_sobolev"]
    lines = m.nd.line_id
    assert (res.j_blue_estimator[lines] == 0).any() and (res.j_blue_estimator[lines] != 0).any()  # both branches of a detailed j


@pytest.mark.parametrize("shells", [3, 20])
def test_the_global_form_and_a_split_give_the_bits_of_the_lds_form(models, shells):
    m = models[shells]
    want = m.solved()
    assert {Engine.nlte_solve_path(n) for n in nref.SPECIES_LEVELS} == {"lds"}
    with Engine(0) as eng:
        stage(eng, m)
        for threshold in (0, 17, 18, 71, -1):  # all global | 17 and 70 global | 70 global | all LDS | the rule
            eng.set_opacity(m.prob.opacity_state)
            eng.set_line_data(m.ld)
            eng.set_plasma_data(m.pd)
            eng.set_nlte_data(m.nd)
            eng.set_option("nlte_lds_levels", threshold)
            eng.update_plasma(m.t_rad, m.w)
            assert_equal(eng, want)


@pytest.mark.parametrize("threshold", [0, 18])  # every species in the global form | 1, 2 and 17 levels in LDS, 70 in the global form
@pytest.mark.parametrize("shells", [3, 20])
def test_every_mode_pair_and_both_j_modes_in_the_global_form_and_a_split(models, shells, threshold):
    """One chain of eight updates -- the four mode pairs, each with the dilute and with the detailed j --, every update on the beta of
    the one before it, against the reference fed the same chain."""
    m = models[shells]
    with Engine(0) as eng:
        stage(eng, m)
        propagate(eng, m.prob)
        t, vol = m.prob.packet_collection.time_of_simulation, m.prob.geometry.volume
        rf = eng.radiation_field(t, vol, 1e-10, False)
        eng.set_option("nlte_lds_levels", threshold)
        beta = None
        for ionization, excitation in MODES:
            for j_mode, j in ((0, m.j0), (1, rf["j_blues"])):
                eng.update_plasma(m.t_rad, m.w, ionization, excitation, j_mode, time_of_simulation=t, volume=vol, w_epsilon=1e-10)
                want = m.reference(m.nd, j, beta, ionization, excitation)
                assert_equal(eng, want)
                beta = want[1]["beta_sobolev"]


def test_the_largest_lds_species_and_the_first_global_one(oracle):
    """141 levels: the LDS form with more than 64 KiB of dynamic LDS; 142: the global form under the rule.  Both again in the other form
    where that exists (142 levels do not fit the LDS whatever the option says)."""
    m = Model(3, counts=nref.BOUNDARY_COUNTS, species=nref.BOUNDARY_SPECIES)
    assert [Engine.nlte_solve_path(n) for n in (141, 142)] == ["lds", "global"]
    first = m.solved()
    assert all(len(steps) >= 3 and max(steps) > 10 for steps in first[0]["swaps"].values()) and np.all(first[0]["relative_populations"] > 0)
    with Engine(0) as eng:
        stage(eng, m)
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, first)
        eng.set_option("nlte_lds_levels", 0)
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, m.reference(m.nd, m.j0, first[1]["beta_sobolev"]))


def test_two_updates_the_second_on_the_firsts_beta(engine, models):
    m = models[20]
    first = m.solved()
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w)
    assert_equal(engine, first)
    t_b, w_b = m.t_rad * 1.05, m.w * 0.7
    j_b = oref.j_blues_dilute_blackbody(m.nu, t_b, w_b)
    second = m.reference(m.nd, j_b, first[1]["beta_sobolev"], t_rad=t_b, w=w_b)
    engine.update_plasma(t_b, w_b)
    assert_equal(engine, second)
    assert first[1]["beta_sobolev"].min() < 1e-3 and not np.array_equal(second[0]["relative_populations"], first[0]["relative_populations"])
    third = m.reference(m.nd, m.j0, second[1]["beta_sobolev"])
    engine.update_plasma(m.t_rad, m.w)
    assert_equal(engine, third)
    assert not np.array_equal(third[0]["relative_populations"], first[0]["relative_populations"])
    # after a set_opacity no update has produced a beta: 1.0 again
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w)
    assert_equal(engine, first)
    # two calls on the same inputs give identical bits
    engine.update_plasma(t_b, w_b)
    a = engine.get_nlte()
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w)
    engine.update_plasma(t_b, w_b)
    b = engine.get_nlte()
    assert all(np.array_equal(a[k], b[k]) for k in NLTE)


@pytest.mark.parametrize("flag", ["coronal_approximation", "classical_nebular"])
def test_the_two_flags(engine, models, flag):
    m = models[3]
    nd = copy.copy(m.nd)
    setattr(nd, flag, True)
    stage(engine, m, nd)
    first = m.reference(nd, m.j0, None)
    engine.update_plasma(m.t_rad, m.w)
    assert_equal(engine, first)
    second = m.reference(nd, m.j0, first[1]["beta_sobolev"])  # (classical_nebular ignores the beta, coronal_approximation the j)
    engine.update_plasma(m.t_rad, m.w)
    assert_equal(engine, second)
    plain = m.solved()[0]["relative_populations"]
    assert not np.array_equal(first[0]["relative_populations"], plain) or flag == "classical_nebular"
    if flag == "classical_nebular":
        assert np.array_equal(second[0]["relative_populations"], first[0]["relative_populations"])
    else:
        assert np.all(first[0]["relative_populations"][2:72][1:] >= 0.0)


def test_j_and_the_rows_of_other_ions(engine, models):
    m = models[20]
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w)
    with_nlte = engine.get_nlte()["level_boltzmann_factor"]
    # the j the reference used for the NLTE lines is the j the same update stored
    assert np.array_equal(engine.get_opacity(**ALL)["j_blues"][m.nd.line_id], m.j0[m.nd.line_id])
    # set_nlte_data(None): the existing reference, and the levels of the other ions keep their Boltzmann factors
    engine.set_nlte_data(None)
    assert _error(engine.get_nlte).code == _abi.ERR_STATE
    engine.update_plasma(m.t_rad, m.w)
    assert _error(engine.get_nlte).code == _abi.ERR_STATE and _error(engine.last_nlte_ms).code == _abi.ERR_STATE
    plain = ref.solve(m.pd, m.t_rad, m.w)
    got = engine.get_plasma()
    for name in PLASMA:
        assert np.array_equal(got[name], plain[name]), name
    edge = m.pd.ion_level_edge
    other = np.ones(len(m.pd.level_g), dtype=bool)
    for i in m.nd.species_ion:
        other[edge[i]:edge[i + 1]] = False
    assert other[edge[6]:edge[7]].all() and not other[edge[5]:edge[6]].any() and not other[edge[7]:edge[8]].any()
    assert np.array_equal(with_nlte[other], plain["level_boltzmann_factor"][other])
    assert not np.array_equal(with_nlte[~other], plain["level_boltzmann_factor"][~other])


def test_a_singular_species_fails_and_leaves_the_state(models):
    m = models[3]
    bad = synthetic.make_nlte_data(13, m.ld, m.pd, species=[2, 5, 3, 7], untouched_level=(3, 9))  # level 9 of the 17: no line
    with pytest.raises(nref.NlteSolveError) as e:
        nref.solve(m.pd, m.ld, bad, m.t_rad, m.w, m.j0)
    # the level's row of the matrix is exactly zero and stays so (0 - l * 0 in every step); the pivot search leaves it behind until
    # it is the last row: the zero pivot is met in the last step, whatever the other entries are
    assert e.value.species == 3 and e.value.shell == 0 and e.value.step == 16
    with Engine(0) as eng:
        stage(eng, m)
        eng.update_plasma(m.t_rad, m.w)
        before, plasma = eng.get_opacity(**ALL), eng.get_plasma()
        ran_before = propagate(eng, m.prob)
        eng.set_nlte_data(bad)
        err = _error(lambda: eng.update_plasma(m.t_rad * 1.1, m.w))
        assert err.code == _abi.ERR_STATE and "species 3" in str(err) and "shell 0" in str(err) and "step 16" in str(err)
        after = eng.get_opacity(**ALL)
        assert all(np.array_equal(after[k], before[k]) for k in TABLES)
        assert _error(eng.get_plasma).code == _abi.ERR_STATE and _error(eng.get_nlte).code == _abi.ERR_STATE
        # the resident electron density is that of before the call: the same packets scatter on the same electrons, and do not on others
        ran_after = propagate(eng, m.prob)
        assert np.array_equal(ran_after.output_nus, ran_before.output_nus) and np.array_equal(ran_after.output_energies, ran_before.output_energies)
        eng.update_opacity(plasma["level_number_density"], plasma["electron_density"] * 1.5, 0, t_radiative=m.t_rad, dilution_factor=m.w)
        assert not np.array_equal(propagate(eng, m.prob).output_nus, ran_before.output_nus)
        eng.update_opacity(plasma["level_number_density"], plasma["electron_density"], 0, t_radiative=m.t_rad, dilution_factor=m.w)
        assert np.array_equal(propagate(eng, m.prob).output_nus, ran_before.output_nus)
        # a following valid update succeeds: on the beta that is resident
        eng.set_nlte_data(m.nd)
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, m.reference(m.nd, m.j0, before["beta_sobolev"]))


def test_what_set_nlte_data_refuses(models):
    m = models[3]
    with Engine(0) as eng:
        eng.set_geometry(m.prob.geometry, m.prob.time_explosion)
        eng.set_opacity(m.prob.opacity_state)
        eng.set_config(m.prob.montecarlo_configuration, m.prob.spectrum_frequency_grid)
        eng.set_line_data(m.ld)
        assert _error(lambda: eng.set_nlte_data(m.nd)).code == _abi.ERR_STATE  # no plasma data
        eng.set_plasma_data(m.pd)
        nd = copy.copy(m.nd)
        nd.species_ion = np.array([2, 5, 3, 12])
        assert _error(lambda: eng.set_nlte_data(nd)).code == _abi.ERR_INVALID_ARGUMENT
        nd = copy.copy(m.nd)
        nd.line_id = m.nd.line_id.copy()
        nd.line_id[5] = nd.line_id[4]
        assert _error(lambda: eng.set_nlte_data(nd)).code == _abi.ERR_INVALID_ARGUMENT and eng.nlte_data is None
        eng.set_nlte_data(m.nd)
        eng.set_plasma_data(m.pd)  # drops the NLTE data
        assert eng.nlte_data is None
        eng.update_plasma(m.t_rad, m.w)
        assert _error(eng.get_nlte).code == _abi.ERR_STATE


def test_the_resident_solver_with_nlte_data(models):
    """run -> update_plasma -> run with NLTE data installed, against a fresh context given the reference's tables through set_opacity."""
    m = models[20]
    sol, tables = m.solved()
    grid = synthetic.make_spectrum_grid(1000)
    cfg = m.prob.montecarlo_configuration
    out = []
    for device in (True, False):
        with Engine(0) as eng:
            solver = transport.MCTransportSolverHIP(grid, copy.copy(cfg), line_interaction_type="macroatom", resident=True, engine=eng)
            op = m.prob.opacity_state
            if device:
                solver.set_line_data(m.ld)
                solver.set_plasma_data(m.pd)
                solver.set_nlte_data(m.nd)
                ts = solver.initialize_transport_state(None, m.prob.geometry, op, m.prob.time_explosion, n_packets=3000, iteration=0, temperature_inner=1.0e4)
                solver.run(ts)
                op = solver.update_plasma(m.t_rad, m.w)
                assert eng.nlte_data is m.nd and np.array_equal(op.electron_density, sol["electron_density"])
                assert np.array_equal(op.tau_sobolev, tables["tau_sobolev"])
            else:
                op = copy.copy(op)
                op.electron_density, op.tau_sobolev, op.transition_probabilities = sol["electron_density"], tables["tau_sobolev"], tables["transition_probabilities"]
            ts = solver.initialize_transport_state(None, m.prob.geometry, op, m.prob.time_explosion, n_packets=3000, iteration=1, temperature_inner=1.0e4)
            solver.run(ts)
            out.append((ts.output_nu.copy(), ts.output_energy.copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert len(np.unique(out[0][0])) > 1000
