"""Collisional rates in the NLTE excitation stage of the device plasma update (tardis_mc_set_nlte_collision_data /
tardis_mc_update_plasma / tardis_mc_get_nlte_collision_rates) against the NumPy restatement of the contract
(tests/nlte_collision_ref.py): c_ul and c_lu, the level Boltzmann factors, the solutions x, the plasma and every opacity table bit for
bit -- over two updates (the second on the first's beta_sobolev AND the first's solved n_e), with the matrices in LDS, in HBM and split,
at the edges of the interpolation, through a level only collisions reach, out of the temperature grid, without the data again, and
through the resident solver.  Every comparison with the restatement is array_equal.

Models (nlte_collision_ref.test_models, 3 shells; tests/test_nlte_collision_host.py asserts that neither the collisional nor the
radiative term is drowned in any of them): the species of 2, 70, 1 and 17 levels with dense pairs on the 70 (2 415 pairs: every
256-thread loop wraps), sparse ones on the 17 and none on the others; the species of 141 and 142 levels, dense."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nlte_collision_ref as cref  # noqa: E402
import nlte_excitation_ref as nref  # noqa: E402
import opacity_update_ref as oref  # noqa: E402
from tardis_amd import _abi, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

PLASMA = ("level_number_density", "ion_number_density", "partition_function", "electron_density")
NLTE = ("level_boltzmann_factor", "relative_populations")
RATES = ("c_ul", "c_lu")
TABLES = ("tau_sobolev", "beta_sobolev", "stimulated_emission_factor", "j_blues", "transition_probabilities")
ALL = dict(tau_sobolev=True, transition_probabilities=True, beta_sobolev=True, stimulated_emission_factor=True, j_blues=True)


class Model:
    def __init__(self, entry):
        self.__dict__.update(entry)
        self.nu = np.asarray(self.prob.opacity_state.line_list_nu, dtype=np.float64)
        self.j0 = oref.j_blues_dilute_blackbody(self.nu, self.t_rad, self.w)
        self._first = {}

    def reference(self, beta, n_e, ionization="nebular", excitation="dilute-lte", j=None, cd="own", nd=None, t_rad=None):
        """(plasma, tables) of an update that finds ``beta`` (None: ones) and the electron density ``n_e`` resident."""
        cd = self.cd if isinstance(cd, str) else cd
        t_rad = self.t_rad if t_rad is None else t_rad
        j = (self.j0 if t_rad is self.t_rad else oref.j_blues_dilute_blackbody(self.nu, t_rad, self.w)) if j is None else j
        sol = cref.solve(self.pd, self.ld, self.nd if nd is None else nd, cd, t_rad, self.w, j, beta, n_e, ionization, excitation)
        return sol, oref.update(self.ld, self.prob.opacity_state, self.prob.time_explosion, sol["level_number_density"], j_blues=j)

    def first(self, ionization="nebular", excitation="dilute-lte"):
        """The reference of a first update after set_opacity (beta of ones, the opacity state's n_e), computed once, never written to."""
        key = (ionization, excitation)
        if key not in self._first:
            self._first[key] = self.reference(None, self.n_e0, ionization, excitation)
        return self._first[key]

    def second(self):
        if "second" not in self._first:
            sol, tables = self.first()
            self._first["second"] = self.reference(tables["beta_sobolev"], sol["electron_density"])
        return self._first["second"]


@pytest.fixture(scope="module")
def models(oracle):
    return {name: Model(entry) for name, entry in cref.test_models().items()}


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as eng:
        yield eng


def stage(eng, m, cd="own", nd=None):
    eng.set_option("nlte_lds_levels", -1)
    eng.set_geometry(m.prob.geometry, m.prob.time_explosion)
    eng.set_opacity(m.prob.opacity_state)
    eng.set_config(m.prob.montecarlo_configuration, m.prob.spectrum_frequency_grid)
    eng.set_line_data(m.ld)
    eng.set_plasma_data(m.pd)
    eng.set_nlte_data(m.nd if nd is None else nd)
    cd = m.cd if isinstance(cd, str) else cd
    if cd is not None:
        eng.set_nlte_collision_data(cd)


def assert_equal(eng, want, rates=True):
    sol, tables = want
    got = eng.get_plasma()
    assert got["iterations"] == sol["iterations"]
    if rates:
        r = eng.get_nlte_collision_rates()
        for name in RATES:
            assert r[name].shape == sol[name].shape, name
            assert np.array_equal(r[name], sol[name]), (name, int((r[name] != sol[name]).sum()))
    n = eng.get_nlte()
    for name in NLTE:
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


@pytest.mark.parametrize("ionization,excitation", [("nebular", "dilute-lte"), ("lte", "lte")])
def test_first_update_equals_the_restatement(engine, models, ionization, excitation):
    m = models["four"]
    want = m.first(ionization, excitation)
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w, ionization, excitation)
    assert_equal(engine, want)
    r = engine.get_nlte_collision_rates()
    pairs = np.diff(m.cd.species_pair_edge)
    assert pairs[1] == 2415 and 0 < pairs[3] < 136 and r["c_ul"].shape == (int(pairs.sum()), 3)
    assert np.all(r["c_ul"] > 0) and np.all(r["c_lu"] > 0) and not np.array_equal(r["c_ul"], r["c_lu"])
    assert set(engine.get_nlte_collision_rates(c_ul=False)) == {"c_lu"} and set(engine.get_nlte_collision_rates(c_lu=False)) == {"c_ul"}
    ms = engine.last_nlte_ms()
    assert set(ms) == {"assemble_ms", "solve_ms"} and ms["assemble_ms"] > 0 and ms["solve_ms"] > 0
    # the collisional rates are in the result: the run without them differs
    assert not np.array_equal(want[0]["relative_populations"], m.reference(None, m.n_e0, ionization, excitation, cd=None)[0]["relative_populations"])


def test_second_update_on_the_firsts_beta_and_electron_density(engine, models):
    m = models["four"]
    first, second = m.first(), m.second()
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w)
    assert_equal(engine, first)
    engine.update_plasma(m.t_rad, m.w)
    assert_equal(engine, second)
    # both "previous" inputs moved: beta, and the n_e the collisional terms are formed with
    assert first[1]["beta_sobolev"].min() < 1e-3 and not np.array_equal(first[0]["electron_density"], m.n_e0)
    assert np.array_equal(first[0]["c_ul"], second[0]["c_ul"])  # (the same t_rad) ...
    assert np.all(first[0]["c_ul"] * m.n_e0[None, :] != second[0]["c_ul"] * first[0]["electron_density"][None, :])  # ... other terms
    assert not np.array_equal(first[0]["relative_populations"], second[0]["relative_populations"])
    # fed the first's beta but the opacity state's n_e, the restatement is another one: the resident n_e is what the device read
    stale = m.reference(first[1]["beta_sobolev"], m.n_e0)
    assert not np.array_equal(stale[0]["relative_populations"], second[0]["relative_populations"])
    # another t_rad: other c, on the second's beta and n_e
    t_b = m.t_rad * 1.05
    engine.update_plasma(t_b, m.w)
    third = m.reference(second[1]["beta_sobolev"], second[0]["electron_density"], t_rad=t_b)
    assert_equal(engine, third)
    assert not np.array_equal(third[0]["c_ul"], first[0]["c_ul"])


def test_detailed_j_blues(engine, models):
    m = models["four"]
    stage(engine, m)
    engine.set_packets(m.prob.packet_collection)
    engine.reset_estimators()
    engine.propagate()
    engine.synchronize()
    res = engine.get_results()
    assert np.count_nonzero(res.j_blue_estimator) > 1000
    t, vol = m.prob.packet_collection.time_of_simulation, m.prob.geometry.volume
    rf = engine.radiation_field(t, vol, 1e-10, False)
    engine.update_plasma(m.t_rad, m.w, "nebular", "dilute-lte", 1, time_of_simulation=t, volume=vol, w_epsilon=1e-10)
    assert_equal(engine, m.reference(None, m.n_e0, j=rf["j_blues"]))


@pytest.mark.parametrize("name,thresholds", [("boundary", (-1, 0, 142)), ("four", (0, 18))])
def test_the_lds_form_the_global_form_and_a_split_give_the_same_bits(models, name, thresholds):
    """boundary: the rule (141 levels in LDS with more than 64 KiB of it, 142 in HBM) | both in HBM | the split forced through the
    option.  four: all in HBM | the 70 in HBM, the others in LDS (all in LDS: the other tests)."""
    m = models[name]
    want = m.first()
    if name == "boundary":
        assert [Engine.nlte_solve_path(n) for n in (141, 142)] == ["lds", "global"]
        assert list(np.diff(m.cd.species_pair_edge)) == [142 * 141 // 2, 141 * 140 // 2]
    with Engine(0) as eng:
        for threshold in thresholds:
            stage(eng, m)
            eng.set_option("nlte_lds_levels", threshold)
            eng.update_plasma(m.t_rad, m.w)
            assert_equal(eng, want)
        if name == "boundary":  # a second update in the global form on the first's beta and n_e
            eng.set_option("nlte_lds_levels", 0)
            eng.update_plasma(m.t_rad, m.w)
            assert_equal(eng, m.second())


def test_the_edges_of_the_interpolation(engine, models):
    """Shell 0: t_e in the first interval, where a share of the pairs has NaN at a bracketing knot; shell 1: t_e exactly a knot;
    shell 2: t_e in the last interval."""
    m = models["edges"]
    x = m.cd.collision_temperatures
    t_e = cref.electron_temperatures(m.pd, m.t_rad)
    assert x[0] < t_e[0] < x[1] and t_e[1] in x[2:-2] and x[-2] < t_e[2] < x[-1]
    want = m.first()
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w)  # succeeds
    assert_equal(engine, want)
    c_ul = engine.get_nlte_collision_rates()["c_ul"]
    holes = np.isnan(m.cd.C_ul[:, 0]) | np.isnan(m.cd.C_ul[:, 1])
    assert holes.sum() > 50 and np.all(c_ul[holes, 0] == 0.0) and np.all(c_ul[~holes, 0] > 0) and np.all(c_ul[:, 1:] > 0)
    knot = int(np.searchsorted(x, t_e[1]))
    slope = (m.cd.C_ul[:, knot] - m.cd.C_ul[:, knot - 1]) / (x[knot] - x[knot - 1])
    assert np.array_equal(c_ul[:, 1], slope * (x[knot] - x[knot - 1]) + m.cd.C_ul[:, knot - 1])  # (hi is the knot itself: side="left")


def test_a_species_without_pairs_keeps_the_bits_of_no_collision_data(engine, models):
    m = models["four"]
    assert list(np.diff(m.cd.species_pair_edge)[:3]) == [0, 2415, 0]
    stage(engine, m, cd=None)
    engine.update_plasma(m.t_rad, m.w)
    assert _error(engine.get_nlte_collision_rates).code == _abi.ERR_STATE
    plain = engine.get_nlte()
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w)
    with_c = engine.get_nlte()
    x0 = np.concatenate(([0], np.cumsum(np.diff(m.pd.ion_level_edge)[m.nd.species_ion])))  # the species' rows of x: 2, 70, 1 and 17 levels
    x, y = plain["relative_populations"], with_c["relative_populations"]
    for pos, same in enumerate((True, False, True, False)):  # 2 levels: no pairs | 70: dense | 1 level | 17: sparse
        assert np.array_equal(x[x0[pos]:x0[pos + 1]], y[x0[pos]:x0[pos + 1]]) == same, pos
        k0, k1 = m.pd.ion_level_edge[m.nd.species_ion[pos]], m.pd.ion_level_edge[m.nd.species_ion[pos] + 1]
        assert np.array_equal(plain["level_boltzmann_factor"][k0:k1], with_c["level_boltzmann_factor"][k0:k1]) == same, pos
    assert np.all(y[72] == 1.0)  # the species of one level
    # only one species with pairs: the others, the 17 included, keep the bits
    only70 = cref.collisions(m.pd, m.nd, (0.0, 1.0, 0.0, 0.0))
    stage(engine, m, cd=only70)
    engine.update_plasma(m.t_rad, m.w)
    assert_equal(engine, m.reference(None, m.n_e0, cd=only70))
    z = engine.get_nlte()["relative_populations"]
    assert np.array_equal(z[x0[3]:x0[4]], x[x0[3]:x0[4]]) and not np.array_equal(z[x0[1]:x0[2]], x[x0[1]:x0[2]])


def test_a_level_only_collisions_reach(models):
    m = models["reached"]
    with pytest.raises(nref.NlteSolveError):
        nref.solve(m.pd, m.ld, m.nd, m.t_rad, m.w, m.j0)
    with Engine(0) as eng:
        stage(eng, m, cd=None)
        err = _error(lambda: eng.update_plasma(m.t_rad, m.w))  # no line reaches level 9 of the 17: singular, as before
        assert err.code == _abi.ERR_STATE and "species 3" in str(err) and "step 16" in str(err)
        eng.set_nlte_collision_data(m.cd)
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, m.first())
        assert np.all(eng.get_nlte()["relative_populations"] > 0)


def test_an_electron_temperature_outside_the_grid_leaves_the_state(models):
    m = models["four"]
    narrow = cref.collisions(m.pd, m.nd, cref.FOUR_FRACTIONS, t_min=5000.0, t_max=20000.0)
    first = m.reference(None, m.n_e0, cd=narrow)
    with Engine(0) as eng:
        stage(eng, m, cd=narrow)
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, first)
        before, plasma, rates = eng.get_opacity(**ALL), eng.get_plasma(), eng.get_nlte_collision_rates()
        for factor, shell in ((2.2, 1), (0.5, 2)):  # t_e above the last knot, below the first; inside the zeta table both times
            t = m.t_rad.copy()
            t[shell] *= factor
            assert m.pd.zeta_temperatures[0] < t[shell] < m.pd.zeta_temperatures[-1]
            err = _error(lambda: eng.update_plasma(t, m.w))
            assert err.code == _abi.ERR_INVALID_ARGUMENT and f"shell {shell}" in str(err) and "collision temperatures" in str(err)
            after, plasma_after, rates_after = eng.get_opacity(**ALL), eng.get_plasma(), eng.get_nlte_collision_rates()
            assert all(np.array_equal(after[k], before[k]) for k in TABLES)
            assert all(np.array_equal(plasma_after[k], plasma[k]) for k in PLASMA) and all(np.array_equal(rates_after[k], rates[k]) for k in RATES)
        # the resident electron density and beta are the first update's: the next update is the restatement's second
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, m.reference(first[1]["beta_sobolev"], first[0]["electron_density"], cd=narrow))


def test_removal_and_what_drops_the_data(models):
    m = models["four"]
    never = m.reference(None, m.n_e0, cd=None)
    with Engine(0) as eng:
        eng.set_geometry(m.prob.geometry, m.prob.time_explosion)
        eng.set_opacity(m.prob.opacity_state)
        eng.set_config(m.prob.montecarlo_configuration, m.prob.spectrum_frequency_grid)
        eng.set_line_data(m.ld)
        eng.set_plasma_data(m.pd)
        assert _error(lambda: eng.set_nlte_collision_data(m.cd)).code == _abi.ERR_STATE  # no NLTE data
        stage(eng, m)
        assert eng.nlte_collision_data is m.cd
        eng.set_nlte_collision_data(None)
        assert eng.nlte_collision_data is None
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, never, rates=False)
        assert _error(eng.get_nlte_collision_rates).code == _abi.ERR_STATE
        # set_plasma_data drops it with the NLTE data; so does a new set_nlte_data
        stage(eng, m)
        eng.set_plasma_data(m.pd)
        assert eng.nlte_data is None and eng.nlte_collision_data is None
        eng.set_nlte_data(m.nd)
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, never, rates=False)
        stage(eng, m)
        eng.set_nlte_data(m.nd)
        assert eng.nlte_collision_data is None
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, never, rates=False)
        # a refused set leaves none installed
        bad = copy.copy(m.cd)
        bad.level_upper = m.cd.level_upper.copy()
        bad.level_upper[5] = 70
        stage(eng, m)
        assert _error(lambda: eng.set_nlte_collision_data(bad)).code == _abi.ERR_INVALID_ARGUMENT and eng.nlte_collision_data is None
        wrong = cref.collisions(models["boundary"].pd, models["boundary"].nd, 0.01)  # two species, not four
        assert _error(lambda: eng.set_nlte_collision_data(wrong)).code == _abi.ERR_INVALID_ARGUMENT
        eng.update_plasma(m.t_rad, m.w)
        assert_equal(eng, never, rates=False)
        # data without a pair: installed, nothing added
        eng.set_nlte_collision_data(synthetic.make_nlte_collision_data(13, m.pd, m.nd, pair_fraction=0.0))
        eng.set_opacity(m.prob.opacity_state)
        assert eng.nlte_collision_data is None


OK, STATE = 0, _abi.ERR_STATE
# what one call leaves of a complete chain: get_opacity(beta_sobolev) | get_plasma | get_nlte | get_nlte_collision_rates
LADDER = [
    ("set_nlte_collision_data", lambda eng, m, pop: eng.set_nlte_collision_data(m.cd), (OK, OK, OK, STATE)),
    ("set_nlte_data", lambda eng, m, pop: eng.set_nlte_data(m.nd), (OK, OK, STATE, STATE)),
    ("set_plasma_data", lambda eng, m, pop: eng.set_plasma_data(m.pd), (OK, STATE, STATE, STATE)),
    ("set_line_data", lambda eng, m, pop: eng.set_line_data(m.ld), (STATE, STATE, STATE, STATE)),
    ("set_opacity", lambda eng, m, pop: eng.set_opacity(m.prob.opacity_state), (STATE, STATE, STATE, STATE)),
    ("update_opacity", lambda eng, m, pop: eng.update_opacity(pop, t_radiative=m.t_rad, dilution_factor=m.w), (OK, STATE, STATE, STATE)),
]


def _code(call):
    try:
        call()
    except RuntimeError as e:
        return e.code
    return OK


@pytest.mark.parametrize("name,call,expect", LADDER, ids=[row[0] for row in LADDER])
def test_the_ladder_what_each_call_invalidates(engine, models, name, call, expect):
    """opacity -> line data -> plasma data -> NLTE data -> collision data: a call that replaces one rung drops the results that sit on
    it and on every rung below it, and nothing above (update_opacity: the populations are the caller's from then on)."""
    m = models["four"]
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w)
    populations = engine.get_plasma()["level_number_density"]
    getters = (lambda: engine.get_opacity(tau_sobolev=False, transition_probabilities=False, beta_sobolev=True), engine.get_plasma, engine.get_nlte,
               engine.get_nlte_collision_rates)
    assert tuple(_code(g) for g in getters) == (OK, OK, OK, OK)
    call(engine, m, populations)
    assert tuple(_code(g) for g in getters) == expect
    if name == "set_opacity":
        assert engine.get_opacity(transition_probabilities=False)["tau_sobolev"].shape == (engine.n_lines, engine.n_shells)


def test_the_resident_solver_over_two_iterations(models):
    """run -> update_plasma -> run -> update_plasma with NLTE and collision data installed on the solver, against the restatement fed by
    hand: the first update on beta of ones and the opacity state's n_e, the second on the first's beta and solved n_e."""
    m = models["four"]
    first, second = m.first(), m.second()
    grid = synthetic.make_spectrum_grid(1000)
    with Engine(0) as eng:
        solver = transport.MCTransportSolverHIP(grid, copy.copy(m.prob.montecarlo_configuration), line_interaction_type="macroatom", resident=True, engine=eng)
        solver.set_line_data(m.ld)
        solver.set_plasma_data(m.pd)
        solver.set_nlte_data(m.nd)
        solver.set_nlte_collision_data(m.cd)
        op = m.prob.opacity_state
        for iteration, want in enumerate((first, second)):
            ts = solver.initialize_transport_state(None, m.prob.geometry, op, m.prob.time_explosion, n_packets=3000, iteration=iteration, temperature_inner=1.0e4)
            solver.run(ts)
            op = solver.update_plasma(m.t_rad, m.w)
            assert eng.nlte_data is m.nd and eng.nlte_collision_data is m.cd
            assert np.array_equal(op.electron_density, want[0]["electron_density"]) and np.array_equal(op.tau_sobolev, want[1]["tau_sobolev"])
            assert_equal(eng, want)
        assert not np.array_equal(first[1]["tau_sobolev"], second[1]["tau_sobolev"])
    # a new engine: the solver installs both again
    with Engine(0) as eng:
        solver._engine = eng
        ts = solver.initialize_transport_state(None, m.prob.geometry, m.prob.opacity_state, m.prob.time_explosion, n_packets=3000, iteration=0, temperature_inner=1.0e4)
        solver.run(ts)
        solver.update_plasma(m.t_rad, m.w)
        assert eng.nlte_collision_data is m.cd
        assert_equal(eng, first)
