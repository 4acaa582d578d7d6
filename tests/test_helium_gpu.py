"""helium_treatment recomb-nlte and delta_treatment in the device plasma step (tardis_mc_set_ionization_options / tardis_mc_update_plasma /
tardis_mc_get_helium) against their NumPy restatement (tests/helium_ref.py): populations, ion rows, partition functions, electron
densities, pass count and both helium arrays bit for bit in every arm, the opacity state behind the populations, options on / cleared /
on again in one context, what drops the options, a failed solve, the refusals, and the resident solver.

Models: the planted one (helium of 20 / 14 / 1 levels among 300 levels on 12 ions, 4 shells; He III of the cold shell far below the
1e-20 cut) and a synthetic one of 600 levels and 65 shells -- the ionisation workgroup gets a second wave with one live lane -- with
helium of 19 / 13 / 1 levels: neither sum a multiple of the eight loads the helium form issues at a time."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import helium_ref as href  # noqa: E402
import opacity_update_ref as oref  # noqa: E402
import plasma_update_ref as ref  # noqa: E402
from tardis_amd import _abi, state as st, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

# the seed of the synthetic model: the first for which the restatement's guard assertion (no delta of any pass within 1e-9 of the 5 %
# threshold) holds in every arm below, found on the CPU (seeds 1, 2, ... tried in order)
SEED, S, L, K, P = 1, 65, 1500, 600, 6000
HELIUM_LEVELS = (19, 13)
PLASMA = ("level_number_density", "ion_number_density", "partition_function", "electron_density")
TABLES = ("tau_sobolev", "beta_sobolev", "stimulated_emission_factor", "j_blues", "transition_probabilities")
ALL = dict(tau_sobolev=True, transition_probabilities=True, beta_sobolev=True, stimulated_emission_factor=True, j_blues=True)
# (helium_treatment, delta_treatment, excitation)
ARMS = {"helium": ("recomb-nlte", None, "dilute-lte"), "helium_delta": ("recomb-nlte", 1.0, "dilute-lte"), "delta": (None, 0.3, "dilute-lte"),
        "helium_lte_excitation": ("recomb-nlte", None, "lte")}


def synthetic_helium_model(seed=SEED):
    prob = synthetic.make_problem(seed=seed, n_packets=P, n_shells=S, n_lines=L, log_tau_mean=-2.0, line_interaction_type="macroatom")
    ld = synthetic.make_line_data(seed, prob.opacity_state, n_levels=K, time_explosion=prob.time_explosion)
    pd = synthetic.make_helium_plasma_data(seed, ld, S, helium_levels=HELIUM_LEVELS, n_elements=4, largest_ion=150)
    t_rad, w = np.linspace(14000.0, 5000.0, S), 0.4 / (1.0 + 0.1 * np.arange(S))
    return prob, ld, pd, t_rad, w


class Model:
    def __init__(self, prob, ld, pd, t_rad, w):
        self.prob, self.ld, self.pd, self.t_rad, self.w = prob, ld, pd, t_rad, w
        self.helium_element = href.helium_element_of(pd)
        self._solved = {}

    def solved(self, arm):
        """The reference plasma of an arm ("plain": no options), computed once and never written to."""
        if arm not in self._solved:
            if arm == "plain":
                self._solved[arm] = ref.solve(self.pd, self.t_rad, self.w)
            else:
                helium, delta, excitation = ARMS[arm]
                self._solved[arm] = href.solve(self.pd, self.t_rad, self.w, self.helium_element if helium else None, delta, excitation=excitation)
        return self._solved[arm]


@pytest.fixture(scope="module")
def models(oracle):
    pd, ld, prob, t_rad, w, facts = href.planted_helium_model()
    planted = Model(prob, ld, pd, t_rad, w)
    planted.facts = facts
    prob, ld, pd, t_rad, w = synthetic_helium_model()
    assert list(np.diff(pd.ion_level_edge)[:3]) == [19, 13, 1] and pd.number_density.shape[1] == 65
    return {"planted": planted, "synthetic": Model(prob, ld, pd, t_rad, w)}


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as eng:
        yield eng


def stage(eng, m, plasma=True):
    eng.set_geometry(m.prob.geometry, m.prob.time_explosion)
    eng.set_opacity(m.prob.opacity_state)
    eng.set_config(m.prob.montecarlo_configuration, m.prob.spectrum_frequency_grid)
    eng.set_line_data(m.ld)
    if plasma:
        eng.set_plasma_data(m.pd)


def update(eng, m, arm):
    helium, delta, excitation = ARMS[arm]
    eng.set_ionization_options(helium, None, delta)
    eng.update_plasma(m.t_rad, m.w, "nebular", excitation)


def propagate(eng, prob):
    eng.set_packets(prob.packet_collection)
    eng.reset_estimators()
    eng.propagate()
    eng.synchronize()
    return eng.get_results()


def assert_plasma_equal(got, want):
    assert got["iterations"] == want["iterations"]
    for name in PLASMA:
        assert got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), (name, int((got[name] != want[name]).sum()))


def assert_helium_equal(got, want):
    for mine, theirs in (("relative_population", "helium_relative"), ("level_number_density", "helium_population")):
        assert got[mine].shape == want[theirs].shape, mine
        assert np.array_equal(got[mine], want[theirs]), (mine, int((got[mine] != want[theirs]).sum()))


def assert_tables_equal(got, want):
    for name in TABLES:
        assert np.array_equal(got[name], want[name]), (name, int((got[name] != want[name]).sum()))


def _code(call):
    with pytest.raises((RuntimeError, NotImplementedError)) as e:
        call()
    return e.value.code


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_plasma_equals_the_restatement(engine, models, name, arm):
    m = models[name]
    want = m.solved(arm)
    stage(engine, m)
    update(engine, m, arm)
    assert_plasma_equal(engine.get_plasma(), want)
    if ARMS[arm][0]:
        assert_helium_equal(engine.get_helium(), want)
        assert engine.last_helium_ms()["relative_ms"] >= 0 and engine.last_plasma_update_ms()["ionization_ms"] > 0
    else:
        assert _code(engine.get_helium) == _abi.ERR_STATE and _code(engine.last_helium_ms) == _abi.ERR_STATE
    assert not np.array_equal(want["electron_density"], m.solved("plain")["electron_density"])
    if name == "planted" and arm == "helium":
        a = m.facts["helium_ions"][0]
        got = engine.get_plasma()["ion_number_density"]
        assert 0.0 < got[a + 2, 0] < 1e-100  # (no 1e-20 cut on the helium rows)


@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_both_partition_forms_give_the_same_bits(models, name):
    m = models[name]
    want = m.solved("helium")
    levels = np.diff(m.pd.ion_level_edge)
    with Engine(0) as eng:
        stage(eng, m)
        for threshold in (0, int(levels.max()) + 1):  # every ion on a 16-lane row | every ion on one lane
            eng.set_option("plasma_update_long_rows", threshold)
            update(eng, m, "helium")
            assert_plasma_equal(eng.get_plasma(), want)
            assert_helium_equal(eng.get_helium(), want)


@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_the_opacity_state_behind_the_populations(engine, models, name):
    m = models[name]
    sol = m.solved("helium")
    want = oref.update(m.ld, m.prob.opacity_state, m.prob.time_explosion, sol["level_number_density"], m.t_rad, m.w)
    stage(engine, m)
    update(engine, m, "helium")
    assert_tables_equal(engine.get_opacity(**ALL), want)
    # the same through update_opacity: no bit differs, and neither getter describes the resident populations any longer
    engine.update_opacity(sol["level_number_density"], sol["electron_density"], 0, t_radiative=m.t_rad, dilution_factor=m.w)
    assert_tables_equal(engine.get_opacity(**ALL), want)
    assert _code(engine.get_plasma) == _abi.ERR_STATE and _code(engine.get_helium) == _abi.ERR_STATE


def test_on_cleared_on_again_in_one_context(engine, models):
    m = models["synthetic"]
    stage(engine, m)
    out = []
    for arm in ("helium", "helium", None, "helium"):
        if arm is None:
            engine.set_ionization_options()
            engine.update_plasma(m.t_rad, m.w)
            assert _code(engine.get_helium) == _abi.ERR_STATE
            out.append((engine.get_plasma(), engine.get_opacity(**ALL), None))
        else:
            update(engine, m, arm)
            out.append((engine.get_plasma(), engine.get_opacity(**ALL), engine.get_helium()))
    assert_plasma_equal(out[0][0], m.solved("helium"))
    assert_plasma_equal(out[2][0], m.solved("plain"))
    for k in (1, 3):  # two identical updates give identical bits; the third update equals the first
        assert_plasma_equal(out[k][0], out[0][0])
        assert_tables_equal(out[k][1], out[0][1])
        for name in ("relative_population", "level_number_density"):
            assert np.array_equal(out[k][2][name], out[0][2][name])
    assert not np.array_equal(out[2][1]["tau_sobolev"], out[0][1]["tau_sobolev"])


def test_what_drops_the_options_and_what_does_not(models):
    m = models["planted"]
    nd = synthetic.make_nlte_data(5, m.ld, m.pd, species=[5])  # Fe II: no helium ion
    with Engine(0) as eng:
        stage(eng, m, plasma=False)
        assert _code(lambda: eng.set_ionization_options("recomb-nlte", 2)) == _abi.ERR_STATE      # before set_plasma_data
        assert eng._L.tardis_mc_set_ionization_options(eng._h, None) == _abi.ERR_STATE
        eng.set_plasma_data(m.pd)
        update(eng, m, "helium")
        assert_plasma_equal(eng.get_plasma(), m.solved("helium"))
        eng.set_nlte_data(nd)                    # keeps the options ...
        eng.set_nlte_data(None)
        eng.update_plasma(m.t_rad, m.w)
        assert_plasma_equal(eng.get_plasma(), m.solved("helium"))
        assert_helium_equal(eng.get_helium(), m.solved("helium"))
        eng.set_plasma_data(m.pd)                # ... set_plasma_data drops them
        assert eng.ionization_options is None and _code(eng.get_helium) == _abi.ERR_STATE
        eng.update_plasma(m.t_rad, m.w)
        assert_plasma_equal(eng.get_plasma(), m.solved("plain"))
        assert _code(eng.get_helium) == _abi.ERR_STATE
        # a refused call leaves none installed
        eng.set_ionization_options("recomb-nlte", None, 1.0)
        assert _code(lambda: eng.set_ionization_options("recomb-nlte", 0)) == _abi.ERR_INVALID_ARGUMENT  # element 0 has four ions
        assert "ions" in eng._L.tardis_mc_last_error(eng._h).decode()
        eng.update_plasma(m.t_rad, m.w)
        assert_plasma_equal(eng.get_plasma(), m.solved("plain"))
        for drop in (lambda: eng.set_line_data(m.ld), lambda: eng.set_opacity(m.prob.opacity_state)):
            eng.set_line_data(m.ld)
            eng.set_plasma_data(m.pd)
            eng.set_ionization_options("recomb-nlte")
            drop()
            assert eng.ionization_options is None
            assert _code(lambda: eng.set_ionization_options("recomb-nlte", 2)) == _abi.ERR_STATE


def test_a_failed_solve_and_the_refusals(models):
    m = models["planted"]
    sol = m.solved("helium")
    with Engine(0) as eng:
        stage(eng, m)
        update(eng, m, "helium")
        before = eng.get_opacity(**ALL)
        assert_plasma_equal(eng.get_plasma(), sol)
        # refusals: nothing resident changes, the getters answer as before
        def unchanged():
            assert_tables_equal(eng.get_opacity(**ALL), before)
            assert_plasma_equal(eng.get_plasma(), sol)
            assert_helium_equal(eng.get_helium(), sol)
        assert _code(lambda: eng.update_plasma(m.t_rad, m.w, "lte")) == _abi.ERR_INVALID_ARGUMENT   # helium with ionisation lte
        unchanged()
        eng.set_nlte_data(synthetic.make_nlte_data(5, m.ld, m.pd, species=[10]))                    # He II in NLTE as well
        assert _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_INVALID_ARGUMENT
        assert "helium" in eng._L.tardis_mc_last_error(eng._h).decode()
        unchanged()
        eng.set_nlte_data(None)
        # delta_treatment alone has no effect in lte: there is no delta in that formula
        eng.set_ionization_options(None, None, 0.3)
        eng.update_plasma(m.t_rad, m.w, "lte")
        assert_plasma_equal(eng.get_plasma(), ref.solve(m.pd, m.t_rad, m.w, "lte"))
        # a failed solve: the opacity state of before the call; get_plasma and get_helium have nothing to report until the next
        # successful update (tardis_mc_get_plasma's rule, which tests/test_plasma_update_gpu.py pins)
        update(eng, m, "helium")
        eng.set_option("plasma_max_iterations", 2)
        assert sol["iterations"] > 2 and _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_STATE
        assert_tables_equal(eng.get_opacity(**ALL), before)
        assert _code(eng.get_plasma) == _abi.ERR_STATE and _code(eng.get_helium) == _abi.ERR_STATE and _code(eng.last_helium_ms) == _abi.ERR_STATE
        eng.set_option("plasma_max_iterations", sol["iterations"])  # exactly enough
        eng.update_plasma(m.t_rad, m.w)
        unchanged()


def test_resident_solver(models):
    m = models["synthetic"]
    sol = m.solved("helium")
    grid = synthetic.make_spectrum_grid(1000)
    with Engine(0) as a, Engine(0) as b:
        solver = transport.MCTransportSolverHIP(grid, copy.copy(m.prob.montecarlo_configuration), line_interaction_type="macroatom", resident=True,
                                                engine=a)
        solver.set_line_data(m.ld)
        solver.set_plasma_data(m.pd)
        solver.set_ionization_options("recomb-nlte")
        ts = solver.initialize_transport_state(None, m.prob.geometry, m.prob.opacity_state, m.prob.time_explosion, n_packets=2000, iteration=0,
                                               temperature_inner=1.0e4)
        solver.run(ts)
        op = solver.update_plasma(m.t_rad, m.w)
        assert isinstance(op, transport.DeviceOpacityState) and a.resident_opacity is op
        assert np.array_equal(op.electron_density, sol["electron_density"])
        assert_helium_equal(a.get_helium(), sol)
        stage_config = lambda eng: eng.set_config(m.prob.montecarlo_configuration, m.prob.spectrum_frequency_grid)  # noqa: E731
        stage_config(a)
        ra = propagate(a, m.prob)
        stage(b, m, plasma=False)
        b.update_opacity(sol["level_number_density"], sol["electron_density"], 0, t_radiative=m.t_rad, dilution_factor=m.w)
        rb = propagate(b, m.prob)
        assert a.last_variant() == b.last_variant()
        assert np.array_equal(ra.output_nus, rb.output_nus) and np.array_equal(ra.output_energies, rb.output_energies)
        for name in st.LastInteractionTrackers.F64_FIELDS + st.LastInteractionTrackers.I64_FIELDS:
            assert np.array_equal(getattr(ra.trackers, name), getattr(rb.trackers, name), equal_nan=True), name
        for name in ("line_visits", "events", "macro_transitions", "rng_draws"):
            assert ra.counters[name] == rb.counters[name], name
        assert int((ra.trackers.interaction_type == 2).sum()) >= 100
