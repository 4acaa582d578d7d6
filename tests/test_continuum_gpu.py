"""The continuum stage of the device plasma step (tardis_mc_set_continuum_data / tardis_mc_update_plasma / tardis_mc_get_continuum_rates /
tardis_mc_get_continuum_opacity) and the batch query tardis_mc_continuum_opacity against their NumPy restatement
(tests/continuum_ref.py): the seven rate tables, chi_bf, the free-free factor, t_electrons and both clamp counts bit for bit in four
arms whose populations differ, the query's five outputs bit for bit on hand-placed frequencies, existing behaviour with the data
installed, the state rules, what drops the rung, and the resident solver.

Models: the planted one (continuum_ref.planted_continuum_model: twelve continua on ions of charge 0 .. 3, 4 shells, every arm of the
arithmetic planted) and a synthetic one of 600 levels and 65 shells -- a workgroup's second wave has one live lane -- with NC = 37
continua whose blocks have 2, 3, 16, 17, 64, 65, 257 and thirty other lengths: no multiple of a row, a wave or a workgroup's stride,
and neither is NP.  There is one form of every kernel, so there is no pair of forms to compare."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import continuum_ref as cref  # noqa: E402
import helium_ref as href  # noqa: E402
import nlte_excitation_ref as nref  # noqa: E402
import opacity_update_ref as oref  # noqa: E402
import plasma_update_ref as ref  # noqa: E402
from tardis_amd import _abi, state as st, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

# the synthetic model is that of tests/test_helium_gpu.py (seed 1: the restatement's guard assertion holds in every arm below)
SEED, S, L, K, P = 1, 65, 1500, 600, 6000
HELIUM_LEVELS = (19, 13)
NC = 37
LENGTHS = (2, 3, 16, 17, 64, 65, 257) + tuple(4 + (7 * j) % 29 for j in range(30))
PLASMA = ("level_number_density", "ion_number_density", "partition_function", "electron_density")
TABLES = ("tau_sobolev", "beta_sobolev", "stimulated_emission_factor", "j_blues", "transition_probabilities")
ALL = dict(tau_sobolev=True, transition_probabilities=True, beta_sobolev=True, stimulated_emission_factor=True, j_blues=True)
ARMS = ("nebular", "lte", "helium", "nlte")
COUNTS = ("n_negative_chi_bf", "n_negative_gamma_corr")
QUERY = ("chi_bf_tot", "chi_ff", "n_current", "chi_bf_each", "x_sect_each")


class Model:
    def __init__(self, prob, ld, pd, t_rad, w, cd, nlte_ion):
        self.prob, self.ld, self.pd, self.t_rad, self.w, self.cd = prob, ld, pd, t_rad, w, cd
        self.helium_element = href.helium_element_of(pd)
        self.nd = synthetic.make_nlte_data(SEED, ld, pd, species=[nlte_ion])
        self._solved = {}

    def solved(self, arm):
        """(the reference plasma of an arm, the continuum stage on it), computed once and never written to."""
        if arm not in self._solved:
            if arm == "nebular":
                sol = ref.solve(self.pd, self.t_rad, self.w)
            elif arm == "lte":
                sol = ref.solve(self.pd, self.t_rad, self.w, "lte", "lte")
            elif arm == "helium":
                sol = href.solve(self.pd, self.t_rad, self.w, self.helium_element)
            else:
                nu = np.asarray(self.prob.opacity_state.line_list_nu, dtype=np.float64)
                sol = nref.solve(self.pd, self.ld, self.nd, self.t_rad, self.w, oref.j_blues_dilute_blackbody(nu, self.t_rad, self.w))
            self._solved[arm] = (sol, cref.stage(self.pd, self.cd, sol, self.t_rad, self.w))
        return self._solved[arm]


def synthetic_model():
    prob = synthetic.make_problem(seed=SEED, n_packets=P, n_shells=S, n_lines=L, log_tau_mean=-2.0, line_interaction_type="macroatom")
    ld = synthetic.make_line_data(SEED, prob.opacity_state, n_levels=K, time_explosion=prob.time_explosion)
    pd = synthetic.make_helium_plasma_data(SEED, ld, S, helium_levels=HELIUM_LEVELS, n_elements=4, largest_ion=150)
    ld = synthetic.lines_within_ions(SEED, ld, pd)
    cd = synthetic.make_continuum_data(SEED, pd, NC, lengths=LENGTHS)
    t_rad, w = np.linspace(14000.0, 5000.0, S), 0.4 / (1.0 + 0.1 * np.arange(S))
    levels = np.diff(pd.ion_level_edge)
    nlte_ion = int(np.flatnonzero((levels >= 10) & (levels <= 40) & (np.arange(len(levels)) >= 3))[0])  # (no helium ion)
    return Model(prob, ld, pd, t_rad, w, cd, nlte_ion)


@pytest.fixture(scope="module")
def models(oracle):
    pd, ld, prob, t_rad, w, cd, facts = cref.planted_continuum_model()
    planted = Model(prob, ld, pd, t_rad, w, cd, 5)
    planted.facts = facts
    cref.assert_planted_facts(pd, cd, planted.solved("nebular"), planted.solved("lte"), facts)
    syn = synthetic_model()
    assert len(syn.cd.level) == NC and set((2, 3, 16, 17, 64, 65, 257)) <= set(np.diff(syn.cd.block_edge)) and syn.pd.number_density.shape[1] == 65
    assert len(syn.pd.level_energy) == K
    return {"planted": planted, "synthetic": syn}


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as eng:
        yield eng


def stage(eng, m, plasma=True, continuum=True):
    eng.set_geometry(m.prob.geometry, m.prob.time_explosion)
    eng.set_opacity(m.prob.opacity_state)
    eng.set_config(m.prob.montecarlo_configuration, m.prob.spectrum_frequency_grid)
    eng.set_line_data(m.ld)
    if plasma:
        eng.set_plasma_data(m.pd)
        if continuum:
            eng.set_continuum_data(m.cd)


def update(eng, m, arm):
    eng.set_nlte_data(m.nd if arm == "nlte" else None)
    eng.set_ionization_options("recomb-nlte" if arm == "helium" else None)
    if arm == "lte":
        eng.update_plasma(m.t_rad, m.w, "lte", "lte")
    else:
        eng.update_plasma(m.t_rad, m.w)


def propagate(eng, prob):
    eng.set_packets(prob.packet_collection)
    eng.reset_estimators()
    eng.propagate()
    eng.synchronize()
    return eng.get_results()


def assert_same(got, want, names):
    for name in names:
        assert np.shape(got[name]) == np.shape(want[name]), name
        assert np.array_equal(got[name], want[name]), (name, int(np.sum(np.asarray(got[name]) != np.asarray(want[name]))))


def assert_stage_equal(eng, out):
    assert_same(eng.get_continuum_rates(), out, cref.RATES)
    got = eng.get_continuum_opacity()
    assert_same(got, out, cref.OPACITY)
    for name in COUNTS:
        assert got[name] == out[name], (name, got[name], out[name])


def _code(call):
    with pytest.raises((RuntimeError, NotImplementedError)) as e:
        call()
    return e.value.code


def getters(eng):
    return (eng.get_continuum_rates, eng.get_continuum_opacity, lambda: eng.continuum_opacity([1e15], 0), eng.last_continuum_ms)


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_the_stage_equals_the_restatement(engine, models, name, arm):
    m = models[name]
    sol, out = m.solved(arm)
    stage(engine, m)
    update(engine, m, arm)
    got = engine.get_plasma()
    assert got["iterations"] == sol["iterations"]
    assert_same(got, sol, PLASMA)
    assert_stage_equal(engine, out)
    ms = engine.last_continuum_ms()
    assert set(ms) == {"thermal_ms", "points_ms", "rates_ms", "opacity_ms"} and all(v >= 0 for v in ms.values())
    assert engine.last_plasma_update_ms()["ionization_ms"] > 0
    if arm != "nebular":  # the populations differ between the arms, the stage must not
        assert not np.array_equal(sol["level_number_density"], m.solved("nebular")[0]["level_number_density"])
    if name == "planted":
        assert out["n_negative_chi_bf"] > 0 and (arm != "lte" or out["n_negative_gamma_corr"] > 0)


@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_batch_queries(engine, models, name):
    m = models[name]
    _, out = m.solved("nebular")
    stage(engine, m)
    update(engine, m, "nebular")
    nu, facts = cref.query_frequencies(m.cd)
    shells = m.pd.number_density.shape[1]
    # every hand-placed frequency in the first, a middle and the last shell
    qn = np.tile(nu, 3)
    qs = np.repeat(np.array([0, shells // 2, shells - 1]), len(nu))
    want = cref.query(m.cd, out, qn, qs)
    got = engine.continuum_opacity(qn, qs, each=True)
    assert_same(got, want, QUERY)
    assert got["n_current"].dtype == np.int64
    for q in (facts["below"], facts["above"]):
        assert got["n_current"][q] == 0 and got["chi_bf_tot"][q] == 0.0 and not got["chi_bf_each"][q].any() and got["chi_ff"][q] > 0.0
    assert got["n_current"][facts["crowded"]] == facts["crowded_count"] >= 2
    # a block's first frequency takes the first interval (the reference would index [-1]): the value at the first point, through one
    # product and one quotient by the interval -- two roundings, 2^-52 relative
    a = int(m.cd.block_edge[0])
    assert abs(got["x_sect_each"][0, 0] - m.cd.x_sect[a]) <= 2.0 ** -52 * m.cd.x_sect[a]
    assert abs(got["chi_bf_each"][0, 0] - out["chi_bf"][a, 0]) <= 2.0 ** -52 * out["chi_bf"][a, 0] and out["chi_bf"][a, 0] > 0
    # a batch of 1, a batch of 65 (a second wave with one live lane); without the per-continuum arrays the three vectors are the same
    one = engine.continuum_opacity(qn[3:4], int(qs[3]), each=True)
    assert_same(one, {k: v[3:4] for k, v in want.items()}, QUERY)
    rng = np.random.default_rng(3)
    lo, hi = m.cd.nu.min(), m.cd.nu.max()
    qn, qs = np.exp(rng.uniform(np.log(0.8 * lo), np.log(1.2 * hi), 65)), rng.integers(0, shells, 65)
    want = cref.query(m.cd, out, qn, qs)
    assert_same(engine.continuum_opacity(qn, qs, each=True), want, QUERY)
    assert_same(engine.continuum_opacity(qn, qs), want, QUERY[:3])
    assert len(set(want["n_current"])) >= 3


@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_existing_behaviour_with_the_data_installed(models, name):
    m = models[name]
    sol, out = m.solved("nebular")
    with Engine(0) as a, Engine(0) as b:
        stage(a, m)
        stage(b, m, continuum=False)
        for eng in (a, b):
            eng.update_plasma(m.t_rad, m.w)
        pa, pb = a.get_plasma(), b.get_plasma()
        assert pa["iterations"] == pb["iterations"]
        assert_same(pa, pb, PLASMA)
        assert_same(pa, sol, PLASMA)
        assert_same(a.get_opacity(**ALL), b.get_opacity(**ALL), TABLES)
        assert all(_code(g) == _abi.ERR_STATE for g in getters(b))
        ra, rb = propagate(a, m.prob), propagate(b, m.prob)
        assert a.last_variant() == b.last_variant()
        assert np.array_equal(ra.output_nus, rb.output_nus) and np.array_equal(ra.output_energies, rb.output_energies)
        for field in st.LastInteractionTrackers.F64_FIELDS + st.LastInteractionTrackers.I64_FIELDS:
            assert np.array_equal(getattr(ra.trackers, field), getattr(rb.trackers, field), equal_nan=True), field
        for field in ("line_visits", "events", "macro_transitions", "rng_draws"):
            assert ra.counters[field] == rb.counters[field], field
        # the stage's tables outlive a propagate; two updates give identical bits
        assert_stage_equal(a, out)
        first = (a.get_continuum_rates(), a.get_continuum_opacity(), a.get_opacity(**ALL))
        a.update_plasma(m.t_rad, m.w)
        assert_same(a.get_continuum_rates(), first[0], cref.RATES)
        assert_same(a.get_continuum_opacity(), first[1], cref.OPACITY + COUNTS)
        # removed: the getters answer ERR_STATE, the next update is the one of before
        a.set_continuum_data(None)
        assert a.continuum_data is None and all(_code(g) == _abi.ERR_STATE for g in getters(a)[:3])
        a.update_plasma(m.t_rad, m.w)
        assert all(_code(g) == _abi.ERR_STATE for g in getters(a))
        assert_same(a.get_plasma(), pb, PLASMA)
        assert_same(a.get_opacity(**ALL), first[2], TABLES)


def test_the_state_rules(models):
    m = models["planted"]
    sol, out = m.solved("nebular")
    with Engine(0) as eng:
        stage(eng, m)
        assert all(_code(g) == _abi.ERR_STATE for g in getters(eng))           # before any update
        eng.update_plasma(m.t_rad, m.w)
        assert_stage_equal(eng, out)
        eng.set_option("plasma_max_iterations", 1)                             # a failed update
        assert sol["iterations"] > 1 and _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_STATE
        assert all(_code(g) == _abi.ERR_STATE for g in getters(eng))
        eng.set_option("plasma_max_iterations", 1000)
        eng.update_plasma(m.t_rad, m.w)
        assert_stage_equal(eng, out)
        # the populations are the caller's from update_opacity on
        eng.update_opacity(sol["level_number_density"], sol["electron_density"], 0, t_radiative=m.t_rad, dilution_factor=m.w)
        assert all(_code(g) == _abi.ERR_STATE for g in getters(eng)[:3]) and _code(eng.get_plasma) == _abi.ERR_STATE
        eng.update_plasma(m.t_rad, m.w)                                        # the data are still installed
        assert_stage_equal(eng, out)
        eng.set_opacity(m.prob.opacity_state)
        assert all(_code(g) == _abi.ERR_STATE for g in getters(eng)[:3])
        # the query's host refusals; the tables are untouched by them
        eng.set_line_data(m.ld); eng.set_plasma_data(m.pd); eng.set_continuum_data(m.cd)
        eng.update_plasma(m.t_rad, m.w)
        shells = len(m.t_rad)
        for nu, shell, word in (([1e15], shells, "shell"), ([1e15], -1, "shell"), ([0.0], 0, "nu"), ([-1e15], 0, "nu"), ([np.nan], 0, "nu"),
                                ([np.inf], 0, "nu"), ([1e15, 1e15, np.nan], [0, 1, 2], "nu[2]")):
            assert _code(lambda: eng.continuum_opacity(nu, shell)) == _abi.ERR_INVALID_ARGUMENT
            assert word in eng._L.tardis_mc_last_error(eng._h).decode()
        assert_stage_equal(eng, out)
        empty = eng.continuum_opacity(np.zeros(0), np.zeros(0, dtype=np.int64), each=True)
        assert empty["chi_bf_tot"].shape == (0,) and empty["chi_bf_each"].shape == (0, len(m.cd.level))


def test_what_drops_the_rung_and_what_keeps_it(models):
    m = models["planted"]
    _, out = m.solved("nebular")
    with Engine(0) as eng:
        stage(eng, m, plasma=False)
        assert _code(lambda: eng.set_continuum_data(m.cd)) == _abi.ERR_STATE    # before set_plasma_data
        assert eng._L.tardis_mc_set_continuum_data(eng._h, None) == _abi.ERR_STATE
        eng.set_plasma_data(m.pd)
        eng.set_continuum_data(m.cd)
        nd = synthetic.make_nlte_data(5, m.ld, m.pd, species=[5])
        eng.set_nlte_data(nd)                                                   # these keep it ...
        eng.set_nlte_collision_data(synthetic.make_nlte_collision_data(5, m.pd, nd, pair_fraction=0.1))
        eng.set_nlte_data(None)
        eng.set_ionization_options(None, None, 0.3)
        eng.set_ionization_options()
        assert eng.continuum_data is m.cd
        eng.update_plasma(m.t_rad, m.w)
        assert_stage_equal(eng, out)
        # ... a refused call leaves none installed ...
        bad = copy.copy(m.cd)
        bad.x_sect = m.cd.x_sect.copy()
        bad.x_sect[3] = -1.0
        assert _code(lambda: eng.set_continuum_data(bad)) == _abi.ERR_INVALID_ARGUMENT
        assert "x_sect[3]" in eng._L.tardis_mc_last_error(eng._h).decode()
        assert all(_code(g) == _abi.ERR_STATE for g in getters(eng)[:3])
        # ... and whatever drops the plasma data drops it
        for drop in (lambda: eng.set_plasma_data(m.pd), lambda: eng.set_line_data(m.ld), lambda: eng.set_opacity(m.prob.opacity_state)):
            eng.set_line_data(m.ld)
            eng.set_plasma_data(m.pd)
            eng.set_continuum_data(m.cd)
            eng.update_plasma(m.t_rad, m.w)
            assert_stage_equal(eng, out)
            drop()
            assert eng.continuum_data is None and all(_code(g) == _abi.ERR_STATE for g in getters(eng)[:3])
        eng.set_line_data(m.ld)
        eng.set_plasma_data(m.pd)
        eng.update_plasma(m.t_rad, m.w)                                         # nothing installed: the stage does not run
        assert all(_code(g) == _abi.ERR_STATE for g in getters(eng))


def test_resident_solver(models):
    m = models["synthetic"]
    sol, out = m.solved("nebular")
    grid = synthetic.make_spectrum_grid(1000)
    with Engine(0) as a:
        solver = transport.MCTransportSolverHIP(grid, copy.copy(m.prob.montecarlo_configuration), line_interaction_type="macroatom", resident=True,
                                                engine=a)
        solver.set_line_data(m.ld)
        solver.set_plasma_data(m.pd)
        solver.set_continuum_data(m.cd)
        ts = solver.initialize_transport_state(None, m.prob.geometry, m.prob.opacity_state, m.prob.time_explosion, n_packets=2000, iteration=0,
                                               temperature_inner=1.0e4)
        solver.run(ts)
        assert a.continuum_data is m.cd
        op = solver.update_plasma(m.t_rad, m.w)
        assert isinstance(op, transport.DeviceOpacityState) and a.resident_opacity is op
        assert np.array_equal(op.electron_density, sol["electron_density"])
        edge = m.cd.block_edge
        assert np.array_equal(op.photo_ion_block_references, edge) and np.array_equal(op.phot_nus, m.cd.nu) and np.array_equal(op.x_sect, m.cd.x_sect)
        assert np.array_equal(op.photo_ion_nu_threshold_mins, m.cd.nu[edge[:-1]]) and np.array_equal(op.photo_ion_nu_threshold_maxs, m.cd.nu[edge[1:] - 1])
        assert np.array_equal(op.bf_threshold_list_nu, m.cd.nu[edge[:-1]])
        assert_same(solver.continuum_rates(), a.get_continuum_rates(), cref.RATES)
        assert_same(solver.continuum_rates(), out, cref.RATES)
        nu, _ = cref.query_frequencies(m.cd)
        assert_same(solver.continuum_opacity(nu, 7, each=True), a.continuum_opacity(nu, 7, each=True), QUERY)
        assert_same(solver.continuum_opacity(nu, 7, each=True), cref.query(m.cd, out, nu, 7), QUERY)
        assert np.array_equal(op.ff_opacity_factor, out["ff_opacity_factor"]) and np.array_equal(op.t_electrons, out["t_electrons"])
        # a handle read after the tables were replaced raises as the other tables do; what was fetched before stays
        # (the three continuum tables come in one fetch: op has them all, op2 below has none)
        op2 = solver.update_plasma(m.t_rad, m.w)
        op3 = solver.update_plasma(m.t_rad, m.w)
        assert np.array_equal(op.chi_bf, out["chi_bf"])
        for name in ("chi_bf", "ff_opacity_factor", "t_electrons", "tau_sobolev"):
            with pytest.raises(RuntimeError, match="replaced"):
                getattr(op2, name)
        assert np.array_equal(op3.chi_bf, out["chi_bf"]) and np.array_equal(op3.photo_ion_block_references, edge)
        # without continuum data the handle is what it was
        solver.set_continuum_data(None)
        op4 = solver.update_plasma(m.t_rad, m.w)
        assert a.continuum_data is None and op4.t_electrons is m.prob.opacity_state.t_electrons and not hasattr(op4, "phot_nus")
        with pytest.raises(AttributeError):
            op4.chi_bf
