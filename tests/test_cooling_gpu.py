"""The cooling sub-stage behind the continuum stage of the device plasma step (tardis_mc_get_cooling_rates / tardis_mc_get_kpacket_tables)
and the batch sampler tardis_mc_kpacket_sample against their NumPy restatement (tests/cooling_ref.py): the six rate tables, the
emission CDFs, the k-packet table and the count of degenerate CDFs bit for bit in four arms whose populations differ, the samplers'
three outputs bit for bit on hand-placed random numbers, existing behaviour with the sub-stage present, the state rules and the
resident solver.

Models: the planted one (continuum_ref.planted_continuum_model: S = 4, NC = 12, blocks of 2 .. 33 points, a degenerate CDF and
zero-width k_cdf entries planted) and the synthetic recipe of tests/test_continuum_gpu.py, built here by the same calls: S = 65 -- a
workgroup's second wave has one live lane --, NC = 37, block lengths including 2, 3, 16, 17, 64, 65, 257.  There is one form of every
kernel, so there is no pair of forms to compare.  Bitwise equality is the standard of the stage this sits behind: every operation is
IEEE or the project's own exp / log."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import continuum_ref as cref  # noqa: E402
import cooling_ref as kref  # noqa: E402
import helium_ref as href  # noqa: E402
import nlte_excitation_ref as nref  # noqa: E402
import opacity_update_ref as oref  # noqa: E402
import plasma_update_ref as ref  # noqa: E402
from tardis_amd import _abi, state as st, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, S, L, K, P = 1, 65, 1500, 600, 6000
HELIUM_LEVELS = (19, 13)
NC = 37
LENGTHS = (2, 3, 16, 17, 64, 65, 257) + tuple(4 + (7 * j) % 29 for j in range(30))
PLASMA = ("level_number_density", "ion_number_density", "partition_function", "electron_density")
OPACITY_TABLES = ("tau_sobolev", "beta_sobolev", "stimulated_emission_factor", "j_blues", "transition_probabilities")
ALL = dict(tau_sobolev=True, transition_probabilities=True, beta_sobolev=True, stimulated_emission_factor=True, j_blues=True)
ARMS = ("nebular", "lte", "helium", "nlte")
SAMPLE = ("kind", "continuum", "nu")


class Model:
    def __init__(self, prob, ld, pd, t_rad, w, cd, nlte_ion):
        self.prob, self.ld, self.pd, self.t_rad, self.w, self.cd = prob, ld, pd, t_rad, w, cd
        self.helium_element = href.helium_element_of(pd)
        self.nd = synthetic.make_nlte_data(SEED, ld, pd, species=[nlte_ion])
        self._solved = {}

    def solved(self, arm):
        """(the reference plasma of an arm, the continuum stage on it, the cooling sub-stage on both), computed once and never written to."""
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
            out = cref.stage(self.pd, self.cd, sol, self.t_rad, self.w)
            self._solved[arm] = (sol, out, kref.stage(self.pd, self.cd, sol, out, self.prob.time_explosion))
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
    syn = synthetic_model()
    assert len(syn.cd.level) == NC and set((2, 3, 16, 17, 64, 65, 257)) <= set(np.diff(syn.cd.block_edge)) and syn.pd.number_density.shape[1] == 65
    assert len(planted.cd.level) == 12 and len(planted.t_rad) == 4 and set(np.diff(planted.cd.block_edge)) >= {2, 33}
    return {"planted": planted, "synthetic": syn}


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as eng:
        yield eng


def stage(eng, m, continuum=True):
    eng.set_geometry(m.prob.geometry, m.prob.time_explosion)
    eng.set_opacity(m.prob.opacity_state)
    eng.set_config(m.prob.montecarlo_configuration, m.prob.spectrum_frequency_grid)
    eng.set_line_data(m.ld)
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


def assert_cooling_equal(eng, cool):
    assert_same(eng.get_cooling_rates(), cool, kref.RATES + kref.SHELL)
    got = eng.get_kpacket_tables()
    assert_same(got, cool, kref.TABLES)
    assert got["n_degenerate_fb_cdf"] == cool["n_degenerate_fb_cdf"], (got["n_degenerate_fb_cdf"], cool["n_degenerate_fb_cdf"])


def _code(call):
    with pytest.raises((RuntimeError, NotImplementedError)) as e:
        call()
    return e.value.code


def getters(eng):
    """The new getters, then the getter whose state rule they follow."""
    return (eng.get_cooling_rates, eng.get_kpacket_tables, lambda: eng.kpacket_sample(0, [0.5], [0.5]), eng.last_cooling_ms), eng.get_continuum_rates


def assert_all_refuse(eng, timer=True):
    new, old = getters(eng)
    assert _code(old) == _abi.ERR_STATE
    assert all(_code(g) == _abi.ERR_STATE for g in (new if timer else new[:3]))


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_the_tables_equal_the_restatement(engine, models, name, arm):
    m = models[name]
    sol, out, cool = m.solved(arm)
    stage(engine, m)
    update(engine, m, arm)
    assert_same(engine.get_plasma(), sol, PLASMA)
    assert_same(engine.get_continuum_rates(), out, cref.RATES)
    assert_cooling_equal(engine, cool)
    assert engine.get_kpacket_tables(fb_emission_cdf=False).keys() == {"k_cdf", "n_degenerate_fb_cdf"}
    ms = engine.last_cooling_ms()
    assert set(ms) == {"points_ms", "blocks_ms", "table_ms"} and all(v >= 0 for v in ms.values())
    assert np.all(cool["k_cdf"][-1] == 1.0)
    if arm != "nebular":  # the populations differ between the arms
        assert not np.array_equal(sol["level_number_density"], m.solved("nebular")[0]["level_number_density"])
    if name == "planted" and arm in ("nebular", "lte"):
        assert cool["degenerate"][9, 0] and cool["n_degenerate_fb_cdf"] >= 1 and int((cool["cool_rate_fb"] == 0.0).sum()) in (13, 14)


@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_the_samplers_on_hand_placed_numbers(engine, models, name):
    m = models[name]
    _, out, cool = m.solved("nebular")
    stage(engine, m)
    update(engine, m, "nebular")
    shells, n_cont = len(m.t_rad), len(m.cd.level)
    # the kind: both ends of every entry of positive width, in every shell; z_nu = 0.375 for those that emit
    shell, z, entry = kref.process_batch(cool)
    z_nu = np.full(len(z), 0.375)
    want = kref.sample(m.cd, out, cool, shell, z, z_nu)
    got = engine.kpacket_sample(shell, z, z_nu)
    assert_same(got, want, SAMPLE)
    assert got["kind"].dtype == np.int64 and got["continuum"].dtype == np.int64
    chosen = np.where(want["kind"] < 2, want["kind"], np.where(want["kind"] == 2, 2 + want["continuum"], 2 + n_cont + want["continuum"]))
    assert np.array_equal(chosen[entry >= 0], entry[entry >= 0]) and np.all(cool["rates"][chosen, shell] > 0.0)
    assert set(want["kind"]) == {0, 1, 2, 3} and np.all((want["nu"] == 0.0) == ((want["kind"] == 1) | (want["kind"] == 3)))
    # the free-bound frequency: every continuum forced, in the first, a middle and the last shell, z_nu at every CDF grid value below 1,
    # at the midpoints, at 0.0 and at 1 - 2^-53 -- the two-point block and (planted) the degenerate block among them
    cont, shell, z_nu = kref.free_bound_batch(m.cd, cool, sorted({0, shells // 2, shells - 1}))
    assert set(cont) == set(range(n_cont))
    half = np.full(len(z_nu), 0.5)
    want = kref.sample(m.cd, out, cool, shell, half, z_nu, np.full(len(z_nu), 2), cont)
    got = engine.kpacket_sample(shell, half, z_nu, 2, cont)
    assert_same(got, want, SAMPLE)
    assert np.all(np.isfinite(want["nu"])) and np.all(want["nu"] > 0.0)
    # free-free, forced and sampled; z_nu = 0.0 gives +inf
    z_ff = np.array([0.0, 2.0 ** -1022, 2.0 ** -53, 0.25, np.exp(-1.0), 0.75, 1.0 - 2.0 ** -53])
    for s in sorted({0, shells - 1}):
        want = kref.sample(m.cd, out, cool, np.full(len(z_ff), s), z_ff, z_ff, np.zeros(len(z_ff), dtype=np.int64), np.full(len(z_ff), -1))
        got = engine.kpacket_sample(s, z_ff, z_ff, 0)
        assert_same(got, want, SAMPLE)
        assert want["nu"][0] == np.inf and np.all(np.diff(want["nu"]) < 0.0) and np.all(want["continuum"] == -1)
    # the kinds that emit nothing, forced: coll_ion keeps its continuum
    got = engine.kpacket_sample(0, [0.5, 0.5], [0.5, 0.5], [1, 3], [-1, n_cont - 1])
    assert got["kind"].tolist() == [1, 3] and got["continuum"].tolist() == [-1, n_cont - 1] and got["nu"].tolist() == [0.0, 0.0]
    # a batch of 1 and a batch of 65 (a second wave with one live lane), everything sampled
    rng = np.random.default_rng(3)
    shell, z, z_nu = rng.integers(0, shells, 65), rng.random(65), rng.random(65)
    want = kref.sample(m.cd, out, cool, shell, z, z_nu)
    assert_same(engine.kpacket_sample(shell, z, z_nu), want, SAMPLE)
    assert_same(engine.kpacket_sample(int(shell[7]), z[7:8], z_nu[7:8]), {k: v[7:8] for k, v in want.items()}, SAMPLE)
    empty = engine.kpacket_sample(np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0))
    assert empty["kind"].shape == (0,) and empty["nu"].shape == (0,)


@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_existing_behaviour_with_the_sub_stage_present(models, name):
    """Engine a fetches every new table and samples before it reads anything else; engine b runs the same update and calls no new
    getter.  Everything the update had before is the same in both, bit for bit, and equals the restatement."""
    m = models[name]
    sol, out, cool = m.solved("nebular")
    with Engine(0) as a, Engine(0) as b:
        for eng in (a, b):
            stage(eng, m)
            eng.update_plasma(m.t_rad, m.w)
        assert_cooling_equal(a, cool)
        a.kpacket_sample(0, [0.25, 0.5], [0.5, 0.75])
        a.last_cooling_ms()
        pa, pb = a.get_plasma(), b.get_plasma()
        assert pa["iterations"] == pb["iterations"] == sol["iterations"]
        assert_same(pa, pb, PLASMA)
        assert_same(pb, sol, PLASMA)
        for eng in (a, b):
            assert_same(eng.get_continuum_rates(), out, cref.RATES)
            got = eng.get_continuum_opacity()
            assert_same(got, out, cref.OPACITY)
            assert got["n_negative_chi_bf"] == out["n_negative_chi_bf"] and got["n_negative_gamma_corr"] == out["n_negative_gamma_corr"]
            assert set(eng.last_continuum_ms()) == {"thermal_ms", "points_ms", "rates_ms", "opacity_ms"}
        assert_same(a.get_opacity(**ALL), b.get_opacity(**ALL), OPACITY_TABLES)
        ra, rb = propagate(a, m.prob), propagate(b, m.prob)
        assert a.last_variant() == b.last_variant()
        assert np.array_equal(ra.output_nus, rb.output_nus) and np.array_equal(ra.output_energies, rb.output_energies)
        for field in st.LastInteractionTrackers.F64_FIELDS + st.LastInteractionTrackers.I64_FIELDS:
            assert np.array_equal(getattr(ra.trackers, field), getattr(rb.trackers, field), equal_nan=True), field
        for field in ("line_visits", "events", "macro_transitions", "rng_draws"):
            assert ra.counters[field] == rb.counters[field], field
        # the tables outlive a propagate; two updates give identical bits
        assert_cooling_equal(b, cool)
        first = (b.get_cooling_rates(), b.get_kpacket_tables())
        b.update_plasma(m.t_rad, m.w)
        assert_same(b.get_cooling_rates(), first[0], kref.RATES + kref.SHELL)
        assert_same(b.get_kpacket_tables(), first[1], kref.TABLES + ("n_degenerate_fb_cdf",))
        # without continuum data the sub-stage does not run
        b.set_continuum_data(None)
        assert_all_refuse(b, timer=False)
        b.update_plasma(m.t_rad, m.w)
        assert_all_refuse(b)
        assert_same(b.get_plasma(), sol, PLASMA)


def test_the_state_rules(models):
    m = models["planted"]
    sol, out, cool = m.solved("nebular")
    with Engine(0) as eng:
        stage(eng, m)
        assert_all_refuse(eng)                                                 # before any update
        eng.update_plasma(m.t_rad, m.w)
        assert_cooling_equal(eng, cool)
        eng.set_option("plasma_max_iterations", 1)                             # a failed update
        assert sol["iterations"] > 1 and _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_STATE
        assert_all_refuse(eng)
        eng.set_option("plasma_max_iterations", 1000)
        eng.update_plasma(m.t_rad, m.w)
        assert_cooling_equal(eng, cool)
        # the populations are the caller's from update_opacity on
        eng.update_opacity(sol["level_number_density"], sol["electron_density"], 0, t_radiative=m.t_rad, dilution_factor=m.w)
        assert_all_refuse(eng, timer=False)
        eng.update_plasma(m.t_rad, m.w)                                        # the data are still installed
        assert_cooling_equal(eng, cool)
        # what keeps the continuum data keeps these, what drops them drops these
        eng.set_ionization_options(None, None, 0.3)
        eng.set_ionization_options()
        eng.update_plasma(m.t_rad, m.w)
        assert_cooling_equal(eng, cool)
        for drop in (lambda: eng.set_plasma_data(m.pd), lambda: eng.set_line_data(m.ld), lambda: eng.set_opacity(m.prob.opacity_state),
                     lambda: eng.set_continuum_data(None)):
            drop()
            assert_all_refuse(eng, timer=False)
            eng.set_line_data(m.ld); eng.set_plasma_data(m.pd); eng.set_continuum_data(m.cd)
            assert_all_refuse(eng, timer=False)
            eng.update_plasma(m.t_rad, m.w)
            assert_cooling_equal(eng, cool)
        # the query's host refusals; the tables are untouched by them
        shells, n_cont = len(m.t_rad), len(m.cd.level)
        ok = dict(shell=0, z_process=[0.5], z_nu=[0.5], force_kind=None, force_continuum=None)
        eng.kpacket_sample(**ok)
        for change, word in ((dict(shell=shells), "shell"), (dict(shell=-1), "shell"),
                             (dict(z_process=[1.0]), "z_process"), (dict(z_process=[-2.0 ** -60]), "z_process"), (dict(z_process=[np.nan]), "z_process"),
                             (dict(z_process=[np.inf]), "z_process"), (dict(z_nu=[1.0]), "z_nu"), (dict(z_nu=[-1.0]), "z_nu"), (dict(z_nu=[np.nan]), "z_nu"),
                             (dict(z_nu=[-np.inf]), "z_nu"), (dict(z_process=[0.5, 0.5, np.nan], z_nu=[0.5] * 3), "z_process[2]"),
                             (dict(force_kind=2, force_continuum=n_cont), "force_continuum"), (dict(force_kind=2, force_continuum=-1), "force_continuum"),
                             (dict(force_kind=3, force_continuum=-2), "force_continuum"), (dict(force_kind=2), "force_continuum"),
                             (dict(force_kind=0, force_continuum=0), "force_continuum"), (dict(force_continuum=0), "force_continuum"),
                             (dict(force_kind=4), "force_kind"), (dict(force_kind=-2), "force_kind")):
            assert _code(lambda: eng.kpacket_sample(**dict(ok, **change))) == _abi.ERR_INVALID_ARGUMENT, change
            assert word in eng._L.tardis_mc_last_error(eng._h).decode(), change
        assert_cooling_equal(eng, cool)


def test_resident_solver(models):
    m = models["synthetic"]
    sol, out, cool = m.solved("nebular")
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
        op = solver.update_plasma(m.t_rad, m.w)
        assert np.array_equal(op.electron_density, sol["electron_density"])
        assert_same(solver.cooling_rates(), cool, kref.RATES + kref.SHELL)
        rng = np.random.default_rng(5)
        shell, z, z_nu = rng.integers(0, S, 40), rng.random(40), rng.random(40)
        want = kref.sample(m.cd, out, cool, shell, z, z_nu)
        assert_same(solver.kpacket_sample(shell, z, z_nu), want, SAMPLE)
        assert_same(solver.kpacket_sample(3, z, z_nu, 2, 4), kref.sample(m.cd, out, cool, np.full(40, 3), z, z_nu, np.full(40, 2), np.full(40, 4)), SAMPLE)
        # the handle serves the two tables lazily, like chi_bf: what was fetched stays, a handle read after the tables were replaced raises
        assert np.array_equal(op.k_cdf, cool["k_cdf"])
        op2 = solver.update_plasma(m.t_rad, m.w)
        op3 = solver.update_plasma(m.t_rad, m.w)
        assert np.array_equal(op.fb_emission_cdf, cool["fb_emission_cdf"])  # (the two tables come in one fetch: op has both, op2 below has none)
        for name in ("fb_emission_cdf", "k_cdf"):
            with pytest.raises(RuntimeError, match="replaced"):
                getattr(op2, name)
        assert np.array_equal(op3.fb_emission_cdf, cool["fb_emission_cdf"]) and np.array_equal(op3.k_cdf, cool["k_cdf"])
        # without continuum data the handle has neither
        solver.set_continuum_data(None)
        op4 = solver.update_plasma(m.t_rad, m.w)
        for name in ("fb_emission_cdf", "k_cdf"):
            with pytest.raises(AttributeError):
                getattr(op4, name)
        assert _code(solver.cooling_rates) == _abi.ERR_STATE
