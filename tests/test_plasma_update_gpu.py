"""The plasma update on the device (tardis_mc_set_plasma_data / tardis_mc_update_plasma / tardis_mc_get_plasma) against the NumPy
restatement of the legacy plasma's arithmetic (tests/plasma_update_ref.py): populations, partition functions, electron densities and the
pass count bit for bit in all four mode pairs, both forms of the partition kernel with the same bits, the opacity state behind the
populations equal to tests/opacity_update_ref.py on the reference populations, a context updated this way indistinguishable from one fed
the same populations through update_opacity, and the resident solver iterating on two [shells] vectors.

Models: the planted one (300 levels on 12 ions and 4 shells: one-level ions, an ion of 120 levels, every edge of the arithmetic) and a
synthetic one of 4000 levels on 30 ions and 20 shells with an ion of 900 levels -- no multiple of a 16-lane row -- among ions of 1 to 800."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opacity_update_ref as oref  # noqa: E402
import plasma_update_ref as ref  # noqa: E402
from tardis_amd import _abi, state as st, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

S, L, K, P = 20, 3000, 4000, 20_000
MODES = [(i, e) for i in ("nebular", "lte") for e in ("dilute-lte", "lte")]
PLASMA = ("level_number_density", "ion_number_density", "partition_function", "electron_density")
TABLES = ("tau_sobolev", "beta_sobolev", "stimulated_emission_factor", "j_blues", "transition_probabilities")
ALL = dict(tau_sobolev=True, transition_probabilities=True, beta_sobolev=True, stimulated_emission_factor=True, j_blues=True)


class Model:
    def __init__(self, prob, ld, pd, t_rad, w):
        self.prob, self.ld, self.pd, self.t_rad, self.w = prob, ld, pd, t_rad, w
        self._solved = {}

    def solved(self, ionization="nebular", excitation="dilute-lte"):
        """The reference plasma of a mode pair, computed once and never written to."""
        key = (ionization, excitation)
        if key not in self._solved:
            self._solved[key] = ref.solve(self.pd, self.t_rad, self.w, ionization, excitation)
        return self._solved[key]


@pytest.fixture(scope="module")
def models(oracle):
    pd, ld, prob, t_rad, w, facts = ref.planted_model()
    planted = Model(prob, ld, pd, t_rad, w)
    planted.facts = facts
    prob = synthetic.make_problem(seed=7, n_packets=P, n_shells=S, n_lines=L, log_tau_mean=-2.0, line_interaction_type="macroatom",
                                  level_sizes="heavy")
    ld = synthetic.make_line_data(7, prob.opacity_state, n_levels=K, level_sizes="heavy", time_explosion=prob.time_explosion)
    pd = synthetic.make_plasma_data(7, ld, S, largest_ion=900)
    assert np.diff(pd.ion_level_edge).max() == 900 and np.diff(pd.ion_level_edge).min() == 1
    return {"planted": planted, "synthetic": Model(prob, ld, pd, pd.t_radiative, pd.dilution_factor)}


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


def assert_tables_equal(got, want):
    for name in TABLES:
        assert np.array_equal(got[name], want[name]), (name, int((got[name] != want[name]).sum()))


def _code(call):
    with pytest.raises((RuntimeError, NotImplementedError)) as e:
        call()
    return e.value.code


@pytest.mark.parametrize("ionization,excitation", MODES)
@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_plasma_equals_the_restatement(engine, models, name, ionization, excitation):
    m = models[name]
    want = m.solved(ionization, excitation)
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w, ionization, excitation)
    got = engine.get_plasma()
    assert_plasma_equal(got, want)
    assert np.count_nonzero(got["level_number_density"]) > 0.3 * got["level_number_density"].size and (got["ion_number_density"] == 0.0).any()
    ms = engine.last_plasma_update_ms()
    stages = ("boltzmann_ms", "partition_ms", "ionization_ms", "population_ms", "line_ms", "block_ms", "derive_ms")
    assert all(ms[k] >= 0 for k in stages) and ms["ionization_ms"] > 0 and engine.last_propagate_ms() > 0
    if name == "planted":
        f = m.facts
        assert got["iterations"] >= 5 and got["level_number_density"][f["underflow_level"], f["underflow_shell"]] == 0.0


@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_both_partition_forms_give_the_same_bits(models, name):
    m = models[name]
    want = m.solved()
    levels = np.diff(m.pd.ion_level_edge)
    assert {Engine.plasma_update_path(int(n)) for n in levels} == {"lane", "row"}
    with Engine(0) as eng:
        stage(eng, m)
        for threshold in (0, int(levels.max()) + 1, -1):  # every ion on a 16-lane row | every ion on one lane | the rule
            eng.set_option("plasma_update_long_rows", threshold)
            eng.update_plasma(m.t_rad, m.w)
            assert_plasma_equal(eng.get_plasma(), want)


@pytest.mark.parametrize("name", ["planted", "synthetic"])
def test_the_opacity_state_behind_the_populations(engine, models, name):
    m = models[name]
    sol = m.solved()
    want = oref.update(m.ld, m.prob.opacity_state, m.prob.time_explosion, sol["level_number_density"], m.t_rad, m.w)
    stage(engine, m)
    engine.update_plasma(m.t_rad, m.w)
    assert_tables_equal(engine.get_opacity(**ALL), want)
    assert (sol["level_number_density"][m.ld.level_lower] == 0.0).any() and (want["tau_sobolev"] > 1e3).any() and (want["tau_sobolev"] == 0.0).any()
    # the same through update_opacity: no bit differs, and get_plasma no longer describes the resident populations
    engine.update_opacity(sol["level_number_density"], sol["electron_density"], 0, t_radiative=m.t_rad, dilution_factor=m.w)
    assert_tables_equal(engine.get_opacity(**ALL), want)
    assert _code(engine.get_plasma) == _abi.ERR_STATE


def test_updated_context_equals_one_fed_the_reference_populations(models):
    m = models["synthetic"]
    sol = m.solved()
    with Engine(0) as a, Engine(0) as b:
        stage(a, m)
        propagate(a, m.prob)  # (everything built lazily from the first tables exists and is stale after the update)
        a.update_plasma(m.t_rad, m.w)
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
        assert int((ra.trackers.interaction_type == 2).sum()) >= 1000
        # the project's GPU estimator tolerance: the summation order is free
        np.testing.assert_allclose(ra.j_estimator, rb.j_estimator, rtol=1e-11, atol=0)
        np.testing.assert_allclose(ra.nu_bar_estimator, rb.nu_bar_estimator, rtol=1e-11, atol=0)


def test_two_updates_are_bit_identical_and_nothing_is_stale(engine, models):
    m = models["synthetic"]
    stage(engine, m)
    t_b, w_b = m.t_rad * 1.1, m.w * 0.5
    out = []
    for t_rad, w in ((m.t_rad, m.w), (m.t_rad, m.w), (t_b, w_b), (m.t_rad, m.w)):
        engine.update_plasma(t_rad, w)
        out.append((engine.get_plasma(), engine.get_opacity(**ALL)))
    assert_plasma_equal(out[0][0], m.solved())
    for k in (1, 3):
        assert_plasma_equal(out[k][0], out[0][0])
        assert_tables_equal(out[k][1], out[0][1])
    want_b = ref.solve(m.pd, t_b, w_b)
    assert_plasma_equal(out[2][0], want_b)
    assert_tables_equal(out[2][1], oref.update(m.ld, m.prob.opacity_state, m.prob.time_explosion, want_b["level_number_density"], t_b, w_b))
    assert not np.array_equal(out[2][0]["electron_density"], out[0][0]["electron_density"])


def test_states_and_errors(models):
    m = models["planted"]
    pd, sol = m.pd, m.solved()
    with Engine(0) as eng:
        stage(eng, m, plasma=False)
        assert _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_STATE   # no plasma data
        assert _code(eng.get_plasma) == _abi.ERR_STATE
        eng.set_plasma_data(pd)
        assert _code(eng.get_plasma) == _abi.ERR_STATE                            # no update yet
        # t_rad outside the zeta table: nebular refuses it, lte does not need the table
        for t_bad in (np.nextafter(2000.0, 0.0), np.nextafter(40000.0, np.inf), np.nan):
            t = m.t_rad.copy()
            t[1] = t_bad
            assert _code(lambda: eng.update_plasma(t, m.w)) == _abi.ERR_INVALID_ARGUMENT
        t = m.t_rad.copy()
        t[3] = 45000.0
        eng.update_plasma(t, m.w, "lte", "dilute-lte")
        assert_plasma_equal(eng.get_plasma(), ref.solve(pd, t, m.w, "lte", "dilute-lte"))
        for bad in (dict(ionization="nlte"), dict(excitation="nlte")):
            with pytest.raises(ValueError):
                eng.update_plasma(m.t_rad, m.w, **bad)
        u = _abi.marshal_plasma_update(m.t_rad, m.w, 4, 2, 0)
        assert eng._L.tardis_mc_update_plasma(eng._h, u.ref()) == _abi.ERR_INVALID_ARGUMENT
        u = _abi.marshal_plasma_update(m.t_rad, m.w, 4, 0, 0, 1, time_of_simulation=1.0, volume=m.prob.geometry.volume)
        assert eng._L.tardis_mc_update_plasma(eng._h, u.ref()) == _abi.ERR_STATE  # detailed j_blues without a propagate
        # a failed solve leaves the opacity state of before the call
        eng.update_plasma(m.t_rad, m.w)
        before = eng.get_opacity(**ALL)
        assert_plasma_equal(eng.get_plasma(), sol)
        stages_before = eng.last_opacity_update_ms()
        eng.set_option("plasma_max_iterations", 2)
        assert sol["iterations"] > 2 and _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_STATE
        assert_tables_equal(eng.get_opacity(**ALL), before)
        # ... and the timing state consistent: the stage times of the last successful update, the device time of the failed solve
        assert eng.last_opacity_update_ms() == stages_before and eng.last_propagate_ms() > 0
        assert _code(eng.last_plasma_update_ms) == _abi.ERR_STATE and _code(eng.get_plasma) == _abi.ERR_STATE
        eng.set_option("plasma_max_iterations", sol["iterations"])               # exactly enough
        eng.update_plasma(m.t_rad, m.w)
        assert_plasma_equal(eng.get_plasma(), sol)
        eng.set_option("plasma_max_iterations", 1000)
        nan = copy.copy(pd)
        nan.number_density = pd.number_density.copy()
        nan.number_density[1, 2] = np.nan
        eng.set_plasma_data(nan)
        assert _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_STATE   # PlasmaIonizationError
        assert_tables_equal(eng.get_opacity(**ALL), before)
        assert _code(eng.get_plasma) == _abi.ERR_STATE
        # what set_plasma_data refuses
        def rc(**changes):
            bad = copy.copy(pd)
            for k, v in changes.items():
                setattr(bad, k, v)
            return eng._L.tardis_mc_set_plasma_data(eng._h, _abi.marshal_plasma_data(bad).ref())
        edge = pd.ion_level_edge.copy()
        edge[4] = edge[3]                                                          # an ion without a level
        assert rc(ion_level_edge=edge) == _abi.ERR_INVALID_ARGUMENT
        edge = pd.ion_level_edge.copy()
        edge[-1] += 1                                                              # past the levels
        assert rc(ion_level_edge=edge) == _abi.ERR_INVALID_ARGUMENT
        assert rc(element_ion_edge=np.array([0, 4, 4, 12])) == _abi.ERR_INVALID_ARGUMENT  # an element without an ion
        g = pd.level_g.copy()
        g[17] = 0.0
        assert rc(level_g=g) == _abi.ERR_INVALID_ARGUMENT
        en = pd.level_energy.copy()
        en[pd.ion_level_edge[2]] = -1e-12
        assert rc(level_energy=en) == _abi.ERR_INVALID_ARGUMENT
        assert rc(zeta_temperatures=pd.zeta_temperatures[:1], zeta=pd.zeta[:, :1]) == _abi.ERR_INVALID_ARGUMENT  # NT < 2
        assert rc(number_density=pd.number_density[:, :3]) == _abi.ERR_INVALID_ARGUMENT   # S mismatch
        drop = int(pd.ion_level_edge[1]) - 1                                       # one level fewer than the line data have
        edge = pd.ion_level_edge.copy()
        edge[1:] -= 1
        assert rc(ion_level_edge=edge, level_energy=np.delete(pd.level_energy, drop), level_g=np.delete(pd.level_g, drop),
                  level_metastable=np.delete(pd.level_metastable, drop)) == _abi.ERR_INVALID_ARGUMENT
        assert _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_STATE   # a refused set_plasma_data leaves none
        eng.set_plasma_data(pd)
        eng.update_plasma(m.t_rad, m.w)
        eng.set_opacity(m.prob.opacity_state)                                      # drops the line data and the plasma data
        assert _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_STATE
        assert eng._L.tardis_mc_set_plasma_data(eng._h, _abi.marshal_plasma_data(pd).ref()) == _abi.ERR_STATE  # no line data
        eng.set_line_data(m.ld)
        assert _code(lambda: eng.update_plasma(m.t_rad, m.w)) == _abi.ERR_STATE


def test_detailed_mode_solves_with_the_given_field_and_takes_the_estimators_j_blues(engine, models):
    """j_blues_mode 1: the populations come from the (t_rad, W) of the call, the mean intensities from the run's estimators -- whose
    own t_rad / W the radiation-field kernels write over the call's only after the plasma kernels have read them."""
    m = models["synthetic"]
    sol = m.solved()
    stage(engine, m)
    res = propagate(engine, m.prob)
    assert np.count_nonzero(res.j_blue_estimator) > 10000
    t, vol = m.prob.packet_collection.time_of_simulation, m.prob.geometry.volume
    rf = engine.radiation_field(t, vol, 1e-10, False)
    assert not np.array_equal(rf["t_radiative"], m.t_rad) and not np.array_equal(rf["dilution_factor"], m.w)
    for _ in range(2):  # (the second call starts from a buffer that holds the estimators' t_rad / W)
        engine.update_plasma(m.t_rad, m.w, "nebular", "dilute-lte", 1, time_of_simulation=t, volume=vol, w_epsilon=1e-10)
        assert_plasma_equal(engine.get_plasma(), sol)
        got = engine.get_opacity(**ALL)
        assert np.array_equal(got["j_blues"], rf["j_blues"])
        assert_tables_equal(got, oref.update(m.ld, m.prob.opacity_state, m.prob.time_explosion, sol["level_number_density"], j_blues=rf["j_blues"]))


def test_more_shells_than_a_workgroup_has_lanes_are_refused(oracle):
    shells = 1025
    prob = synthetic.make_problem(seed=3, n_packets=16, n_shells=shells, n_lines=64, line_interaction_type="macroatom")
    ld = synthetic.make_line_data(3, prob.opacity_state, n_levels=40, time_explosion=prob.time_explosion)
    pd = synthetic.make_plasma_data(3, ld, shells, n_elements=2)
    with Engine(0) as eng:
        stage(eng, Model(prob, ld, pd, pd.t_radiative, pd.dilution_factor))
        before = eng.get_opacity()
        t_rad, w = np.full(shells, 9000.0), np.full(shells, 0.3)
        with pytest.raises(NotImplementedError) as e:
            eng.update_plasma(t_rad, w)
        assert e.value.code == _abi.ERR_UNSUPPORTED
        assert np.array_equal(eng.get_opacity()["tau_sobolev"], before["tau_sobolev"]) and eng.resident_opacity is prob.opacity_state


def test_the_handles_electron_density_survives_later_updates(models):
    m = models["planted"]
    sol = m.solved()
    grid = synthetic.make_spectrum_grid(1000)
    with Engine(0) as eng:
        solver = transport.MCTransportSolverHIP(grid, copy.copy(m.prob.montecarlo_configuration), line_interaction_type="macroatom", resident=True,
                                                engine=eng)
        solver.set_line_data(m.ld)
        solver.set_plasma_data(m.pd)
        ts = solver.initialize_transport_state(None, m.prob.geometry, m.prob.opacity_state, m.prob.time_explosion, n_packets=2000, iteration=0,
                                               temperature_inner=1.0e4)
        solver.run(ts)
        first = solver.update_plasma(m.t_rad, m.w)
        # a failed solve: the handle of the state that is still resident stays the engine's, and stays readable
        eng.set_option("plasma_max_iterations", 2)
        with pytest.raises(RuntimeError) as e:
            solver.update_plasma(m.t_rad, m.w)
        assert e.value.code == _abi.ERR_STATE and eng.resident_opacity is first
        assert np.array_equal(first.electron_density, sol["electron_density"])
        assert np.array_equal(first.tau_sobolev, oref.update(m.ld, m.prob.opacity_state, m.prob.time_explosion, sol["level_number_density"],
                                                             m.t_rad, m.w)["tau_sobolev"])
        eng.set_option("plasma_max_iterations", 1000)
        # update_opacity with electron_density=None keeps the resident values: those of a handle that update_plasma returned
        second = solver.update_plasma(m.t_rad, m.w)
        third = solver.update_opacity(sol["level_number_density"] * 2.0, None, "dilute-blackbody", t_radiative=m.t_rad, dilution_factor=m.w)
        assert eng.resident_opacity is third and np.array_equal(third.electron_density, sol["electron_density"])
        assert np.array_equal(second.electron_density, sol["electron_density"])


SOLVER_PACKETS, SOLVER_BINS = 3000, 2_000_000


def test_resident_solver_iterates_on_two_shell_vectors(models):
    """Three iterations on the device packet source.  The device solver takes (t_rad, W) from radiation_field() -- clipped into the zeta
    table and the unit interval, the caller's S-sized arithmetic -- and hands them to update_plasma(); the host solver computes the
    restatement's populations from the SAME two vectors (the estimators behind them are summed with atomics and differ in the last bit
    from run to run, so they are taken from the device solver's iterations) and passes them through update_opacity().  The device
    spectrum is compared with array_equal on a grid where no bin holds more than two packets, as tests/test_opacity_update_gpu.py does
    and for its reason, and the test checks that from the outputs."""
    m = models["synthetic"]
    prob, geo, cfg = m.prob, m.prob.geometry, m.prob.montecarlo_configuration
    grid = synthetic.make_spectrum_grid(SOLVER_BINS)
    zt = m.pd.zeta_temperatures

    def iterate(fields):
        device = fields is None
        with Engine(0) as eng:
            uploads, big = [], []
            upload = eng.set_opacity
            eng.set_opacity = lambda op: (uploads.append(op), upload(op))[1]
            if device:  # nothing of [levels, shells] or [lines, shells] goes in through the two update calls
                for name in ("update_plasma", "update_opacity"):
                    call = getattr(eng, name)
                    def spy(*a, _call=call, **kw):
                        big.extend(np.size(x) for x in list(a) + list(kw.values()) if x is not None and np.size(x) > S)
                        return _call(*a, **kw)
                    setattr(eng, name, spy)
            solver = transport.MCTransportSolverHIP(grid, copy.copy(cfg), line_interaction_type="macroatom", resident=True, engine=eng)
            solver.set_line_data(m.ld)
            solver.set_plasma_data(m.pd)
            op, out, used = prob.opacity_state, [], []
            for it in range(3):
                ts = solver.initialize_transport_state(None, geo, op, prob.time_explosion, n_packets=SOLVER_PACKETS, iteration=it,
                                                       temperature_inner=1.0e4)
                solver.run(ts)
                sp = ts.packet_spectrum(grid)
                for sign in (ts.output_energy >= 0, ts.output_energy < 0):  # at most two addends per bin: the sums have one value
                    assert np.histogram(ts.output_nu[sign], grid)[0].max() <= 2
                assert np.count_nonzero(sp["montecarlo_emitted_luminosity"]) > SOLVER_PACKETS // 4
                out.append((ts.output_nu.copy(), ts.output_energy.copy(), sp["montecarlo_emitted_luminosity"], sp["montecarlo_reabsorbed_luminosity"]))
                if it == 2:
                    break
                if device:
                    rf = ts.radiation_field(geo.volume, want_j_blues=False)
                    t_rad, w = np.clip(rf["t_radiative"], zt[0], zt[-1]), np.clip(rf["dilution_factor"], 1e-3, 1.0)
                    used.append((t_rad, w))
                    op = solver.update_plasma(t_rad, w)
                    assert isinstance(op, transport.DeviceOpacityState) and eng.resident_opacity is op
                    if it == 0:  # fetched on first access
                        want = ref.solve(m.pd, t_rad, w)
                        assert np.array_equal(op.electron_density, want["electron_density"])
                        assert np.array_equal(op.tau_sobolev, oref.update(m.ld, prob.opacity_state, prob.time_explosion, want["level_number_density"],
                                                                          t_rad, w)["tau_sobolev"])
                else:
                    t_rad, w = fields[it]
                    want = ref.solve(m.pd, t_rad, w)
                    op = solver.update_opacity(want["level_number_density"], want["electron_density"], "dilute-blackbody", t_radiative=t_rad,
                                               dilution_factor=w)
            return out, len(uploads), used, big

    dev, dev_uploads, used, big = iterate(None)
    host, host_uploads, _, _ = iterate(used)
    assert dev_uploads == 1 and host_uploads == 1 and big == []
    assert not np.array_equal(used[0][0], used[1][0])
    for it in range(3):
        for x, y in zip(dev[it], host[it]):
            assert np.array_equal(x, y), it
    assert not np.array_equal(dev[0][0][:100], dev[1][0][:100])
