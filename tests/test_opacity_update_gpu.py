"""The opacity update on the device (tardis_mc_set_line_data / tardis_mc_update_opacity / tardis_mc_get_opacity) against the NumPy
restatement of the legacy plasma's arithmetic (tests/opacity_update_ref.py): every table bit for bit, the context after an update
indistinguishable from a fresh one given the same tables through set_opacity, and the resident solver iterating without an upload.

Models: 3000 lines on 20 shells; level_sizes="heavy" plants macro-atom blocks of 33, 96, 99, 192, 300 and 2100 rows -- either side of a
16-lane row and of a wave, and multiples of both -- among hundreds of short ones; the downbranch model and the planted model have blocks
on either side of the threshold between the two forms of the block kernel."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opacity_update_ref as ref  # noqa: E402
from tardis_amd import _abi, state as st, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

S, L, P = 20, 3000, 20_000
TABLES = ("tau_sobolev", "beta_sobolev", "stimulated_emission_factor", "j_blues")
ALL = dict(tau_sobolev=True, transition_probabilities=True, beta_sobolev=True, stimulated_emission_factor=True, j_blues=True)
CASES = {
    "macroatom_heavy": dict(line_interaction_type="macroatom", level_sizes="heavy"),
    "macroatom_uniform": dict(line_interaction_type="macroatom", level_sizes="uniform"),
    "downbranch": dict(line_interaction_type="downbranch", level_sizes="heavy"),
    "scatter": dict(line_interaction_type="scatter"),
}


def model(case="macroatom_heavy", seed=7, n_packets=P, **kw):
    args = dict(CASES[case], **kw)
    prob = synthetic.make_problem(seed=seed, n_packets=n_packets, n_shells=S, n_lines=L, log_tau_mean=-2.0, **args)
    ld = synthetic.make_line_data(seed, prob.opacity_state, level_sizes=args.get("level_sizes", "uniform"), time_explosion=prob.time_explosion)
    return prob, ld


def stage(eng, prob, ld=None):
    eng.set_geometry(prob.geometry, prob.time_explosion)
    eng.set_opacity(prob.opacity_state)
    eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
    if ld is not None:
        eng.set_line_data(ld)


def update_mode0(eng, ld, n=None, t_rad=None, w=None):
    eng.update_opacity(ld.level_number_density if n is None else n, ld.electron_density, 0,
                       t_radiative=ld.t_radiative if t_rad is None else t_rad, dilution_factor=ld.dilution_factor if w is None else w)


def propagate(eng, prob):
    eng.set_packets(prob.packet_collection)
    eng.reset_estimators()
    eng.propagate()
    eng.synchronize()
    return eng.get_results()


def assert_tables_equal(got, want, names):
    for name in names:
        assert got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), (name, int((got[name] != want[name]).sum()))


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as eng:
        yield eng


@pytest.fixture(scope="module")
def heavy(oracle):
    """The heavy-tailed macroatom model and its reference tables, computed once."""
    prob, ld = model("macroatom_heavy")
    want = ref.update(ld, prob.opacity_state, prob.time_explosion, ld.level_number_density, ld.t_radiative, ld.dilution_factor)
    return prob, ld, want


@pytest.mark.parametrize("case", list(CASES))
def test_dilute_blackbody_update_equals_the_restatement(engine, oracle, case, heavy):
    if case == "macroatom_heavy":
        prob, ld, want = heavy
    else:
        prob, ld = model(case)
        want = ref.update(ld, prob.opacity_state, prob.time_explosion, ld.level_number_density, ld.t_radiative, ld.dilution_factor)
    stage(engine, prob, ld)
    before = engine.get_opacity()
    assert np.array_equal(before["tau_sobolev"], prob.opacity_state.tau_sobolev)
    update_mode0(engine, ld)
    assert engine.last_propagate_ms() > 0
    got = engine.get_opacity(**ALL)
    assert_tables_equal(got, want, TABLES)
    tau = want["tau_sobolev"]
    n_l, n_u = ld.level_number_density[ld.level_lower], ld.level_number_density[ld.level_upper]
    assert (tau > 1e3).sum() > 100 and ((tau > 0) & (tau < 1e-4)).sum() > 100 and ((tau >= 1e-4) & (tau <= 1e3)).sum() > 100
    assert (n_l == 0.0).sum() > 10 and ((n_l != 0.0) & (ld.g_lower[:, None] * n_u > ld.g_upper[:, None] * n_l)).sum() > 100
    if case == "scatter":
        assert ld.transition_probability_coef is None and want["transition_probabilities"] is None
        assert np.array_equal(got["transition_probabilities"], before["transition_probabilities"])
    else:
        assert_tables_equal(got, want, ("transition_probabilities",))
        rows = np.diff(prob.opacity_state.macro_block_edge_index)
        forms = {Engine.opacity_update_path(int(r)) for r in rows}
        assert "row" in forms and (case != "downbranch" or "lane" in forms)  # (the planted model below has both, too)
        if CASES[case].get("level_sizes") == "heavy":
            planted = {33, 96, 99, 192, 300, 2100} if case == "macroatom_heavy" else {11, 32, 33, 64, 100, 700}
            assert planted <= set(rows.tolist())
        if case == "macroatom_heavy":
            assert (prob.opacity_state.transition_type == 1).sum() == L and np.count_nonzero(got["transition_probabilities"]) > 0.9 * 3 * L * S


def test_planted_edges_on_the_device(engine, oracle):
    ld, op, t_exp, n, t_rad, w, facts = ref.planted_model()
    geo = synthetic.make_geometry(3)
    assert geo.time_explosion == t_exp
    engine.set_geometry(geo, t_exp)
    engine.set_opacity(op)
    engine.set_line_data(ld)
    update_mode0(engine, ld)
    want = ref.update(ld, op, t_exp, n, t_rad, w)
    got = engine.get_opacity(**ALL)
    assert_tables_equal(got, want, TABLES + ("transition_probabilities",))
    edge = op.macro_block_edge_index
    zb, zs = facts["zero_norm_block"], facts["zero_norm_shell"]
    assert np.all(got["transition_probabilities"][edge[zb]:edge[zb + 1], zs] == 0.0)  # (no propagate: that block must not be walked)
    assert got["tau_sobolev"][0, 0] == 1e3 and got["tau_sobolev"][1, 0] == 1e-4 and (got["tau_sobolev"] == 0.0).any()


def test_detailed_mode_takes_the_radiation_fields_j_blues(engine, oracle, heavy):
    prob, ld, _ = heavy
    stage(engine, prob, ld)
    res = propagate(engine, prob)
    assert np.count_nonzero(res.j_blue_estimator) > 10000
    t, vol = prob.packet_collection.time_of_simulation, prob.geometry.volume
    for window in (False, True):
        engine.update_opacity(ld.level_number_density, None, 1, time_of_simulation=t, volume=vol, w_epsilon=1e-10, detailed_optical_window=window)
        got = engine.get_opacity(**ALL)
        jb = engine.radiation_field(t, vol, 1e-10, window)["j_blues"]
        assert np.array_equal(got["j_blues"], jb)
        want = ref.update(ld, prob.opacity_state, prob.time_explosion, ld.level_number_density, j_blues=jb)
        assert_tables_equal(got, want, TABLES + ("transition_probabilities",))
    # estimators and packets are still the run's
    again = engine.get_results()
    assert np.array_equal(again.j_blue_estimator, res.j_blue_estimator) and np.array_equal(again.output_nus, res.output_nus)


def _fresh_upload(prob, tables):
    op = prob.opacity_state
    return st.OpacityState(op.electron_density, op.t_electrons, op.line_list_nu, tables["tau_sobolev"], tables["transition_probabilities"],
                           op.line2macro_level_upper, op.macro_block_edge_index, op.transition_type, op.destination_level_id,
                           op.transition_line_id)


@pytest.mark.parametrize("n_vpackets", [0, 2])
def test_updated_context_equals_a_fresh_upload_of_the_same_tables(oracle, n_vpackets):
    prob, ld = model("macroatom_heavy", n_vpackets=n_vpackets)
    with Engine(0) as a, Engine(0) as b:
        if n_vpackets:
            a.set_option("vpacket_screening", 1)
            b.set_option("vpacket_screening", 1)
        stage(a, prob, ld)
        propagate(a, prob)  # (everything built lazily from the first tables exists and is stale after the update)
        update_mode0(a, ld)
        tables = a.get_opacity()
        ra = propagate(a, prob)
        b.set_geometry(prob.geometry, prob.time_explosion)
        b.set_opacity(_fresh_upload(prob, tables))
        b.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        rb = propagate(b, prob)
        assert a.last_variant() == b.last_variant()
        assert np.array_equal(ra.output_nus, rb.output_nus) and np.array_equal(ra.output_energies, rb.output_energies)
        for name in st.LastInteractionTrackers.F64_FIELDS + st.LastInteractionTrackers.I64_FIELDS:
            assert np.array_equal(getattr(ra.trackers, name), getattr(rb.trackers, name), equal_nan=True), name
        for name in ("line_visits", "events", "macro_transitions", "rng_draws", "vpacket_line_visits", "vpackets"):
            assert ra.counters[name] == rb.counters[name], name
        assert int((ra.trackers.interaction_type == 2).sum()) >= 1000
        # the project's GPU estimator tolerance: the summation order is free
        np.testing.assert_allclose(ra.j_estimator, rb.j_estimator, rtol=1e-11, atol=0)
        np.testing.assert_allclose(ra.nu_bar_estimator, rb.nu_bar_estimator, rtol=1e-11, atol=0)
        if n_vpackets:
            assert ra.counters["vpackets"] > 0 and ra.v_packets_energy_hist.sum() > 0
            np.testing.assert_allclose(ra.v_packets_energy_hist, rb.v_packets_energy_hist, rtol=1e-11, atol=0)


def test_two_updates_are_bit_identical_and_nothing_is_stale(engine, oracle, heavy):
    prob, ld, want = heavy
    stage(engine, prob, ld)
    n_b, t_b, w_b = ld.level_number_density * 1.7, ld.t_radiative * 0.9, ld.dilution_factor * 0.5
    update_mode0(engine, ld)
    a1 = engine.get_opacity(**ALL)
    update_mode0(engine, ld)
    a2 = engine.get_opacity(**ALL)
    update_mode0(engine, ld, n_b, t_b, w_b)
    b = engine.get_opacity(**ALL)
    update_mode0(engine, ld)
    a3 = engine.get_opacity(**ALL)
    assert_tables_equal(a1, want, TABLES + ("transition_probabilities",))
    for other in (a2, a3):
        assert_tables_equal(other, a1, TABLES + ("transition_probabilities",))
    want_b = ref.update(ld, prob.opacity_state, prob.time_explosion, n_b, t_b, w_b)
    assert_tables_equal(b, want_b, TABLES + ("transition_probabilities",))
    assert not np.array_equal(b["tau_sobolev"], a1["tau_sobolev"]) and not np.array_equal(b["transition_probabilities"], a1["transition_probabilities"])


def _rc_set_line_data(eng, ld, n_transitions):
    return eng._L.tardis_mc_set_line_data(eng._h, _abi.marshal_line_data(ld, n_transitions).ref())


def _code(call):
    with pytest.raises((RuntimeError, NotImplementedError)) as e:
        call()
    return e.value.code


def test_states_and_errors(oracle, heavy):
    prob, ld, _ = heavy
    T = len(prob.opacity_state.transition_type)
    with Engine(0) as eng:
        stage(eng, prob)
        assert _code(lambda: update_mode0(eng, ld)) == _abi.ERR_STATE                      # no line data
        assert _code(lambda: eng.get_opacity(beta_sobolev=True)) == _abi.ERR_STATE         # nothing produced them yet
        eng.set_line_data(ld)
        assert _code(lambda: eng.update_opacity(ld.level_number_density, None, 1, time_of_simulation=1.0, volume=prob.geometry.volume)) == _abi.ERR_STATE  # no propagate yet
        update_mode0(eng, ld)
        eng.set_opacity(prob.opacity_state)
        assert _code(lambda: update_mode0(eng, ld)) == _abi.ERR_STATE                      # a later set_opacity drops the line data
        bad = copy.copy(ld)
        bad.level_upper = ld.level_upper.copy()
        bad.level_upper[5] = ld.n_levels
        assert _rc_set_line_data(eng, bad, T) == _abi.ERR_INVALID_ARGUMENT
        bad.level_upper[5] = -1
        assert _rc_set_line_data(eng, bad, T) == _abi.ERR_INVALID_ARGUMENT
        short = copy.copy(ld)
        short.transition_probability_coef = ld.transition_probability_coef[:-1]
        assert _rc_set_line_data(eng, short, T - 1) == _abi.ERR_INVALID_ARGUMENT            # T mismatch
        for name in ("f_lu", "wavelength_cm", "g_lower", "g_upper", "level_lower", "level_upper"):
            setattr(short, name, getattr(ld, name)[:-1])
        short.transition_probability_coef = ld.transition_probability_coef
        assert _rc_set_line_data(eng, short, T) == _abi.ERR_INVALID_ARGUMENT                # L mismatch
        assert _code(lambda: update_mode0(eng, ld)) == _abi.ERR_STATE                      # a refused set_line_data leaves none
        # a type-2 row: set_opacity takes it (the walk reports it if a packet gets there), the update refuses it
        op2 = copy.copy(prob.opacity_state)
        op2.transition_type = prob.opacity_state.transition_type.copy()
        op2.destination_level_id = prob.opacity_state.destination_level_id.copy()
        op2.transition_type[7], op2.destination_level_id[7] = 2, 0
        eng.set_opacity(op2)
        assert _rc_set_line_data(eng, ld, T) == _abi.ERR_UNSUPPORTED
        # a non-emission row whose line is out of range: set_opacity does not look at it, set_line_data does
        op3 = copy.copy(prob.opacity_state)
        op3.transition_line_id = prob.opacity_state.transition_line_id.copy()
        k = int(np.flatnonzero(prob.opacity_state.transition_type == 0)[3])
        op3.transition_line_id[k] = L
        eng.set_opacity(op3)
        assert _rc_set_line_data(eng, ld, T) == _abi.ERR_INVALID_ARGUMENT
        # the resident source function does not survive an update
        stage(eng, prob, ld)
        propagate(eng, prob)
        eng.source_function(prob.packet_collection.time_of_simulation, prob.geometry.volume, want_arrays=False)
        nu = prob.opacity_state.line_list_nu
        freqs = np.linspace(nu[-1] * 1.05, nu[0] * 0.95, 8)
        eng.formal_integral_resident(1.0e4, freqs, 20)
        update_mode0(eng, ld)
        assert _code(lambda: eng.formal_integral_resident(1.0e4, freqs, 20)) == _abi.ERR_STATE


SOLVER_PACKETS, SOLVER_BINS = 3000, 2_000_000


def test_resident_solver_iterates_without_uploading_tables(oracle, heavy):
    """Three iterations on the device packet source, the opacity step on the device against the restatement uploaded through
    set_opacity.  The packet outputs are bit-reproducible.  The device spectrum is a histogram accumulated with fp64 atomics, so a bin
    of three or more packets depends on the order in which they arrive and differs in the last bit between two runs of the SAME call;
    a bin of one or two does not (a + b == b + a).  The comparison with array_equal therefore runs on a grid fine enough that no bin
    holds more than two packets of a run -- 3000 packets on 2e6 bins -- and the test checks that from the outputs."""
    prob, ld, _ = heavy
    geo, cfg = prob.geometry, prob.montecarlo_configuration
    grid = synthetic.make_spectrum_grid(SOLVER_BINS)
    states = [(ld.level_number_density * f, ld.t_radiative * g, ld.dilution_factor) for f, g in ((1.0, 1.0), (1.3, 0.97))]

    def iterate(device_update):
        with Engine(0) as eng:
            uploads = []
            upload = eng.set_opacity
            eng.set_opacity = lambda op: (uploads.append(op), upload(op))[1]
            solver = transport.MCTransportSolverHIP(grid, copy.copy(cfg), line_interaction_type="macroatom", resident=True, engine=eng)
            solver.set_line_data(ld)
            op, out = prob.opacity_state, []
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
                n, t_rad, w = states[it]
                want = ref.update(ld, prob.opacity_state, prob.time_explosion, n, t_rad, w)
                if device_update:
                    previous = op
                    op = solver.update_opacity(n, ld.electron_density, "dilute-blackbody", t_radiative=t_rad, dilution_factor=w)
                    assert isinstance(op, transport.DeviceOpacityState) and eng.resident_opacity is op
                    if it == 0:  # fetched on first access, like the estimators of a resident run
                        assert np.array_equal(op.tau_sobolev, want["tau_sobolev"])
                        assert np.array_equal(op.transition_probabilities, want["transition_probabilities"])
                        assert op.line_list_nu is prob.opacity_state.line_list_nu
                    else:  # a handle that was never read does not hand out the next state's tables
                        assert previous.tau_sobolev is not None  # (read before: its copy stays)
                        stale = transport.DeviceOpacityState(eng, previous, ld.electron_density)
                        stale._gen -= 1
                        with pytest.raises(RuntimeError):
                            stale.beta_sobolev
                else:
                    op = _fresh_upload(prob, want)
            return out, len(uploads)

    dev, dev_uploads = iterate(True)
    host, host_uploads = iterate(False)
    assert dev_uploads == 1 and host_uploads == 3
    for it in range(3):
        for x, y in zip(dev[it], host[it]):
            assert np.array_equal(x, y), it
    assert not np.array_equal(dev[0][0][:100], dev[1][0][:100])
