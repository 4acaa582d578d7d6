"""The mean opacities on the device (tardis_mc_mean_opacity) against the serial restatement (tests/mean_opacity_ref.py): every output bit
for bit, in both forms of the shell reduction, on the smallest shapes that can break the indexing -- one shell, a list shorter than a
bin, bins of one line, bin counts on either side of a 16-lane step and of the 256-lane workgroup of the bin kernel -- and on tables with
cells of 0, 1e-20, 1e8, a negative cell, a cold shell whose bluest bins overflow, and duplicate lines away from the bin edges."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mean_opacity_ref as ref  # noqa: E402
import opacity_update_ref  # noqa: E402
from tardis_amd import _abi, state as st, synthetic, transport  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

OUTPUTS = ("kappa_planck", "kappa_rosseland", "tau_planck", "tau_rosseland", "kappa_expansion", "bins_low", "delta_nu")
BIN_SIZES = (1, 3, 10, 16, 17, 64, 65, 200)
FORMS = {"lane": 1 << 60, "row": 0}  # option mean_opacity_long_bins: the row form from that many bins upward


@pytest.fixture(scope="module")
def engine():
    with Engine(0) as eng:
        yield eng
        eng.set_option("mean_opacity_long_bins", -1)


def stage(eng, geo, op, t_exp, disable_scattering=False):
    cfg = st.MonteCarloConfiguration()
    cfg.DISABLE_ELECTRON_SCATTERING = bool(disable_scattering)
    eng.set_geometry(geo, t_exp)
    eng.set_opacity(op)
    eng.set_config(cfg, synthetic.make_spectrum_grid(100))


def assert_outputs_equal(got, want, what):
    for name in OUTPUTS:
        assert got[name].shape == want[name].shape, (what, name)
        assert np.array_equal(got[name], want[name]), (what, name, int((got[name] != want[name]).sum()))


def check_forms(eng, geo, op, t_exp, t_rad, m, what, sigma=ref.SIGMA_THOMSON):
    want = ref.reference(geo, op, t_exp, t_rad, m, sigma)
    for name in ("kappa_planck", "kappa_rosseland", "tau_planck", "tau_rosseland", "kappa_expansion"):
        assert np.all(np.isfinite(want[name])), (what, name)
    for form, threshold in FORMS.items():
        eng.set_option("mean_opacity_long_bins", threshold)
        got = eng.mean_opacity(t_rad, m, want_expansion=True)
        assert got["n_bins"] == len(want["bins_low"]) and got["bin_size"] == m
        assert_outputs_equal(got, want, (what, m, form))
    eng.set_option("mean_opacity_long_bins", -1)
    return want


@pytest.mark.parametrize("n_lines", [7, 10, 160, 1601])
@pytest.mark.parametrize("n_shells", [1, 3, 20])
def test_every_output_equals_the_restatement(engine, oracle, n_shells, n_lines):
    # a pair of equal lines inside a bin for every m >= 2 (bins of one line refuse any pair: they get the list without it)
    geo, op, t_exp, t_rad = ref.model(11, n_shells, n_lines, duplicate_run=2, duplicate_at=n_lines // 2)
    assert (np.diff(op.line_list_nu) == 0.0).sum() == 1
    stage(engine, geo, op, t_exp)
    for m in BIN_SIZES[1:]:
        assert Engine.mean_opacity_bins(op.line_list_nu, m)[1] == -1
        check_forms(engine, geo, op, t_exp, t_rad, m, (n_shells, n_lines))
    tau = op.tau_sobolev
    if n_lines >= 160:
        assert (tau == 0.0).sum() > 3 and (tau == 1e-20).sum() > 3 and (tau == 1e8).sum() > 3
        if n_shells > 1:  # the bluest bins of the cold shell are out of its sums, the others are in
            with np.errstate(over="ignore"):
                E = np.exp(ref.H_PLANCK * op.line_list_nu / (ref.K_BOLTZMANN * t_rad[-1]))
            assert t_rad[-1] == 300.0 and 0 < np.isinf(E).sum() < n_lines
    assert (tau < 0.0).sum() == 1
    geo, op, t_exp, t_rad = ref.model(11, n_shells, n_lines)
    stage(engine, geo, op, t_exp)
    check_forms(engine, geo, op, t_exp, t_rad, 1, (n_shells, n_lines))


@pytest.mark.parametrize("n_bins", [15, 16, 17, 1023, 1024, 1025])
def test_bin_counts_around_a_row_step_and_a_workgroup(engine, oracle, n_bins):
    geo, op, t_exp, t_rad = ref.model(12, 3, n_bins - 1)
    assert Engine.mean_opacity_bins(op.line_list_nu, 1) == (n_bins, -1)
    stage(engine, geo, op, t_exp)
    check_forms(engine, geo, op, t_exp, t_rad, 1, n_bins)
    assert Engine.mean_opacity_path(n_bins) == ("row" if n_bins >= 16 else "lane")


def test_scattering_disabled_and_two_calls_give_identical_bits(engine, oracle):
    geo, op, t_exp, t_rad = ref.model(13, 20, 1601)
    stage(engine, geo, op, t_exp, disable_scattering=True)
    want = check_forms(engine, geo, op, t_exp, t_rad, 10, "sigma 1e-200", sigma=1e-200)
    assert not np.array_equal(want["kappa_planck"], ref.reference(geo, op, t_exp, t_rad, 10)["kappa_planck"])
    a = engine.mean_opacity(t_rad, 10, want_expansion=True)
    ms = engine.last_mean_opacity_ms()
    assert ms["bin_ms"] > 0 and ms["reduce_ms"] > 0 and abs(engine.last_propagate_ms() - (ms["bin_ms"] + ms["reduce_ms"])) < 0.05
    b = engine.mean_opacity(t_rad, 10, want_expansion=True)
    assert_outputs_equal(a, b, "second call")
    assert "kappa_expansion" not in engine.mean_opacity(t_rad, 10)
    # the table is still the one uploaded
    assert np.array_equal(engine.get_opacity(transition_probabilities=False)["tau_sobolev"], op.tau_sobolev)


def test_refusals_come_before_any_launch(engine, oracle):
    geo, op, t_exp, t_rad = ref.model(14, 3, 160, duplicate_run=4, duplicate_at=30)  # (bin 11 at m = 3: tests/test_mean_opacity_host.py)
    stage(engine, geo, op, t_exp)
    good = engine.mean_opacity(t_rad, 10)
    ms = engine.last_mean_opacity_ms()

    def refused(text, *args):
        with pytest.raises(RuntimeError, match=text) as err:
            engine.mean_opacity(*args)
        assert err.value.code == _abi.ERR_INVALID_ARGUMENT
        assert engine.last_mean_opacity_ms() == ms  # (the events of the last call that ran: nothing was recorded since)

    refused("bin 11 of 54 has width 0 at bin_size 3", t_rad, 3)
    refused("bin_size 0, it must be at least 1", t_rad, 0)
    refused("t_radiative is missing", None, 10)
    for bad in (0.0, -5000.0, np.inf, np.nan):
        t = t_rad.copy()
        t[1] = bad
        refused(r"t_radiative\[1\] = .* is not finite and positive", t, 10)
    low = st.OpacityState(op.electron_density, op.t_electrons, op.line_list_nu.copy(), op.tau_sobolev, *[getattr(op, n) for n in (
        "transition_probabilities", "line2macro_level_upper", "macro_block_edge_index", "transition_type", "destination_level_id",
        "transition_line_id")])
    low.line_list_nu[-1] = 11.0
    engine.set_opacity(low)
    refused("does not lie above the 11 pads", t_rad, 10)
    engine.set_opacity(op)
    again = engine.mean_opacity(t_rad, 10)
    for name in ("kappa_planck", "kappa_rosseland", "tau_planck", "tau_rosseland"):
        assert np.array_equal(again[name], good[name])
    with Engine(0) as fresh:
        with pytest.raises(RuntimeError, match="set_geometry and set_opacity must precede") as err:
            fresh.mean_opacity(t_rad, 10)
        assert err.value.code == _abi.ERR_STATE
        with pytest.raises(RuntimeError) as err:
            fresh.last_mean_opacity_ms()
        assert err.value.code == _abi.ERR_STATE


def test_after_update_opacity_equals_a_fresh_context_given_the_same_tau(engine, oracle):
    ld, op, t_exp, n, t_rad, w, _ = opacity_update_ref.planted_model()
    geo = synthetic.make_geometry(3)
    stage(engine, geo, op, t_exp)
    engine.set_line_data(ld)
    engine.update_opacity(n, ld.electron_density, 0, t_radiative=t_rad, dilution_factor=w)
    got = engine.mean_opacity(t_rad, 10, want_expansion=True)
    tables = engine.get_opacity()
    assert np.count_nonzero(tables["tau_sobolev"]) > 100
    op2 = st.OpacityState(op.electron_density, op.t_electrons, op.line_list_nu, tables["tau_sobolev"], tables["transition_probabilities"],
                          op.line2macro_level_upper, op.macro_block_edge_index, op.transition_type, op.destination_level_id,
                          op.transition_line_id)
    with Engine(0) as fresh:
        stage(fresh, geo, op2, t_exp)
        assert_outputs_equal(fresh.mean_opacity(t_rad, 10, want_expansion=True), got, "fresh context")
    assert_outputs_equal(got, ref.reference(geo, op2, t_exp, t_rad, 10), "restatement on the updated tau")


def test_propagation_is_untouched_by_the_call(engine, oracle):
    prob = synthetic.make_problem(seed=5, n_packets=2000, n_shells=20, n_lines=1601, line_interaction_type="macroatom", log_tau_mean=-2.0)
    engine.set_geometry(prob.geometry, prob.time_explosion)
    engine.set_opacity(prob.opacity_state)
    engine.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)

    def run():
        engine.set_packets(prob.packet_collection)
        engine.reset_estimators()
        engine.propagate()
        engine.synchronize()
        return engine.get_results(), engine.last_kernel_key()

    packets, estimators = ("output_nus", "output_energies"), ("j_estimator", "nu_bar_estimator", "j_blue_estimator", "edotlu_estimator")
    t_rad = np.linspace(12000.0, 7000.0, 20)
    (before, key_before) = run()
    out = engine.mean_opacity(t_rad, 10)
    assert np.all(out["tau_rosseland"] > 0) and np.all(np.diff(out["tau_rosseland"]) < 0)
    # what is resident is untouched: the same packets and estimators come back, bit for bit
    resident = engine.get_results()
    for name in packets + estimators:
        assert np.array_equal(getattr(resident, name), getattr(before, name)), ("resident", name)
    # and the next propagate is the one it would have been: the same kernel, the same packets bit for bit, the same counters.  Its
    # estimators are a new sum with atomics, whose order is free: two propagates of this problem with nothing between them differed in
    # 9 / 14 / 669 / 662 cells of j / nu_bar / j_blue / Edotlu when this was written, with the call between them in 10 / 9 / 553 / 597 --
    # so across propagates they are held to the project's estimator tolerance, and bit for bit only above, where nothing was summed again
    (after, key_after) = run()
    assert key_before == key_after and key_before[0] is not None
    assert before.counters == after.counters
    for name in packets:
        assert np.array_equal(getattr(after, name), getattr(before, name)), ("after", name)
    for name in estimators:
        np.testing.assert_allclose(getattr(after, name), getattr(before, name), rtol=1e-11, atol=0, err_msg=name)


def test_solver_mean_optical_depths_and_v_inner(oracle):
    prob = synthetic.make_problem(seed=6, n_packets=2000, n_shells=20, n_lines=1601, line_interaction_type="macroatom", log_tau_mean=-2.0)
    asc = prob.opacity_state.line_list_nu[::-1].copy()
    asc[20:31] = asc[20]  # eleven equal lines from padded member 30 on (e = 9): bin 3 has width 0 at m = 10, none at m = 11
    prob.opacity_state.line_list_nu = np.ascontiguousarray(asc[::-1])
    assert Engine.mean_opacity_bins(prob.opacity_state.line_list_nu, 10) == (_abi.ERR_INVALID_ARGUMENT, 3)
    t_rad = np.linspace(12000.0, 7000.0, 20)
    with Engine(0) as eng:
        solver = transport.MCTransportSolverHIP(prob.spectrum_frequency_grid, prob.montecarlo_configuration, resident=True, engine=eng)
        with pytest.raises(RuntimeError, match="initialize_transport_state"):
            solver.mean_optical_depths(t_rad)
        ts = solver.initialize_transport_state(prob.packet_collection, prob.geometry, prob.opacity_state, prob.time_explosion)
        out = solver.mean_optical_depths(t_rad)
        assert out["bin_size"] == 11 and eng.resident_opacity is prob.opacity_state
        want = ref.reference(prob.geometry, prob.opacity_state, prob.time_explosion, t_rad, 11)
        for name in ("kappa_planck", "kappa_rosseland", "tau_planck", "tau_rosseland"):
            assert np.array_equal(out[name], want[name]), name
        with pytest.raises(RuntimeError, match="width 0"):
            solver.mean_optical_depths(t_rad, bin_size=10)
        generation = eng.opacity_generation
        solver.run(ts)
        assert eng.opacity_generation == generation  # (the run found the tables resident)
        v = transport.estimate_v_inner(out["tau_rosseland"], prob.geometry.v_inner)
        assert np.isfinite(v)
