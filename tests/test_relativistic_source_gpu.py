"""Relativistic black-body packet source on the device (BlackBodySimpleSourceRelativistic, the source of a full-relativity run)
against the plain-NumPy restatement in relativistic_source_ref.py: draws, shards, the rejected-seed bookkeeping, the simple
source beside it, transport on the drawn packets against the oracle, and the solver's choice of source."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import relativistic_source_ref as ref  # noqa: E402
from tardis_amd import _abi, state as st, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

T_EXP = 13 * ref.DAY
T_INNER = 9974.0
EXACT = ("packet_seeds", "initial_mus", "initial_energies", "initial_radii")


@pytest.fixture(scope="module")
def engine():
    from tardis_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def problem():
    return synthetic.make_problem(seed=5, n_packets=2000, n_shells=10, n_lines=1500, line_interaction_type="downbranch",
                                  enable_full_relativity=True)


@pytest.mark.parametrize("n,seed_offset", [(1, 0), (1000, 3), (300_001, 1)])
@pytest.mark.parametrize("v_inner", [1.1e9, 1e10])
def test_device_source_matches_reference(engine, v_inner, n, seed_offset):
    radius = v_inner * T_EXP
    want = ref.packets(n, radius, T_INNER, T_EXP, seed_offset=seed_offset)
    engine.create_blackbody_packets(n, radius, T_INNER, seed_offset=seed_offset)
    simple = engine.get_packets()
    engine.create_blackbody_packets(n, radius, T_INNER, seed_offset=seed_offset, time_explosion=T_EXP)
    got = engine.get_packets()
    for k in EXACT:
        assert np.array_equal(got[k], getattr(want, k)), k
    assert np.array_equal(got["initial_nus"], simple["initial_nus"])  # the same kernel code at the same stream positions
    assert not np.array_equal(got["initial_mus"], simple["initial_mus"])
    # shards reproduce slices of the global draw; the energy is 1 / the GLOBAL count times the factor
    if n > 10:
        lo, hi = n // 3, n // 3 + n // 2
        engine.create_blackbody_packets(n, radius, T_INNER, seed_offset=seed_offset, first=lo, count=hi - lo, time_explosion=T_EXP)
        part = engine.get_packets()
        assert len(part["initial_mus"]) == hi - lo
        for k in got:
            assert np.array_equal(part[k], got[k][lo:hi]), k


def test_device_source_rejection_path(engine):
    """A seed range with a 1 % Lemire rejection rate: the direction stream starts after the consumed u32 draws."""
    n, max_val, radius = 20_000, 4252017623, 1.1e9 * T_EXP
    want = ref.packets(n, radius, 1.0e4, T_EXP, max_seed_val=max_val)
    engine.create_blackbody_packets(n, radius, 1.0e4, max_seed_val=max_val, time_explosion=T_EXP)
    got = engine.get_packets()
    assert np.array_equal(got["packet_seeds"], want.packet_seeds)
    assert np.array_equal(got["initial_mus"], want.initial_mus)
    assert np.array_equal(got["initial_energies"], want.initial_energies)


def test_beta_zero_is_the_simple_source(engine):
    n = 1000
    engine.create_blackbody_packets(n, 0.0, T_INNER)
    simple = engine.get_packets()
    engine.create_blackbody_packets(n, 0.0, T_INNER, time_explosion=T_EXP)
    got = engine.get_packets()
    for k in got:
        assert np.array_equal(got[k], simple[k]), k
    assert np.array_equal(got["initial_mus"], np.sqrt(ref.packets(n, 0.0, T_INNER, T_EXP).z))
    assert np.array_equal(got["initial_energies"], np.full(n, 1.0 / n))


def test_simple_source_unchanged_beside_it(engine):
    n, radius = 1000, 1.2e15
    engine.create_blackbody_packets(n, radius, T_INNER, seed_offset=3, time_explosion=T_EXP)
    engine.create_blackbody_packets(n, radius, T_INNER, seed_offset=3)
    got = engine.get_packets()
    want = synthetic.black_body_packets(n, radius, T_INNER, seed_offset=3)
    for k in EXACT:
        assert np.array_equal(got[k], getattr(want, k)), k
    np.testing.assert_allclose(got["initial_nus"], want.initial_nus, rtol=2e-15, atol=0)
    assert np.array_equal(got["initial_energies"], np.full(n, 1.0 / n))


@pytest.mark.parametrize("radius,time_explosion,n,word", [
    (1.0e15, 0.0, 10, "time_explosion"), (1.0e15, -1.0, 10, "time_explosion"), (1.0e15, float("nan"), 10, "time_explosion"),
    (1.0e15, float("inf"), 10, "time_explosion"), (-1.0, T_EXP, 10, "radius"), (float("nan"), T_EXP, 10, "radius"),
    (ref.C_SPEED_OF_LIGHT * T_EXP, T_EXP, 10, "beta"), (1.0e15, T_EXP, 0, "n_total")])
def test_argument_errors_leave_the_resident_packets(engine, radius, time_explosion, n, word):
    engine.create_blackbody_packets(100, 1.2e15, T_INNER)
    before = engine.get_packets()
    generation = engine.packets_generation
    with pytest.raises(RuntimeError) as e:
        engine.create_blackbody_packets(n, radius, T_INNER, time_explosion=time_explosion)
    assert e.value.code == _abi.ERR_INVALID_ARGUMENT and word in str(e.value)
    assert engine.packets_generation == generation and engine.n_packets == 100
    after = engine.get_packets()
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def _propagate(engine):
    engine.reset_estimators(); engine.propagate(); engine.synchronize()
    return engine.get_results(track_last_interaction=False, want_line_estimators=False)


def test_transport_on_device_drawn_packets(engine, problem, oracle):
    """Full-relativity transport on packets the device drew: the same as on those packets handed back through set_packets, and
    bit for bit the oracle's."""
    prob = problem
    n, radius = prob.packet_collection.number_of_packets, float(prob.geometry.r_inner[0])
    engine.set_geometry(prob.geometry, prob.time_explosion)
    engine.set_opacity(prob.opacity_state)
    engine.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
    engine.create_blackbody_packets(n, radius, 1.0e4, time_explosion=prob.time_explosion)
    dev = engine.get_packets()
    host = synthetic.black_body_packets(n, radius, 1.0e4, time_explosion=prob.time_explosion)
    for k in EXACT:
        assert np.array_equal(dev[k], getattr(host, k)), k
    np.testing.assert_allclose(dev["initial_nus"], host.initial_nus, rtol=2e-15, atol=0)
    a = _propagate(engine)
    pc = st.PacketCollection(dev["initial_radii"], dev["initial_nus"], dev["initial_mus"], dev["initial_energies"], dev["packet_seeds"],
                             host.radiation_field_luminosity)
    engine.set_packets(pc)
    b = _propagate(engine)
    assert np.array_equal(a.output_nus, b.output_nus) and np.array_equal(a.output_energies, b.output_energies)
    # the oracle on the host-drawn collection, its nus the device's (NumPy's log may differ from the portable one by an ulp)
    want = oracle.run(pc, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                      prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE)
    assert want.return_code == 0
    assert np.array_equal(a.output_nus, want.output_nus), "per-packet output_nus differ from the oracle"
    assert np.array_equal(a.output_energies, want.output_energies), "per-packet output_energies differ from the oracle"
    assert np.count_nonzero(a.output_energies > 0) > n // 10  # packets do leave through the outer boundary


@pytest.mark.parametrize("full_relativity,relativistic_source,relativistic", [
    (True, None, True), (True, False, False), (False, None, False), (False, True, True)])
def test_solver_follows_full_relativity(engine, problem, full_relativity, relativistic_source, relativistic):
    from tardis_amd import transport
    prob, n = problem, 1000
    solver = transport.MCTransportSolverHIP(prob.spectrum_frequency_grid, copy.copy(prob.montecarlo_configuration),
                                            line_interaction_type="downbranch", enable_full_relativity=full_relativity, resident=True,
                                            engine=engine)
    ts = solver.initialize_transport_state(None, prob.geometry, prob.opacity_state, prob.time_explosion, n_packets=n, iteration=2,
                                           temperature_inner=1.0e4, relativistic_source=relativistic_source)
    solver.run(ts)
    radius = float(prob.geometry.r_inner[0])
    want = ref.packets(n, radius, 1.0e4, prob.time_explosion if relativistic else None, seed_offset=2)
    pc = ts.packet_collection
    assert np.array_equal(pc.initial_mus, want.initial_mus)
    assert np.array_equal(pc.initial_energies, want.initial_energies)
    assert np.array_equal(pc.packet_seeds, want.packet_seeds)
    # the luminosity normalisation is the simple source's in both forms
    simple = synthetic.black_body_packets(n, radius, 1.0e4, seed_offset=2)
    assert pc.radiation_field_luminosity == simple.radiation_field_luminosity and pc.time_of_simulation == simple.time_of_simulation
