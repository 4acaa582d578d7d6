"""The lane-sweep wave kernel on packets that live through many MT19937 generations (option `rng_complete`, include/tardis_mc.h;
tardis_amd/csrc/mt_generation.hpp; the algorithm itself is checked on the host in tests/test_mt_generation.py).

The small problems of the other GPU tests never leave a packet's first generation of 624 state words (312 draws): their longest packet has a few dozen
events.  Two optically thick problems give long chains at small size: A, 12 shells x 3 000 lines, whose longest packet has thousands of events, and B,
12 shells x 30 000 lines, where the macro-atom walks draw five numbers per event, so that the refills inside the walk dominate.  Every event draws at
least once: a packet of 1 000 events is in its fourth generation at the least.  With `rng_complete` 1 the wave finishes a packet's generation at the top
of a pass and the packet's refills read it; with 0 every refill regenerates its 8 words itself.  Both must give the oracle's bits -- in one launch, over
several launches (lanes suspended with the generation complete and not), with the drain's lanes packed into other waves, and the option must change
nothing where the kernel does not have the path (v-packets, full relativity)."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

import _golden
import kernel_table_recipes as ktr
from tardis_amd import synthetic

pytestmark = pytest.mark.gpu

N_PACKETS = 6037
PROBLEMS = {
    "A": (dict(n_lines=3_000, electron_density_0=3e11), 200),
    "B": (dict(n_lines=30_000, electron_density_0=3e10), 100),
}
_cases = {}


def case(oracle, name):
    """(problem, oracle result), computed once; the floor on the long chains is asserted from the oracle alone."""
    if name not in _cases:
        kw, floor = PROBLEMS[name]
        prob = synthetic.make_problem(seed=1, n_packets=N_PACKETS, n_shells=12, line_interaction_type="macroatom", level_sizes="heavy", log_tau_mean=1.0, **kw)
        ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                         prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=oracle.max_threads(), track_last_interaction=True)
        assert ref.return_code == 0
        n_long = int((ref.trackers.interactions_count >= 1000).sum())
        print(name, "packets with >= 1000 events:", n_long, "longest:", int(ref.trackers.interactions_count.max()),
              "draws per packet: %.0f" % (ref.counters["rng_draws"] / N_PACKETS))
        assert n_long >= floor, (name, n_long)
        _cases[name] = (prob, ref)
    return _cases[name]


def run(prob, track=True, **options):
    from tardis_amd.engine import Engine
    with Engine(0) as eng:
        eng.set_option("track_last_interaction", int(track))
        for k, v in options.items():
            eng.set_option(k, v)
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        res = eng.get_results(track_last_interaction=bool(track))
        return res, eng.last_kernel_key(), eng.last_kernel_times()["launches"], eng.last_compactions()


def same_as_oracle(res, ref, track=True):
    ktr.same_per_packet(res, ref, trackers=track)  # bit for bit
    ktr.same_estimators_and_counters(res, ref)     # estimators to 1e-11, line_visits / events / macro_transitions / rng_draws exactly
    assert np.array_equal(res.j_blue_estimator == 0.0, ref.j_blue_estimator == 0.0)


def production_lane_sweep(row, wps, track):
    k = dict(zip(ktr.FIELDS["wave"], row[1]))
    return row[0] == "wave" and k["LS"] == 1 and k["VPK"] == 0 and k["XWALK"] == 0 and k["WPE"] == wps and k["TRACK"] == int(track)


@pytest.mark.parametrize("track", [True, False], ids=["tracked", "untracked"])
@pytest.mark.parametrize("wps", [4, 3], ids=["sixteen-waves", "twelve-waves"])
@pytest.mark.parametrize("rng_complete", [1, 0])
@pytest.mark.parametrize("name", ["A", "B"])
def test_long_chains_match_the_oracle(oracle, name, rng_complete, wps, track):
    prob, ref = case(oracle, name)
    res, row, launches, _ = run(prob, track, variant=3, ls_waves_per_simd=wps, rng_complete=rng_complete)
    print(name, rng_complete, wps, track, "->", row, "launches", launches)
    assert production_lane_sweep(row, wps, track), row
    same_as_oracle(res, ref, track)


@pytest.mark.parametrize("wps", [4, 3], ids=["sixteen-waves", "twelve-waves"])
@pytest.mark.parametrize("rng_complete", [1, 0])
def test_long_chains_over_several_launches(oracle, rng_complete, wps):
    """A small log: the waves suspend again and again, lanes are stored and resumed with the generation complete and with it open."""
    prob, ref = case(oracle, "A")
    # (the smallest pool the engine runs with, one chunk of 256 records per wave: in this thick problem most traces stop at their first line and log
    # nothing, a fifth of the events -- the capacity of tests/test_edge_kinematics_gpu.py -- is more than half of the records)
    capacity = 256 * ((N_PACKETS + 63) // 64)
    res, row, launches, _ = run(prob, True, variant=3, ls_waves_per_simd=wps, rng_complete=rng_complete, log_capacity=capacity, log_chunk_records=257)
    print(rng_complete, wps, "log capacity", capacity, "launches", launches, row)
    assert production_lane_sweep(row, wps, True), row
    assert launches >= 3
    same_as_oracle(res, ref)


@pytest.mark.parametrize("rng_complete", [1, 0])
def test_long_chains_through_the_packed_drain(oracle, rng_complete):
    """drain_compact: the last live lanes -- the long chains -- and their state buffers are copied into other waves, the bit travels with them."""
    prob, ref = case(oracle, "A")
    res, row, launches, packed = run(prob, True, variant=3, ls_waves_per_simd=4, rng_complete=rng_complete, drain_compact=16)
    print(rng_complete, "launches", launches, "packed", packed, row)
    assert production_lane_sweep(row, 4, True), row
    assert packed >= 1 and launches >= 2
    same_as_oracle(res, ref)


@pytest.mark.parametrize("name", ["macroatom_nv3_log", "downbranch_fullrel"])
def test_the_option_is_inert_without_the_path(oracle, name):
    """V-packets and full relativity run instantiations that do not have the completion: same results with the option on and off."""
    prob, g = _golden.load_case(name)
    prob.montecarlo_configuration.ENABLE_VPACKET_TRACKING = False
    ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                     prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=True)
    got = {}
    for rng_complete in (1, 0):
        res, row, _, _ = run(prob, True, rng_complete=rng_complete)
        k = dict(zip(ktr.FIELDS[row[0]], row[1]))
        print(name, rng_complete, "->", row)
        assert not (row[0] == "wave" and k["LS"] and not k["VPK"]), "a problem for the other kernels"
        same_as_oracle(res, ref)
        assert_allclose(res.output_nus, g["output_nus"], rtol=1e-13, atol=0)
        assert_allclose(res.output_energies, g["output_energies"], rtol=1e-13, atol=0)
        got[rng_complete] = (res, row)
    assert got[0][1] == got[1][1]
    ktr.same_per_packet(got[1][0], got[0][0], trackers=True)
    if prob.montecarlo_configuration.NUMBER_OF_VPACKETS > 0:
        assert_allclose(got[1][0].v_packets_energy_hist, ref.v_packets_energy_hist, rtol=ktr.EST_RTOL, atol=0)
        assert_allclose(got[1][0].v_packets_energy_hist, got[0][0].v_packets_energy_hist, rtol=ktr.EST_RTOL, atol=0)
