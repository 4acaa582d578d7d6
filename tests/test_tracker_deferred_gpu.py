"""The deferred last-interaction record of the lane-sweep kernel (variant 3 without v-packets; option tracker_defer, default 1).

The reference's tracker (packets/trackers/tracker_last_interaction.py) keeps, per packet, the state around its LAST interaction.  The
wave kernel used to store a 64-byte record at every interaction, each overwriting the one before; with tracker_defer 1 the record of
the interaction in progress stays in six per-lane LDS doubles (three before-values, r, mu, one packed word: type | shell | absorbing
line | emitting line, mc_device.hpp tracker_pack) and is stored once, when the packet ends.  Nothing the caller sees may change:

  (a) all 14 tracker fields and both outputs equal the CPU oracle bit for bit, and equal the per-interaction path (tracker_defer 0);
  (b) the same through >= 20 launches of one call (the LDS values travel in LaneSave), with walks carried over in nearly every pass
      (the shell-sorted log reaches that count at this size; on the headline's own instantiation the smallest log gives about five);
  (c) downbranch and scatter modes, and the dense-electron golden (last interaction = electron scattering, both line ids -1);
  (d) a problem "beyond" the packed widths (narrowed by the test option tracker_pack_max_lines) takes the per-interaction path;
  (e) a failed call raises as before, and the failed packets' records are the empty record.

Shape: 20 shells x 2 000 lines, heavy-tailed macro-atom blocks, 20 000 packets (313 waves), variant 3 forced.  The seed was chosen on
the oracle so that the sample holds packets without any interaction, packets whose last interaction is a line, and packets that cross
two or more shells after their last interaction (asserted below).
"""
import numpy as np
import pytest

import _golden
from tardis_amd import synthetic

pytestmark = pytest.mark.gpu

S, L, P, SEED = 20, 2_000, 20_000, 31
EPOCHS = dict(log_capacity=4_096, log_chunk_records=256)  # (the line-log options of test_estimator_pipelines.py: a log far smaller than the call writes)


def _problem(mode="macroatom"):
    return synthetic.make_problem(seed=SEED, n_packets=P, n_shells=S, n_lines=L, line_interaction_type=mode, level_sizes="heavy")


def _oracle(oracle, prob):
    return oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                      prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=oracle.max_threads(), track_last_interaction=True)


def _run(prob, **options):
    """One call on a fresh engine, variant 3.  Returns (results, launches, last_tracker_defer)."""
    from tardis_amd.engine import Engine
    with Engine(0) as eng:
        eng.set_option("variant", 3)
        for k, v in options.items():
            eng.set_option(k, v)
        eng.set_geometry(prob.geometry, prob.time_explosion); eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid); eng.set_packets(prob.packet_collection)
        eng.reset_estimators(); eng.propagate(); eng.synchronize()
        got = eng.get_results(track_last_interaction=True, want_line_estimators=False)
        assert eng.last_variant() == 3
        return got, eng.last_kernel_times()["launches"], eng.last_tracker_defer()


def _same(got, ref):
    assert np.array_equal(got.output_nus, ref.output_nus)
    assert np.array_equal(got.output_energies, ref.output_energies)
    assert len(_golden.TRACKER_I64 + _golden.TRACKER_F64) == 14
    for f in _golden.TRACKER_I64:
        assert np.array_equal(getattr(got.trackers, f), getattr(ref.trackers, f)), f
    for f in _golden.TRACKER_F64:
        assert np.array_equal(getattr(got.trackers, f), getattr(ref.trackers, f), equal_nan=True), f


@pytest.fixture(scope="module")
def base(oracle):
    prob = _problem()
    return prob, _oracle(oracle, prob)


def test_macroatom_default_options_match_oracle_and_per_interaction_stores(base):
    prob, ref = base
    t = ref.trackers
    emitted = ref.output_energies > 0
    n_none = int((t.interactions_count == 0).sum())
    n_line = int((t.interaction_type == 2).sum())
    # (an emitted packet whose last interaction was in shell s leaves through shells s + 1 ... S - 1: s <= S - 3 crosses two or more)
    n_far = int((emitted & (t.interactions_count > 0) & (t.shell_id <= S - 3)).sum())
    print("no interaction", n_none, "last = line", n_line, "last = electron", int((t.interaction_type == 4).sum()), ">= 2 shells after the last", n_far,
          "most interactions", int(t.interactions_count.max()))
    assert n_none > 100 and n_line > 100 and n_far > 100
    got, launches, defer = _run(prob)
    print("launches", launches, "tracker_defer", defer)
    assert defer == 1
    _same(got, ref)
    per, _, defer0 = _run(prob, tracker_defer=0)
    assert defer0 == 0
    _same(per, ref)
    _same(got, per)


@pytest.mark.parametrize("walk_min_active", [None, 48])
@pytest.mark.parametrize("by_shell", [1, 0])
def test_many_epochs_and_carried_walks(base, walk_min_active, by_shell):
    """The record waits in LDS through suspensions (LaneSave) and beside walks that are carried from pass to pass and across launches.
    The smallest log a call of 313 waves can be given is one 256-record chunk per wave, a fifth of what this call writes: about five launches
    (by_shell 0, the headline's instantiation; >= 4 asserted).  With the shell-sorted log (log_by_shell 1, the same kernel's SL instantiations) a wave
    wants a chunk per shell, the pool runs dry at once and the call takes many more (26 measured): there the >= 20 launches are asserted."""
    prob, ref = base
    options = dict(EPOCHS, log_by_shell=by_shell)
    if by_shell:
        options["ls_waves_per_simd"] = 4  # (the shell-sorted log exists for the sixteen-wave form on the interleaved table; a call this small would take the twelve-wave one)
    if walk_min_active is not None:
        options["walk_min_active"] = walk_min_active
    got, launches, defer = _run(prob, **options)
    print("log_by_shell", by_shell, "walk_min_active", walk_min_active, "launches", launches, "tracker_defer", defer)
    assert defer == 1 and launches >= (20 if by_shell else 4)
    _same(got, ref)


@pytest.mark.parametrize("mode", ["downbranch", "scatter"])
def test_other_interaction_modes(oracle, mode):
    prob = _problem(mode)
    ref = _oracle(oracle, prob)
    assert (ref.trackers.interaction_type == 2).sum() > 100 and (ref.trackers.interaction_type == 4).sum() > 100
    got, _, defer = _run(prob)
    assert defer == 1
    _same(got, ref)
    got, launches, defer = _run(prob, **EPOCHS)
    assert defer == 1 and launches >= 2
    _same(got, ref)


def test_dense_electrons_last_interaction_is_electron_scattering(oracle):
    prob, _ = _golden.load_case("scatter_dense_electrons")
    ref = _oracle(oracle, prob)
    es = ref.trackers.interaction_type == 4
    assert es.sum() > 0.5 * (ref.trackers.interactions_count > 0).sum()
    got, _, defer = _run(prob)
    assert defer == 1
    _same(got, ref)
    assert np.all(got.trackers.interaction_line_absorb_id[es] == -1) and np.all(got.trackers.interaction_line_emit_id[es] == -1)


def test_problem_beyond_the_packed_widths_takes_the_per_interaction_path(base):
    """2 000 lines against a packed word narrowed to 1 000 (tracker_pack_max_lines; the real bound, 2^24 - 1 lines, needs tables of GBs)."""
    prob, ref = base
    got, _, defer = _run(prob, tracker_pack_max_lines=1_000)
    assert defer == 0
    _same(got, ref)
    got, _, defer = _run(prob, tracker_pack_max_lines=L)  # (exactly at the bound: it fits)
    assert defer == 1
    _same(got, ref)


def _raw_records(eng, first, count):
    raw = eng.debug_eval(100, np.array([float(first)]), n=8 * count).reshape(count, 8)
    ints = np.ascontiguousarray(raw[:, 5:8]).view(np.int32).reshape(count, 6)  # shell | type | absorb | emit | count | valid
    return raw[:, :5], ints


@pytest.mark.parametrize("defer", [1, 0])
def test_failed_call_raises_and_leaves_empty_records(defer):
    """Emission rows of an unsupported (continuum) transition type: every packet whose walk reaches one fails -- after interactions of its own."""
    from tardis_amd.engine import Engine
    prob = _problem()
    op = prob.opacity_state
    rows = np.flatnonzero(op.transition_type == -1)
    op.transition_type[rows[::7]] = -2
    with Engine(0) as eng:
        eng.set_option("variant", 3)
        eng.set_option("tracker_defer", defer)
        eng.set_geometry(prob.geometry, prob.time_explosion); eng.set_opacity(op)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid); eng.set_packets(prob.packet_collection)
        eng.reset_estimators(); eng.propagate(); eng.synchronize()
        nus, ens = np.zeros(P), np.zeros(P)
        with pytest.raises(NotImplementedError) as ei:
            eng.get_results(output_nus=nus, output_energies=ens, track_last_interaction=True, want_line_estimators=False)
        assert eng.last_variant() == 3 and eng.last_tracker_defer() == defer
        failed = np.flatnonzero(ens == -99.0)
        print("failed packets", len(failed), "first", int(failed[0]))
        assert len(failed) > 100 and len(failed) < P and ei.value.packet_index == failed[0]
        assert np.all(nus[failed] == -5.0)  # (ERR_UNSUPPORTED, the code the reference's NotImplementedError maps to)
        if defer:
            f64, ints = _raw_records(eng, 0, P)
            assert np.all(f64[failed] == 0.0)
            assert np.all(ints[failed] == np.array([-1, -1, -1, -1, 0, 0], dtype=np.int32))
            done = np.setdiff1d(np.arange(P), failed)
            assert (ints[done, 5] == 1).sum() > 100  # (the packets that ended well kept their records)
