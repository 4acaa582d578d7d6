"""Line lists with coincident and near-coincident lines, on the CPU oracle alone (tests/coincident_lines.py; the device side is
tests/test_coincident_lines_gpu.py).

(1) The clustered sample hits what it is for: the floors below are conditions on the sample, for each of the four configurations of
    tests/kernel_table_recipes.py (0 or 3 v-packets, partial or full relativity).
(2) A metamorphic property of the reference: inserting lines of optical depth 0 that coincide with existing lines changes nothing --
    per-packet results, J and nu_bar, the v-packet histogram and the number of draws bit for bit, j_blue and Edotlu on the old lines
    bit for bit.  (A twin's own j_blue is NOT its original's: in partial relativity the estimator carries the line's frequency through
    the Doppler factor of the packet's position at the twin, which legitimately differs.)
(3) The degenerate lists -- every line at one frequency, two frequencies -- run, and interact.
"""
import numpy as np
import pytest

import coincident_lines as cl
import kernel_table_recipes as ktr

CONFIGS = [(False, 0), (False, ktr.N_VPACKETS), (True, 0), (True, ktr.N_VPACKETS)]
# the floors of the sample (per configuration)
PER_KIND, RESTARTS, BLUEWARD, REDWARD, PER_CLASS = 100, 400, 300, 200, 500


def test_the_list_is_what_it_says():
    nu, kind, place = cl.clustered()
    L = ktr.N_LINES
    assert len(nu) == L and np.all(np.diff(nu) <= 0)
    lam = cl.st.C_SPEED_OF_LIGHT / nu / cl.synthetic.ANGSTROM
    assert 2500.0 <= lam.min() and lam.max() <= 10000.0
    gap = cl.relative_gap(nu)
    # the fixed places: [0, 13), 20 lines straddling line 2048, 17 lines ending at L - 1, all of equal lines
    for where, a, b in ((cl.AT_LINE_0, 0, 13), (cl.AT_TILE_BOUNDARY, 2038, 2058), (cl.AT_LAST_LINE, L - 17, L)):
        assert np.array_equal(np.flatnonzero(place == where), np.arange(a, b))
        assert np.all(nu[a:b] == nu[a]) and np.all(kind[a:b] == cl.EQUAL)
        assert (a == 0 or nu[a - 1] > nu[a]) and (b == L or nu[b] < nu[a])
    assert 2038 < ktr.EST_TILE < 2057
    # the runs: maximal stretches of one kind
    edges = np.flatnonzero(np.diff(np.concatenate(([0], kind, [0]))) != 0)
    runs = [(a, b - a, int(kind[a])) for a, b in zip(edges[:-1], edges[1:]) if kind[a]]
    assert all(kind[a - 1] == 0 for a, _, _ in runs if a) and len(runs) > 60
    seen = {(n, k) for _, n, k in runs}
    assert {(n, k) for n in cl.RUN_LENGTHS for k in cl.KINDS} <= seen, "not every length in every kind"
    for a, n, k in runs:
        inside = gap[a:a + n - 1]
        if k == cl.EQUAL:
            assert np.all(inside == 0)
        elif k == cl.ULP_APART:
            assert np.array_equal(nu[a + 1:a + n], np.nextafter(nu[a:a + n - 1], 0.0))
        elif k == cl.INSIDE:
            assert np.all(np.abs(nu[a:a + n] - nu[a]) / nu[a] < cl.CLOSE_LINE_THRESHOLD) and nu[a + n - 1] < nu[a]
        else:
            assert np.all(inside > cl.CLOSE_LINE_THRESHOLD) and np.all(inside < 4e-14)
        if k != cl.OUTSIDE:
            assert np.all(inside < cl.CLOSE_LINE_THRESHOLD)
    # outside the runs the list is the continuous draw: nothing close
    free = (kind[:-1] == 0) | (kind[1:] == 0)
    assert np.all(gap[free] > 1e-9)


@pytest.mark.parametrize("full,n_vpackets", CONFIGS)
def test_the_sample_hits_what_it_is_for(oracle, full, n_vpackets):
    prob, ref = ktr.case(oracle, full, n_vpackets, "clustered")  # (asserts return code 0)
    nu, kind, place = cl.clustered()
    assert np.array_equal(prob.opacity_state.line_list_nu, nu)
    classes = ktr.sample_mix(ref)
    m = cl.mix(ref, nu, kind, place, prob.packet_collection, prob.geometry, full)
    print(full, n_vpackets, classes, m, "macro transitions", ref.counters["macro_transitions"])
    for what, n in classes.items():
        assert n >= PER_CLASS, what
    assert ref.counters["macro_transitions"] > 0
    for k in cl.KINDS:
        assert m["absorbed in kind"][k] >= PER_KIND, cl.KIND_NAMES[k]
        assert m["emitted in kind"][k] >= PER_KIND, cl.KIND_NAMES[k]
    assert m["restarts on a close line"] >= RESTARTS
    assert m["start blueward of line 0"] >= BLUEWARD
    assert m["start redward of the last line"] >= REDWARD
    for where in cl.PLACES:
        assert np.any(ref.j_blue_estimator[place == where] != 0.0), where
    if n_vpackets:
        assert ref.vpacket_log_count > 1000


def _oracle(oracle, prob):
    ref = oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
                     prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=True)
    assert ref.return_code == 0
    return ref


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("full,n_vpackets", CONFIGS)
def test_zero_depth_twins_change_nothing(oracle, full, n_vpackets):
    base, twins, old_of_new = cl.twin_problems(full, n_vpackets)
    old = old_of_new >= 0
    assert (~old).sum() > 2000 and old.sum() == ktr.N_LINES
    assert np.all(twins.opacity_state.tau_sobolev[~old] == 0.0)
    a, b = _oracle(oracle, base), _oracle(oracle, twins)
    assert int((a.trackers.interaction_type == 2).sum()) > 500
    assert same_bits(a.output_nus, b.output_nus) and same_bits(a.output_energies, b.output_energies)
    for f in ("interaction_type", "interactions_count", "shell_id"):
        assert np.array_equal(getattr(a.trackers, f), getattr(b.trackers, f)), f
    assert same_bits(a.j_estimator, b.j_estimator) and same_bits(a.nu_bar_estimator, b.nu_bar_estimator)
    assert same_bits(a.v_packets_energy_hist, b.v_packets_energy_hist)
    assert a.counters["rng_draws"] == b.counters["rng_draws"]
    assert same_bits(a.j_blue_estimator, b.j_blue_estimator[old]) and same_bits(a.edotlu_estimator, b.edotlu_estimator[old])
    for f in ("interaction_line_absorb_id", "interaction_line_emit_id"):
        ids_a, ids_b = getattr(a.trackers, f), getattr(b.trackers, f)
        line = a.trackers.interaction_type == 2
        assert np.array_equal(ids_a[line], old_of_new[ids_b[line]]), f
        assert np.array_equal(ids_a[~line], ids_b[~line]), f
    if n_vpackets:
        assert a.vpacket_log_count == b.vpacket_log_count > 1000
        assert same_bits(a.vpacket_nus, b.vpacket_nus) and same_bits(a.vpacket_energies, b.vpacket_energies)


@pytest.mark.parametrize("n_frequencies", [1, 2])
@pytest.mark.parametrize("full,n_vpackets", CONFIGS)
def test_degenerate_lists(oracle, n_frequencies, full, n_vpackets):
    prob = cl.degenerate_problem(n_frequencies, full, n_vpackets)
    assert len(np.unique(prob.opacity_state.line_list_nu)) == n_frequencies and len(prob.opacity_state.line_list_nu) == 200
    ref = _oracle(oracle, prob)
    t = ref.trackers
    lines = int((t.interaction_type == 2).sum())
    print(n_frequencies, full, n_vpackets, "last is a line", lines, "line visits", ref.counters["line_visits"])
    assert lines > 0
    if n_frequencies == 2:  # both frequencies absorb
        absorbed = t.interaction_line_absorb_id[t.interaction_type == 2]
        assert (absorbed < 100).any() and (absorbed >= 100).any()
