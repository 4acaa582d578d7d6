"""Degenerate packets, thin shells and extreme scales on the CPU oracle alone (tests/edge_kinematics.py; the device side is
tests/test_edge_kinematics_gpu.py).

(a) A numpy restatement of calculate_distance_boundary equals the oracle's bit for bit, distance and branch, on every initial packet of
    the "edges" family and on a grid of the edge values of mu against r on and one ulp inside the boundaries of shell 0 and of the two
    thin shells.
(b) The sample hits what it is for: the caps below are conditions on the sample, for each of the four configurations of
    tests/kernel_table_recipes.py (0 or 3 v-packets, partial or full relativity).  Where one fails, change the family's seed.
(c) The problems at extreme scales run (return code 0) and stay below 3e5 events, which keeps a device call at a few seconds.
"""
import ctypes as C

import numpy as np
import pytest

import edge_kinematics as ek
import kernel_table_recipes as ktr
from tardis_amd import state as st

CONFIGS = [(False, 0), (False, ktr.N_VPACKETS), (True, 0), (True, ktr.N_VPACKETS)]
GRAZING_PER_SIGN, LINES_IN_EMPTY_SHELL, ELECTRONS_IN_DENSE_SHELL, MAX_EVENTS = 20, 50, 1000, 300_000
START_LINE_SAMPLE = 12  # packets per kind of nu whose first line is read back from the oracle


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _oracle_distance_boundary(oracle, r, mu, r_inner, r_outer):
    r, mu, r_inner, r_outer = np.broadcast_arrays(r, mu, r_inner, r_outer)
    d, delta = np.empty(r.size), np.empty(r.size, dtype=np.int64)
    for i, args in enumerate(zip(r.ravel(), mu.ravel(), r_inner.ravel(), r_outer.ravel())):
        d[i], delta[i] = oracle.distance_boundary(*(float(a) for a in args))
    return d, delta


# ---- (a) the restatement --------------------------------------------------------------------------------------------------------

def test_distance_boundary_restatement_on_the_initial_packets(oracle):
    prob = ktr.make_problem(False, 0, "edges")
    pk, geo = prob.packet_collection, prob.geometry
    d, delta, check = ek.distance_boundary(pk.initial_radii, pk.initial_mus, geo.r_inner[0], geo.r_outer[0])
    want_d, want_delta = _oracle_distance_boundary(oracle, pk.initial_radii, pk.initial_mus, geo.r_inner[0], geo.r_outer[0])
    assert np.array_equal(_bits(d), _bits(want_d)) and np.array_equal(delta, want_delta)
    # every branch is taken, and distances of both signs of zero and below zero occur
    inward = delta == -1
    assert ((pk.initial_mus > 0) & ~inward).any() and ((pk.initial_mus <= 0) & inward).any() and ((pk.initial_mus <= 0) & ~inward).any()
    print("initial distances: == +0.0", int((_bits(d) == 0).sum()), "== -0.0", int((_bits(d) == _bits(-0.0)).sum()), "< 0", int((d < 0).sum()),
          "in (0, 1e-6 r)", int(((d > 0) & (d < 1e-6 * geo.r_inner[0])).sum()))
    assert (_bits(d) == 0).any() and (_bits(d) == _bits(-0.0)).any()
    assert np.isfinite(d).all() and np.isfinite(check).all()


def test_distance_boundary_restatement_on_the_grid(oracle):
    geo = ek.edge_geometry()
    rng = np.random.default_rng(3)
    up, down = np.inf, -np.inf
    cases = []
    for s in (0,) + ek.THIN_SHELLS:
        ri, ro = geo.r_inner[s], geo.r_outer[s]
        radii = {ri, ro, min(np.nextafter(ri, up), ro), max(np.nextafter(ro, down), ri), ri + 0.5 * (ro - ri), ri + 0.25 * (ro - ri)}
        for r in sorted(radii):
            graze = -np.sqrt(1.0 - (ri / r) * (ri / r))
            mus = [0.0, -0.0, 1.0, -1.0, np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0), graze, np.nextafter(graze, 0.0), np.nextafter(graze, -1.0),
                   -graze, 5e-324, -5e-324]
            mus += [s_ * np.ldexp(1.0, -k) for k in (1, 26, 27, 30, 52, 53, 511, 537, 538, 1000, 1022, 1074) for s_ in (1.0, -1.0)]
            mus += list(rng.uniform(-1.0, 1.0, 8))
            cases += [(r, m, ri, ro) for m in mus]
    r, mu, ri, ro = (np.array(c) for c in zip(*cases))
    d, delta, check = ek.distance_boundary(r, mu, ri, ro)
    want_d, want_delta = _oracle_distance_boundary(oracle, r, mu, ri, ro)
    assert len(r) > 500 and np.isfinite(d).all()
    assert np.array_equal(_bits(d), _bits(want_d)) and np.array_equal(delta, want_delta)
    thin = ro - ri < 1e-8 * ri
    print("grid:", len(r), "cases;", int((d <= 0).sum()), "distances <= 0,", int((d[thin] <= 0).sum()), "of them in a thin shell; check == 0:",
          int(((mu <= 0) & (check == 0)).sum()))
    assert (d[thin] < 0).any() and (d[thin] == 0).any() and ((mu <= 0) & (check == 0)).any() and ((mu <= 0) & (check < 0)).any()


# ---- (b) the sample -------------------------------------------------------------------------------------------------------------

def test_the_family_is_what_it_says():
    for full in (False, True):
        prob = ktr.make_problem(full, 0, "edges")
        e, pk, geo, op = prob.edges, prob.packet_collection, prob.geometry, prob.opacity_state
        assert pk.number_of_packets == ktr.N_PACKETS and len(geo.r_inner) == ktr.N_SHELLS and len(op.line_list_nu) == ktr.N_LINES
        assert np.all(np.diff(np.append(geo.r_inner, geo.r_outer[-1])) > 0) and np.array_equal(geo.r_inner[1:], geo.r_outer[:-1])
        width = (geo.r_outer - geo.r_inner) / geo.r_inner
        assert 0.5e-9 < width[3] < 2e-9 and 0 < width[7] < 4e-16 and np.all(np.delete(width, ek.THIN_SHELLS) > 1e-2)
        assert np.all(op.electron_density[list(ek.EMPTY_SHELLS)] == 0.0) and np.all(np.delete(op.electron_density, ek.EMPTY_SHELLS) > 0)
        mu, r = pk.initial_mus, pk.initial_radii
        assert np.all(e.kind[:64] == ek.WAVE_OF_ZEROS) and np.all(_bits(mu[:64]) == 0)
        assert np.array_equal(e.kind[64:], (np.arange(64, ktr.N_PACKETS) - 64) % 12)
        assert np.all(_bits(mu[e.kind == ek.MU_PLUS_0]) == 0) and np.all(_bits(mu[e.kind == ek.MU_MINUS_0]) == _bits(-0.0))
        assert np.all(mu[e.kind == ek.MU_PLUS_1] == 1.0) and np.all(mu[e.kind == ek.MU_MINUS_1] == -1.0)
        inward = mu[e.kind == ek.INWARD]
        assert np.all((inward > -1) & (inward < 0)) and inward.min() < -0.95 and inward.max() > -0.05
        on_inner = np.isin(e.kind, (ek.GRAZING, ek.ON_R_OUTER, ek.MU_ALMOST_1), invert=True)
        assert np.all(r[on_inner] == geo.r_inner[0]) and np.all(r[e.kind == ek.ON_R_OUTER] == geo.r_outer[0])
        graze = e.kind == ek.GRAZING
        assert np.all((r[graze] > geo.r_inner[0]) & (r[graze] < geo.r_outer[0])) and np.all(mu[graze] < 0)
        tiny = mu[e.kind == ek.MU_TINY]
        assert np.all(np.frexp(tiny)[0] == 0.5) and tiny.max() <= 2.0**-30 and 0 < tiny.min() <= 2.0**-900
        assert np.all(pk.initial_energies[e.kind == ek.ENERGY_TINY] == 1e-150) and pk.initial_energies.max() < 1e140
        assert np.all(pk.initial_energies[e.kind != ek.ENERGY_TINY] == 1.0 / ktr.N_PACKETS)
        almost = np.flatnonzero(e.kind == ek.MU_ALMOST_1)
        assert np.all(mu[almost] == np.nextafter(1.0, 0.0))
        assert np.all(r[almost[::2]] == np.nextafter(geo.r_outer[0], 0.0)) and np.all(r[almost[1::2]] == geo.r_inner[0])
        L = ktr.N_LINES
        for which, value in ((ek.ABOVE, 2.0 * op.line_list_nu[0]), (ek.BELOW, op.line_list_nu[L - 1] / 2.0), (ek.FIRST_LINE, op.line_list_nu[0]),
                             (ek.LAST_LINE, op.line_list_nu[L - 1])):
            assert (e.nu_kind == which).sum() >= 90 and np.all(pk.initial_nus[e.nu_kind == which] == value)
        assert np.all(e.kind[e.nu_kind >= 0] == ek.NU_EDGE)
        # neighbouring lanes differ, and the last wave is ragged
        assert np.all(np.diff(e.kind[64:]) != 0) and ktr.N_PACKETS % 64 == 21


def _first_line_from_the_oracle(oracle, prob, i):
    """The next_line_id packet i starts its first trace with, read from the oracle's trace log of a one-packet run."""
    pk = prob.packet_collection
    one = st.PacketCollection(pk.initial_radii[i:i + 1], pk.initial_nus[i:i + 1], pk.initial_mus[i:i + 1], pk.initial_energies[i:i + 1],
                              pk.packet_seeds[i:i + 1], pk.radiation_field_luminosity)
    lib = oracle.lib()
    lib.oracle_set_trace_log.restype = None
    lib.oracle_set_trace_log.argtypes = [C.c_void_p, C.c_int64]
    lib.oracle_trace_log_count.restype = C.c_int64
    buf = np.full((1 << 16, 4), -1, dtype=np.int64)
    lib.oracle_set_trace_log(buf.ctypes.data, len(buf))
    try:
        ref = oracle.run(one, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration, prob.spectrum_frequency_grid,
                         math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=False)
        n = int(lib.oracle_trace_log_count())
    finally:
        lib.oracle_set_trace_log(None, 0)
    assert ref.return_code == 0 and n >= 1 and buf[0, 0] == 0
    return int(buf[0, 1])


@pytest.mark.parametrize("full,n_vpackets", CONFIGS)
def test_the_sample_hits_what_it_is_for(oracle, full, n_vpackets):
    prob, ref = ktr.case(oracle, full, n_vpackets, "edges")  # (asserts return code 0)
    e, pk, t = prob.edges, prob.packet_collection, ref.trackers
    classes, m = ktr.sample_mix(ref), ek.mix(prob, ref)
    print("full", full, "v-packets", n_vpackets, classes, m)
    for what, n in classes.items():
        assert n > 0, what
    for n in m["grazing: check > 0 / == 0 / < 0"]:
        assert n >= GRAZING_PER_SIGN
    reabsorbed, emitted, untouched = ref.output_energies < 0, ref.output_energies > 0, t.interactions_count == 0
    # kinds 4 and 5: reabsorbed at their first event.  Full relativity takes the initial mu for a comoving one and aberrates it at the
    # start, mu' = (mu + beta) / (1 + beta mu): the packets of kind 5 with mu in (-beta, 0) -- beta = 0.037, a few per cent of a uniform
    # draw, whatever the seed -- then start OUTWARD in the lab frame, and the cap holds for every packet whose lab-frame mu is <= 0.
    _, mu_start, comov = ek.start_state(pk.initial_radii, pk.initial_mus, pk.initial_nus, prob.time_explosion, full)
    inward = np.isin(e.kind, (ek.MU_MINUS_1, ek.INWARD))
    beta = pk.initial_radii / prob.time_explosion / st.C_SPEED_OF_LIGHT
    if not full:
        assert np.all(mu_start[inward] <= 0)
    else:
        assert np.array_equal(mu_start[inward] > 0, pk.initial_mus[inward] > -beta[inward]) and np.all(mu_start[e.kind == ek.MU_MINUS_1] == -1.0)
        assert (mu_start[inward] > 0).sum() < 0.1 * (e.kind == ek.INWARD).sum()
    assert np.all((reabsorbed & untouched)[inward & (mu_start <= 0)]) and (inward & (mu_start <= 0)).sum() > 900
    zero = np.isin(e.kind, (ek.MU_PLUS_0, ek.MU_MINUS_0, ek.WAVE_OF_ZEROS))
    if not full:
        assert np.all((reabsorbed & untouched)[zero])
    else:
        kinds_1_2 = np.isin(e.kind, (ek.MU_PLUS_0, ek.MU_MINUS_0))
        assert np.all(mu_start[zero] == beta[zero]) and emitted[kinds_1_2].sum() > 0.5 * kinds_1_2.sum()
        assert not (reabsorbed & untouched)[zero].any(), "the start-up aberration turns mu = 0 outward: the first wave runs normally"
    for s in ek.THIN_SHELLS:
        assert ref.j_estimator[s] > 0, s
    if n_vpackets:  # (without v-packets there is no log to restate from; the r-packets' own thin-shell distances are not in a result)
        d, _ = ek.vpacket_thin_shell_distances(prob, ref)
        assert (d <= 0).sum() >= 1 and ref.vpacket_log_count > 1000
    assert ((t.shell_id == 2) & (t.interaction_type == 2)).sum() >= LINES_IN_EMPTY_SHELL
    assert ((t.shell_id == ek.DENSE_SHELL) & (t.interaction_type == 4)).sum() >= ELECTRONS_IN_DENSE_SHELL
    assert not (np.isin(t.shell_id, ek.EMPTY_SHELLS) & (t.interaction_type == 4)).any()
    # the start-up search
    nu_line = prob.opacity_state.line_list_nu
    L = len(nu_line)
    on = e.on_line >= 0
    assert 2 * on.sum() >= e.on_a_line_tried and np.array_equal(comov[on], nu_line[e.on_line[on]])
    want = ek.first_line_id(nu_line, comov)
    assert np.all(want[e.nu_kind == ek.ABOVE] == 0) and np.all(want[e.nu_kind == ek.BELOW] == L - 1)
    assert np.array_equal(want[on], np.minimum(e.on_line[on] + 1, L - 1)), "the >= tie: the search steps over a line equal to comov_nu"
    assert np.all(np.isin(want[e.nu_kind == ek.FIRST_LINE], (0, 1))) and np.all(want[e.nu_kind == ek.LAST_LINE] == L - 1)
    for which in (ek.ABOVE, ek.BELOW, ek.FIRST_LINE, ek.LAST_LINE, ek.ON_A_LINE):
        for i in np.flatnonzero(e.nu_kind == which)[:START_LINE_SAMPLE]:
            assert _first_line_from_the_oracle(oracle, prob, i) == want[i], (ek.NU_NAMES[which], i)
    assert ref.counters["events"] < MAX_EVENTS


# ---- (c) the extreme scales -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("full,n_vpackets", CONFIGS)
@pytest.mark.parametrize("kind", ek.SCALES)
def test_scaled_problems_run(oracle, kind, full, n_vpackets):
    prob, ref = ek.scaled_case(oracle, kind, full, n_vpackets)
    classes = ktr.sample_mix(ref)
    print(kind, "full", full, "v-packets", n_vpackets, "events", ref.counters["events"], classes)
    assert ref.return_code == 0 and ref.counters["events"] < MAX_EVENTS
    assert np.all(prob.packet_collection.initial_radii == prob.geometry.r_inner[0])
    assert np.isfinite(ref.j_estimator).all() and np.isfinite(ref.j_blue_estimator).all() and np.all(ref.j_estimator > 0)
    for what, n in classes.items():
        assert n > 0, what
    if kind == "beta 0.5":
        assert prob.geometry.v_outer[-1] / st.C_SPEED_OF_LIGHT > 0.5
    if kind.startswith("energy"):
        e = prob.packet_collection.initial_energies
        assert np.all((e < 1e-140) | (e > 1e140)), "every lane outside mid_range"
