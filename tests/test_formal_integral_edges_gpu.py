"""The formal-integral kernels (fi_intersections_kernel, fi_rays_kernel, fi_trapezoid_kernel) on the edges, against the long-double
restatement and the closed forms of tests/formal_integral_ref.py and against the oracle.

The edge model puts impact parameters ON r_inner[0] and ON r_outer[0..2] (N = 9, 17, 33), has N = 2 and N = 3, duplicate lines, a
transparent and an opaque line, and 129 frequencies -- two full waves and one lane -- of which one starts every ray behind the last
line and one reaches no line at all.  Held to: the oracle and the restatement at rtol 1e-11 (the project's bar for this kernel:
device exp against libm), without electron scattering every ray to the derived (4 K + 64) 2^-53, the zero pattern exactly, and the
work counter to the number of resonances the restatement crossed, exactly, in full and in partial waves.

Measured largest relative deviation from the restatement over all edge inputs: device I 1.5e-15, L 1.3e-15; oracle I 1.5e-15,
L 1.3e-15 (device against oracle: 1.9e-16).  Worst ray against the derived bound: 13.3 x 2^-53, at K = 1."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import formal_integral_ref as ref  # noqa: E402
from tardis_amd import synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-11
T_INNER = 1.0e4
N_RESIDENT = 33
RESIDENT_MODELS = {  # the "short" and "two_shells" models of tests/test_formal_interpolate_gpu.py
    "short": dict(n_shells=20, n_lines=40, line_interaction_type="macroatom", level_sizes="uniform"),
    "two_shells": dict(n_shells=2, n_lines=3000, line_interaction_type="macroatom", level_sizes="heavy"),
}


class Geo:
    def __init__(self, r_inner, r_outer):
        self.r_inner, self.r_outer = np.asarray(r_inner), np.asarray(r_outer)


@contextlib.contextmanager
def device(m, N):
    """(integrator, its engine) on the model's geometry, line list, optical depths and electron densities.  The integrator does
    not hand out the engine it would make, and the counter is read from the engine: it is built here, as _ensure_engine does."""
    from tardis_amd import state as st
    from tardis_amd.engine import Engine
    from tardis_amd.formal_integral import FormalIntegratorHIP
    geo = Geo(m["r_inner"], m["r_outer"])
    nu, n_e = np.asarray(m["line_list_nu"]), np.asarray(m["electron_density"])
    L, S = len(nu), len(n_e)
    ost = st.OpacityState(n_e, np.zeros(S), nu, np.asarray(m["tau_sobolev"]), np.ones((L, S)), np.arange(L, dtype=np.int64),
                          np.arange(L + 1, dtype=np.int64), -np.ones(L, dtype=np.int64), np.zeros(L, dtype=np.int64),
                          np.arange(L, dtype=np.int64))
    with Engine(0) as eng:
        eng.set_geometry(geo, float(m["time_explosion"]))
        eng.set_opacity(ost)
        fi = FormalIntegratorHIP(geo, float(m["time_explosion"]), ost, N, engine=eng)
        try:
            yield fi, eng
        finally:
            fi.close()


def integrate(fi, eng, m, N, frequencies=None):
    """(L_nu, I_nu_p, line_visits) of one host-fed call."""
    freqs = m["frequencies"] if frequencies is None else frequencies
    lum, inten = fi.formal_integral(float(m["inner_temperature"]), freqs, m["att_S_ul"], m["Jred_lu"], m["Jblue_lu"], m["tau_sobolev"],
                                    m["electron_density"], N)
    return lum, inten, eng.last_counters()["line_visits"]


def oracle_call(m, N):
    from oracle import formal
    return ref.call(formal.formal_integral, m, N)


def assert_bit_equal(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def full_run():
    """(L, N, electrons) -> (L_nu, I_nu_p, line_visits) of the device on all 129 frequencies, run once."""
    done = {}

    def get(L, N, electrons=True):
        if (L, N, electrons) not in done:
            m, _ = ref.edge_reference(L, N, electrons)
            with device(m, N) as (fi, eng):
                done[L, N, electrons] = integrate(fi, eng, m, N)
            for a in done[L, N, electrons][:2]:
                a.setflags(write=False)
        return done[L, N, electrons]
    return get


@pytest.mark.parametrize("L,N,electrons", ref.EDGE_CASES, ids=[f"L{L}-N{N}-{'ne' if e else 'ne0'}" for L, N, e in ref.EDGE_CASES])
def test_edge_model(full_run, L, N, electrons):
    m, (lum_r, inten_r, K) = ref.edge_reference(L, N, electrons)
    lum, inten, visits = full_run(L, N, electrons)
    lum_o, inten_o = oracle_call(m, N)
    print(f"L {L} N {N} electrons {electrons}: device max relative deviation from the reference I {ref.max_rel(inten, inten_r):.3g} "
          f"L {ref.max_rel(lum, lum_r):.3g}, from the oracle I {ref.max_rel(inten, inten_o):.3g} L {ref.max_rel(lum, lum_o):.3g}; "
          f"oracle from the reference I {ref.max_rel(inten_o, inten_r):.3g} L {ref.max_rel(lum_o, lum_r):.3g}; "
          f"line_visits {visits} resonances {int(K.sum())}")
    assert inten.shape == (129, N) and lum.shape == (129,)
    assert np.isfinite(inten).all() and np.isfinite(lum).all() and (inten >= 0).all() and (lum >= 0).all()
    assert np.array_equal(inten == 0, inten_r == 0) and np.array_equal(lum == 0, lum_r == 0)
    assert visits == K.sum()
    if N == 2:
        assert (inten == 0).all() and (lum == 0).all() and visits == 0
        return
    assert ref.max_rel(inten, inten_o) <= RTOL and ref.max_rel(lum, lum_o) <= RTOL
    assert ref.max_rel(inten, inten_r) <= RTOL and ref.max_rel(lum, lum_r) <= RTOL
    if not electrons:
        nz = inten_r != 0
        err = np.abs(inten.astype(ref.LD) - inten_r)[nz] / inten_r[nz]
        worst = np.argmax(err / ref.ray_bound(K[nz]))
        print(f"  worst ray against (4K + 64) 2^-53: {float(err[worst]) / ref.EPS:.1f} x 2^-53 at K = {int(K[nz][worst])}")
        assert (err <= ref.ray_bound(K[nz])).all()


def test_partial_waves_counter_and_rows(full_run):
    """frequencies[:n]: n = 1 and 65 leave 63 lanes of a wave without a ray, the p_idx = 0 blocks do no work at all.  The counter is
    the resonances of exactly those rays, and a ray does not depend on how many neighbours it has."""
    L, N = 37, 9
    m, (_, _, K) = ref.edge_reference(L, N, True)
    lum, inten, visits = full_run(L, N, True)
    assert visits == K.sum()
    with device(m, N) as (fi, eng):
        for n in (1, 63, 64, 65, 129):
            lum_n, inten_n, visits_n = integrate(fi, eng, m, N, m["frequencies"][:n])
            print("n", n, "line_visits", visits_n, "resonances", int(K[:n].sum()))
            assert visits_n == K[:n].sum(), n
            assert_bit_equal(inten_n, inten[:n])
            assert_bit_equal(lum_n, lum[:n])
        # one lane and one wave plus a lane of rays that do cross lines (frequencies[0] and [1] reach none)
        for lo, hi in ((64, 65), (2, 67)):
            lum_n, inten_n, visits_n = integrate(fi, eng, m, N, m["frequencies"][lo:hi])
            print("frequencies", lo, "to", hi, "line_visits", visits_n, "resonances", int(K[lo:hi].sum()))
            assert visits_n == K[lo:hi].sum() > 0, (lo, hi)
            assert_bit_equal(inten_n, inten[lo:hi])
            assert_bit_equal(lum_n, lum[lo:hi])


def test_shuffled_frequencies(full_run):
    L, N = 37, 17
    m, (_, _, K) = ref.edge_reference(L, N, True)
    lum, inten, visits = full_run(L, N, True)
    order = np.random.default_rng(3).permutation(129)
    assert (order != np.arange(129)).any()
    with device(m, N) as (fi, eng):
        lum_s, inten_s, visits_s = integrate(fi, eng, m, N, m["frequencies"][order])
    assert visits_s == visits == K.sum()
    assert_bit_equal(inten_s, inten[order])
    assert_bit_equal(lum_s, lum[order])


@pytest.mark.parametrize("L,N", [(37, 9), (37, 2), (2000, 17)])
def test_without_intensities(full_run, L, N):
    """want_intensities=False (intensities_nu_p == nullptr in the library): the same luminosities and the same counter."""
    m, (_, _, K) = ref.edge_reference(L, N, True)
    lum, _, visits = full_run(L, N, True)
    with device(m, N) as (fi, eng):
        lum_n, none = eng.formal_integral(float(m["inner_temperature"]), m["frequencies"], m["att_S_ul"], m["Jred_lu"], m["Jblue_lu"], N,
                                          want_intensities=False)
        assert none is None and eng.last_counters()["line_visits"] == visits == K.sum()
    assert_bit_equal(lum_n, lum)


@pytest.mark.parametrize("n_lines", [1, 2])
def test_closed_forms(n_lines):
    """One shell, one and two lines (formal_integral_ref.closed_form_one_shell): the crossing rays at rtol 1e-13, the core rays --
    a black body times p, p_idx = 4 ON r_inner included -- at the derived 64 * 2^-53, every other ray exactly 0."""
    m = ref.closed_form_model(n_lines)
    N = ref.CLOSED_N
    want, crossing = ref.closed_form_one_shell(m)
    with device(m, N) as (fi, eng):
        lum, inten, visits = integrate(fi, eng, m, N)
    core = np.zeros_like(crossing)
    core[:, 1:5] = True
    assert ref.H_CGS * m["frequencies"].max() / (ref.KB_CGS * m["inner_temperature"]) <= 8  # (core rays: z0 < 1)
    err = np.abs(inten.astype(ref.LD) - want) / np.where(want != 0, want, 1)
    print(n_lines, "line(s): device against the closed form: crossing rays", float(err[crossing].max()), "core rays",
          float(err[core].max()) / ref.EPS, "x 2^-53; line_visits", visits)
    assert np.array_equal(inten == 0, want == 0)
    assert np.array_equal(want != 0, crossing | core)
    assert (err[crossing] <= 1e-13).all()
    assert (err[core] <= 64 * ref.EPS).all()
    _, _, K = ref.call(ref.reference, m, N)
    assert visits == K.sum() and K.sum() >= crossing.sum()
    want_lum = ref.closed_form_luminosity(want, m["r_outer"][0])
    assert ref.max_rel(lum, want_lum) <= RTOL


# ---- resident and interpolated entry points -------------------------------------------------------------------------------

def run_resident(eng, name):
    """The model `name` propagated on `eng`, its source function resident: (problem, source function arrays)."""
    prob = synthetic.make_problem(seed=7, n_packets=20_000, log_tau_mean=-2.0, **RESIDENT_MODELS[name])
    eng.set_geometry(prob.geometry, prob.time_explosion)
    eng.set_opacity(prob.opacity_state)
    eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
    eng.set_packets(prob.packet_collection)
    eng.reset_estimators()
    eng.propagate()
    eng.synchronize()
    sf = eng.source_function(prob.packet_collection.time_of_simulation, prob.geometry.volume)
    return prob, sf


def host_fed(prob, r_inner, r_outer, tau, n_e, tables, freqs):
    """A host-fed integrator of its own on the given shells and tables: (L_nu, I_nu_p)."""
    from tardis_amd.formal_integral import FormalIntegratorHIP
    fi = FormalIntegratorHIP(Geo(r_inner, r_outer), prob.time_explosion, prob.opacity_state, N_RESIDENT)
    try:
        return fi.formal_integral(T_INNER, freqs, tables["att_S_ul"], tables["Jred_lu"], tables["Jblue_lu"], tau, n_e, N_RESIDENT)
    finally:
        fi.close()


def resonances(prob, r_inner, r_outer, tau, n_e, tables, freqs):
    return ref.reference(r_inner, r_outer, prob.time_explosion, prob.opacity_state.line_list_nu, tau, n_e, T_INNER, freqs,
                         tables["att_S_ul"], tables["Jred_lu"], tables["Jblue_lu"], N_RESIDENT)[2]


@pytest.mark.parametrize("name", list(RESIDENT_MODELS))
def test_resident_entry_points_on_the_ragged_frequencies(name):
    """formal_integral_resident and (model "short") formal_integral_interpolated(8) with the 129 frequencies of the edge recipe on
    the model's own line list: the host-fed path on the downloaded tables bit for bit, the counter to the restatement's count."""
    from tardis_amd.engine import Engine
    with Engine(0) as eng:
        prob, sf = run_resident(eng, name)
        geo, op = prob.geometry, prob.opacity_state
        freqs = ref.recipe_frequencies(op.line_list_nu, geo.r_outer[-1], prob.time_explosion)
        assert len(freqs) == 129 and np.count_nonzero(sf["att_S_ul"]) > 0
        lum, inten = eng.formal_integral_resident(T_INNER, freqs, N_RESIDENT, want_intensities=True)
        visits = eng.last_counters()["line_visits"]
        if name == "short":
            src = eng.interpolated_source(8)
            freqs_i = ref.recipe_frequencies(op.line_list_nu, src["r_outer"][-1], prob.time_explosion)
            lum_i, inten_i = eng.formal_integral_interpolated(8, T_INNER, freqs_i, N_RESIDENT, want_intensities=True)
            visits_i = eng.last_counters()["line_visits"]
    lum_h, inten_h = host_fed(prob, geo.r_inner, geo.r_outer, op.tau_sobolev, op.electron_density, sf, freqs)
    assert_bit_equal(lum, lum_h)
    assert_bit_equal(inten, inten_h)
    K = resonances(prob, geo.r_inner, geo.r_outer, op.tau_sobolev, op.electron_density, sf, freqs)
    print(name, "resident: line_visits", visits, "resonances", int(K.sum()))
    assert K[0].sum() == 0 and K[1].sum() == 0 and K.sum() > 0
    assert visits == K.sum()
    if name == "short":
        L = RESIDENT_MODELS[name]["n_lines"]
        tau_i = np.ascontiguousarray(src["tau_sobolev"].reshape(7, L).T)  # [L, S'], as an opacity state holds it
        lum_h, inten_h = host_fed(prob, src["r_inner"], src["r_outer"], tau_i, src["electron_density"], src, freqs_i)
        assert_bit_equal(lum_i, lum_h)
        assert_bit_equal(inten_i, inten_h)
        K_i = resonances(prob, src["r_inner"], src["r_outer"], tau_i, src["electron_density"], src, freqs_i)
        print(name, "interpolated: line_visits", visits_i, "resonances", int(K_i.sum()))
        assert K_i.sum() > 0 and visits_i == K_i.sum()
