"""Photo-ionisation and heating estimators from the transport on the device (option bf_estimators; csrc/bf_estimators.hpp) against
tests/bf_estimator_ref.py: the segment log of the lane kernel and of the wave-owner kernel, the accumulate pass, its edges through
tardis_mc_debug_bf_accumulate, what the option must not move, dropped records, the rates and option continuum_field, the state rules.

The problem: 4 shells, 300 lines, 4096 packets (64 waves, a log of some 130 chunks of 128 records; every packet moves at least once), downbranch and macroatom.  The continua,
NC = 4, laid over synthetic.comoving_frequency_range(): A two points over the whole range with x = X nu; B 33 points over the middle
third (of the logarithmic range: where a 1e4-K photosphere's packets are); C five points above every comoving frequency; D three
points whose last frequency lies inside the range.

Tolerances, u = 2^-53.  A sum of n non-negative terms added in any order is within (n - 1) u of the exact sum, relatively, and math.fsum
is within u of it: two such sums of the same terms are held to n 2^-52 = 2 n u.  That is the bound of the log against J and nu_bar (same
terms bit for bit) and of a table cell against the reference (n = the cell's statistics).
The consequence of A: x_c = ((fl(X nu_hi) hw) + (fl(X nu_lo) lw)) / interval is X nu (1 + d), |d| <= 4 u (table entry, product, sum of two
positive terms, quotient); inc = (ed x_c) / nu adds two roundings: every term of photo_ion[A,s] is X ed (1 + 6 u), the sum adds n u, J
another n u and the product X J one more: (8 + 2 n) u relative.  A heating term is (ed x_c)(1 - nu_i / nu): the bracket lies in [0, 1]
with an ABSOLUTE error <= 2 u (quotient, difference), so the term is within X ed nu 8 u of X ed (nu - nu_i) absolutely -- relative to X
nu_bar, not to the difference, which cancels for frequencies near nu_i.  The right-hand side X (nu_bar - nu_i J) carries (n + 2) u of
nu_bar and of nu_i J each.  Bound used: X (nu_bar + nu_i J) (10 + 3 n) u, absolute."""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bf_estimator_ref as bref  # noqa: E402
from tardis_amd import _abi, synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, S, L, K, P = 7, 4, 300, 60, 4096
X = 1.0e-33   # cm^2 / Hz: x = X nu is ~1e-18 cm^2 at 1e15 Hz
U = 2.0 ** -53
T_E = np.array([11000.0, 9500.0, 8200.0, 7000.0])
TABLES = bref.TABLES + ("statistics",)
A, B, C_, D = 0, 1, 2, 3


class Model:
    def __init__(self, mode, full, n_levels=K):
        self.prob = synthetic.make_problem(seed=SEED, n_packets=P, n_shells=S, n_lines=L, line_interaction_type=mode, enable_full_relativity=full,
                                           n_bins=2000)
        self.ld = synthetic.make_line_data(SEED, self.prob.opacity_state, n_levels=n_levels, time_explosion=self.prob.time_explosion)
        self.pd = synthetic.make_plasma_data(SEED, self.ld, S)
        lo, hi = synthetic.comoving_frequency_range(self.prob)
        self.lo, self.hi = lo, hi
        a = np.array([lo, hi])
        b = np.geomspace(lo ** (2 / 3) * hi ** (1 / 3), lo ** (1 / 3) * hi ** (2 / 3), 33)
        c = np.linspace(1.5 * hi, 3.0 * hi, 5)
        d = np.array([lo, np.sqrt(lo * b[0]), b[8]])
        self.blocks = [(a, X * a), (b, 6.3e-18 * (b[0] / b) ** 3), (c, 1e-18 * np.ones(5)), (d, np.array([2e-18, 1e-18, 5e-19]))]
        self.cd = synthetic.make_covering_continuum_data(self.pd, self.blocks)


_MODELS, _RUNS = {}, {}


def model(mode="macroatom", full=False):
    if (mode, full) not in _MODELS:
        _MODELS[mode, full] = Model(mode, full)
    return _MODELS[mode, full]


@pytest.fixture(scope="module")
def eng(oracle):
    with Engine(0) as e:
        yield e


def stage(eng, m, cd=None, pd=None, ld=None):
    eng.set_geometry(m.prob.geometry, m.prob.time_explosion)
    eng.set_opacity(m.prob.opacity_state)
    eng.set_config(m.prob.montecarlo_configuration, m.prob.spectrum_frequency_grid)
    eng.set_line_data(ld or m.ld)
    eng.set_plasma_data(pd or m.pd)
    eng.set_continuum_data(cd or m.cd)


OPTION_DEFAULTS = {"variant": -1, "bf_estimators": 0, "track_full": 0, "segment_log_capacity": 0, "segment_log_keep": 0, "continuum_field": 0,
                   "event_log_capacity": 0}


def propagate(eng, m, bf=True, reset=True, **options):
    """One staged propagate of the model's packets; the dict of what the call left."""
    options = dict(options, bf_estimators=int(bf), segment_log_keep=int(bf))
    for k, v in options.items():
        eng.set_option(k, v)
    try:
        eng.set_packets(m.prob.packet_collection)
        if reset:
            eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        track_full = bool(options.get("track_full"))
        res = eng.get_results(track_full=track_full)
        out = {"res": res, "variant": eng.last_variant(), "key": eng.last_kernel_key()}
        if bf:
            out["log"] = eng.get_segment_log()
            try:
                out["tables"] = eng.get_bf_estimators()
            except RuntimeError as e:
                out["error"] = e
        return out
    finally:
        for k in options:
            eng.set_option(k, OPTION_DEFAULTS[k])


def run(eng, mode, full, variant, bf=True, track_full=False):
    """The runs the tests share, made once and never written to."""
    key = (mode, full, variant, bf, track_full)
    if key not in _RUNS:
        m = model(mode, full)
        stage(eng, m)
        if bf:
            eng.set_bf_estimators(T_E)
        _RUNS[key] = propagate(eng, m, bf, variant=variant, track_full=int(track_full), event_log_capacity=64 * P if track_full else 0)
        assert _RUNS[key]["variant"] == variant
    return _RUNS[key]


def reference(m, log):
    return bref.tables(m.cd, T_E, S, log["nu"], log["ed"], log["shell"])


def assert_tables(got, want):
    """The statistics exact, every sum within statistics * 2^-52 of the reference's, relatively (module docstring)."""
    assert np.array_equal(got["statistics"], want["statistics"])
    n = want["statistics"].astype(np.float64)
    for name in bref.TABLES:
        assert np.all(np.abs(got[name] - want[name]) <= n * 2.0 ** -52 * want[name]), name
        assert np.all((want[name] == 0.0) == (got[name] == 0.0)), name


MODES = ["downbranch", "macroatom"]


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("mode", MODES)
def test_the_log_sums_to_j_and_nu_bar(eng, mode, variant):
    """Partial relativity: ed is the term added to J, ed nu the term added to nu_bar, and every record names the move's shell."""
    r = run(eng, mode, False, variant)
    log, res = r["log"], r["res"]
    assert r["key"][0] == ("lane" if variant == 0 else "wave")
    assert len(log["nu"]) >= P and np.all(log["ed"] > 0) and np.all(log["nu"] > 0) and log["shell"].min() == 0 and log["shell"].max() == S - 1
    n_s = np.bincount(log["shell"], minlength=S)
    j, nu_bar = bref.shell_fsum(log["ed"], log["shell"], S), bref.shell_fsum(log["ed"] * log["nu"], log["shell"], S)
    assert np.all(np.abs(j - res.j_estimator) <= n_s * 2.0 ** -52 * j)
    assert np.all(np.abs(nu_bar - res.nu_bar_estimator) <= n_s * 2.0 ** -52 * nu_bar)
    assert r["tables"]["n_records"] == len(log["nu"]) and r["tables"]["n_dropped"] == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("full", [False, True])
def test_both_kernels_log_the_same_records(eng, mode, full):
    """The per-packet arithmetic of the two kernels is bit-identical, so their logs are the same multiset of records."""
    a, b = run(eng, mode, full, 0)["log"], run(eng, mode, full, 2)["log"]

    def ordered(log):
        order = np.lexsort((log["ed"], log["nu"], log["shell"]))
        return [log[k][order] for k in ("shell", "nu", "ed")]
    for x, y in zip(ordered(a), ordered(b)):
        assert np.array_equal(x, y)


def moved_rows(ft, initial_radii):
    """The rows of an event log whose move had a positive length: a move of positive length changes the packet's radius or its direction
    (barring a length below the rounding of both), one of length zero changes neither.  A row's radius and before_mu are the packet's
    after the move; the previous row's radius and after_mu (a packet's first row: its initial radius) are those before it."""
    first = ft.offsets[:-1]
    prev_r, prev_mu = np.empty(ft.n_rows), np.empty(ft.n_rows)
    prev_r[1:], prev_mu[1:] = ft.radius[:-1], ft.after_mu[:-1]
    prev_r[first] = initial_radii
    prev_mu[first] = ft.before_mu[first]  # (a packet's first move is judged by its radius alone)
    return int(np.count_nonzero((ft.radius != prev_r) | (ft.before_mu != prev_mu)))


@pytest.mark.parametrize("variant", [0, 2])
def test_full_relativity_record_count_against_the_event_log(eng, variant):
    """Full relativity (ed is no longer J's term: the distance is logged before its Doppler scaling): a record per move of positive length
    -- the rows of the same call's event log that moved.  On this problem every move has a positive length; the next test has the others."""
    r = run(eng, "macroatom", True, variant, track_full=True)
    ft = r["res"].full_trackers
    assert len(r["log"]["nu"]) == moved_rows(ft, model("macroatom", True).prob.packet_collection.initial_radii)
    j = bref.shell_fsum(r["log"]["ed"], r["log"]["shell"], S)
    assert np.all(np.abs(j / r["res"].j_estimator - 1.0) < 0.1) and not np.allclose(j, r["res"].j_estimator, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("full", [False, True])
def test_a_move_of_length_zero_writes_no_record(eng, full, variant):
    """This project's decision, on 200 lines of ONE frequency (tests/coincident_lines.py): a packet emitted by a line stands on the next
    line, so the next trace has length zero -- a row of the event log, no segment record."""
    import coincident_lines as cl
    prob = cl.degenerate_problem(1, full, 0)
    S8 = len(prob.geometry.r_inner)
    m = SimpleNamespace(prob=prob, ld=synthetic.make_line_data(SEED, prob.opacity_state, n_levels=K, time_explosion=prob.time_explosion))
    m.pd = synthetic.make_plasma_data(SEED, m.ld, S8)
    lo, hi = synthetic.comoving_frequency_range(prob)
    m.cd = synthetic.make_covering_continuum_data(m.pd, [(np.array([lo, hi]), X * np.array([lo, hi]))])
    stage(eng, m)
    eng.set_bf_estimators(np.linspace(11000.0, 7000.0, S8))
    r = propagate(eng, m, variant=variant, track_full=1, event_log_capacity=256 * prob.packet_collection.number_of_packets)
    assert r["variant"] == variant
    ft = r["res"].full_trackers
    moved, n = moved_rows(ft, prob.packet_collection.initial_radii), len(r["log"]["nu"])
    assert moved < ft.n_rows - 100   # (a condition on the input: the problem has moves of length zero)
    assert n == moved and r["tables"]["n_records"] == n and r["tables"]["statistics"].sum() == n
    assert np.all(r["log"]["ed"] > 0)


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("mode,full", [("downbranch", False), ("macroatom", False), ("macroatom", True)])
def test_the_pass_against_the_reference(eng, mode, full, variant):
    r = run(eng, mode, full, variant)
    m = model(mode, full)
    want = reference(m, r["log"])
    # conditions on the inputs, not on the code
    assert np.all(want["statistics"][A] > 0) and np.all(want["statistics"][B] > 0) and not want["statistics"][C_].any()
    assert np.all(want["statistics"][D] > 0) and np.all(want["statistics"][D] < want["statistics"][A])
    assert r["tables"]["n_dropped"] == 0
    assert_tables(r["tables"], want)
    assert np.array_equal(want["statistics"][A], np.bincount(r["log"]["shell"], minlength=S))  # (A is current for every record)


@pytest.mark.parametrize("variant", [0, 2])
def test_consequence_of_a_linear_cross_section(eng, variant):
    """x = X nu: photo_ion[A,s] = X J[s] and bf_heating[A,s] = X (nu_bar[s] - nu_i J[s]); the bounds are derived in the module docstring."""
    r = run(eng, "macroatom", False, variant)
    m = model("macroatom", False)
    t, res = r["tables"], r["res"]
    n = t["statistics"][A].astype(np.float64)
    j, nu_bar = res.j_estimator, res.nu_bar_estimator
    assert np.all(np.abs(t["photo_ion"][A] - X * j) <= (8 + 2 * n) * U * (X * j))
    assert np.all(np.abs(t["bf_heating"][A] - X * (nu_bar - m.lo * j)) <= (10 + 3 * n) * U * X * (nu_bar + m.lo * j))


@pytest.mark.parametrize("variant", [0, 2])
def test_nothing_else_moves(eng, variant):
    """Option on against option off on the same forced variant: per-packet results bit for bit, the estimators to the parity tests' 1e-11."""
    on, off = run(eng, "macroatom", False, variant)["res"], run(eng, "macroatom", False, variant, bf=False)["res"]
    assert np.array_equal(on.output_nus, off.output_nus) and np.array_equal(on.output_energies, off.output_energies)
    for f in on.trackers.F64_FIELDS + on.trackers.I64_FIELDS:
        assert np.array_equal(getattr(on.trackers, f), getattr(off.trackers, f), equal_nan=True), f
    for f in ("j_estimator", "nu_bar_estimator", "j_blue_estimator", "edotlu_estimator"):
        np.testing.assert_allclose(getattr(on, f), getattr(off, f), rtol=1e-11, atol=0.0, err_msg=f)


@pytest.mark.parametrize("variant", [0, 2])
def test_the_event_log_does_not_change(eng, variant):
    """track_full with the estimators on: the event log of track_full alone, column by column."""
    both = run(eng, "macroatom", True, variant, track_full=True)["res"].full_trackers
    alone = run(eng, "macroatom", True, variant, bf=False, track_full=True)["res"].full_trackers
    assert both.n_rows == alone.n_rows and np.array_equal(both.offsets, alone.offsets)
    for f in both.F64_FIELDS + both.I64_FIELDS:
        assert np.array_equal(getattr(both, f), getattr(alone, f), equal_nan=True), f


def test_estimators_without_full_tracking_write_no_event_log(eng):
    run(eng, "macroatom", False, 2)
    m = model("macroatom", False)
    stage(eng, m)
    eng.set_bf_estimators(T_E)
    propagate(eng, m, variant=2)
    with pytest.raises(RuntimeError) as e:
        eng.get_event_log()
    assert e.value.code == _abi.ERR_STATE


def test_dropped_records(eng):
    """A pool too small for the call: the getter refuses with the exact counts, the per-packet results do not change."""
    full = run(eng, "macroatom", False, 0)
    m = model("macroatom", False)
    stage(eng, m)
    eng.set_bf_estimators(T_E)
    r = propagate(eng, m, variant=0, segment_log_capacity=64)
    e = r["error"]
    assert e.code == _abi.ERR_STATE and e.n_dropped > 0 and "dropped" in str(e)
    assert e.n_records + e.n_dropped == len(full["log"]["nu"]) and e.n_records == len(r["log"]["nu"])
    assert np.array_equal(r["res"].output_nus, full["res"].output_nus) and np.array_equal(r["res"].output_energies, full["res"].output_energies)
    eng.reset_estimators()
    assert eng.get_bf_estimators()["n_dropped"] == 0


# ---- the pass alone, on hand-placed records
def edge_records(m):
    """Records at nu_min and nu_max of B and D, one ulp outside each, at grid points and between them; shell 2 gets none."""
    nu = []
    for b, _ in (m.blocks[B], m.blocks[D]):
        nu += [b[0], b[-1], np.nextafter(b[0], 0.0), np.nextafter(b[0], np.inf), np.nextafter(b[-1], 0.0), np.nextafter(b[-1], np.inf), b[1],
               0.5 * (b[0] + b[1]), 0.5 * (b[-2] + b[-1])]
    nu = np.array(nu + [m.lo, m.hi])
    shell = np.array([0, 1, 3] * len(nu))[:len(nu)]
    ed = np.linspace(1.0, 2.0, len(nu)) * 1e-3
    return nu, ed, shell


def fresh(eng, m=None, **kw):
    m = m or model()
    stage(eng, m, **kw)
    eng.set_bf_estimators(T_E)
    return m


def test_edges_of_the_blocks(eng):
    m = fresh(eng)
    nu, ed, shell = edge_records(m)
    eng.debug_bf_accumulate(nu, ed, shell)
    got, want = eng.get_bf_estimators(), bref.tables(m.cd, T_E, S, nu, ed, shell)
    per = bref.terms(m.cd, T_E, nu, ed, shell)
    for c, first in ((B, 0), (D, 9)):  # the ends and one ulp inside are current, one ulp outside is not (conditions on the reference)
        current = set(per[c][0].tolist())
        assert {first, first + 1, first + 3, first + 4} <= current and not ({first + 2, first + 5} & current)
    assert not want["statistics"][:, 2].any() and want["statistics"][A].sum() == len(nu) - 1  # (one ulp below D's first frequency lies below A)
    assert_tables(got, want)
    assert got["n_records"] == len(nu) and got["n_dropped"] == 0


def test_zero_records_and_reset(eng):
    m = fresh(eng)
    eng.debug_bf_accumulate(np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64))
    t = eng.get_bf_estimators()
    assert all(not t[k].any() for k in TABLES) and t["n_records"] == 0
    nu, ed, shell = edge_records(m)
    eng.debug_bf_accumulate(nu, ed, shell)
    assert eng.get_bf_estimators()["statistics"].any()
    eng.reset_estimators()
    t = eng.get_bf_estimators()
    assert all(not t[k].any() for k in TABLES) and t["n_records"] == 0


def test_two_calls_accumulate(eng):
    m = fresh(eng)
    nu, ed, shell = edge_records(m)
    eng.debug_bf_accumulate(nu, ed, shell)
    eng.debug_bf_accumulate(nu[::-1].copy(), 2.0 * ed[::-1], shell[::-1].copy())
    got = eng.get_bf_estimators()
    want = bref.tables(m.cd, T_E, S, np.concatenate((nu, nu[::-1])), np.concatenate((ed, 2.0 * ed[::-1])), np.concatenate((shell, shell[::-1])))
    assert_tables(got, want)
    assert got["n_records"] == 2 * len(nu)


def test_the_slice_boundary(eng):
    """65537 records of one shell: two slices, the second of one record; a few in another shell."""
    m = fresh(eng)
    rng = np.random.default_rng(SEED)
    n = 65537
    nu = np.concatenate((np.exp(rng.uniform(np.log(m.lo), np.log(m.hi), n)), [m.blocks[B][0][3], m.blocks[B][0][4]]))
    ed = rng.uniform(0.5, 1.5, n + 2)
    shell = np.concatenate((np.full(n, 1), [3, 3]))
    eng.debug_bf_accumulate(nu, ed, shell)
    got, want = eng.get_bf_estimators(), bref.tables(m.cd, T_E, S, nu, ed, shell)
    assert want["statistics"][A, 1] == n and want["statistics"][B, 3] == 2
    assert_tables(got, want)
    ms = eng.last_bf_estimator_ms()
    assert ms["group_ms"] > 0 and ms["accumulate_ms"] > 0


@pytest.mark.parametrize("n_continua", [3, 300])
def test_other_continuum_counts(eng, n_continua):
    """3 continua: 85 threads share each and one thread of the workgroup has none; 300: two passes over the records, the second with 44."""
    m = model()
    big = Model("macroatom", False, n_levels=420) if n_continua > 4 else m
    rng = np.random.default_rng(SEED + n_continua)
    blocks = []
    for c in range(n_continua):
        a, b = np.sort(np.exp(rng.uniform(np.log(m.lo), np.log(m.hi), 2)))
        grid = np.geomspace(a, max(b, a * 1.01), int(rng.integers(2, 20)))
        blocks.append((grid, 1e-18 * rng.uniform(0.1, 1.0, len(grid))))
    cd = synthetic.make_covering_continuum_data(big.pd, blocks)
    stage(eng, big, cd=cd)
    eng.set_bf_estimators(T_E)
    n = 1000
    nu = np.exp(rng.uniform(np.log(m.lo), np.log(m.hi), n))
    nu[:n_continua] = [b[0][0] for b in blocks][:n]   # every threshold once
    ed, shell = rng.uniform(0.5, 1.5, n), rng.integers(0, S, n)
    eng.debug_bf_accumulate(nu, ed, shell)
    want = bref.tables(cd, T_E, S, nu, ed, shell)
    assert np.all(want["statistics"].sum(axis=1) > 0)
    assert_tables(eng.get_bf_estimators(), want)


def test_records_are_checked_on_the_host(eng):
    fresh(eng)
    for nu, ed, shell, text in (([0.0], [1.0], [0], "nu[0]"), ([1e15, np.nan], [1.0, 1.0], [0, 0], "nu[1]"), ([1e15], [np.inf], [0], "ed[0]"),
                                ([1e15], [1.0], [S], "shell[0]"), ([1e15], [1.0], [-1], "shell[0]")):
        with pytest.raises(RuntimeError) as e:
            eng.debug_bf_accumulate(np.array(nu), np.array(ed), np.array(shell))
        assert e.value.code == _abi.ERR_INVALID_ARGUMENT and text in str(e.value)


# ---- rates, option continuum_field
T_RAD, W = np.linspace(12000.0, 8000.0, S), 0.4 / (1.0 + 0.2 * np.arange(S))
RATE_TABLES = ("phi_ik", "alpha_sp", "coll_ion", "coll_recomb")


def test_rates_and_the_continuum_field(eng):
    m = fresh(eng)
    run_tables = run(eng, "macroatom", False, 0)["log"]
    stage(eng, m)
    eng.set_bf_estimators(T_E)
    eng.debug_bf_accumulate(run_tables["nu"], run_tables["ed"], run_tables["shell"])
    tab = eng.get_bf_estimators()
    tos, volume = 3.7e5, np.linspace(2.0e44, 9.0e44, S)
    got = eng.bf_estimator_rates(tos, volume)
    want = bref.rates(tab, tos, volume)
    assert np.array_equal(got["gamma_est"], want["gamma_est"]) and np.array_equal(got["stim_est"], want["stim_est"])
    assert got["gamma_est"][A].all() and not got["gamma_est"][C_].any()
    eng.reset_estimators()   # the rates survive it
    eng.update_plasma(T_RAD, W)
    black = {**eng.get_continuum_rates(), **eng.get_continuum_opacity(), **eng.get_cooling_rates(), **eng.get_kpacket_tables()}
    eng.set_option("continuum_field", 1)
    try:
        eng.update_plasma(T_RAD, W)
    finally:
        eng.set_option("continuum_field", 0)
    est = {**eng.get_continuum_rates(), **eng.get_continuum_opacity(), **eng.get_cooling_rates(), **eng.get_kpacket_tables()}
    plasma = eng.get_plasma()
    assert np.array_equal(est["gamma"], got["gamma_est"])
    assert np.array_equal(est["alpha_stim"], got["stim_est"] * est["phi_ik"])
    assert not np.array_equal(est["gamma"], black["gamma"])
    level = np.asarray(m.cd.level)
    ion = np.repeat(np.arange(len(m.pd.ion_level_edge) - 1), np.diff(m.pd.ion_level_edge))[level]
    n_i, n_up, n_e = plasma["level_number_density"][level], plasma["ion_number_density"][ion + 1], plasma["electron_density"]
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = np.where(n_i == 0.0, est["gamma"], est["gamma"] - ((est["alpha_stim"] * n_up) * n_e[None, :]) / n_i)
    assert np.array_equal(est["gamma_corr"], np.where(corr < 0.0, 0.0, corr))
    for name in RATE_TABLES + ("chi_bf", "ff_opacity_factor", "t_electrons", "c_fb_sp", "cool_rate_fb", "cool_rate_coll_ion", "cool_rate_ff",
                               "cool_rate_adiabatic", "cool_rate_total", "fb_emission_cdf", "k_cdf"):
        assert np.array_equal(est[name], black[name]), name
    # the option back at 0: the dilute black body's bits again
    eng.update_plasma(T_RAD, W)
    again = eng.get_continuum_rates()
    for name in Engine.CONTINUUM_RATES:
        assert np.array_equal(again[name], black[name]), name


def test_continuum_field_needs_rates(eng):
    fresh(eng)
    eng.set_option("continuum_field", 1)
    try:
        with pytest.raises(RuntimeError) as e:
            eng.update_plasma(T_RAD, W)
        assert e.value.code == _abi.ERR_STATE and "continuum_field" in str(e.value)
    finally:
        eng.set_option("continuum_field", 0)
    with pytest.raises(RuntimeError) as e:
        eng.set_option("continuum_field", 2)
    assert e.value.code == _abi.ERR_INVALID_ARGUMENT


# ---- state rules
def test_state_rules(eng):
    m = model()
    stage(eng, m)
    with pytest.raises(RuntimeError) as e:   # the option on, no setup
        propagate(eng, m, variant=0)
    assert e.value.code == _abi.ERR_STATE and "set_bf_estimators" in str(e.value)
    eng.set_continuum_data(None)
    with pytest.raises(RuntimeError) as e:   # a setup without continuum data
        eng.set_bf_estimators(T_E)
    assert e.value.code == _abi.ERR_STATE
    eng.set_continuum_data(m.cd)
    with pytest.raises(RuntimeError) as e:
        eng.set_bf_estimators(np.array([1.0, 2.0, -3.0, 4.0]))
    assert e.value.code == _abi.ERR_INVALID_ARGUMENT and "t_electrons[2]" in str(e.value)
    eng.set_bf_estimators(T_E)
    assert eng.get_bf_estimators()["n_records"] == 0
    with pytest.raises(RuntimeError):        # a refused call leaves the setup that was there
        eng.set_bf_estimators(np.array([1.0, np.nan, 3.0, 4.0]))
    assert eng.get_bf_estimators()["n_records"] == 0
    with pytest.raises(RuntimeError) as e:   # no kept log
        eng.get_segment_log()
    assert e.value.code == _abi.ERR_STATE
    eng.set_opacity(m.prob.opacity_state)    # drops the continuum data and the setup with them
    with pytest.raises(RuntimeError) as e:
        eng.get_bf_estimators()
    assert e.value.code == _abi.ERR_STATE
    stage(eng, m)
    eng.set_bf_estimators(T_E)
    eng.set_bf_estimators(None)              # off
    with pytest.raises(RuntimeError) as e:
        eng.get_bf_estimators()
    assert e.value.code == _abi.ERR_STATE
    with pytest.raises(RuntimeError) as e:   # over the bound on the log's memory
        eng.set_bf_estimators(T_E)
        propagate(eng, m, variant=0, segment_log_capacity=10 ** 11)
    assert e.value.code == _abi.ERR_INVALID_ARGUMENT and "segment_log_max_bytes" in str(e.value)


def test_the_resident_solver(eng):
    """MCTransportSolverHIP: enable_bf_estimators() with the continuum stage's own t_electrons, a run, bf_estimators(), and an
    update_plasma on the estimators' field."""
    from tardis_amd import transport
    m = model()
    solver = transport.MCTransportSolverHIP(m.prob.spectrum_frequency_grid, copy.copy(m.prob.montecarlo_configuration), line_interaction_type="macroatom",
                                            resident=True, engine=eng)
    solver.set_line_data(m.ld)
    solver.set_plasma_data(m.pd)
    solver.set_continuum_data(m.cd)
    ts = solver.initialize_transport_state(m.prob.packet_collection, m.prob.geometry, m.prob.opacity_state, m.prob.time_explosion)
    solver.run(ts)
    with pytest.raises(RuntimeError):
        solver.enable_bf_estimators()   # no update_plasma yet, no temperatures given
    op = solver.update_plasma(T_RAD, W)
    solver.enable_bf_estimators()
    assert np.array_equal(solver.bf_t_electrons, m.pd.link_t_rad_t_electron * T_RAD)
    ts = solver.initialize_transport_state(m.prob.packet_collection, m.prob.geometry, op, m.prob.time_explosion)
    solver.run(ts)
    t = solver.bf_estimators()
    assert t["n_records"] >= P and t["n_dropped"] == 0 and np.all(t["statistics"][A] > 0)
    volume = np.linspace(2.0e44, 9.0e44, S)
    solver.update_plasma(T_RAD, W, continuum_field="estimators", volume=volume, time_of_simulation=3.7e5)
    rates = solver.continuum_rates()
    assert np.array_equal(rates["gamma"], bref.rates(t, 3.7e5, volume)["gamma_est"])
    solver.update_plasma(T_RAD, W)
    assert not np.array_equal(solver.continuum_rates()["gamma"], rates["gamma"])
    solver.enable_bf_estimators(False)
