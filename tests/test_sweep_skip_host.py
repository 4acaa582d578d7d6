"""CPU check of the lane sweep's block skip (tardis_amd/csrc/sweep_skip.hpp, used by the sixteen-wave lane-sweep kernel of
tardis_amd/csrc/propagate_wave.hpp) and of the plan that turns it on (plan::plan_sweep_skip, tardis_amd/csrc/propagate_plan.hpp).

A shim compiled with the host compiler builds, for synthetic tables of 4 shells, the interleaved rows, the double-double prefix sums (two-sum, as
tau_prefix_kernel) and the coarse table, and runs every trace twice: through ssk::trace -- the kernel's sweep with the header's own coarse_scan and
interval_take, one lane at a time -- and through `reference`, a straight restatement of trace_packet's loop over the lines (serial optical-depth sum,
three-way minimum, for-else).  Outcome, stopping line and distance must agree bit for bit on every trace; a trace may fall back to the line-by-line
sweep only where the reference ends in electron scattering (or raises), or where tau_event lies within the stated margin g = 8 M of the reference's own
decisive sum at the line the fall-back happened at.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tardis_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tardis_amd", "csrc")
C_LIGHT = 2.99792458e10

SHIM = r"""
#include "sweep_skip.hpp"
#include "propagate_plan.hpp"
#include <vector>
#include <cmath>
namespace {
struct Tables { int S, L, stride; std::vector<double> nt, ct, pfx, pn, nu; double m; };
Tables T;
void two_sum(double &hi, double &lo, double x) { const double s = hi + x, bb = s - hi; lo += (hi - (s - bb)) + (x - bb); hi = s; }
}
extern "C" double build_tables(const double *nu, const double *tau_t, int S, int L, double margin_scale)
{
    T.S = S; T.L = L; T.stride = (L + 7) & ~7;
    const int rows = T.stride / 8;
    T.nu.assign(nu, nu + L);
    T.nt.assign((size_t)2 * (T.stride * S + 32), 0.0);
    T.pfx.assign((size_t)S * (L + 1), 0.0);
    T.ct.assign((size_t)2 * (rows * S + 16), 0.0);
    double rmax = 0.0;
    for (int s = 0; s < S; ++s) {
        double hi = 0.0, lo = 0.0;
        for (int l = 0; l < L; ++l) { T.pfx[(size_t)s * (L + 1) + l] = hi + lo; two_sum(hi, lo, tau_t[(size_t)s * L + l]); }
        T.pfx[(size_t)s * (L + 1) + L] = hi + lo;
        if (hi + lo > rmax) rmax = hi + lo;
    }
    for (long long i = 0; i < (long long)T.stride * S + 32; ++i) {
        const long long s = i / T.stride, l = i - s * T.stride;
        const bool in = s < S && l < L;
        T.nt[2 * i] = (in && l < L - 1) ? nu[l] : -INFINITY;
        T.nt[2 * i + 1] = in ? tau_t[s * L + l] : 0.0;
    }
    for (long long i = 0; i < (long long)rows * S + 16; ++i) {
        const long long s = i / rows, b = i - s * rows;
        if (s < S) { T.ct[2 * i] = T.nt[2 * (s * T.stride + 8 * b + 7)]; T.ct[2 * i + 1] = T.pfx[s * (L + 1) + std::min<long long>(8 * b + 8, L)]; }
        else { T.ct[2 * i] = -INFINITY; T.ct[2 * i + 1] = T.pfx[(size_t)(S - 1) * (L + 1) + L]; }
    }
    T.pn.assign((size_t)2 * S * (L + 1), 0.0);
    for (long long s = 0; s < S; ++s)
        for (long long l = 0; l <= L; ++l) { T.pn[2 * (s * (L + 1) + l)] = l < L - 1 ? nu[l] : -INFINITY; T.pn[2 * (s * (L + 1) + l) + 1] = T.pfx[s * (L + 1) + l]; }
    T.m = margin_scale * ssk::margin(L, rmax);
    return T.m;
}
// trace_packet's loop (modes/homologous_rad_packet_transport.py:100-172), line scattering enabled.  decisive: tau_combined of the stopping line (code 3), else
// the serial sum in front of the stopping line
extern "C" int reference(int shell, int start, double nu, double comov, double chi, double tau_event, double d_boundary, double t_exp, int *line_out,
                         double *dist_out, double *decisive)
{
    const int L = T.L;
    const double *tau = &T.nt[(size_t)2 * shell * T.stride];
    double tau_trace = 0.0;
    for (int line = start; line < L; ++line) {
        double dist;
        const double tau_line = tau[2 * line + 1];
        const int code = ssk::exact_line(L, t_exp, line, T.nu[line], tau_line, tau_trace, nu, comov, chi, tau_event, d_boundary, dist);
        if (code) {
            *line_out = line; *dist_out = dist;
            *decisive = code == 3 ? (tau_trace + tau_line) + chi * dist : tau_trace;
            return code;
        }
        tau_trace = tau_trace + tau_line;
    }
    const double d_cont = (tau_event - tau_trace) / chi;
    const bool cont = d_cont < d_boundary;
    *line_out = 0; *dist_out = cont ? d_cont : d_boundary; *decisive = tau_trace;
    return (cont ? 2 : 1) | 8;
}
// the reference's serial sum from `start` to the end of block (start / 8 + j), plus RN(K' X) of that block's last line: what a coarse test compares with tau_event
extern "C" double block_threshold(int shell, int start, int j, double comov, double kp)
{
    const double *row = &T.nt[(size_t)2 * shell * T.stride];
    const int e = std::min(8 * (start / 8 + j) + 8, T.L);
    double s = 0.0;
    for (int l = start; l < e; ++l) s = s + row[2 * l + 1];
    const double X = comov - row[2 * (e - 1)];
    return std::isfinite(X) ? s + kp * X : s;
}
extern "C" int skip_trace(int shell, int start, double nu, double comov, double chi, double tau_event, double d_boundary, double t_exp, int skip, int force,
                          int *line_out, double *dist_out, int *info, double *fb_gap)
{
    ssk::TraceIn in{};
    in.nt = &T.nt[(size_t)2 * shell * T.stride]; in.ct = &T.ct[(size_t)2 * shell * (T.stride / 8)]; in.pn = &T.pn[(size_t)2 * shell * (T.L + 1)];
    in.n_lines = T.L; in.start = start; in.nu = nu; in.comov = comov; in.chi = chi; in.tau_event = tau_event; in.d_boundary = d_boundary; in.t_exp = t_exp;
    const double tc = t_exp * ssk::C_LIGHT_, rcp_tc = 1.0 / tc;
    in.kp = ((chi * tc) / nu) * (1.0 + 0x1p-40);
    in.xb = ((d_boundary * nu) * rcp_tc) * (1.0 - 0x1p-40);
    in.m = T.m; in.force_fallback = force; in.skip = skip; in.fine_chunk = 10;
    const ssk::TraceOut o = ssk::trace(in, T.nu.data());
    *line_out = o.line; *dist_out = o.dist;
    info[0] = o.fell_back; info[1] = o.coarse_steps; info[2] = o.fine_steps; info[3] = o.interval; info[4] = o.fb_code; info[5] = o.fb_line;
    fb_gap[0] = o.fb_gap; fb_gap[1] = o.fb_u;
    return o.code;
}
// the reference's own quantities at line `line` of a trace from `start` (line = L: behind the list): out[0] the serial sum in front of the line, out[1] its optical
// depth, out[2] the distance to the line as trace_packet computes it (MISS_DISTANCE for the last line and behind the list)
extern "C" void reference_at(int shell, int start, int line, double nu, double comov, double t_exp, double *out)
{
    const double *row = &T.nt[(size_t)2 * shell * T.stride];
    double s = 0.0;
    for (int l = start; l < line && l < T.L; ++l) s = s + row[2 * l + 1];
    out[0] = s; out[1] = line < T.L ? row[2 * line + 1] : 0.0;
    if (line >= T.L - 1) out[2] = ssk::MISS_;
    else {
        const double q = (comov - T.nu[line]) / nu;
        out[2] = (q < 0 ? -q : q) < ssk::CLOSE_ ? 0.0 : q * ssk::C_LIGHT_ * t_exp;
    }
}
extern "C" double kprime(double chi, double nu, double t_exp) { return ((chi * (t_exp * ssk::C_LIGHT_)) / nu) * (1.0 + 0x1p-40); }
extern "C" int plan_skip(int sweep_skip, int lane_sweep, int vpk, int full_relativity, int wide, int cross_check, int shell_log, int full_tracking,
                         int waves_per_simd, int nt, int line_scattering, int nt_negative, int pfx_negative)
{
    plan::SkipInput in{};
    in.sweep_skip = sweep_skip; in.lane_sweep = lane_sweep; in.vpk = vpk; in.full_relativity = full_relativity; in.wide = wide; in.cross_check = cross_check;
    in.shell_log = shell_log; in.full_tracking = full_tracking; in.waves_per_simd = waves_per_simd; in.nt = nt; in.line_scattering = line_scattering;
    in.nt_negative = nt_negative; in.pfx_negative = pfx_negative;
    return plan::plan_sweep_skip(in) ? 1 : 0;
}
"""

_d, _i, _pi, _pd = C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)


def load_shim(d, source=SHIM):
    """The shim compiled in directory `d` and bound (`source`: SHIM, or SHIM with more entry points behind it -- tests/test_prefix_tables_host.py)."""
    src, lib = d / "shim.cpp", d / "libssk.so"
    src.write_text(source)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.build_tables.restype, L.build_tables.argtypes = _d, [C.c_void_p, C.c_void_p, _i, _i, _d]
    L.reference.restype, L.reference.argtypes = _i, [_i, _i, _d, _d, _d, _d, _d, _d, _pi, _pd, _pd]
    L.block_threshold.restype, L.block_threshold.argtypes = _d, [_i, _i, _i, _d, _d]
    L.skip_trace.restype, L.skip_trace.argtypes = _i, [_i, _i, _d, _d, _d, _d, _d, _d, _i, _i, _pi, _pd, _pi, _pd]
    L.reference_at.restype, L.reference_at.argtypes = None, [_i, _i, _i, _d, _d, _d, _pd]
    L.kprime.restype, L.kprime.argtypes = _d, [_d, _d, _d]
    L.plan_skip.restype, L.plan_skip.argtypes = _i, [_i] * 13
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_shim(tmp_path_factory.mktemp("sweep_skip"))


N_SHELLS = 4


def tables(n_lines, seed=7):
    geo = synthetic.make_geometry(N_SHELLS)
    op = synthetic.make_opacity_state(seed, geo, n_lines, "scatter")
    nu = np.ascontiguousarray(op.line_list_nu, dtype=np.float64)
    tau_t = np.ascontiguousarray(np.asarray(op.tau_sobolev, dtype=np.float64).T)  # [shell][line]
    return geo, nu, tau_t


def make_traces(rng, geo, nu_line, n):
    """Trace inputs as the prologue of a trace produces them: a packet in shell s whose comoving frequency lies just blueward of line `start`."""
    L = len(nu_line)
    t_exp = float(geo.time_explosion)
    shell = rng.integers(0, N_SHELLS, n)
    start = rng.integers(1, L, n)
    start[: n // 50] = L - rng.integers(0, 40, n // 50)           # traces that run into the end of the list, or start behind it (start = L: the for-else)
    start[n // 50: n // 25] = rng.integers(1, 12, n // 25 - n // 50)
    nu_ext = np.append(nu_line, nu_line[-1] * (1.0 - 1e-3))
    comov = nu_ext[start] + rng.random(n) * (nu_ext[start - 1] - nu_ext[start])
    comov = np.maximum(comov, np.nextafter(nu_ext[start], np.inf))
    beta = rng.uniform(0.035, 0.067, n) * rng.uniform(-1.0, 1.0, n)
    nu = comov / (1.0 - beta)
    chi = 1e9 * 6.6524587158e-25 * 10.0 ** rng.uniform(-1.0, 2.5, n)
    tau_event = -np.log(1.0 - rng.random(n))
    d_boundary = 10.0 ** rng.uniform(12.0, 15.3, n)
    return shell, start, nu, comov, chi, tau_event, d_boundary, t_exp


def run_pair(shim, tr, k, tau_event=None, force=0, skip=1):
    shell, start, nu, comov, chi, te, db, t_exp = tr
    te_k = float(te[k] if tau_event is None else tau_event)
    args = (int(shell[k]), int(start[k]), float(nu[k]), float(comov[k]), float(chi[k]), te_k, float(db[k]), t_exp)
    rl, rd, dec = _i(), _d(), _d()
    rc = shim.reference(*args, C.byref(rl), C.byref(rd), C.byref(dec))
    sl, sd = _i(), _d()
    gap = (_d * 2)()
    info = (_i * 6)()
    sc = shim.skip_trace(*args, skip, force, C.byref(sl), C.byref(sd), info, gap)
    return (rc, rl.value, rd.value, dec.value), (sc, sl.value, sd.value), tuple(info), tuple(gap)


def check(shim, tr, k, g, stats, tau_event=None):
    ref, got, info, (_, fb_u) = run_pair(shim, tr, k, tau_event)
    assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[2], (k, tau_event, ref, got, info)
    if info[0]:  # fell back
        escat_or_error = (ref[0] & 7) in (2, 4)
        if not escat_or_error:
            # The reference ends on a line or a boundary, so the fall-back has to be one of ambiguity: at the line it happened at, tau_event lies within g
            # of the REFERENCE's own sum there -- including the line and chi d_trace where the lane saw a line stop (code 3), in front of the line plus chi
            # times the nearer of line and boundary where it saw the continuum first (codes 2 and 10).  Not a quantity of the lane's: its upper bound only
            # has to lie within [T, T + g] of the reference's sum T.
            shell, start, nu, comov, chi, te, db, t_exp = tr
            te_k = float(te[k] if tau_event is None else tau_event)
            q = (_d * 3)()
            shim.reference_at(int(shell[k]), int(start[k]), info[5], float(nu[k]), float(comov[k]), t_exp, q)
            t_prev, tau_line, d_trace = q[0], q[1], q[2]
            slack = 8e-16 * max(1.0, t_prev + tau_line, te_k)  # (the roundings of the few operations below)
            assert -slack <= fb_u - t_prev <= g + slack, (k, fb_u, t_prev, g)
            if info[4] == 3:
                pivot = (t_prev + tau_line) + float(chi[k]) * d_trace
            else:
                assert info[4] in (2, 10), info
                pivot = t_prev + float(chi[k]) * min(d_trace, float(db[k]))
            assert abs(te_k - pivot) <= g + slack, (k, tau_event, ref, got, info, te_k - pivot, g)
        stats["fallback_margin" if not escat_or_error else "fallback_escat"] += 1
    stats["code%d" % ref[0]] += 1
    stats["interval"] += info[3]
    stats["coarse2"] += info[1] >= 2
    stats["first_block"] += (ref[0] & 8) == 0 and ref[1] // 8 == int(tr[1][k]) // 8
    return ref, info


@pytest.mark.parametrize("n_lines", [20000, 20003])
def test_block_skip_equals_the_reference_loop(shim, n_lines):
    from collections import Counter
    geo, nu_line, tau_t = tables(n_lines)
    m = shim.build_tables(nu_line.ctypes.data, tau_t.ctypes.data, N_SHELLS, n_lines, 1.0)
    g = 8.0 * m
    rng = np.random.default_rng(n_lines)
    n = 100000
    tr = make_traces(rng, geo, nu_line, n)
    stats = Counter()
    offsets = set()
    planted = 0
    for k in range(n):
        ref, info = check(shim, tr, k, g, stats)
        offsets.add(int(tr[1][k]) % 8)
        if k % 16 == 0:
            # tau_event within a few ulps on either side of the decisive sum of the reference's outcome ...
            for ulps in (-3, -1, 0, 1, 3):
                te = float(ref[3]) * (1.0 + ulps * 2.0 ** -52)
                if te > 1e-6:
                    check(shim, tr, k, g, stats, te)
                    planted += 1
            # ... and of what the coarse tests compare it with, at the ends of the first, second and tenth block
            kp = shim.kprime(float(tr[4][k]), float(tr[2][k]), tr[7])
            for j in (0, 1, 9):
                thr = shim.block_threshold(int(tr[0][k]), int(tr[1][k]), j, float(tr[3][k]), kp)
                for ulps in (-2, 0, 2):
                    te = thr * (1.0 + ulps * 2.0 ** -52)
                    if te > 1e-6:
                        check(shim, tr, k, g, stats, te)
                        planted += 1
    print(n_lines, "margin", m, "planted", planted, dict(stats))
    assert offsets == set(range(8))
    for code in (1, 2, 3, 9, 10):  # boundary, electron scattering, line, and the list exhausted either way
        assert stats["code%d" % code] > 0, code
    assert stats["interval"] > n // 4 and stats["coarse2"] > 100 and stats["first_block"] > 1000
    assert stats["fallback_margin"] > 0  # (the planted thresholds do land inside the margin)


def test_last_block_and_forced_fallback(shim):
    from collections import Counter
    n_lines = 20003
    geo, nu_line, tau_t = tables(n_lines)
    m = shim.build_tables(nu_line.ctypes.data, tau_t.ctypes.data, N_SHELLS, n_lines, 1.0)
    rng = np.random.default_rng(5)
    tr = make_traces(rng, geo, nu_line, 4000)
    tr[1][:2000] = n_lines - rng.integers(0, 120, 2000)  # starts in the last fifteen blocks of the row, or behind the last line
    tr[1][:200] = n_lines                                # (the for-else: nothing left to pass)
    tr[3][:2000] = np.nextafter(np.append(nu_line, nu_line[-1] * (1.0 - 1e-3))[tr[1][:2000]], np.inf)
    tr[2][:2000] = tr[3][:2000] / 0.97
    stats = Counter()
    for k in range(4000):
        check(shim, tr, k, 8.0 * m, stats)
        ref, got, info, _ = run_pair(shim, tr, k, force=1)
        assert got == ref[:3], (k, ref, got)
        assert info[0] == 1 or info[3] == 0 or (ref[0] & 8)  # forced: every trace that reached interval mode and stopped on a line fell back
        ref, got, info, _ = run_pair(shim, tr, k, skip=0)
        assert got == ref[:3] and info[1] == 0, (k, ref, got)
    assert stats["code9"] + stats["code10"] > 100


ALLOWED = dict(sweep_skip=-1, lane_sweep=1, vpk=0, full_relativity=0, wide=0, cross_check=0, shell_log=0, full_tracking=0, waves_per_simd=4, nt=1,
               line_scattering=1, nt_negative=0, pfx_negative=0)


@pytest.mark.parametrize("change,expect", [
    (dict(), 1),                      # the configs[2] shape: sixteen-wave lane sweeps on the interleaved table, no v-packets
    (dict(sweep_skip=1), 1),
    (dict(sweep_skip=0), 0),
    (dict(nt_negative=1), 0), (dict(pfx_negative=1), 0),
    (dict(vpk=1), 0), (dict(full_relativity=1), 0), (dict(wide=1), 0),
    (dict(shell_log=1), 0), (dict(cross_check=1), 0), (dict(full_tracking=1), 0),
    (dict(waves_per_simd=3), 0), (dict(nt=0), 0), (dict(nt=2), 0), (dict(lane_sweep=0), 0), (dict(line_scattering=0), 0),
    (dict(sweep_skip=1, nt_negative=1), 0), (dict(sweep_skip=1, vpk=1), 0),
])
def test_plan(shim, change, expect):
    a = dict(ALLOWED, **change)
    assert shim.plan_skip(*[a[k] for k in ALLOWED]) == expect
