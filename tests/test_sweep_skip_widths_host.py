"""CPU check of the block skip's step width (tardis_amd/csrc/sweep_skip.hpp: ssk::coarse_scan<N>, TraceIn::loads): the widths the kernel is compiled
at -- eight loads per step in the sixteen-wave instantiation, ten in the twelve-wave one -- and twelve, the widest the header's host restatement takes.

The tables, the traces, the planted thresholds, the reference loop and the rule for fall-backs are those of tests/test_sweep_skip_host.py, whose shim is
compiled here with ONE change: ssk::trace gets its width (coarse loads = lines of a fine step, as in the kernel) from a setter instead of the default.
At every width, on the same inputs:
  * outcome, stopping line and distance equal the reference loop's bit for bit;
  * a trace falls back to the line-by-line sweep only where the reference ends in electron scattering, the error code or the continuum at the list's
    end, or where tau_event lies within g = 8 M of the reference's decisive sum at the line the fall-back happened at (base.check asserts both);
  * thresholds are also planted at the ends of the blocks a full coarse step of THIS width ends on (the advance after a full step is N - 2 blocks).
The proof in the header does not depend on the width; what does is how often a trace takes a second coarse step and where interval mode starts, which
the statistics at the end pin down.

Run once in a scratch copy, not committed: with the margin M = 0 (build_tables(..., margin_scale=0)) all six cases of the first test fail within the first
hundred traces, each on a planted threshold -- at eight loads on the 20 000-line table at trace 80: the reference passes line 19 975 and ends in electron
scattering in front of line 19 976, the lane, whose interval-mode sum is no upper bound any more and whose interval check has no gap left, takes line
19 975 as a line stop.
"""
import ctypes as C
import subprocess
from collections import Counter

import numpy as np
import pytest

import test_sweep_skip_host as base

WIDTHS = (8, 10, 12)

_SETTER = r"""
namespace { int g_loads = 0, g_chunk = 10; }
extern "C" void set_width(int loads) { g_loads = loads; g_chunk = loads; }
extern "C" void set_coarse_loads(int loads) { g_loads = loads; }
// plan::plan_sweep_skip of a build whose twelve-wave instantiation carries the skip (the shim's plan_skip leaves SkipInput::twelve_wave_skip at zero)
extern "C" int plan_skip_both_forms(int sweep_skip, int waves_per_simd, int nt, int shell_log, int line_scattering, int nt_negative, int pfx_negative)
{
    plan::SkipInput in{};
    in.sweep_skip = sweep_skip; in.lane_sweep = true; in.waves_per_simd = waves_per_simd; in.nt = nt; in.shell_log = shell_log; in.line_scattering = line_scattering;
    in.nt_negative = nt_negative; in.pfx_negative = pfx_negative; in.twelve_wave_skip = true;
    return plan::plan_sweep_skip(in) ? 1 : 0;
}
extern "C" int skip_trace("""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    src_text = base.SHIM
    assert src_text.count('extern "C" int skip_trace(') == 1 and src_text.count("in.fine_chunk = 10;") == 1
    src_text = src_text.replace('extern "C" int skip_trace(', _SETTER).replace("in.fine_chunk = 10;", "in.fine_chunk = g_chunk; in.loads = g_loads;")
    d = tmp_path_factory.mktemp("sweep_skip_widths")
    src, lib = d / "shim.cpp", d / "libsskw.so"
    src.write_text(src_text)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", base.CSRC, str(src), "-o", str(lib)], check=True)
    L = C.CDLL(str(lib))
    _d, _i, _pi, _pd = base._d, base._i, base._pi, base._pd
    L.build_tables.restype, L.build_tables.argtypes = _d, [C.c_void_p, C.c_void_p, _i, _i, _d]
    L.reference.restype, L.reference.argtypes = _i, [_i, _i, _d, _d, _d, _d, _d, _d, _pi, _pd, _pd]
    L.block_threshold.restype, L.block_threshold.argtypes = _d, [_i, _i, _i, _d, _d]
    L.skip_trace.restype, L.skip_trace.argtypes = _i, [_i, _i, _d, _d, _d, _d, _d, _d, _i, _i, _pi, _pd, _pi, _pd]
    L.reference_at.restype, L.reference_at.argtypes = None, [_i, _i, _i, _d, _d, _d, _pd]
    L.kprime.restype, L.kprime.argtypes = _d, [_d, _d, _d]
    L.set_width.restype, L.set_width.argtypes = None, [_i]
    L.set_coarse_loads.restype, L.set_coarse_loads.argtypes = None, [_i]
    L.plan_skip_both_forms.restype, L.plan_skip_both_forms.argtypes = _i, [_i] * 7
    return L


@pytest.mark.parametrize("loads", WIDTHS)
@pytest.mark.parametrize("n_lines", [20000, 20003])
def test_block_skip_equals_the_reference_loop_at_every_width(shim, n_lines, loads, margin_scale=1.0):
    geo, nu_line, tau_t = base.tables(n_lines)
    m = shim.build_tables(nu_line.ctypes.data, tau_t.ctypes.data, base.N_SHELLS, n_lines, margin_scale)
    shim.set_width(loads)
    g = 8.0 * m
    rng = np.random.default_rng(n_lines)
    n = 100000
    tr = base.make_traces(rng, geo, nu_line, n)  # (the parent test's traces: same generator, same seed)
    stats = Counter()
    planted = 0
    steps = Counter()
    # blocks whose ends a coarse test of this width compares tau_event with: the first two, the tenth (the parent's), the last of a full step, the first and
    # the last of the step after it
    blocks = sorted({0, 1, 9, loads - 2, loads - 1, 2 * loads - 4})
    for k in range(n):
        ref, info = base.check(shim, tr, k, g, stats)
        steps["coarse"] += info[1]; steps["fine"] += info[2]; steps["traces"] += 1
        if k % 16 == 0:
            for ulps in (-3, -1, 0, 1, 3):
                te = float(ref[3]) * (1.0 + ulps * 2.0 ** -52)
                if te > 1e-6:
                    base.check(shim, tr, k, g, stats, te)
                    planted += 1
            kp = shim.kprime(float(tr[4][k]), float(tr[2][k]), tr[7])
            for j in blocks:
                thr = shim.block_threshold(int(tr[0][k]), int(tr[1][k]), j, float(tr[3][k]), kp)
                for ulps in (-2, 0, 2):
                    te = thr * (1.0 + ulps * 2.0 ** -52)
                    if te > 1e-6:
                        base.check(shim, tr, k, g, stats, te)
                        planted += 1
    print(n_lines, "loads", loads, "margin", m, "planted", planted, dict(stats), "steps per random trace: coarse %.3f fine %.3f" %
          (steps["coarse"] / steps["traces"], steps["fine"] / steps["traces"]))
    for code in (1, 2, 3, 9, 10):
        assert stats["code%d" % code] > 0, code
    assert stats["interval"] > n // 4 and stats["coarse2"] > 100 and stats["first_block"] > 1000
    assert stats["fallback_margin"] > 0 and stats["fallback_escat"] > 0


@pytest.mark.parametrize("loads", WIDTHS)
def test_last_block_forced_fallback_and_skip_off(shim, loads):
    n_lines = 20003
    geo, nu_line, tau_t = base.tables(n_lines)
    m = shim.build_tables(nu_line.ctypes.data, tau_t.ctypes.data, base.N_SHELLS, n_lines, 1.0)
    shim.set_width(loads)
    rng = np.random.default_rng(5)
    tr = base.make_traces(rng, geo, nu_line, 4000)
    tr[1][:2000] = n_lines - rng.integers(0, 120, 2000)  # starts in the last fifteen blocks of the row, or behind the last line
    tr[1][:200] = n_lines
    tr[3][:2000] = np.nextafter(np.append(nu_line, nu_line[-1] * (1.0 - 1e-3))[tr[1][:2000]], np.inf)
    tr[2][:2000] = tr[3][:2000] / 0.97
    stats = Counter()
    for k in range(4000):
        base.check(shim, tr, k, 8.0 * m, stats)
        ref, got, info, _ = base.run_pair(shim, tr, k, force=1)
        assert got == ref[:3], (k, ref, got)
        assert info[0] == 1 or info[3] == 0 or (ref[0] & 8)
        ref, got, info, _ = base.run_pair(shim, tr, k, skip=0)  # the skip off: fine steps of this width only
        assert got == ref[:3] and info[1] == 0, (k, ref, got)
    assert stats["code9"] + stats["code10"] > 100


def test_zero_width_field_is_ten_loads(shim):
    """TraceIn::loads = 0 (what tests/test_sweep_skip_host.py leaves it at) walks exactly as 10."""
    n_lines = 20003
    geo, nu_line, tau_t = base.tables(n_lines)
    shim.build_tables(nu_line.ctypes.data, tau_t.ctypes.data, base.N_SHELLS, n_lines, 1.0)
    tr = base.make_traces(np.random.default_rng(11), geo, nu_line, 3000)
    seen = Counter()
    for k in range(3000):
        shim.set_width(10)
        a = base.run_pair(shim, tr, k)
        shim.set_coarse_loads(0)  # (the fine step stays at ten lines)
        b = base.run_pair(shim, tr, k)
        assert a == b, (k, a, b)
        seen["coarse2"] += a[2][1] >= 2
    assert seen["coarse2"] > 0


PLAN = dict(sweep_skip=-1, waves_per_simd=3, nt=1, shell_log=0, line_scattering=1, nt_negative=0, pfx_negative=0)


@pytest.mark.parametrize("change,expect", [
    (dict(), 1), (dict(sweep_skip=1), 1), (dict(waves_per_simd=4), 1),  # twelve waves under the conditions of sixteen
    (dict(sweep_skip=0), 0), (dict(nt=0), 0), (dict(nt=2), 0), (dict(shell_log=1), 0), (dict(line_scattering=0), 0), (dict(nt_negative=1), 0),
    (dict(pfx_negative=1), 0), (dict(waves_per_simd=2), 0),
])
def test_plan_allows_the_twelve_wave_form(shim, change, expect):
    a = dict(PLAN, **change)
    assert shim.plan_skip_both_forms(*[a[k] for k in PLAN]) == expect
