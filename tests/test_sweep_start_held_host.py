"""CPU check of the held start entry of a post-emission trace (ssk::MODE_START_HELD, tardis_amd/csrc/sweep_skip.hpp; option `sweep_start_held`).

An emission that a hot sector of the macro-atom walk decided reads pn[shell][emit] and pn[shell][emit + 1] together; the second is the start entry
{nu_start, p_start} of the trace that follows (start = emit + 1).  The prologue of that trace evaluates coarse_scan's start guard on it, a trace that fails
the guard takes no coarse step at all, and the coarse steps of the others take p_start from the lane instead of loading pn[shell][start].

The tables, the traces (same generator, same seed), the planted thresholds, the reference loop and the rule for fall-backs are those of
tests/test_sweep_skip_host.py, whose shim is compiled here with a switch in front of ssk::trace: every trace with start - 1 < L - 1 is started as a
post-emission trace with the entry held (TraceIn::start_held, held_nu, held_p), at 8 and 10 loads per step.  Each trace runs on the held path and on the
load path.  Both are held to the reference's loop in code, line and distance, and they must agree with each other on every output of ssk::trace --
fall-backs, their line, code, gap and bound, interval mode, fine steps -- and in coarse steps up to the one step the load path spends on a start that
fails the guard; the held path issues no load of pn[start], the load path one per coarse step.

Planted on top of the random traces: emit + 1 on a block boundary; emit = L - 3, L - 2, L - 1 (the last: no pair, the present read); a line list in which
nu[emit + 1] == nu[emit] and one in which it lies one ulp below, with the packet's comoving frequency within ulps of the line on either side (the guard
must send what the reference counts as a close or a negative frequency difference to the exact evaluation); starts whose guard fails on xb."""
import ctypes as C
import subprocess
from collections import Counter

import numpy as np
import pytest

import test_sweep_skip_host as base

WIDTHS = (8, 10)

_SETTER = r"""
namespace { int g_loads = 0, g_chunk = 10, g_held = 0, g_start_loads = 0, g_guard_failed = 0; }
extern "C" void set_width(int loads) { g_loads = loads; g_chunk = loads; }
extern "C" void set_held(int held) { g_held = held; }
extern "C" int last_start_loads() { return g_start_loads; }
extern "C" int last_guard_failed() { return g_guard_failed; }
extern "C" int skip_trace("""
_INPUTS = ("in.fine_chunk = g_chunk; in.loads = g_loads; in.start_held = g_held && start >= 1 && start - 1 < T.L - 1;"
           " if (in.start_held) { in.held_nu = in.pn[2 * start]; in.held_p = in.pn[2 * start + 1]; }")
_OUTPUTS = "g_start_loads = o.start_loads; g_guard_failed = o.guard_failed; *line_out = o.line;"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    text = base.SHIM
    assert text.count('extern "C" int skip_trace(') == 1 and text.count("in.fine_chunk = 10;") == 1 and text.count("*line_out = o.line;") == 1
    text = text.replace('extern "C" int skip_trace(', _SETTER).replace("in.fine_chunk = 10;", _INPUTS).replace("*line_out = o.line;", _OUTPUTS)
    d = tmp_path_factory.mktemp("sweep_start_held")
    src, lib = d / "shim.cpp", d / "libsskh.so"
    src.write_text(text)
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
    L.set_held.restype, L.set_held.argtypes = None, [_i]
    L.last_start_loads.restype, L.last_guard_failed.restype = _i, _i
    return L


def both_paths(shim, tr, k, g, stats, tau_event=None):
    """Trace k on the held path and on the load path: each against the reference's loop (base.check), and against each other."""
    L = len(shim.nu_line)
    pair = 1 <= int(tr[1][k]) and int(tr[1][k]) - 1 < L - 1  # (emit < L - 1: the walk reads the pair)
    shim.set_held(1)
    ref, held = base.check(shim, tr, k, g, stats, tau_event)
    held_loads, held_failed = shim.last_start_loads(), shim.last_guard_failed()
    _, got_h, info_h, gap_h = base.run_pair(shim, tr, k, tau_event)
    shim.set_held(0)
    _, load = base.check(shim, tr, k, g, Counter(), tau_event)
    load_loads, load_failed = shim.last_start_loads(), shim.last_guard_failed()
    _, got_l, info_l, gap_l = base.run_pair(shim, tr, k, tau_event)
    assert got_h == got_l and gap_h == gap_l, (k, tau_event, got_h, got_l, gap_h, gap_l)
    assert info_h == held and info_l == load
    # fell_back, fine steps, interval mode, fall-back code and line
    assert (held[0], held[2], held[3], held[4], held[5]) == (load[0], load[2], load[3], load[4], load[5]), (k, tau_event, held, load)
    assert load_failed == 0 and load_loads == load[1]
    if pair:
        assert held_loads == 0 and load[1] == held[1] + held_failed, (k, tau_event, held, load, held_failed)
        if held_failed:
            assert held[1] == 0 and load[1] == 1 and held[3] == 0 and held[0] == 0  # the one step that returned 0; line by line from the first line on
        stats["held"] += 1
        stats["guard_failed"] += held_failed
        stats["held_coarse_steps"] += held[1]
    else:
        assert (held_loads, held_failed, held[1]) == (load_loads, 0, load[1])
        stats["no_pair"] += 1
    return ref, held


def build(shim, nu_line, tau_t, n_lines, loads):
    m = shim.build_tables(nu_line.ctypes.data, tau_t.ctypes.data, base.N_SHELLS, n_lines, 1.0)
    shim.set_width(loads)
    shim.nu_line = nu_line
    return m


@pytest.mark.parametrize("loads", WIDTHS)
@pytest.mark.parametrize("n_lines", [20000, 20003])
def test_held_start_entry_equals_the_reference_loop_and_the_load_path(shim, n_lines, loads):
    geo, nu_line, tau_t = base.tables(n_lines)
    m = build(shim, nu_line, tau_t, n_lines, loads)
    g = 8.0 * m
    rng = np.random.default_rng(n_lines)
    n = 100000
    tr = base.make_traces(rng, geo, nu_line, n)  # (the parent test's traces: same generator, same seed)
    stats = Counter()
    planted = 0
    for k in range(n):
        ref, info = both_paths(shim, tr, k, g, stats)
        if k % 16 == 0:
            # thresholds within 8 M of the decisive sums, as tests/test_sweep_skip_host.py plants them
            for ulps in (-3, -1, 0, 1, 3):
                te = float(ref[3]) * (1.0 + ulps * 2.0 ** -52)
                if te > 1e-6:
                    both_paths(shim, tr, k, g, stats, te)
                    planted += 1
            kp = shim.kprime(float(tr[4][k]), float(tr[2][k]), tr[7])
            for j in (0, 1, 9):
                thr = shim.block_threshold(int(tr[0][k]), int(tr[1][k]), j, float(tr[3][k]), kp)
                for ulps in (-2, 0, 2):
                    te = thr * (1.0 + ulps * 2.0 ** -52)
                    if te > 1e-6:
                        both_paths(shim, tr, k, g, stats, te)
                        planted += 1
    print(n_lines, "loads", loads, "margin", m, "planted", planted, dict(stats))
    for code in (1, 2, 3, 9, 10):
        assert stats["code%d" % code] > 0, code
    assert stats["interval"] > n // 4 and stats["coarse2"] > 100 and stats["first_block"] > 1000
    assert stats["fallback_margin"] > 0 and stats["fallback_escat"] > 0
    assert stats["held"] > n and stats["no_pair"] > 0 and stats["held_coarse_steps"] > n // 2
    assert stats["guard_failed"] > 100  # (a boundary nearer than the first line: the guard fails on xb)


def _near(x, ulps):
    for _ in range(abs(ulps)):
        x = np.nextafter(x, np.inf if ulps > 0 else 0.0)
    return x


@pytest.mark.parametrize("loads", WIDTHS)
@pytest.mark.parametrize("n_lines", [20000, 20003])
def test_planted_starts(shim, n_lines, loads):
    geo, nu_line, tau_t = base.tables(n_lines)
    nu_line = nu_line.copy()
    L = n_lines
    rng = np.random.default_rng(17 + n_lines)
    # coincident neighbours and neighbours one ulp apart, 400 each, away from each other and from the end of the list
    sites = rng.choice(np.arange(8, L - 64, 4), 800, replace=False)
    equal, ulp = sites[:400], sites[400:]
    nu_line[equal + 1] = nu_line[equal]
    nu_line[ulp + 1] = np.nextafter(nu_line[ulp], 0.0)
    assert np.all(np.diff(nu_line) <= 0)
    m = build(shim, nu_line, tau_t, n_lines, loads)
    g = 8.0 * m
    stats = Counter()

    def traces(start, comov=None):
        tr = list(base.make_traces(rng, geo, nu_line, len(start)))
        tr[1] = np.asarray(start, dtype=np.int64)
        nu_ext = np.append(nu_line, nu_line[-1] * (1.0 - 1e-3))
        if comov is None:
            comov = np.maximum(nu_ext[tr[1]] + rng.random(len(start)) * (nu_ext[tr[1] - 1] - nu_ext[tr[1]]), np.nextafter(nu_ext[tr[1]], np.inf))
        ratio = tr[3] / tr[2]  # (the generator's comov / nu = 1 - beta)
        tr[3] = np.asarray(comov, dtype=np.float64)
        tr[2] = tr[3] / ratio
        return tuple(tr)

    def sweep(tr, name):
        before = Counter(stats)
        for k in range(len(tr[1])):
            both_paths(shim, tr, k, g, stats)
        return {key: stats[key] - before[key] for key in stats if stats[key] != before[key]}

    # emit + 1 on a block boundary, first and last blocks of the row included
    d = sweep(traces(8 * rng.integers(1, (L - 1) // 8 + 1, 3000)), "boundary")
    assert d["held"] == 3000 and d["held_coarse_steps"] > 1500
    # emit = L - 3, L - 2, L - 1: start entries {nu[L - 2], .}, {-inf, .} (the last line: the guard fails), and no pair at all
    for emit, pair in ((L - 3, True), (L - 2, True), (L - 1, False)):
        d = sweep(traces(np.full(300, emit + 1)), "end")
        if pair:
            assert d["held"] == 300 and d.get("no_pair", 0) == 0
        else:
            assert d["no_pair"] == 300 and d.get("held", 0) == 0
        if emit == L - 2:
            assert d["guard_failed"] == 300 and d.get("held_coarse_steps", 0) == 0
    # nu[emit + 1] == nu[emit], and one ulp below: the packet's comoving frequency within ulps of the emission line, on either side of it
    for name, where in (("equal", equal), ("ulp", ulp)):
        for ulps in (-2, -1, 0, 1, 2):
            comov = np.array([_near(nu_line[e], ulps) for e in where])
            d = sweep(traces(where + 1, comov), name)
            assert d["held"] == 400
            below = comov < nu_line[where + 1]
            # (a negative frequency difference on the first line never passes the guard)
            assert d.get("guard_failed", 0) >= int(below.sum()), (name, ulps, d, int(below.sum()))
    # a start whose guard fails on xb: the boundary nearer than the first line
    tr = list(traces(rng.integers(1, L - 1, 2000)))
    x_first = tr[3] - nu_line[tr[1]]
    t_exp = tr[7]
    tr[6] = (x_first / tr[2]) * base.C_LIGHT * t_exp * rng.uniform(0.2, 0.999, 2000)
    d = sweep(tuple(tr), "xb")
    assert d["guard_failed"] > 1900
    print(n_lines, "loads", loads, dict(stats))
