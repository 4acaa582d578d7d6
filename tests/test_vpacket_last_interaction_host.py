"""The v-packet log's last-interaction columns without a GPU: the yardstick (tests/vpacket_last_interaction_ref.py) on a hand-written
event log, the host statement of the virtual decomposition (tardis_amd.spectrum.vpacket_decomposition) against a brute-force loop, and
the ABI pieces (the exported symbols, the mirror struct against the C header's)."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vpacket_last_interaction_ref as vref  # noqa: E402
from tardis_amd import _abi, _lib, spectrum  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_yardstick_on_a_hand_written_event_log():
    """Three packets, spawn window [2, 8], two v-packets per volley.
    packet 0: launched at nu 5 (volley), a LINE row leaving at nu 9 (volley skipped), a boundary row, an ESCATTERING row leaving at
              nu 8 (on the edge: volley), a boundary row out;
    packet 1: launched at nu 1 (launch volley skipped), a LINE row leaving at nu 3 (volley), a boundary row out;
    packet 2: launched at nu 2 (on the edge: volley), no interaction, one boundary row."""
    #        packet 0                      | packet 1     | packet 2
    itype = [2,    1,    4,    1,            2,    1,       1]
    b_nu = [5.0,  9.0,  9.0,  8.0,          1.0,  3.0,     2.0]
    a_nu = [9.0,  9.0,  8.0,  8.0,          3.0,  3.0,     2.0]
    rad = [1.5,  2.0,  1.75, 3.0,          1.25, 3.0,     3.0]
    absorb = [17,  -1,   -1,   -1,           4,    -1,      -1]
    emit = [11,    -1,   -1,   -1,           9,    -1,      -1]
    shell = [1,    1,    2,    2,            0,    2,       2]
    offsets = [0, 4, 6, 7]
    nu0 = vref.launch_nus(offsets, b_nu)
    assert nu0.tolist() == [5.0, 1.0, 2.0]
    out = vref.expected_log(offsets, itype, b_nu, a_nu, rad, absorb, emit, shell, nu0, 2.0, 8.0, 2)
    assert out["offsets"].tolist() == [0, 4, 6, 8]
    assert out["source_packet"].tolist() == [0, 0, 0, 0, 1, 1, 2, 2]
    assert out["last_interaction_type"].tolist() == [-1, -1, 4, 4, 2, 2, -1, -1]
    assert out["last_interaction_in_id"].tolist() == [-1, -1, -1, -1, 4, 4, -1, -1]
    assert out["last_interaction_out_id"].tolist() == [-1, -1, -1, -1, 9, 9, -1, -1]
    assert out["last_interaction_shell_id"].tolist() == [-1, -1, 2, 2, 0, 0, -1, -1]
    assert vref.same_bits(out["last_interaction_in_nu"], [NAN, NAN, 9.0, 9.0, 1.0, 1.0, NAN, NAN])
    assert vref.same_bits(out["last_interaction_in_r"], [NAN, NAN, 1.75, 1.75, 1.25, 1.25, NAN, NAN])
    assert (out["launch_volleys"], out["launch_skipped"], out["interaction_volleys"], out["interaction_skipped"]) == (2, 1, 2, 1)
    for f in vref.INT_FIELDS + ("source_packet", "offsets"):
        assert out[f].dtype == np.int64
    # a window that admits everything / nothing
    wide = vref.expected_log(offsets, itype, b_nu, a_nu, rad, absorb, emit, shell, nu0, 0.0, np.inf, 3)
    assert wide["offsets"].tolist() == [0, 9, 15, 18] and wide["last_interaction_type"][3:6].tolist() == [2, 2, 2]
    none = vref.expected_log(offsets, itype, b_nu, a_nu, rad, absorb, emit, shell, nu0, 20.0, 30.0, 3)
    assert none["offsets"].tolist() == [0, 0, 0, 0] and len(none["source_packet"]) == 0
    assert not vref.same_bits([NAN, 1.0], [1.0, NAN]) and not vref.same_bits([1.0], [np.nextafter(1.0, 2.0)])


def test_host_vpacket_decomposition_equals_a_brute_force_loop():
    """About 50 hand-made entries: the three kinds, dropped v-packets (energy 0.0), frequencies off the grid and on its end points,
    a strict window."""
    rng = np.random.default_rng(3)
    n, L, S, C, t = 52, 6, 3, 3, 4.0
    grid = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    B = len(grid) - 1
    cls = np.array([0, 1, 2, 0, 1, 2])
    itype = np.array([-1, 2, 4, 2] * 13)
    nu = np.round(rng.uniform(0.5, 5.5, n), 2)
    nu[:4] = [1.0, 5.0, 5.0, 1.0]                    # the grid's end points: the last bin is closed on the right
    energy = rng.integers(0, 4, n) * 0.25            # multiples of 1/4: every sum below is exact in any order
    in_nu = np.where(itype == -1, NAN, np.round(rng.uniform(0.5, 5.5, n), 2))
    out_id = np.where(itype == 2, rng.integers(0, L, n), -1)
    in_id = np.where(itype == 2, rng.integers(0, L, n), -1)
    shell = np.where(itype == -1, -1, rng.integers(0, S, n))
    assert (energy == 0).sum() > 5 and ((nu < 1) | (nu > 5)).sum() > 3

    def bin_of(x):
        if not (grid[0] <= x <= grid[-1]):
            return None
        return min(int(np.searchsorted(grid, x, side="right")) - 1, B - 1)

    for lo, hi in ((0.0, np.inf), (1.0, 5.0), (2.25, 4.5)):
        want = {"emission": np.zeros((C, B)), "absorption": np.zeros((C, B)), "no_interaction": np.zeros(B), "electron_scatter": np.zeros(B),
                "shell_packets": np.zeros((C + 1, S), dtype=np.int64), "line_emit_packets": np.zeros(L, dtype=np.int64),
                "line_absorb_packets": np.zeros(L, dtype=np.int64), "n_selected": 0, "n_line": 0, "n_electron_scatter": 0, "n_no_interaction": 0}
        for i in range(n):
            if not (lo < nu[i] < hi):
                continue
            want["n_selected"] += 1
            w, k = energy[i] / t, bin_of(nu[i])
            if itype[i] == 2:
                want["n_line"] += 1
                if k is not None:
                    want["emission"][cls[out_id[i]], k] += w
                k_in = bin_of(in_nu[i])
                if k_in is not None:
                    want["absorption"][cls[in_id[i]], k_in] += w
                want["shell_packets"][cls[out_id[i]], shell[i]] += 1
                want["line_emit_packets"][out_id[i]] += 1
                want["line_absorb_packets"][in_id[i]] += 1
            elif itype[i] == 4:
                want["n_electron_scatter"] += 1
                if k is not None:
                    want["electron_scatter"][k] += w
                want["shell_packets"][C, shell[i]] += 1
            else:
                want["n_no_interaction"] += 1
                if k is not None:
                    want["no_interaction"][k] += w
        got = spectrum.vpacket_decomposition(nu, energy, t, grid, itype, out_id, in_id, in_nu, shell, cls, S, C, lo, hi)
        assert set(got) == set(want)
        for key, v in want.items():
            assert np.array_equal(got[key], v), (key, lo, hi)
        assert want["n_selected"] == want["n_line"] + want["n_electron_scatter"] + want["n_no_interaction"]
    assert want["n_selected"] < n  # (the last window drops entries)


FIELDS = ["capacity", "count", "offsets", "source_packet", "nus", "energies", "initial_mus", "initial_rs", "last_interaction_in_nu",
          "last_interaction_in_r", "last_interaction_type", "last_interaction_in_id", "last_interaction_out_id", "last_interaction_shell_id"]

SHIM = r"""
#include <stddef.h>
#include "tardis_mc.h"
long long size_shim(void) { return (long long)sizeof(TardisMcVpacketLog); }
long long offset_shim(int k)
{
    const size_t o[] = {%s};
    return (long long)o[k];
}
long long result_size_shim(void) { return (long long)sizeof(TardisMcResult); }
""" % ", ".join("offsetof(TardisMcVpacketLog, %s)" % f for f in FIELDS)


def test_library_exports_both_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert hasattr(L, "tardis_mc_get_vpacket_log") and hasattr(L, "tardis_mc_vpacket_decomposition")
    assert "tardis_mc_get_vpacket_log" in _lib.SYMBOLS and "tardis_mc_vpacket_decomposition" in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    assert "int tardis_mc_get_vpacket_log(TardisMcContext *ctx, TardisMcVpacketLog *log);" in header
    assert "int tardis_mc_vpacket_decomposition(TardisMcContext *ctx, TardisMcDecomposition *d);" in header
    assert "#define TARDIS_MC_ABI_VERSION 2 " in header
    from tardis_amd.engine import Engine
    from tardis_amd.transport import MonteCarloTransportState
    for name in ("get_vpacket_log", "vpacket_decomposition"):
        assert callable(getattr(Engine, name, None))
    assert callable(getattr(MonteCarloTransportState, "vpacket_decomposition", None))


def test_mirror_struct_is_the_headers(tmp_path):
    """The struct the issue gives has fourteen 8-byte members -- capacity, count, two index arrays, four + two float64 columns and four
    int64 columns -- so it is 14 x 8 = 112 bytes (the issue's prose says fifteen; its own declaration, which this mirrors member by
    member, has fourteen).  The mirror is held against the C header itself: size and every offset."""
    assert [f[0] for f in _abi.TardisMcVpacketLog._fields_] == FIELDS
    assert ctypes.sizeof(_abi.TardisMcVpacketLog) == 14 * 8
    assert ctypes.sizeof(_abi.TardisMcResult) == 37 * 8  # TardisMcResult keeps its layout
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler (gcc / cc / clang) to compile include/tardis_mc.h")
    src, so = tmp_path / "shim.c", tmp_path / "shim.so"
    src.write_text(SHIM)
    subprocess.run([cc, "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.size_shim.restype = lib.offset_shim.restype = lib.result_size_shim.restype = ctypes.c_longlong
    assert lib.size_shim() == ctypes.sizeof(_abi.TardisMcVpacketLog)
    assert lib.result_size_shim() == ctypes.sizeof(_abi.TardisMcResult)
    for k, f in enumerate(FIELDS):
        assert lib.offset_shim(k) == getattr(_abi.TardisMcVpacketLog, f).offset, f
