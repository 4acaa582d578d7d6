"""The kernel choice of tardis_mc_propagate as a pure function (tardis_amd/csrc/propagate_plan.hpp), pinned without a GPU.

A few-line extern "C" shim around plan::plan_propagate is compiled with the host C++ compiler into a temporary shared object.  The expected
values of every row are written from the rules as INTEGRATION.md, include/tardis_mc.h and the comments of the rules state them, not copied
from the function's answers.

The last field of a row says whether it was also confirmed on the GPU: the row's shape, config and options run through the engine library of
the commit before the plan existed, and through this one, gave the expected last_variant / last_table_offsets / error.  The other rows need
tables of 2^28 or 2^32 entries, 2^31 packets, or a fact a caller cannot set through the API (unsorted lines and negative probabilities are
properties of the tables, a negative optical depth in the screening tables and missing walk tables likewise): those are pinned here only.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tardis_amd", "csrc")

SHIM = r"""
#include "propagate_plan.hpp"
#include <cstring>
extern "C" int plan_shim(int n_shells, int n_lines, int n_trans, long long n_packets, long long n_vpackets, double survival, int full_relativity,
                         int line_interaction_type, int lines_sorted, int prob_negative, int have_walk_tables, int variant, int table_offsets,
                         int vpacket_screening, long long vpk_wave_min_packets, int track_full, int debug_flags, int pfx_valid, int pfx_negative,
                         int *out, char *message, int message_cap)
{
    plan::PlanInput in{};
    in.n_shells = n_shells; in.n_lines = n_lines; in.n_trans = n_trans; in.n_packets = n_packets;
    in.number_of_vpackets = n_vpackets; in.survival_probability = survival; in.enable_full_relativity = full_relativity;
    in.line_interaction_type = line_interaction_type; in.lines_sorted = lines_sorted != 0; in.prob_negative = prob_negative != 0;
    in.have_walk_tables = have_walk_tables != 0; in.variant = variant; in.table_offsets = table_offsets; in.vpacket_screening = vpacket_screening;
    in.vpk_wave_min_packets = vpk_wave_min_packets; in.track_full = track_full != 0; in.debug_flags = debug_flags;
    in.pfx_valid = pfx_valid != 0; in.pfx_negative = pfx_negative != 0;
    const plan::Plan p = plan::plan_propagate(in);
    out[0] = p.last_variant; out[1] = p.last_table_offsets; out[2] = p.screen_on; out[3] = p.variant; out[4] = p.cooperative; out[5] = p.w64;
    std::strncpy(message, p.message, message_cap - 1);
    message[message_cap - 1] = 0;
    return p.error;
}
"""

FIELDS = ["n_shells", "n_lines", "n_trans", "n_packets", "n_vpackets", "survival", "full_relativity", "line_interaction_type", "lines_sorted",
          "prob_negative", "have_walk_tables", "variant", "table_offsets", "vpacket_screening", "vpk_wave_min_packets", "track_full", "debug_flags",
          "pfx_valid", "pfx_negative"]
# the tardis_example shape (<= 30 shells, <= 1e5 lines), macroatom, partial relativity, no v-packets, every option at its default
DEFAULTS = dict(n_shells=20, n_lines=29224, n_trans=90000, n_packets=40000, n_vpackets=0, survival=0.0, full_relativity=0, line_interaction_type=2,
                lines_sorted=1, prob_negative=0, have_walk_tables=1, variant=-1, table_offsets=-1, vpacket_screening=-1, vpk_wave_min_packets=100000,
                track_full=0, debug_flags=0, pfx_valid=0, pfx_negative=0)
FINE = dict(n_shells=100, n_lines=500000, n_trans=1500000)        # a fine grid, n_lines >= 2500 n_shells: screening on by default
FINE_SHORT = dict(n_shells=100, n_lines=200000, n_trans=600000)   # ... n_lines < 2500 n_shells: off by default
V10 = dict(n_vpackets=10)
B28_LO, B28_HI = 2684354, 2684355     # x 100 shells: 268 435 400 < 2^28 = 268 435 456 <= 268 435 500
BELOW28 = dict(n_shells=100, n_lines=B28_LO)
ABOVE28 = dict(n_shells=100, n_lines=B28_HI)
TRANS_BELOW28 = dict(FINE, n_trans=B28_LO)
TRANS_ABOVE28 = dict(FINE, n_trans=B28_HI)
ABOVE32 = dict(n_shells=3000, n_lines=1431656)  # 4 294 968 000 >= 2^32 = 4 294 967 296
INVALID = -1  # TARDIS_MC_ERR_INVALID_ARGUMENT


# expect: (last_variant, last_table_offsets, screen_on) or ("error", a substring of its text)
ROWS = [
    # -- the automatic choice
    ("example", (3, 32, False), [], dict(), True),                                     # no v-packets, partial relativity: lane sweeps
    ("example-fullrel", (2, 32, False), [], dict(full_relativity=1), True),            # lane sweeps need partial relativity
    ("example-vpk", (2, 32, False), [V10], dict(), True),                              # small shape: pooled volleys; 29224 < 2500 * 20: no screening
    ("example-vpk-screen1", (2, 32, True), [V10], dict(vpacket_screening=1), True),
    ("example-vpk-screen0", (2, 32, False), [V10], dict(vpacket_screening=0), True),
    ("fine-vpk-below-min", (1, 32, True), [FINE, V10], dict(n_packets=99999), True),    # screened, but too short a call for the wave kernel
    ("fine-vpk-at-min", (2, 32, True), [FINE, V10], dict(n_packets=100000), True),
    ("fine-vpk-min-option", (2, 32, True), [FINE, V10], dict(n_packets=20000, vpk_wave_min_packets=20000), True),
    ("fine-vpk-screen0", (1, 32, False), [FINE, V10], dict(n_packets=1000000, vpacket_screening=0), True),  # without screening: the group kernel
    ("fine-vpk-noscreen-flag", (1, 32, False), [FINE, V10], dict(n_packets=1000000, debug_flags=33554432), True),
    ("fine-short-vpk-auto", (1, 32, False), [FINE_SHORT, V10], dict(n_packets=1000000), True),
    ("fine-short-vpk-screen1", (2, 32, True), [FINE_SHORT, V10], dict(n_packets=1000000, vpacket_screening=1), True),
    ("fine-short-vpk-screen1-short", (1, 32, True), [FINE_SHORT, V10], dict(n_packets=50000, vpacket_screening=1), True),
    ("fine-novpk", (3, 32, False), [FINE], dict(n_packets=1000000), True),
    ("vpk-33", (0, 64, False), [V10], dict(n_vpackets=33, n_packets=4000), True),                       # more than 32 v-packets per volley: the lane kernel
    ("fine-vpk-33-screen1", (0, 64, False), [FINE], dict(n_vpackets=33, vpacket_screening=1, n_packets=2000), True),   # ... which traces line by line
    ("forced-2-vpk-33", (0, 64, False), [], dict(n_vpackets=33, variant=2, n_packets=4000), True),
    ("unsorted", (0, 64, False), [], dict(lines_sorted=0), False),
    ("unsorted-forced-1", (0, 64, False), [], dict(lines_sorted=0, variant=1), False),
    ("forced-0", (0, 64, False), [], dict(variant=0), True),
    ("forced-1", (1, 32, False), [], dict(variant=1), True),
    ("forced-2", (2, 32, False), [], dict(variant=2), True),
    # -- negative probabilities: the wave kernel searches the monotone running sums
    ("probneg-auto", (1, 32, False), [], dict(prob_negative=1), False),
    ("probneg-2", (1, 32, False), [], dict(prob_negative=1, variant=2), False),
    ("probneg-3", (1, 32, False), [], dict(prob_negative=1, variant=3), False),
    ("probneg-4", (1, 32, False), [V10], dict(prob_negative=1, variant=4), False),
    # -- surviving v-packets: the group kernel
    ("survival-auto", (1, 32, False), [V10], dict(survival=0.5), True),
    ("survival-3", (1, 32, False), [V10], dict(survival=0.5, variant=3), True),
    ("survival-4", (1, 32, False), [V10], dict(survival=0.5, variant=4), True),
    ("survival-no-vpk", (3, 32, False), [], dict(survival=0.5), True),
    # -- variant 4 (the volley queue) and variant 3 under full relativity
    ("v4-vpk", (4, 32, False), [V10], dict(variant=4), True),
    ("v4-no-vpk", (3, 32, False), [], dict(variant=4), True),
    ("v4-no-vpk-fullrel", (2, 32, False), [], dict(variant=4, full_relativity=1), True),
    ("v3-fullrel", (2, 32, False), [], dict(variant=3, full_relativity=1), True),
    ("v3-vpk", (3, 32, False), [V10], dict(variant=3), True),
    # -- full r-packet tracking: variant 2 where it can run the call, else the lane kernel
    ("track-auto", (2, 32, False), [], dict(track_full=1), True),
    ("track-vpk", (2, 32, False), [V10], dict(track_full=1), True),
    ("track-forced-1", (2, 32, False), [], dict(track_full=1, variant=1), True),
    ("track-forced-4", (2, 32, False), [V10], dict(track_full=1, variant=4), True),
    ("track-forced-0", (0, 64, False), [], dict(track_full=1, variant=0), True),
    ("track-unsorted", (0, 64, False), [], dict(track_full=1, lines_sorted=0), False),
    ("track-probneg", (0, 64, False), [], dict(track_full=1, prob_negative=1), False),
    ("track-vpk-33", (0, 64, False), [], dict(track_full=1, n_vpackets=33, n_packets=4000), True),
    ("track-survival", (0, 64, False), [V10], dict(track_full=1, survival=0.5), True),
    ("track-no-walk-tables", (0, 64, False), [], dict(track_full=1, have_walk_tables=0), False),
    ("track-scatter-no-walk-tables", (2, 32, False), [], dict(track_full=1, have_walk_tables=0, line_interaction_type=0), False),
    ("track-flag-128", (0, 64, False), [], dict(track_full=1, debug_flags=128), True),
    ("track-flag-8192", (0, 64, False), [], dict(track_full=1, debug_flags=8192), True),
    ("track-flag-long", (0, 64, False), [], dict(track_full=1, debug_flags=1048576), True),
    ("track-flag-counter", (0, 64, False), [], dict(track_full=1, debug_flags=16), True),
    ("track-2^31-packets", (0, 64, False), [], dict(track_full=1, n_packets=1 << 31), False),
    # -- table_offsets -1 / 0 / 1 on both sides of 2^28 entries, by n_shells * n_lines and by n_shells * n_trans
    ("lines-below-auto", (3, 32, False), [BELOW28], dict(), False),
    ("lines-above-auto", (3, 64, False), [ABOVE28], dict(), False),
    ("lines-below-0", (3, 32, False), [BELOW28], dict(table_offsets=0), False),
    ("lines-above-0", ("error", "option table_offsets is 0"), [ABOVE28], dict(table_offsets=0), False),
    ("lines-below-1", (3, 64, False), [BELOW28], dict(table_offsets=1), False),
    ("lines-above-1", (3, 64, False), [ABOVE28], dict(table_offsets=1), False),
    ("trans-below-auto", (3, 32, False), [TRANS_BELOW28], dict(), False),
    ("trans-above-auto", (3, 64, False), [TRANS_ABOVE28], dict(), False),
    ("trans-below-0", (3, 32, False), [TRANS_BELOW28], dict(table_offsets=0), False),
    ("trans-above-0", ("error", "2^28"), [TRANS_ABOVE28], dict(table_offsets=0), False),
    ("trans-below-1", (3, 64, False), [TRANS_BELOW28], dict(table_offsets=1), False),
    ("trans-above-1", (3, 64, False), [TRANS_ABOVE28], dict(table_offsets=1), False),
    ("lines-above-group", (1, 64, False), [ABOVE28], dict(variant=1), False),
    ("lines-above-lane-0", (0, 64, False), [ABOVE28], dict(variant=0, table_offsets=0), False),  # the lane kernel always has 64-bit offsets
    ("example-offsets-1", (3, 64, False), [], dict(table_offsets=1), True),
    ("example-offsets-1-group", (1, 64, False), [], dict(table_offsets=1, variant=1), True),
    ("example-offsets-1-vpk-screen", (2, 64, True), [V10], dict(table_offsets=1, vpacket_screening=1), True),
    ("offsets-1-v4", ("error", "variant 4 (the volley queue) has no 64-bit table offsets"), [V10], dict(table_offsets=1, variant=4), True),
    ("offsets-1-flag-128", ("error", "cross-check instantiations of the wave kernel"), [], dict(table_offsets=1, debug_flags=128), True),
    ("offsets-1-flag-counter", ("error", "cross-check instantiations of the wave kernel"), [], dict(table_offsets=1, variant=2, debug_flags=4), True),
    ("offsets-1-flag-128-group", (1, 64, False), [], dict(table_offsets=1, variant=1, debug_flags=128), True),
    # -- 2^32 line entries: the wave kernels' line-visit log indexes (shell, line) in 32 bits
    ("2^32-auto", (1, 64, False), [ABOVE32], dict(), False),
    ("2^32-forced-3", ("error", "n_shells * n_lines reaches 2^32"), [ABOVE32], dict(variant=3), False),
    ("2^32-forced-2", ("error", "n_shells * n_lines reaches 2^32"), [ABOVE32], dict(variant=2), False),
    ("2^32-track", (0, 64, False), [ABOVE32], dict(track_full=1), False),
    ("2^32-offsets-0", ("error", "option table_offsets is 0"), [ABOVE32], dict(table_offsets=0), False),
    # -- 64-bit offsets without the compact walk tables: the fp64 walks are only in the 32-bit cross-check instantiations
    ("offsets-1-no-walk-tables", (0, 64, False), [], dict(table_offsets=1, have_walk_tables=0), False),
    ("offsets-1-no-walk-tables-scatter", (3, 64, False), [], dict(table_offsets=1, have_walk_tables=0, line_interaction_type=0), False),
    ("offsets-1-no-walk-tables-group", (1, 64, False), [], dict(table_offsets=1, have_walk_tables=0, variant=1), False),
    # -- the screening's second look: the tables hold a negative optical depth
    ("second-look-before", (2, 32, True), [FINE, V10], dict(n_packets=1000000), True),
    ("second-look-built-fine", (2, 32, True), [FINE, V10], dict(n_packets=1000000, pfx_valid=1), True),
    ("second-look-negative", (1, 32, False), [FINE, V10], dict(n_packets=1000000, pfx_valid=1, pfx_negative=1), False),
    ("second-look-negative-small-shape", (2, 32, False), [V10], dict(vpacket_screening=1, pfx_valid=1, pfx_negative=1), False),
    ("second-look-negative-forced-2", (2, 32, False), [FINE, V10], dict(n_packets=1000000, variant=2, pfx_valid=1, pfx_negative=1), False),
    ("second-look-negative-offsets-1", (1, 64, False), [FINE, V10], dict(n_packets=1000000, table_offsets=1, pfx_valid=1, pfx_negative=1), False),
]


def inputs_of(parts, kw):
    d = dict(DEFAULTS)
    for p in parts:
        d.update(p)
    d.update(kw)
    return d


GPU_ROWS = [(name, inputs_of(parts, kw), expect) for name, expect, parts, kw, gpu in ROWS if gpu]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("plan")
    src = d / "plan_shim.cpp"
    src.write_text(SHIM)
    so = d / "plan_shim.so"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)], check=True)
    f = ctypes.CDLL(str(so)).plan_shim
    i, ll = ctypes.c_int, ctypes.c_longlong
    f.argtypes = [i, i, i, ll, ll, ctypes.c_double] + [i] * 8 + [ll] + [i] * 4 + [ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, i]
    f.restype = i
    return f


def test_header_is_free_of_hip():
    text = open(os.path.join(CSRC, "propagate_plan.hpp")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ['"../../include/tardis_mc.h"']
    assert "__global__" not in text and "__device__" not in text and "hipError_t" not in text


@pytest.mark.parametrize("name,expect,parts,kw,gpu", ROWS, ids=[r[0] for r in ROWS])
def test_plan_row(shim, name, expect, parts, kw, gpu):
    d = inputs_of(parts, kw)
    out = (ctypes.c_int * 6)()
    msg = ctypes.create_string_buffer(512)
    rc = shim(*[d[k] for k in FIELDS], out, msg, 512)
    last_variant, offsets, screen_on, variant, cooperative, w64 = list(out)
    if expect[0] == "error":
        assert rc == INVALID and expect[1] in msg.value.decode()
        return
    assert rc == 0 and msg.value == b""
    assert (last_variant, offsets, bool(screen_on)) == expect
    # what the fields mean to each other
    assert bool(cooperative) == (last_variant != 0)
    assert offsets == (64 if (w64 or not cooperative) else 32)
    if cooperative and not (variant == 3 and d["full_relativity"]):
        assert variant == last_variant
