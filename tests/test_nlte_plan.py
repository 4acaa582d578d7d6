"""The launches of the NLTE solve kernel as a pure function (nlte::plan_launches, tardis_amd/csrc/nlte_plan.hpp), pinned without a GPU.

A few-line extern "C" shim around the function is compiled with the host C++ compiler into a temporary shared object.  The expected values
are worked out here from the header's stated rules -- the size classes of 8, 16, 32, 64, 96 and 141 levels, the working set of a species
(a column-major n x n fp64 matrix of odd leading dimension n | 1 and four vectors of n), the global form from 142 levels on, and the
2^30-byte bound on all slabs -- not copied from the function's answers.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tardis_amd", "csrc")

SHIM = r"""
#include "nlte_plan.hpp"
// out: {entries of the list, launches, scratch doubles, largest LDS request, refused species, its bytes, the bytes before it};
// launches: {first, count, lds_bytes, global} each; returns 0, or 1 where a capacity is too small
extern "C" int plan_shim(const int *levels, int n_species, long long n_shells, long long threshold, int cap, int *list, long long *slab,
                         long long *launches, long long *out)
{
    const nlte::LaunchPlan p = nlte::plan_launches(std::vector<int>(levels, levels + n_species), n_shells, threshold);
    if ((int)p.list.size() > cap || (int)p.launches.size() > cap || p.slab.size() != p.list.size()) return 1;
    for (size_t i = 0; i < p.list.size(); ++i) { list[i] = p.list[i]; slab[i] = p.slab[i]; }
    for (size_t i = 0; i < p.launches.size(); ++i) {
        launches[4 * i] = p.launches[i].first; launches[4 * i + 1] = p.launches[i].count;
        launches[4 * i + 2] = (long long)p.launches[i].lds_bytes; launches[4 * i + 3] = p.launches[i].global;
    }
    out[0] = (long long)p.list.size(); out[1] = (long long)p.launches.size(); out[2] = p.scratch_doubles; out[3] = (long long)p.max_lds_bytes;
    out[4] = p.refused; out[5] = p.refused_bytes; out[6] = p.refused_before_bytes;
    return 0;
}
"""

COUNTS = [3, 142, 40, 8, 9, 200, 141]
MAX_SCRATCH_BYTES = 1 << 30


def work_bytes(n):
    """The header's working set: the matrix of leading dimension n | 1 and the four vectors b, l, pivots, x."""
    return 8 * ((n | 1) * n + 4 * n)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("nlte_plan")
    src = d / "nlte_plan_shim.cpp"
    src.write_text(SHIM)
    so = d / "nlte_plan_shim.so"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)], check=True)
    f = ctypes.CDLL(str(so)).plan_shim
    ll = ctypes.c_longlong
    f.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ll, ll, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ll), ctypes.POINTER(ll),
                  ctypes.POINTER(ll)]
    f.restype = ctypes.c_int

    def call(levels, n_shells, threshold=-1):
        cap = len(levels) + 8
        c_levels = (ctypes.c_int * max(1, len(levels)))(*levels)
        lst, slab, launches, out = (ctypes.c_int * cap)(), (ll * cap)(), (ll * (4 * cap))(), (ll * 7)()
        assert f(c_levels, len(levels), n_shells, threshold, cap, lst, slab, launches, out) == 0
        n, m = out[0], out[1]
        return dict(list=list(lst[:n]), slab=list(slab[:n]), launches=[tuple(launches[4 * i:4 * i + 4]) for i in range(m)], scratch_doubles=out[2],
                    max_lds_bytes=out[3], refused=out[4], refused_bytes=out[5], refused_before_bytes=out[6])

    return call


def test_header_is_free_of_hip():
    text = open(os.path.join(CSRC, "nlte_plan.hpp")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert all(inc.startswith("<") for inc in includes), includes
    assert "__global__" not in text and "__device__" not in text and "hipError_t" not in text


def test_the_rule_classes_then_the_global_form(plan):
    """3 and 8 levels share the class of up to 8, 9 falls into that of up to 16, 40 into that of up to 64, 141 into the last; 142 and 200
    take the global form, a slab of work_bytes per shell each: 2 x 166 992 B = 41 748 doubles, then 2 x 328 000 B = 82 000."""
    assert [work_bytes(n) for n in (8, 9, 40, 141, 142, 200)] == [832, 936, 14400, 163560, 166992, 328000]
    p = plan(COUNTS, 2)
    assert p["refused"] == -1
    assert p["list"] == [0, 3, 4, 2, 6, 1, 5]
    assert p["slab"] == [0, 0, 0, 0, 0, 0, 41748]
    assert p["launches"] == [(0, 2, 832, 0), (2, 1, 936, 0), (3, 1, 14400, 0), (4, 1, 163560, 0), (5, 2, 0, 1)]
    assert p["scratch_doubles"] == 123748 == 2 * (166992 + 328000) // 8
    assert p["max_lds_bytes"] == 163560


def test_a_threshold_of_nine_levels(plan):
    """Species of 9 levels and more go to the global form, in index order: 142, 40, 9, 200, 141.  Only the class of up to 8 is left."""
    p = plan(COUNTS, 2, 9)
    assert p["refused"] == -1
    assert p["list"] == [0, 3, 1, 2, 4, 5, 6]
    sizes = [2 * work_bytes(n) // 8 for n in (142, 40, 9, 200, 141)]
    assert p["slab"] == [0, 0] + [sum(sizes[:i]) for i in range(5)]
    assert p["launches"] == [(0, 2, 832, 0), (2, 5, 0, 1)]
    assert p["scratch_doubles"] == sum(sizes)
    assert p["max_lds_bytes"] == 832


def test_a_threshold_cannot_put_a_species_into_lds_that_does_not_fit(plan):
    p = plan([142, 141], 3, 1000)
    assert p["list"] == [1, 0] and p["launches"] == [(0, 1, 163560, 0), (1, 1, 0, 1)] and p["slab"] == [0, 0]
    assert p["scratch_doubles"] == 3 * 166992 // 8


def test_no_species_no_launch(plan):
    p = plan([], 20)
    assert p["list"] == [] and p["slab"] == [] and p["launches"] == []
    assert p["scratch_doubles"] == 0 and p["max_lds_bytes"] == 0 and p["refused"] == -1


def test_the_scratch_bound(plan):
    """1071 levels: 8 x (1071 x 1071 + 4 x 1071) = 9 210 600 bytes per shell; 116 shells stay below 2^30 = 1 073 741 824, 117 do not."""
    assert work_bytes(1071) == 9210600 and 116 * 9210600 == 1068429600 < MAX_SCRATCH_BYTES < 117 * 9210600 == 1077640200
    p = plan([1071], 116)
    assert p["refused"] == -1 and p["launches"] == [(0, 1, 0, 1)] and p["list"] == [0] and p["slab"] == [0]
    assert p["scratch_doubles"] == 1068429600 // 8
    p = plan([1071], 117)
    assert p["refused"] == 0 and p["refused_bytes"] == 1077640200 and p["refused_before_bytes"] == 0


def test_the_running_total_refuses_the_species_that_crosses_the_bound(plan):
    """Two species of 1071 levels over 60 shells: 552 636 000 bytes each, the second crosses 2^30 with the first's bytes before it; the
    species of 5 levels between them is no part of the sum."""
    p = plan([1071, 5, 1071], 60)
    assert p["refused"] == 2 and p["refused_bytes"] == 552636000 and p["refused_before_bytes"] == 552636000
