"""The packed word of the deferred last-interaction record (csrc/mc_device.hpp: tracker_pack / tracker_unpack / tracker_pack_fits), on the host.

A small stand-alone program, compiled for the host only, packs and unpacks every combination of the edge values of the four fields -- both
interaction types, shells 0 and 2^15 - 1, line ids -1 ("no line"), 0 and 2^24 - 2 (the last line of the longest list that fits) -- and checks the
bounds tracker_pack_fits draws.  No GPU is needed: the functions are __host__ __device__ and the kernel uses the same source.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tardis_amd", "csrc")

PROGRAM = r"""
#include "mc_device.hpp"
#include <cstdio>
int main()
{
    using namespace mc;
    static_assert(tracker_pack_fits(1 << 15, (1 << 24) - 1), "the widest problem that fits");
    static_assert(!tracker_pack_fits((1 << 15) + 1, 10) && !tracker_pack_fits(20, 1 << 24), "one shell / one line more does not");
    static_assert(tracker_pack_fits(20, 500000), "the headline");
    const int shells[] = {0, 1, 19, (1 << 15) - 1}, lines[] = {-1, 0, 1, 499999, (1 << 24) - 3, (1 << 24) - 2};
    long n = 0, bad = 0;
    for (int type : {(int)IT_LINE, (int)IT_ESCATTERING})
        for (int s : shells)
            for (int a : lines)
                for (int e : lines) {
                    int t2 = 0, s2 = -7, a2 = -7, e2 = -7;
                    tracker_unpack(tracker_pack(type, s, a, e), t2, s2, a2, e2);
                    bad += !(t2 == type && s2 == s && a2 == a && e2 == e);
                    ++n;
                }
    // the fields do not overlap: each one alone sets only its own bits
    bad += (tracker_pack(IT_ESCATTERING, (1 << 15) - 1, -1, -1) != 0xfffeull);
    bad += (tracker_pack(IT_LINE, 0, -1, -1) != 1ull);
    bad += (tracker_pack(IT_ESCATTERING, 0, (1 << 24) - 2, -1) != (0xffffffull << 16));
    bad += (tracker_pack(IT_ESCATTERING, 0, -1, (1 << 24) - 2) != (0xffffffull << 40));
    std::printf("%ld round trips, %ld bad\n", n, bad);
    return bad != 0;
}
"""


def test_pack_unpack_round_trip_and_bounds(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "tracker_pack.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "tracker_pack"
    subprocess.run([hipcc, "--offload-host-only", "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("288 round trips, 0 bad"), r.stdout
