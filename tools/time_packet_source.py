"""Time the device packet source (GPU box): one warm-up call, then the timed calls of one form, each ending in the call's own
stream synchronise.  The kernel's share is read from a kernel trace of the same command (rocprofv3 --kernel-trace --stats in a
run of its own; profiles/relativistic_source.txt).
    python tools/time_packet_source.py simple|relativistic [packets] [calls]
TARDIS_MC_LIB=<an older build> times that build's simple source."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tardis_amd import synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

form = sys.argv[1] if len(sys.argv) > 1 else "simple"
n = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10_000_000
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 5
if form not in ("simple", "relativistic"):
    sys.exit("form: simple | relativistic")
geometry = synthetic.make_geometry()
kw = dict(time_explosion=geometry.time_explosion) if form == "relativistic" else {}
radius = float(geometry.r_inner[0])

with Engine(0) as eng:
    eng.create_blackbody_packets(n, radius, 1.0e4, **kw)  # warm-up: code object, packet buffers
    ms = []
    for it in range(calls):
        t0 = time.perf_counter()
        eng.create_blackbody_packets(n, radius, 1.0e4, seed_offset=it + 1, **kw)
        ms.append(1e3 * (time.perf_counter() - t0))
    mus = eng.get_packets()["initial_mus"]
print(f"{form} n={n} calls={calls} median_ms={statistics.median(ms):.3f} min_ms={min(ms):.3f} max_ms={max(ms):.3f} "
      f"mean_mu={mus.mean():.6f} lib={os.environ.get('TARDIS_MC_LIB', 'in-tree')}", flush=True)
