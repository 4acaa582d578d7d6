"""Device time of the last-interaction decomposition (tardis_mc_packet_decomposition) beside the host route it replaces: the
download of the per-packet outputs and the fourteen tracker arrays (get_results) and the numpy reduction over them -- both the
numpy implementation of tardis_amd.spectrum and the tests' yardstick (math.fsum per cell).  Shape: configs[2] tables (20 shells,
5e5 lines, macroatom, heavy-tailed levels), packets from the device packet source, C classes x B bins.  The device call is
repeated --repeats times after a warm-up (median, minimum, maximum), for the direct path (C x B as given) and for a shape that
takes the privatised path (--private-classes x --private-bins); the streaming copy of tardis_mc_debug_microbench 15 is measured in
the same process.

    python tools/time_packet_decomposition.py [--packets 10000000] [--lines 500000] [--classes 30] [--bins 10000] [--repeats 5]
                                              [--private-classes 3] [--private-bins 1000] [--skip-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tardis_amd import spectrum, state as st, synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=10_000_000)
    ap.add_argument("--lines", type=int, default=500_000)
    ap.add_argument("--classes", type=int, default=30)
    ap.add_argument("--bins", type=int, default=10_000)
    ap.add_argument("--private-classes", type=int, default=3)
    ap.add_argument("--private-bins", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    S, P, L = 20, args.packets, args.lines
    spread = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    prob = synthetic.make_problem(seed=1, n_packets=16, n_shells=S, n_lines=L, line_interaction_type="macroatom", level_sizes="heavy",
                                  n_bins=args.bins)
    radius, t_inner = float(prob.geometry.r_inner[0]), 1.0e4
    t_sim = 1.0 / (4 * np.pi * st.SIGMA_SB * radius**2 * t_inner**4)
    out = {"packets": P, "lines": L, "shells": S, "repeats": args.repeats}
    with Engine(0) as eng:
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        grids = {"direct": (args.classes, args.bins), "privatised": (args.private_classes, args.private_bins)}
        for name, (C, B) in grids.items():
            assert eng.decomposition_path(C, B, S) == name, (name, C, B)
            eng.set_config(prob.montecarlo_configuration, synthetic.make_spectrum_grid(B))
            eng.create_blackbody_packets(P, radius, t_inner)
            eng.reset_estimators()
            eng.propagate()
            eng.synchronize()
            propagate_ms = eng.last_propagate_ms()
            cls = (np.arange(L) * 7919 % C).astype(np.int64)
            ms, walls = [], []
            for rep in range(args.repeats + 1):  # (the first call warms up)
                dec, w = wall(lambda: eng.packet_decomposition(t_sim, cls, C))
                if rep:
                    ms.append(eng.last_propagate_ms())
                    walls.append(w)
            row = {"classes": C, "bins": B, "propagate_ms": propagate_ms, "device_ms": spread(ms), "wall_ms": spread(walls),
                   "bytes_per_packet": 56, "streamed_TB_per_s": 56.0 * P / (statistics.median(ms) * 1e-3) / 1e12,
                   "n_selected": dec["n_selected"], "n_line": dec["n_line"]}
            if name == "direct" and not args.skip_host:
                res, row["host_get_results_wall_ms"] = wall(lambda: eng.get_results(want_line_estimators=False))
                t = res.trackers
                host, row["host_numpy_wall_ms"] = wall(lambda: spectrum.packet_decomposition(
                    res.output_nus, res.output_energies, t_sim, synthetic.make_spectrum_grid(B), t.interaction_type, t.interaction_line_emit_id,
                    t.interaction_line_absorb_id, t.before_nu, t.shell_id, cls, S, C))
                import packet_decomposition_ref as ref
                (want, n), row["host_yardstick_wall_ms"] = wall(lambda: ref.decompose(
                    res.output_nus, res.output_energies, t_sim, synthetic.make_spectrum_grid(B), t, cls, C, S))
                ref.assert_matches(dec, want, n, "device")
                ref.assert_matches(host, want, n, "host numpy")
                row["device_within_bound_of_yardstick"] = True
            out[name] = row
            print(name, json.dumps(row), file=sys.stderr, flush=True)
        n_doubles, iters = 1 << 28, 4  # (bench.py's measured_stream_peak: the best of three grids)
        copy_ms = [min(eng.debug_microbench(15, n_doubles, iters, blocks) for blocks in (4096, 16384, 65536)) for _ in range(3)]
        out["stream_copy_TB_per_s"] = n_doubles * 8.0 * iters / (statistics.median(copy_ms) * 1e-3) / 1e12
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
