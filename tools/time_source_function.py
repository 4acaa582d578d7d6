"""Device time of the source function of the formal integral (tardis_mc_source_function) and of the resident formal integral
after it, beside the host route they replace: the download of the [L,S] j_blue / Edotlu estimators, the numpy / scipy fixed-point
restatement of make_source_function (tests/source_function_ref.py, shells solved on --threads threads) and the formal integral fed
from the host (three [S*L] uploads).  Shapes: configs[1] (3e4 lines, downbranch) and configs[2] (5e5 lines, macroatom, heavy-tailed
levels).  Protocol of DESIGN.md 7b: one warm-up, then the device and the host route alternated --repeats times; medians.

    python tools/time_source_function.py [--shapes 1 2] [--packets 100000] [--repeats 3] [--threads 16] [--frequencies 2000]
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

import source_function_ref as ref  # noqa: E402
from tardis_amd import synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

SHAPES = {
    1: dict(n_lines=30_000, line_interaction_type="downbranch"),
    2: dict(n_lines=500_000, line_interaction_type="macroatom", level_sizes="heavy"),
}


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--packets", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--frequencies", type=int, default=2000)
    ap.add_argument("--impact-parameters", type=int, default=1000)
    args = ap.parse_args()
    med = statistics.median
    with Engine(0) as eng:
        for shape in args.shapes:
            kw = SHAPES[shape]
            prob = synthetic.make_problem(seed=1, n_packets=args.packets, n_shells=20, **kw)
            op, geo, tsim = prob.opacity_state, prob.geometry, prob.packet_collection.time_of_simulation
            eng.set_geometry(geo, prob.time_explosion)
            eng.set_opacity(op)
            eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
            eng.set_packets(prob.packet_collection)
            eng.reset_estimators()
            eng.propagate()
            eng.synchronize()
            nu = op.line_list_nu
            freqs = np.linspace(nu[-1] * 1.05, nu[0] * 0.95, args.frequencies)
            solver = "none" if kw["line_interaction_type"] == "downbranch" else "fixed_point"
            rows = {k: [] for k in ("source_ms", "source_wall_ms", "resident_integral_ms", "resident_integral_wall_ms", "download_wall_ms",
                                    "host_source_wall_ms", "host_fed_integral_ms", "host_fed_integral_wall_ms")}
            host = None
            for rep in range(args.repeats + 1):  # (the first round warms up)
                _, w = wall(lambda: eng.source_function(tsim, geo.volume, want_arrays=False))
                r = {"source_wall_ms": w, "source_ms": eng.last_propagate_ms()}
                (lum_r, _), w = wall(lambda: eng.formal_integral_resident(1.0e4, freqs, args.impact_parameters))
                r.update(resident_integral_wall_ms=w, resident_integral_ms=eng.last_propagate_ms())
                res, w = wall(lambda: eng.get_results(track_last_interaction=False, want_packet_outputs=False))
                r["download_wall_ms"] = w
                host, w = wall(lambda: ref.make_source_function(op, res.j_blue_estimator, res.edotlu_estimator, tsim, geo.volume,
                                                                prob.time_explosion, solver=solver, threads=args.threads))
                r["host_source_wall_ms"] = w
                (lum_h, _), w = wall(lambda: eng.formal_integral(1.0e4, freqs, host["att_S_ul"], host["Jred_lu"], host["Jblue_lu"],
                                                                 args.impact_parameters))
                r.update(host_fed_integral_wall_ms=w, host_fed_integral_ms=eng.last_propagate_ms())
                if rep:
                    for k, v in r.items():
                        rows[k].append(v)
            out = {"shape": shape, "lines": kw["n_lines"], "mode": kw["line_interaction_type"], "packets": args.packets,
                   "frequencies": args.frequencies, "impact_parameters": args.impact_parameters, "threads": args.threads,
                   "iterations_device": eng.last_source_iterations(),
                   "iterations_host_max": max(host["iterations"]) if host["iterations"] else 0,
                   "spectrum_max_rel_diff": float(np.abs(lum_r - lum_h).max() / np.abs(lum_h).max())}
            out.update({k: med(v) for k, v in rows.items()})
            out["device_route_wall_ms"] = out["source_wall_ms"] + out["resident_integral_wall_ms"]
            out["host_route_wall_ms"] = out["download_wall_ms"] + out["host_source_wall_ms"] + out["host_fed_integral_wall_ms"]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
