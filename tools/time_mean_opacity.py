"""Cost of the mean opacities and optical depths of an outer iteration, on the GPU: tardis_mc_mean_opacity (S temperatures in, four
vectors of S doubles out, the resident tau_sobolev read where it is) against the path it replaces for the same four vectors -- the
download of tau_sobolev [L,S] (get_opacity) plus the host pass over it (the restatement tests/mean_opacity_ref.py with libm exp).
Per shape: bin_ms and reduce_ms of the call, its wall time, and the two parts of the host path.  Then the shell reduction alone in both
forms (option mean_opacity_long_bins) at bin counts from 4 to the shape's own, reached through the bin size: the figures behind
mopl::LONG_BINS (csrc/mean_opacity_plan.hpp).
Shapes: the configs[2] tables (5e5 lines, 20 shells) and the tardis_example shape (3e4 lines, 20 shells).
One warm-up call, then the median of --reps timed calls.  Prints one line per timed call and a JSON summary.
Usage: python tools/time_mean_opacity.py [--reps 7] [--shapes config2,tardis_example] [--bins 4,8,12,16,24,32,64,256,1024]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tardis_amd import synthetic  # noqa: E402

SHAPES = {"config2": 500_000, "tardis_example": 30_000}
ALL_LANE, ALL_ROW = 1 << 60, 0


def median(ts):
    return round(statistics.median(ts), 4)


def timed(fn, reps, label):
    rows = []
    for r in range(reps + 1):  # (rep 0: warm-up)
        t = fn()
        if r:
            rows.append(t)
        print(f"{label} rep {r}: " + "  ".join(f"{k} {v:9.4f}" for k, v in t.items()), flush=True)
    return {k: median([t[k] for t in rows]) for k in rows[0]}


def shape(name, reps, bin_counts):
    import mean_opacity_ref as ref
    from tardis_amd.engine import Engine

    L = SHAPES[name]
    prob = synthetic.make_problem(seed=1, n_packets=16, n_shells=20, line_interaction_type="scatter", n_lines=L, log_tau_mean=-2.0)
    geo, op = prob.geometry, prob.opacity_state
    t_rad = np.linspace(12000.0, 7000.0, 20)
    m = 10
    while Engine.mean_opacity_bins(op.line_list_nu, m)[1] >= 0:
        m += 1
    out = {"lines": L, "shells": 20, "bin_size": m}
    with Engine(0) as eng:
        eng.set_geometry(geo, prob.time_explosion)
        eng.set_opacity(op)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)

        def device(size=m):
            t0 = time.perf_counter()
            res = eng.mean_opacity(t_rad, size)
            wall = (time.perf_counter() - t0) * 1e3
            return res, dict(wall_ms=wall, device_ms=eng.last_propagate_ms(), **eng.last_mean_opacity_ms())

        def host():
            t0 = time.perf_counter()
            tau = eng.get_opacity(tau_sobolev=True, transition_probabilities=False)["tau_sobolev"]
            t1 = time.perf_counter()
            ref.mean_opacity(op.line_list_nu, tau, op.electron_density, geo.r_inner, geo.r_outer, prob.time_explosion, t_rad, m, exp=np.exp)
            t2 = time.perf_counter()
            return dict(wall_ms=(t2 - t0) * 1e3, download_ms=(t1 - t0) * 1e3, host_pass_ms=(t2 - t1) * 1e3)

        res, _ = device()
        out["n_bins"] = int(res["n_bins"])
        out["form"] = Engine.mean_opacity_path(out["n_bins"])
        want = ref.mean_opacity(op.line_list_nu, op.tau_sobolev, op.electron_density, geo.r_inner, geo.r_outer, prob.time_explosion, t_rad, m)
        out["equals_restatement"] = bool(all(np.array_equal(res[k], want[k]) for k in ("kappa_planck", "kappa_rosseland", "tau_planck", "tau_rosseland")))
        out["tau_rosseland_inner"], out["tau_planck_inner"] = float(res["tau_rosseland"][0]), float(res["tau_planck"][0])
        out["device"] = timed(lambda: device()[1], reps, f"{name} device")
        out["host"] = timed(host, reps, f"{name}   host")
        # the reduction alone, both forms, at bin counts reached through the bin size (the bin kernel's time changes with it, reduce_ms does not)
        forms = {}
        for n in sorted(set(bin_counts + [out["n_bins"]])):
            size = m if n == out["n_bins"] else max(1, -(-L // n))
            n_got, first = Engine.mean_opacity_bins(op.line_list_nu, size)
            if n_got < 0:
                continue
            row = {"bin_size": size}
            for form, threshold in (("lane", ALL_LANE), ("row", ALL_ROW)):
                eng.set_option("mean_opacity_long_bins", threshold)
                row[form + "_reduce_ms"] = timed(lambda: device(size)[1], reps, f"{name} {n_got:6d} bins {form}")["reduce_ms"]
            forms[str(n_got)] = row
        eng.set_option("mean_opacity_long_bins", -1)
        out["reduce_ms_by_bins"] = forms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="config2,tardis_example")
    ap.add_argument("--bins", default="4,8,12,16,24,32,64,256,1024")
    args = ap.parse_args()
    bins = [int(b) for b in args.bins.split(",")]
    print(json.dumps({name: shape(name, args.reps, bins) for name in args.shapes.split(",")}))


if __name__ == "__main__":
    main()
