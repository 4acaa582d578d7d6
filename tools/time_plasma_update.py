"""Cost of the plasma step of an outer iteration, on the GPU: tardis_mc_update_plasma (two [S] vectors in, populations and the opacity
state computed on the device) against the path it replaces for the same state -- the populations solved on the host (the NumPy
restatement tests/plasma_update_ref.py, itself far cheaper than the pandas plasma it restates) plus tardis_mc_update_opacity with its
[K,S] upload and transpose.  Per-stage device times of the update: Boltzmann factors, partition functions, phi and the electron-density
iteration, populations, then the three stages of the opacity update; and the partition kernel alone with every ion on a 16-lane row,
every ion on one lane, and at thresholds in between (option plasma_update_long_rows).
Shapes: the configs[2] tables (5e5 lines, 5e4 levels, 20 shells) and the tardis_example shape (3e4 lines, 3e3 levels, 20 shells).
One process per arm (the parent starts them one after the other and never opens the GPU itself); in it one warm-up call, then the
median of --reps timed calls.  Prints one line per timed call and a JSON summary.
--helium: the arms of profiles/helium_treatment.txt instead -- on plasma data with a helium element in front (He I 50 levels, He II 30,
He III 1: synthetic.make_helium_plasma_data) update_plasma with no options installed ("plain") and with helium_treatment recomb-nlte
("helium"), the stage times with last_helium_ms beside them; no thresholds, no host arm.
Usage: python tools/time_plasma_update.py [--reps 5] [--shapes config2,tardis_example] [--thresholds 0,4,8,16,32,64,-2] [--helium]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tardis_amd import synthetic  # noqa: E402

SHAPES = {
    "config2": dict(n_lines=500_000, level_sizes="heavy", largest_ion=5000),
    "tardis_example": dict(n_lines=30_000, level_sizes="uniform", largest_ion=400),
}
STAGES = ("boltzmann_ms", "partition_ms", "ionization_ms", "population_ms", "line_ms", "block_ms", "derive_ms")
ALL_LANE = 1 << 40  # no ion has that many levels: every ion takes the lane form
HELIUM_LEVELS = (50, 30)  # He I, He II of the --helium arms (He III: one level)


def median(ts):
    return round(statistics.median(ts), 3)


def arm(name, which, reps, thresholds):
    import plasma_update_ref as ref
    from tardis_amd.engine import Engine

    kw = SHAPES[name]
    prob = synthetic.make_problem(seed=1, n_packets=16, n_shells=20, line_interaction_type="macroatom", n_lines=kw["n_lines"],
                                  level_sizes=kw["level_sizes"])
    ld = synthetic.make_line_data(1, prob.opacity_state, level_sizes=kw["level_sizes"], time_explosion=prob.time_explosion)
    if which in ("plain", "helium"):
        pd = synthetic.make_helium_plasma_data(1, ld, 20, helium_levels=HELIUM_LEVELS, n_elements=8, largest_ion=kw["largest_ion"])
    else:
        pd = synthetic.make_plasma_data(1, ld, 20, n_elements=8, largest_ion=kw["largest_ion"])
    levels = np.diff(pd.ion_level_edge)
    out = {"lines": int(kw["n_lines"]), "levels": int(ld.n_levels), "ions": int(len(levels)), "longest_ion": int(levels.max()),
           "ions_ge_8_levels": int((levels >= 8).sum())}
    with Engine(0) as eng:
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_line_data(ld)
        eng.set_plasma_data(pd)
        if which == "helium":
            eng.set_ionization_options("recomb-nlte")
            out["helium_levels"] = int(eng.n_helium_levels)

        def device():
            t0 = time.perf_counter()
            eng.update_plasma(pd.t_radiative, pd.dilution_factor)
            wall = (time.perf_counter() - t0) * 1e3
            extra = dict(helium_relative_ms=eng.last_helium_ms()["relative_ms"]) if which == "helium" else {}
            return dict(wall_ms=wall, device_ms=eng.last_propagate_ms(), **eng.last_plasma_update_ms(), **extra)

        def host():
            t0 = time.perf_counter()
            sol = ref.solve(pd, pd.t_radiative, pd.dilution_factor)
            t1 = time.perf_counter()
            eng.update_opacity(sol["level_number_density"], sol["electron_density"], 0, t_radiative=pd.t_radiative,
                               dilution_factor=pd.dilution_factor)
            t2 = time.perf_counter()
            return dict(wall_ms=(t2 - t0) * 1e3, host_solve_ms=(t1 - t0) * 1e3, update_opacity_wall_ms=(t2 - t1) * 1e3,
                        device_ms=eng.last_propagate_ms(), **eng.last_opacity_update_ms())

        fn = host if which == "host" else device
        times = []
        for r in range(reps + 1):  # (rep 0: warm-up)
            t = fn()
            if r:
                times.append(t)
            print(f"{name} {which:>6} rep {r}: " + "  ".join(f"{k} {v:9.3f}" for k, v in t.items()), flush=True)
        for k in times[0]:
            out[k] = median([t[k] for t in times])
        if which in ("plain", "helium"):
            out["iterations"] = eng.get_plasma(False, False, False, False)["iterations"]
            out["ionization_ms_reps"] = [round(t["ionization_ms"], 4) for t in times]
        if which == "device":
            out["iterations"] = eng.get_plasma(False, False, False, False)["iterations"]
            part = {t: [] for t in thresholds}
            for r in range(reps + 1):
                for t in thresholds:
                    eng.set_option("plasma_update_long_rows", ALL_LANE if t == -2 else t)
                    ms = device()["partition_ms"]
                    if r:
                        part[t].append(ms)
            eng.set_option("plasma_update_long_rows", -1)
            out["partition_ms_by_threshold"] = {("all_lane" if t == -2 else "all_row" if t == 0 else str(t)): median(v) for t, v in part.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="config2,tardis_example")
    ap.add_argument("--thresholds", default="0,4,8,16,32,64,-2")
    ap.add_argument("--helium", action="store_true", help="the arms 'plain' and 'helium' on plasma data with a helium element")
    ap.add_argument("--arm", choices=("device", "host", "plain", "helium"), help="run one arm in this process (the parent passes it)")
    args = ap.parse_args()
    thresholds = [int(t) for t in args.thresholds.split(",")]
    if args.arm:
        print(json.dumps({name: arm(name, args.arm, args.reps, thresholds) for name in args.shapes.split(",")}))
        return
    out = {}
    for which in (("plain", "helium") if args.helium else ("host", "device")):
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", which, "--reps", str(args.reps), "--shapes", args.shapes, "--thresholds",
               args.thresholds]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True)
        sys.stdout.write(r.stdout)
        out[which] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
