"""Cost of the collisional rates in the NLTE excitation stage, on the GPU: tardis_mc_update_plasma with NLTE data installed, without and
with dense collision data on the same species (every level pair of every NLTE species; synthetic.make_nlte_collision_data).  Shapes, species
and method are those of tools/time_nlte_excitation.py (its SHAPES and its choice of three NLTE species are imported): one process per arm
(the parent starts them one after the other and never opens the GPU itself), in each one warm-up call, then the median of --reps timed
calls.  Arms: "radiative" (no collision data: the parent commit's stage) and "collisional".  Each arm times the three species together
(assemble_ms: the rates kernel and, in the second arm, the collision kernel; solve_ms: the (species, shell) workgroups with the added
assembly phase) and then every species that fits the LDS alone, which is where an added phase would show against a short elimination.
Usage: python tools/time_nlte_collisions.py [--reps 5] [--shapes config2,tardis_example] [--max-levels 1200]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import time_nlte_excitation as base  # noqa: E402  (puts the repository and tests/ on sys.path)

from tardis_amd import synthetic  # noqa: E402

ARMS = ("radiative", "collisional")


def arm(name, which, reps, max_levels):
    from tardis_amd.engine import Engine

    kw = base.SHAPES[name]
    S = 20
    prob = synthetic.make_problem(seed=1, n_packets=16, n_shells=S, line_interaction_type="macroatom", n_lines=kw["n_lines"],
                                  level_sizes=kw["level_sizes"])
    ld = synthetic.make_line_data(1, prob.opacity_state, level_sizes=kw["level_sizes"], time_explosion=prob.time_explosion)
    pd = synthetic.make_plasma_data(1, ld, S, n_elements=8, largest_ion=kw["largest_ion"])
    ld = synthetic.lines_within_ions(1, ld, pd)
    levels = np.diff(pd.ion_level_edge)
    fits = np.flatnonzero((base.work_bytes(levels) * S <= base.SCRATCH_CAP // 2) & (levels <= max_levels))
    species = sorted({int(np.argmin(np.abs(levels - t) + (levels < 2) * 1e9)) for t in (16, 100)} | {int(fits[np.argmax(levels[fits])])})
    out = {"nlte_species_levels": [int(levels[i]) for i in species]}
    with Engine(0) as eng:
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_line_data(ld)
        eng.set_plasma_data(pd)

        def install(ions):
            nd = synthetic.make_nlte_data(1, ld, pd, species=ions)
            eng.set_nlte_data(nd)
            if which == "collisional":  # (the electron temperatures of the shape lie inside the default grid, 2000 K .. 40000 K)
                cd = synthetic.make_nlte_collision_data(1, pd, nd, pair_fraction=1.0)
                eng.set_nlte_collision_data(cd)
                return int(len(nd.line_id)), int(len(cd.level_lower))
            return int(len(nd.line_id)), 0

        def timed(label):
            times = []
            for r in range(reps + 1):  # (rep 0: warm-up)
                t0 = time.perf_counter()
                eng.update_plasma(pd.t_radiative, pd.dilution_factor)
                t = dict(wall_ms=(time.perf_counter() - t0) * 1e3, device_ms=eng.last_propagate_ms(), **eng.last_nlte_ms(), **eng.last_plasma_update_ms())
                if r:
                    times.append(t)
                print(f"{name} {which} {label:>8} rep {r}: " + "  ".join(f"{k} {v:9.3f}" for k, v in t.items()), flush=True)
            return {k: base.median([t[k] for t in times]) for k in times[0]}

        out["nlte_lines"], out["pairs"] = install(species)
        out["together"] = timed("all")
        out["alone"] = {}
        for i in species:
            if levels[i] > base.LARGEST_LDS_LEVELS:
                continue
            lines, pairs = install([i])
            out["alone"][str(int(levels[i]))] = dict(timed(f"n={int(levels[i])}"), nlte_lines=lines, pairs=pairs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="config2,tardis_example")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--max-levels", type=int, default=1200, help="the longest NLTE species taken, as in tools/time_nlte_excitation.py")
    ap.add_argument("--arm", choices=ARMS, help="run one arm in this process (the parent passes it)")
    args = ap.parse_args()
    if args.arm:
        print(json.dumps({name: arm(name, args.arm, args.reps, args.max_levels) for name in args.shapes.split(",")}))
        return
    out = {}
    for which in args.arms.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", which, "--reps", str(args.reps), "--shapes", args.shapes, "--max-levels",
               str(args.max_levels)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True)
        sys.stdout.write(r.stdout)
        out[which] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
