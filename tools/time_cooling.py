"""Cost of the cooling sub-stage behind the continuum stage of tardis_mc_update_plasma, on the GPU: update_plasma with photo-ionisation
data installed ("continuum", which since the sub-stage exists also runs it) against update_plasma without them ("plain") on the same
commit, tables and plasma data.  Per call: the wall time, the sub-stage's three figures (last_cooling_ms: points, blocks, table) beside
the continuum stage's four (last_continuum_ms) and the stages of the rest of the update (last_plasma_update_ms), and one batch of
--queries k-packets (kpacket_sample, wall time with its uploads and downloads).
Shape and protocol: those of tools/time_continuum.py -- the configs[2] tables (5e5 lines, 5e4 levels, 20 shells), the plasma data of
tools/time_plasma_update.py, a synthetic continuum set of --continua levels whose blocks have --points-min .. --points-max points; one
process per arm (the parent starts them one after the other and never opens the GPU itself); in it one warm-up call, then the median
of --reps timed calls.  Prints one line per timed call and a JSON summary; profiles/cooling_rates.txt records a run.
Usage: python tools/time_cooling.py [--reps 5] [--continua 400] [--points-min 20] [--points-max 200] [--queries 100000]"""
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

from tardis_amd import synthetic  # noqa: E402

SHAPE = dict(n_lines=500_000, level_sizes="heavy", largest_ion=5000)  # (configs[2]: tools/time_plasma_update.py's "config2")


def median(ts):
    return round(statistics.median(ts), 4)


def arm(which, args):
    from tardis_amd.engine import Engine

    prob = synthetic.make_problem(seed=1, n_packets=16, n_shells=20, line_interaction_type="macroatom", n_lines=SHAPE["n_lines"],
                                  level_sizes=SHAPE["level_sizes"])
    ld = synthetic.make_line_data(1, prob.opacity_state, level_sizes=SHAPE["level_sizes"], time_explosion=prob.time_explosion)
    pd = synthetic.make_plasma_data(1, ld, 20, n_elements=8, largest_ion=SHAPE["largest_ion"])
    cd = synthetic.make_continuum_data(1, pd, args.continua, points=(args.points_min, args.points_max))
    lengths = np.diff(cd.block_edge)
    out = {"lines": int(SHAPE["n_lines"]), "levels": int(ld.n_levels), "ions": int(len(pd.ion_charge)), "shells": 20, "continua": int(len(cd.level)),
           "points": int(cd.block_edge[-1]), "shortest_block": int(lengths.min()), "longest_block": int(lengths.max())}
    with Engine(0) as eng:
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_line_data(ld)
        eng.set_plasma_data(pd)
        if which == "continuum":
            eng.set_continuum_data(cd)
        rng = np.random.default_rng(7)
        q_shell, q_z, q_z_nu = rng.integers(0, 20, args.queries), rng.random(args.queries), rng.random(args.queries)
        times = []
        for r in range(args.reps + 1):  # (rep 0: warm-up)
            t0 = time.perf_counter()
            eng.update_plasma(pd.t_radiative, pd.dilution_factor)
            eng.synchronize()
            t = dict(wall_ms=(time.perf_counter() - t0) * 1e3, **eng.last_plasma_update_ms())
            if which == "continuum":
                t["continuum_ms"] = sum(eng.last_continuum_ms().values())
                t.update(eng.last_cooling_ms())
                t["cooling_ms"] = sum(eng.last_cooling_ms().values())
                t0 = time.perf_counter()
                got = eng.kpacket_sample(q_shell, q_z, q_z_nu)
                t["sample_wall_ms"] = (time.perf_counter() - t0) * 1e3
            if r:
                times.append(t)
            print(f"{which:>9} rep {r}: " + "  ".join(f"{k} {v:9.4f}" for k, v in t.items()), flush=True)
        for k in times[0]:
            out[k] = median([t[k] for t in times])
        if which == "continuum":
            out["n_degenerate_fb_cdf"] = eng.get_kpacket_tables(fb_emission_cdf=False)["n_degenerate_fb_cdf"]
            out["kinds_sampled"] = np.bincount(got["kind"], minlength=4).tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--continua", type=int, default=400)
    ap.add_argument("--points-min", type=int, default=20)
    ap.add_argument("--points-max", type=int, default=200)
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--arm", choices=("plain", "continuum"), help="run one arm in this process (the parent passes it)")
    args = ap.parse_args()
    if args.arm:
        print(json.dumps(arm(args.arm, args)))
        return
    out = {}
    for which in ("plain", "continuum", "plain", "continuum"):  # interleaved, twice over
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", which, "--reps", str(args.reps), "--continua", str(args.continua), "--points-min",
               str(args.points_min), "--points-max", str(args.points_max), "--queries", str(args.queries)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=240)
        sys.stdout.write(r.stdout)
        out.setdefault(which, []).append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
