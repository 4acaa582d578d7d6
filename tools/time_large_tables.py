"""Cost of the 64-bit table offsets (option table_offsets), on the GPU, in one process with the runs alternated:
  (a) the configs[4] table shape (100 shells, 5e5 lines, macroatom, heavy blocks), 0 and 10 v-packets: 32-bit offsets, 32-bit offsets without the
      interleaved sweep table (option sweep_table 0: the 64-bit forms never read it), and forced 64-bit offsets;
  (b) a 200-shell x 5e5-line macroatom model (S x T over 2^28): the automatic choice (64-bit) vs variant 0.
Every arm runs the same lane-sweep shape (option ls_waves_per_simd, --ls, default 4): left automatic, the engine's tuner would time the arms
of one table shape as one key and hand them different kernels.  Prints one line per timed call (propagate + synchronize) and a JSON summary.
Usage: python tools/time_large_tables.py [--packets N] [--vpk-packets N] [--reps R] [--ls 3|4] [--legs a0,a10,b]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tardis_amd import synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

DEFAULTS = {"variant": -1, "table_offsets": -1, "sweep_table": -1}


def leg(eng, name, shells, n_vpackets, packets, reps, arms):
    prob = synthetic.make_problem(seed=1, n_packets=packets, n_shells=shells, n_lines=500_000, line_interaction_type="macroatom",
                                  n_vpackets=n_vpackets, n_bins=10_000, level_sizes="heavy", shell_independent_probabilities=True)
    eng.set_geometry(prob.geometry, prob.time_explosion)
    eng.set_opacity(prob.opacity_state)
    eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
    eng.set_packets(prob.packet_collection)
    times = {a: [] for a in arms}
    for r in range(reps + 1):  # (rep 0: warm-up of every arm)
        for arm, opts in arms.items():
            for k, v in opts.items():
                eng.set_option(k, v)
            eng.reset_estimators()
            t0 = time.perf_counter()
            eng.propagate()
            eng.synchronize()
            dt = time.perf_counter() - t0
            info = (eng.last_variant(), eng.last_table_offsets())
            for k in opts:
                eng.set_option(k, DEFAULTS[k])
            if r:
                times[arm].append(dt)
            print(f"{name} {arm:>14} rep {r}: {dt * 1e3:9.1f} ms  {packets / dt / 1e6:7.3f} Mpkt/s  variant {info[0]} offsets {info[1]}", flush=True)
    return {arm: {"ms": [round(t * 1e3, 1) for t in ts], "best_ms": round(min(ts) * 1e3, 1), "mpkt_s": round(packets / min(ts) / 1e6, 3)}
            for arm, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=10_000_000)
    ap.add_argument("--vpk-packets", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--ls", type=int, default=4, choices=(3, 4))
    ap.add_argument("--legs", default="a0,a10,b")
    args = ap.parse_args()
    out = {"ls_waves_per_simd": args.ls}
    with Engine(0) as eng:
        eng.set_option("track_last_interaction", 0)
        eng.set_option("ls_waves_per_simd", args.ls)
        a_arms = {"32-bit": {"table_offsets": 0}, "32-bit no table": {"table_offsets": 0, "sweep_table": 0}, "64-bit": {"table_offsets": 1}}
        legs = args.legs.split(",")
        if "a0" in legs:
            out["a_nv0"] = leg(eng, "a nv0", 100, 0, args.packets, args.reps, a_arms)
        if "a10" in legs:  # (v-packet calls run the group sweeps: no sweep table either way)
            out["a_nv10"] = leg(eng, "a nv10", 100, 10, args.vpk_packets, args.reps, {k: a_arms[k] for k in ("32-bit", "64-bit")})
        if "b" in legs:
            out["b_200"] = leg(eng, "b 200sh", 200, 0, args.packets, args.reps, {"auto": {}, "variant0": {"variant": 0}})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
