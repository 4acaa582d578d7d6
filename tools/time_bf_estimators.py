"""Device time of the photo-ionisation estimators (option bf_estimators) on the configs[2] tables (20 shells x 5e5 lines, macroatom, heavy-tailed
levels): the propagate call on the wave-owner kernel with group sweeps (variant 2) without and with the segment log, the records per packet, and
the accumulate pass behind the call -- grouping the record slots by shell, accumulating -- for NC continua of 16 points each laid over the
packets' comoving frequencies.  For comparison the automatic variant (the production lane sweeps) with the option off.

    python tools/time_bf_estimators.py [--packets 1000000] [--continua 16 1024] [--repeats 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tardis_amd import synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402


def propagate_ms(eng, repeats):
    ms = []
    for _ in range(repeats + 1):  # (the first call warms up)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        ms.append(eng.last_propagate_ms())
    return ms[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--continua", type=int, nargs="+", default=[16, 1024])
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    shape = dict(synthetic.BASELINE_CONFIGS[3], n_packets=args.packets, level_sizes="heavy")
    prob = synthetic.make_problem(seed=1, **shape)
    S = len(prob.geometry.r_inner)
    ld = synthetic.make_line_data(1, prob.opacity_state, time_explosion=prob.time_explosion)
    pd = synthetic.make_plasma_data(1, ld, S)
    lo, hi = synthetic.comoving_frequency_range(prob)
    t_e = np.linspace(11000.0, 7000.0, S)
    rng = np.random.default_rng(1)
    with Engine(0) as eng:
        for nc in args.continua:
            blocks = []
            for _ in range(nc):
                a = np.exp(rng.uniform(np.log(lo), np.log(hi / 1.5)))
                grid = np.geomspace(a, min(hi, a * rng.uniform(1.5, 6.0)), 16)
                blocks.append((grid, 6.3e-18 * (grid[0] / grid) ** 3))
            cd = synthetic.make_covering_continuum_data(pd, blocks)
            eng.set_geometry(prob.geometry, prob.time_explosion)
            eng.set_opacity(prob.opacity_state)
            eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
            eng.set_line_data(ld)
            eng.set_plasma_data(pd)
            eng.set_continuum_data(cd)
            eng.set_bf_estimators(t_e)
            eng.set_packets(prob.packet_collection)
            row = {"packets": args.packets, "continua": nc, "points": int(cd.block_edge[-1])}
            eng.set_option("variant", -1)
            row["auto_off_ms"] = propagate_ms(eng, args.repeats)
            row["auto_off_variant"] = eng.last_variant()
            eng.set_option("variant", 2)
            row["v2_off_ms"] = propagate_ms(eng, args.repeats)
            eng.set_option("bf_estimators", 1)
            try:
                row["v2_on_ms"] = propagate_ms(eng, args.repeats)
                row["v2_on_variant"] = eng.last_variant()
                row.update(eng.last_bf_estimator_ms())
                t = eng.get_bf_estimators()
            finally:
                eng.set_option("bf_estimators", 0)
                eng.set_option("variant", -1)
            row["records_per_packet"] = t["n_records"] / args.packets
            row["terms_per_record"] = float(t["statistics"].sum()) / t["n_records"]
            row["pass_over_propagate"] = (row["group_ms"] + row["accumulate_ms"]) / min(row["v2_on_ms"])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
