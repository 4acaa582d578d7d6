"""Cost of the opacity step of an outer iteration, on the GPU, in one process: tardis_mc_update_opacity (a [K,S] upload, the tables
computed on the device) against tardis_mc_set_opacity of the same tables ([L,S] + [T,S] uploaded, transposed, derived), then the block
kernel alone with the row form forced on, forced off and at thresholds in between (option opacity_update_long_rows).
Shapes: configs[2] (5e5 lines, heavy-tailed blocks, 20 shells, macroatom) and the tardis_example shape (3e4 lines, 20 shells, macroatom).
Every arm is warmed up once, then the timed calls alternate.  Prints one line per timed call and a JSON summary.
Usage: python tools/time_opacity_update.py [--reps R] [--shapes config2,tardis_example] [--thresholds 1,8,16,32,64,128,256,0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tardis_amd import state as st, synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402

SHAPES = {
    "config2": dict(n_lines=500_000, level_sizes="heavy"),
    "tardis_example": dict(n_lines=30_000, level_sizes="uniform"),
}
ALL_LANE = 1 << 40  # no block is that long: every block takes the lane form


def best(ts):
    return round(min(ts), 3)


def shape(eng, name, reps, thresholds):
    kw = SHAPES[name]
    prob = synthetic.make_problem(seed=1, n_packets=16, n_shells=20, line_interaction_type="macroatom", **kw)
    ld = synthetic.make_line_data(1, prob.opacity_state, level_sizes=kw["level_sizes"], time_explosion=prob.time_explosion)
    op = prob.opacity_state
    rows = np.diff(op.macro_block_edge_index)
    eng.set_geometry(prob.geometry, prob.time_explosion)
    eng.set_opacity(op)
    eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
    eng.set_line_data(ld)

    def update():
        t0 = time.perf_counter()
        eng.update_opacity(ld.level_number_density, ld.electron_density, 0, t_radiative=ld.t_radiative, dilution_factor=ld.dilution_factor)
        wall = (time.perf_counter() - t0) * 1e3
        return dict(wall_ms=wall, device_ms=eng.last_propagate_ms(), **eng.last_opacity_update_ms())

    update()
    tables = eng.get_opacity()
    same = st.OpacityState(op.electron_density, op.t_electrons, op.line_list_nu, tables["tau_sobolev"], tables["transition_probabilities"],
                           op.line2macro_level_upper, op.macro_block_edge_index, op.transition_type, op.destination_level_id,
                           op.transition_line_id)

    def upload():
        t0 = time.perf_counter()
        eng.set_opacity(same)
        wall = (time.perf_counter() - t0) * 1e3
        eng.set_line_data(ld)  # (set_opacity drops the line data; not part of its time)
        return dict(wall_ms=wall)

    out = {"lines": int(kw["n_lines"]), "transitions": int(len(op.transition_type)), "levels": int(ld.n_levels), "blocks": int(len(rows)),
           "blocks_ge_32_rows": int((rows >= 32).sum()), "rows_in_blocks_ge_32": int(rows[rows >= 32].sum()), "longest_block": int(rows.max())}
    arms = {"set_opacity": upload, "update_opacity": update}
    times = {a: [] for a in arms}
    for r in range(reps + 1):  # (rep 0: warm-up of every arm)
        for arm, fn in arms.items():
            t = fn()
            if r:
                times[arm].append(t)
            print(f"{name} {arm:>15} rep {r}: " + "  ".join(f"{k} {v:9.3f}" for k, v in t.items()), flush=True)
    out["set_opacity_wall_ms"] = best([t["wall_ms"] for t in times["set_opacity"]])
    for k in ("wall_ms", "device_ms", "line_ms", "block_ms", "derive_ms"):
        out["update_opacity_" + k] = best([t[k] for t in times["update_opacity"]])
    # the block kernel alone, per threshold (0 in the list: the lane form for every block)
    block = {t: [] for t in thresholds}
    for r in range(reps + 1):
        for t in thresholds:
            eng.set_option("opacity_update_long_rows", ALL_LANE if t == 0 else t)
            ms = update()["block_ms"]
            if r:
                block[t].append(ms)
            print(f"{name} block kernel, row form from {t if t else 'never':>5} rows, rep {r}: {ms:9.3f} ms", flush=True)
    eng.set_option("opacity_update_long_rows", -1)
    out["block_ms_by_threshold"] = {("all_lane" if t == 0 else str(t)): best(v) for t, v in block.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="config2,tardis_example")
    ap.add_argument("--thresholds", default="1,8,16,32,64,128,256,0")
    args = ap.parse_args()
    thresholds = [int(t) for t in args.thresholds.split(",")]
    out = {}
    with Engine(0) as eng:
        for name in args.shapes.split(","):
            out[name] = shape(eng, name, args.reps, thresholds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
