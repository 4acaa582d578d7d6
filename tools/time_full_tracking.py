"""Device time of full r-packet tracking (option track_full) against untracked runs, on the configs[1] shape
(20 shells x 3e4 lines, downbranch): the automatic choice tracked (the wave-owner kernel, variant 2) and untracked, and the lane kernel
(variant 0) tracked and untracked; rows per packet, log bytes,
and the wall time of the post pass (scan + scatter + copies, Engine.get_event_log).

    python tools/time_full_tracking.py [--packets 100000 1000000] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tardis_amd import synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    shape = dict(synthetic.BASELINE_CONFIGS[2])
    out = []
    with Engine(0) as eng:
        for n in args.packets:
            shape["n_packets"] = n
            prob = synthetic.make_problem(seed=1, **shape)
            eng.set_geometry(prob.geometry, prob.time_explosion)
            eng.set_opacity(prob.opacity_state)
            eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
            eng.set_packets(prob.packet_collection)
            row = {"packets": n}
            for name, variant, full in (("auto_untracked", -1, 0), ("auto_tracked", -1, 1), ("lane_untracked", 0, 0), ("lane_tracked", 0, 1)):
                eng.set_option("variant", variant)
                eng.set_option("track_full", full)
                ms = []
                for _ in range(args.repeats + 1):  # (the first call warms up)
                    eng.reset_estimators()
                    eng.propagate()
                    eng.synchronize()
                    ms.append(eng.last_propagate_ms())
                row[name + "_ms"] = min(ms[1:])
                row[name + "_variant"] = eng.last_variant()
                if full and variant < 0:
                    eng.get_results(track_last_interaction=False, want_line_estimators=False)
                    t0 = time.perf_counter()
                    log = eng.get_event_log()
                    row["post_pass_wall_ms"] = (time.perf_counter() - t0) * 1e3
                    row["rows"] = log.n_rows
                    row["rows_per_packet"] = log.n_rows / n
                    row["log_bytes_device_pool"] = log.n_rows * 96
                    row["log_bytes_host_columns"] = log.n_rows * 112 + (n + 1) * 8
            eng.set_option("variant", -1)
            eng.set_option("track_full", 0)
            row["tracked_over_lane_untracked"] = row["lane_tracked_ms"] / row["lane_untracked_ms"]
            row["auto_tracked_over_auto_untracked"] = row["auto_tracked_ms"] / row["auto_untracked_ms"]
            print(json.dumps(row), flush=True)
            out.append(row)
    return out


if __name__ == "__main__":
    main()
