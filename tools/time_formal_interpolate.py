"""Device time of the formal integral with interpolate_shells (tardis_mc_formal_integral_interpolated) beside the host route it
replaces: the download of att_S_ul / Jred_lu / Jblue_lu, scipy's interp1d on one core, a second engine's set_geometry /
set_opacity with the interpolated tau_sobolev and electron densities, and the formal integral fed from the host.  Shape:
configs[2] tables (20 shells, 5e5 lines, macroatom, heavy-tailed levels).  One warm-up round, then the two routes alternated
--repeats times; median, minimum and maximum of every figure.  Also the interpolation kernel alone (the device time of
tardis_mc_interpolated_source with no output asked for) as bytes per second -- 7 row reads and 4 row writes of 8 L bytes per
output shell -- beside the streaming copy of tardis_mc_debug_microbench 15.

    python tools/time_formal_interpolate.py [--lines 500000] [--packets 100000] [--interpolate-shells 81] [--repeats 3]
                                            [--frequencies 1000] [--impact-parameters 1000] [--skip-host]
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

from tardis_amd import state as st, synthetic  # noqa: E402
from tardis_amd.engine import Engine  # noqa: E402


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def host_route(eng, prob, sf_keys, n, t_inner, freqs, points):
    """What a caller without the device interpolation does; returns (luminosities, {stage: wall ms})."""
    from scipy.interpolate import interp1d
    op, geo = prob.opacity_state, prob.geometry
    S, L = len(geo.r_inner), len(op.line_list_nu)
    t = {}
    src, t["download"] = wall(lambda: eng.source_function(prob.packet_collection.time_of_simulation, geo.volume))

    def interpolate():
        x = (geo.r_inner + geo.r_outer) / 2.0
        r = np.linspace(geo.r_inner[0], geo.r_outer[-1], n)
        xn = (r[:-1] + r[1:]) / 2.0
        lin = {k: interp1d(x, src[k].reshape(S, L), axis=0, fill_value="extrapolate")(xn).clip(0.0) for k in sf_keys}
        tau = interp1d(x, op.tau_sobolev, axis=1, kind="nearest", fill_value="extrapolate")(xn)
        n_e = interp1d(x, op.electron_density, kind="nearest", fill_value="extrapolate")(xn)
        return r, lin, tau, n_e
    (r, lin, tau, n_e), t["scipy"] = wall(interpolate)

    def second_engine():
        e2 = Engine(0)
        e2.set_geometry(st.HomologousRadial1DGeometry(r[:-1], r[1:], r[:-1] / prob.time_explosion, r[1:] / prob.time_explosion,
                                                      prob.time_explosion), prob.time_explosion)
        Si = n - 1
        e2.set_opacity(st.OpacityState(n_e, np.zeros(Si), op.line_list_nu, tau, np.ones((L, Si)), np.arange(L, dtype=np.int64),
                                       np.arange(L + 1, dtype=np.int64), -np.ones(L, dtype=np.int64), np.zeros(L, dtype=np.int64),
                                       np.arange(L, dtype=np.int64)))
        return e2
    e2, t["second_engine"] = wall(second_engine)
    try:
        (lum, _), t["host_fed_integral"] = wall(lambda: e2.formal_integral(t_inner, freqs, lin["att_S_ul"], lin["Jred_lu"], lin["Jblue_lu"], points))
    finally:
        e2.close()
    t["total"] = sum(t.values())
    return lum, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=500_000)
    ap.add_argument("--packets", type=int, default=100_000)
    ap.add_argument("--interpolate-shells", type=int, default=81)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frequencies", type=int, default=1000)
    ap.add_argument("--impact-parameters", type=int, default=1000)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    n, S = args.interpolate_shells, 20
    sf_keys = ("att_S_ul", "Jred_lu", "Jblue_lu")
    spread = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    with Engine(0) as eng:
        prob = synthetic.make_problem(seed=1, n_packets=args.packets, n_shells=S, n_lines=args.lines, line_interaction_type="macroatom",
                                      level_sizes="heavy")
        op, geo, tsim = prob.opacity_state, prob.geometry, prob.packet_collection.time_of_simulation
        eng.set_geometry(geo, prob.time_explosion)
        eng.set_opacity(op)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_packets(prob.packet_collection)
        eng.reset_estimators()
        eng.propagate()
        eng.synchronize()
        eng.source_function(tsim, geo.volume, want_arrays=False)
        nu = op.line_list_nu
        freqs = np.linspace(nu[-1] * 1.05, nu[0] * 0.95, args.frequencies)
        rows = {}
        lum_d = lum_h = None
        for rep in range(args.repeats + 1):  # (the first round warms up)
            (lum_d, _), w = wall(lambda: eng.formal_integral_interpolated(n, 1.0e4, freqs, args.impact_parameters))
            r = {"interpolated_integral_wall_ms": w, "interpolated_integral_ms": eng.last_propagate_ms()}
            _, w = wall(lambda: eng.formal_integral_resident(1.0e4, freqs, args.impact_parameters))
            r.update(resident_integral_wall_ms=w, resident_integral_ms=eng.last_propagate_ms())
            if not args.skip_host:
                lum_h, t = host_route(eng, prob, sf_keys, n, 1.0e4, freqs, args.impact_parameters)
                r.update({"host_" + k + "_wall_ms": v for k, v in t.items()})
            print("round", rep, json.dumps(r), file=sys.stderr, flush=True)
            if rep:
                for k, v in r.items():
                    rows.setdefault(k, []).append(v)
        # the interpolation kernel alone, and the box's streaming copy in the same session
        kernel_ms = []
        for rep in range(args.repeats + 1):  # (no output asked for: the tables are built and dropped, nothing is downloaded)
            eng._check(eng._L.tardis_mc_interpolated_source(eng._h, n, *([None] * 8)), "interpolated_source")
            if rep:
                kernel_ms.append(eng.last_propagate_ms())
        moved = (7 + 4) * 8.0 * args.lines * (n - 1)
        n_doubles, iters = 1 << 28, 4  # (bench.py's measured_stream_peak: the best of three grids)
        copy_ms = [min(eng.debug_microbench(15, n_doubles, iters, blocks) for blocks in (4096, 16384, 65536)) for _ in range(args.repeats)]
        out = {"lines": args.lines, "shells": S, "interpolate_shells": n, "packets": args.packets, "frequencies": args.frequencies,
               "impact_parameters": args.impact_parameters, "repeats": args.repeats,
               "interpolation_kernels_ms": spread(kernel_ms), "interpolation_bytes": moved,
               "interpolation_TB_per_s": moved / (statistics.median(kernel_ms) * 1e-3) / 1e12,
               "stream_copy_TB_per_s": n_doubles * 8.0 * iters / (statistics.median(copy_ms) * 1e-3) / 1e12}
        out.update({k: spread(v) for k, v in rows.items()})
        if lum_h is not None:
            out["spectrum_max_rel_diff"] = float(np.abs(lum_d - lum_h).max() / np.abs(lum_h).max())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
