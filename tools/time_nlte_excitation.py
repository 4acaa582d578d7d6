"""Cost of NLTE excitation in the plasma step of an outer iteration, on the GPU: tardis_mc_update_plasma with NLTE data installed (the
rates kernel and the (species, shell) workgroups between the Boltzmann and the partition stage) against the same update without NLTE data
and against the path it replaces -- beta_sobolev and j_blues downloaded through tardis_mc_get_opacity ([L,S] each), the rate matrices built
and solved on the host with numpy.linalg.solve per (species, shell) as the legacy plasma does, the remaining plasma stages in NumPy
(tests/plasma_update_ref.py) and tardis_mc_update_opacity with its [K,S] upload.
Shapes: the configs[2] tables (5e5 lines, 5e4 levels, 20 shells) and the tardis_example shape (3e4 lines, 3e3 levels, 20 shells), the lines
moved inside the ions (synthetic.lines_within_ions).  NLTE species, three: the ion closest to 16 and to 100 levels and the longest ion whose
slabs stay under the plan's scratch cap (csrc/nlte_plan.hpp) and under --max-levels.
Arms, one process each (the parent starts them one after the other and never opens the GPU itself), in each one warm-up call, then the
median of --reps timed calls: "plain" (no NLTE data), "lds" (the plan's rule), "global" (option nlte_lds_levels 0: every species in the
global form), "host" (the replaced path), and "sweep": every species that fits the LDS installed alone, its solve timed in both forms --
the measurement the rule of csrc/nlte_plan.hpp is set from.  The forms of a species in HBM, through option nlte_blocked_levels: "one_wg"
(LDS where it fits, else one workgroup per (species, shell) on its slab), "blocked" (LDS where it fits, else the blocked form), "global"
now meaning every species on a slab with one workgroup, and "blocked_sweep": every species that does not fit the LDS (up to
--max-levels) installed alone, its solve timed in both forms -- the measurement BLOCKED_FORM_LEVELS is set from.  With TARDIS_MC_LIB
naming an older build, the arms it knows ("lds", "global") time that build.
Usage: python tools/time_nlte_excitation.py [--reps 5] [--shapes config2,tardis_example] [--max-levels 1200]"""
import argparse
import json
import os
import re
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
_PLAN = open(os.path.join(ROOT, "tardis_amd", "csrc", "nlte_plan.hpp")).read()
SCRATCH_CAP = 1 << int(re.search(r"MAX_SCRATCH_BYTES = 1LL << (\d+);", _PLAN).group(1))
LARGEST_LDS_LEVELS = int(re.search(r"GLOBAL_FORM_LEVELS = (\d+);", _PLAN).group(1)) - 1
ARMS = ("plain", "lds", "global", "one_wg", "blocked", "host", "sweep", "blocked_sweep")
NEVER_BLOCKED = 1 << 40  # a value of option nlte_blocked_levels no species reaches
# options (nlte_lds_levels, nlte_blocked_levels) of an arm
FORM_OPTIONS = {"lds": (-1, -1), "global": (0, NEVER_BLOCKED), "one_wg": (-1, NEVER_BLOCKED), "blocked": (-1, 0)}


def median(ts):
    return round(statistics.median(ts), 3)


def work_bytes(n):
    return 8 * ((n | 1) * n + 4 * n)


def arm(name, which, reps, max_levels):
    import nlte_excitation_ref as nref
    from tardis_amd.engine import Engine

    kw = SHAPES[name]
    S = 20
    prob = synthetic.make_problem(seed=1, n_packets=16, n_shells=S, line_interaction_type="macroatom", n_lines=kw["n_lines"],
                                  level_sizes=kw["level_sizes"])
    ld = synthetic.make_line_data(1, prob.opacity_state, level_sizes=kw["level_sizes"], time_explosion=prob.time_explosion)
    pd = synthetic.make_plasma_data(1, ld, S, n_elements=8, largest_ion=kw["largest_ion"])
    ld = synthetic.lines_within_ions(1, ld, pd)
    levels = np.diff(pd.ion_level_edge)
    fits = np.flatnonzero((work_bytes(levels) * S <= SCRATCH_CAP // 2) & (levels <= max_levels))  # (half the cap: room for the others)
    species = sorted({int(np.argmin(np.abs(levels - t) + (levels < 2) * 1e9)) for t in (16, 100)} | {int(fits[np.argmax(levels[fits])])})
    nd = synthetic.make_nlte_data(1, ld, pd, species=species)
    out = {"lines": int(kw["n_lines"]), "levels": int(ld.n_levels), "ions": int(len(levels)), "nlte_species_levels": [int(levels[i]) for i in species],
           "nlte_lines": int(len(nd.line_id))}
    with Engine(0) as eng:
        eng.set_geometry(prob.geometry, prob.time_explosion)
        eng.set_opacity(prob.opacity_state)
        eng.set_config(prob.montecarlo_configuration, prob.spectrum_frequency_grid)
        eng.set_line_data(ld)
        eng.set_plasma_data(pd)

        def device():
            t0 = time.perf_counter()
            eng.update_plasma(pd.t_radiative, pd.dilution_factor)
            wall = (time.perf_counter() - t0) * 1e3
            t = dict(wall_ms=wall, device_ms=eng.last_propagate_ms(), **eng.last_plasma_update_ms())
            if eng.nlte_data is not None:
                t.update(eng.last_nlte_ms())
            return t

        def host():
            t0 = time.perf_counter()
            tabs = eng.get_opacity(False, False, beta_sobolev=True, j_blues=True)
            t1 = time.perf_counter()
            # (the same radiation field every repetition: the j the last update stored are the j of this one)
            sol = nref.solve(pd, ld, nd, pd.t_radiative, pd.dilution_factor, tabs["j_blues"], tabs["beta_sobolev"], solver=nref.lapack_solve)
            t2 = time.perf_counter()
            eng.update_opacity(sol["level_number_density"], sol["electron_density"], 0, t_radiative=pd.t_radiative,
                               dilution_factor=pd.dilution_factor)
            t3 = time.perf_counter()
            return dict(wall_ms=(t3 - t0) * 1e3, download_ms=(t1 - t0) * 1e3, host_solve_ms=(t2 - t1) * 1e3, update_opacity_wall_ms=(t3 - t2) * 1e3)

        def timed(fn, label):
            times = []
            for r in range(reps + 1):  # (rep 0: warm-up)
                t = fn()
                if r:
                    times.append(t)
                print(f"{name} {label:>10} rep {r}: " + "  ".join(f"{k} {v:9.3f}" for k, v in t.items()), flush=True)
            return {k: median([t[k] for t in times]) for k in times[0]}

        def set_forms(lds_levels, blocked_levels):
            eng.set_option("nlte_lds_levels", lds_levels)
            if not os.environ.get("TARDIS_MC_LIB"):  # (an older build has one form for a species in HBM and no such option)
                eng.set_option("nlte_blocked_levels", blocked_levels)

        if which == "blocked_sweep":
            out["solve_ms_by_levels"] = {}
            seen = []
            for i in sorted((i for i in range(len(levels)) if LARGEST_LDS_LEVELS < levels[i] <= max_levels and work_bytes(levels[i]) * S <= SCRATCH_CAP),
                            key=lambda i: levels[i]):
                if seen and levels[i] < 1.25 * seen[-1]:  # (sizes a quarter apart)
                    continue
                seen.append(int(levels[i]))
                eng.set_nlte_data(synthetic.make_nlte_data(1, ld, pd, species=[i]))
                row = {}
                for form in ("one_wg", "blocked"):
                    set_forms(*FORM_OPTIONS[form])
                    m = timed(device, f"n={int(levels[i])} {form}")
                    row[form] = m["solve_ms"]
                    row[form + "_update_ms"] = m["device_ms"]
                out["solve_ms_by_levels"][str(int(levels[i]))] = row
            return out
        if which == "sweep":
            out["solve_ms_by_levels"] = {}
            for i in (i for i in range(len(levels)) if 2 <= levels[i] <= LARGEST_LDS_LEVELS):
                if not any(abs(int(levels[i]) - t) <= max(2, t // 10) for t in (4, 8, 16, 24, 32, 48, 64, 80, 96, 112, 128, LARGEST_LDS_LEVELS)):
                    continue
                if str(int(levels[i])) in out["solve_ms_by_levels"]:
                    continue
                eng.set_nlte_data(synthetic.make_nlte_data(1, ld, pd, species=[i]))
                row = {}
                for form in ("lds", "global"):
                    set_forms(*FORM_OPTIONS[form])
                    row[form] = timed(device, f"n={int(levels[i])} {form}")["solve_ms"]
                out["solve_ms_by_levels"][str(int(levels[i]))] = row
            return out
        if which == "host":
            eng.update_plasma(pd.t_radiative, pd.dilution_factor)  # (an update has to have produced beta and j)
            out.update(timed(host, which))
            return out
        if which != "plain":
            eng.set_nlte_data(nd)
            set_forms(*FORM_OPTIONS[which])
        out.update(timed(device, which))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="config2,tardis_example")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--max-levels", type=int, default=1200, help="the longest NLTE species taken (the solve is one workgroup per shell: n^3 work)")
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
