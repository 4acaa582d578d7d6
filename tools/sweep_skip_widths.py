"""Dependent steps and 16-byte loads per trace of the lane sweep with the block skip (csrc/sweep_skip.hpp) at a step of N loads -- a CPU count on the
oracle's traces of the configs[2] tables, as tools/sweep_study.py counts the sweep without the skip.

The oracle's trace log gives first line, lines examined and outcome of every trace.  From those the count follows the kernel's step logic:
  * the blocks cleared are the whole 8-line blocks between the trace's first line and the block of its last line (the margin of the coarse test is 1e-7 of
    an optical depth of order one: the traces it keeps from clearing such a block are not counted);
  * a coarse step clears up to N - 1 blocks, a step that clears all of them goes on from its last block (N - 2 further blocks per step);
  * none cleared: the trace sweeps line by line from its first line, N lines per step; else interval mode: line by line from the block of the last line;
  * a trace that ends in electron scattering after interval mode falls back: line by line from its first line on top of the above.

    EXP_LEVELS=heavy python tools/sweep_skip_widths.py [packets=20000]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402  (analysis tool: the oracle is the trace source here, nothing is measured against it)
from tardis_amd import synthetic  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20000
LEVELS = os.environ.get("EXP_LEVELS", "heavy")
S, L = 20, 500_000
prob = synthetic.make_problem(seed=1, n_packets=N, n_shells=S, n_lines=L, line_interaction_type="macroatom", level_sizes=LEVELS)
cap = 600 * N
buf = np.zeros((cap, 4), dtype=np.int64)
lib = oracle.lib()
lib.oracle_set_trace_log.restype = None
lib.oracle_set_trace_log.argtypes = [oracle.C.c_void_p, oracle.C.c_int64]
lib.oracle_trace_log_count.restype = oracle.C.c_int64
lib.oracle_set_trace_log(buf.ctypes.data, cap)
oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, prob.opacity_state, prob.montecarlo_configuration,
           prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=False)
n = int(lib.oracle_trace_log_count())
lib.oracle_set_trace_log(None, 0)
assert n < cap
tr = buf[:n]
start, cnt, typ = tr[:, 1], np.maximum(tr[:, 2], 1), tr[:, 3]
last = start + cnt - 1
cleared = (last >> 3) - (start >> 3)
escat = typ == 4
print(f"workload: BASELINE configs[2] tables ({S} shells x {L} lines, macroatom, {LEVELS} levels), {N} packets on the CPU oracle (serial run)")
print(f"traces {n} = {n / N:.1f} per packet; lines per trace: mean {cnt.mean():.1f}, median {np.median(cnt):.0f}, 90 % {np.percentile(cnt, 90):.0f}; "
      f"traces that clear no block {np.mean(cleared == 0):.3f}; traces that end in electron scattering {escat.mean():.3f}")
print(f"{'loads/step':>10s} {'coarse':>8s} {'fine':>8s} {'fall-back':>10s} {'steps per trace':>16s} {'loads per trace':>16s}")
for loads in (8, 9, 10, 12):
    coarse = np.ones(n, dtype=np.int64)
    rem = cleared.copy()
    more = rem >= loads - 1
    while more.any():
        rem[more] -= loads - 2
        coarse[more] += 1
        more = rem >= loads - 1
    in_block = last - (last & ~7) + 1  # lines of the last block up to the stopping line
    fine = np.where(cleared == 0, (cnt + loads - 1) // loads, (in_block + loads - 1) // loads)
    fallback = np.where(escat & (cleared > 0), (cnt + loads - 1) // loads, 0)
    steps = coarse + fine + fallback
    print(f"{loads:10d} {coarse.mean():8.3f} {fine.mean():8.3f} {fallback.mean():10.3f} {steps.mean():16.3f} {(steps * loads).mean():16.2f}")
print("without the skip: " + ", ".join(f"{lines} lines per step {((cnt + lines - 1) // lines).mean():.2f} steps / {(((cnt + lines - 1) // lines) * lines).mean():.1f} loads"
                                       for lines in (8, 10, 12)))
