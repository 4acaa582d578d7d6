"""What the held start entry of a post-emission trace (ssk::MODE_START_HELD, csrc/sweep_skip.hpp; option sweep_start_held) changes in requests -- a CPU
count on the oracle's jump log and trace log of the configs[2] tables, in the manner of tools/sweep_skip_widths.py.

Per packet:
  * line interactions, and those whose emission a hot sector decided (the last jump of the walk left a block that is entered through its hot sector, and the
    number drawn fell into one of the block's six widest intervals in that shell: tests/degenerate_blocks.py restates the tables) with emit < L - 1 -- these
    read the pair pn[shell][emit], pn[shell][emit + 1] and hold the second entry;
  * how many of those pairs lie in one 64-byte sector, and in one 128-byte line, of the table as the library lays it out (sk_pn_off, rows of L + 1 entries);
  * the traces among them that clear no block (they touched the sector of nt_t that the walk's read used to fetch: their prefetch is gone).
The predicted change in requests that leave the L2, per packet: -(held) for the N-th load of the first coarse step, +(pairs that straddle a sector),
+(traces that clear no block).

    EXP_LEVELS=heavy python tools/sweep_start_held_count.py [packets=20000]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import degenerate_blocks as db  # noqa: E402  (the restatement of the hot-sector tables)
from oracle import oracle  # noqa: E402  (analysis tool: the oracle is the trace source here, nothing is measured against it)
from tardis_amd import synthetic  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20000
LEVELS = os.environ.get("EXP_LEVELS", "heavy")
S, L = 20, 500_000
prob = synthetic.make_problem(seed=1, n_packets=N, n_shells=S, n_lines=L, line_interaction_type="macroatom", level_sizes=LEVELS)
op = prob.opacity_state
lib = oracle.lib()
for name in ("trace", "jump"):
    getattr(lib, f"oracle_set_{name}_log").restype = None
    getattr(lib, f"oracle_set_{name}_log").argtypes = [oracle.C.c_void_p, oracle.C.c_int64]
    getattr(lib, f"oracle_{name}_log_count").restype = oracle.C.c_int64
cap_t, cap_j = 600 * N, 2000 * N
tbuf, jbuf = np.zeros((cap_t, 4), dtype=np.int64), np.zeros((cap_j, 4), dtype=np.int64)
lib.oracle_set_trace_log(tbuf.ctypes.data, cap_t)
lib.oracle_set_jump_log(jbuf.ctypes.data, cap_j)
oracle.run(prob.packet_collection, prob.geometry, prob.time_explosion, op, prob.montecarlo_configuration,
           prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=1, track_last_interaction=False)
n_t, n_j = int(lib.oracle_trace_log_count()), int(lib.oracle_jump_log_count())
lib.oracle_set_trace_log(None, 0)
lib.oracle_set_jump_log(None, 0)
assert n_t < cap_t and n_j < cap_j
tr, jl = tbuf[:n_t], jbuf[:n_j]

# the emissions: jumps whose selected row is an emission (transition_type -1), in the order of the line interactions of the trace log
edge = np.asarray(op.macro_block_edge_index)
ttype, tline = np.asarray(op.transition_type), np.asarray(op.transition_line_id)
sel = jl[:, 2] >= 0
at = np.where(sel, jl[:, 1] + jl[:, 2], 0)
emission = sel & (ttype[at] == -1)
ej = jl[emission]
emit = tline[at[emission]]
line_traces = np.flatnonzero(tr[:, 3] == 2)
assert len(line_traces) == len(ej), (len(line_traces), len(ej))
nxt = line_traces + 1  # (a packet goes on after a line interaction: the next row of the log is its next trace)
assert np.array_equal(tr[nxt, 1], emit + 1) and np.array_equal(tr[nxt, 0], ej[:, 0])

# decided by a hot sector: the block is on a hot sector (the automatic choice: its six widest intervals cover 800 per mille of it on average over the shells, 400
# for a block of more than one window) and the number lies in the selected row's interval, one of the six widest of the shell (walk_tables.hpp, restated as
# tests/degenerate_blocks.py does, vectorised; among rows of equal width the earlier one is kept, where the kernel's insertion may keep another)
P = np.asarray(op.transition_probabilities)
x = np.floor(db.events_of(ej) * 65536.0).astype(np.int64)
decided = np.zeros(len(ej), dtype=bool)
order = np.argsort(ej[:, 1], kind="stable")
ends = {int(edge[b]): int(edge[b + 1]) for b in range(len(edge) - 1) if edge[b + 1] > edge[b]}
for grp in np.split(order, np.flatnonzero(np.diff(ej[order, 1])) + 1):
    b0 = int(ej[grp[0], 1])
    b1 = ends[b0]
    n = b1 - b0
    t = np.cumsum(P[b0:b1], axis=0) * 65536.0
    c16 = np.where(t >= 65535.0, 65535.0, np.floor(t)).astype(np.int64)
    lo = np.zeros_like(c16)
    lo[1:] = c16[:-1] + 1
    ok = (c16 > lo) & (ttype[b0:b1] >= -1)[:, None] & (np.arange(n) < db.HOT_ROW_LIMIT)[:, None]
    w = np.where(ok, c16 - lo, 0)
    top = np.argsort(-w, axis=0, kind="stable")[:db.HOT_ENTRIES]                   # [<= 6, S]
    mass = np.take_along_axis(w, top, axis=0).sum(axis=0)
    if float(mass.sum()) / (65536.0 * S) < 1e-3 * (400.0 if n > db.WINDOW else 800.0):
        continue
    s, row = ej[grp, 0], ej[grp, 2]
    in_six = ((top[:, s] == row[None, :]) & (w[row, s] > 0)[None, :]).any(axis=0)
    decided[grp] = in_six & (x[grp] >= lo[row, s]) & (x[grp] < c16[row, s])

held = decided & (emit < L - 1)
stride = (L + 7) & ~7
pn_off = (stride * S + 32) + ((stride // 8) * S + 16)  # sk_pn_off, in 16-byte entries from a 256-byte aligned base
idx = pn_off + ej[:, 0] * (L + 1) + emit
same_sector, same_line = (idx & 3) != 3, (idx & 7) != 7
cnt = np.maximum(tr[nxt, 2], 1)
cleared = ((tr[nxt, 1] + cnt - 1) >> 3) - (tr[nxt, 1] >> 3)
no_block = cleared == 0
h = held.sum()
print(f"workload: BASELINE configs[2] tables ({S} shells x {L} lines, macroatom, {LEVELS} levels), {N} packets on the CPU oracle (serial run)")
print(f"per packet: traces {n_t / N:.1f}, jumps {n_j / N:.1f}, line interactions {len(ej) / N:.2f}")
print(f"per packet: emissions decided by a hot sector {decided.sum() / N:.2f}, of those with emit < L - 1 (the pair is read, the entry held) {h / N:.2f}")
print(f"per packet: pairs in one 64-byte sector {(held & same_sector).sum() / N:.2f} ({(held & same_sector).sum() / h:.3f}), "
      f"in one 128-byte line {(held & same_line).sum() / N:.2f} ({(held & same_line).sum() / h:.3f})")
print(f"per packet: held traces that clear no block {(held & no_block).sum() / N:.2f} ({(held & no_block).sum() / h:.3f})")
pred = -h + (held & ~same_sector).sum() + (held & no_block).sum()
print(f"predicted change in requests that leave the L2, per packet: -{h / N:.2f} (N-th load) +{(held & ~same_sector).sum() / N:.2f} (straddling pairs) "
      f"+{(held & no_block).sum() / N:.2f} (lost prefetch) = {pred / N:.2f}")
