"""Degenerate transition-probability tables for the macro-atom walk, for tests/test_degenerate_blocks_host.py and
tests/test_degenerate_blocks_gpu.py.

Every other transport test draws its transition probabilities continuously (synthetic.make_opacity_state): every row strictly positive, no
two running sums equal, every block summing to 1 within rounding.  Real tables have rows that are exactly 0 (plateaus of the running sums),
long blocks most of whose rows lie below 2**-16 of the sum, blocks that sum to 1 +- a few ulp -- or not to 1 at all after a plasma step
that misbehaved, on which the reference raises MacroAtomError on a particular packet.  The device's walk argues about exactly
these: ties of 16-bit running sums, saturated entries and the 0xffff padding, the window search of long blocks, the six hot intervals.

`KINDS` are the ways a block is overwritten (in place, per shell, every value >= 0: a negative one would take the problem off the compact
walk).  The problems: the "degenerate" family of tests/kernel_table_recipes.py; `giant_problem` (two blocks of 65 538 and 131 073 rows);
`chain_problem` (4 shells x 6000 lines, both modes; in macro-atom mode walks of many jumps); `error_problem` (blocks that sum to 0.75 in
one shell, a reachable empty block, a reachable row of transition type -3).  `insert_zero_rows` inserts rows of probability 0, which no
jump can select.  `census` counts what a sample exercises from the tables and the oracle's jump log alone -- it restates the 16-bit sums,
the windows and the hot intervals of tardis_amd/csrc/walk_tables.hpp in NumPy and never sees a device result.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kernel_table_recipes as ktr  # noqa: E402
from tardis_amd import state as st, synthetic  # noqa: E402

KINDS = ("zeros", "dyadic_equal", "sub_unit", "quantised", "one_row", "scaled_up", "barely_off", "continuous")
SCALES = {"scaled_up": (1.5, 1.25), "barely_off": (1.0 + 2.0 ** -30, float(np.nextafter(1.0, 2.0)))}  # (even shells, odd shells)
SUB_UNIT = 2.0 ** -np.array([17.0, 18.0, 19.0])  # runs of 2, 4 and 8 entries share one 16-bit value
SUB_UNIT_STRETCH = 16                            # rows of one value in a row
WINDOW, QUAD, SECTOR = 32, 8, 32                 # entries: one window of the walk (4 quads of 8), one 64-byte sector of 2-byte entries
HOT_ENTRIES, HOT_ROW_LIMIT = 6, 65535
GIANT_A_LINES, GIANT_B_LINES, GIANT_LINES = 21846, 43691, 66000


# ---- the kinds -----------------------------------------------------------------------------------------------------------------------

def apply_kind(op, b, kind, rng, one_row_blocks=()):
    """Overwrite block `b` of op.transition_probabilities in place as `kind` says; returns the kind really written ("continuous" for a
    block too short for it).

    zeros          a leading and a trailing run of max(1, n // 5) rows, and per shell a tenth of the rows between them at random, are
                   exactly 0 (about 45 % of the rows; the pattern differs from shell to shell); one emission row between the runs stays
                   non-zero; renormalised.
    dyadic_equal   every row 2**-u with n 2**-u <= 1/2 (u <= 16), one emission row (drawn per shell) takes the rest: every running sum is
                   an exact multiple of a 16-bit unit.
    sub_unit       stretches of 16 rows of 2**-17, 2**-18, 2**-19 (shifted from shell to shell); one emission row takes the rest.
    quantised      the continuous draw floored to multiples of 2**-18, the remainder on the largest emission row: the sum is exactly 1.
    one_row        one row 1.0, all others 0: the block's middle row in even shells (unless that row leads to another one_row block:
                   a walk could then circle for ever), the middle emission row else.
    scaled_up      the continuous draw x 1.5 (even shells) and x 1.25 (odd shells).
    barely_off     x (1 + 2**-30) and x nextafter(1, 2).
    continuous     untouched."""
    P = op.transition_probabilities
    S = P.shape[1]
    b0, b1 = int(op.macro_block_edge_index[b]), int(op.macro_block_edge_index[b + 1])
    n = b1 - b0
    em = np.flatnonzero(op.transition_type[b0:b1] == -1)
    if kind == "continuous" or n < 3 or len(em) == 0:
        return "continuous"
    blk = P[b0:b1]
    if kind == "zeros":
        run = max(1, n // 5)
        inner_em = em[(em >= run) & (em < n - run)]
        if len(inner_em) == 0:
            return "continuous"
        for s in range(S):
            zero = np.zeros(n, dtype=bool)
            zero[:run] = True
            zero[n - run:] = True
            inner = np.arange(run, n - run)
            zero[rng.choice(inner, len(inner) // 10, replace=False)] = True
            if zero[inner_em].all():
                zero[inner_em[rng.integers(len(inner_em))]] = False
            blk[zero, s] = 0.0
            blk[:, s] /= blk[:, s].sum()
    elif kind == "dyadic_equal":
        u = max(1, int(np.ceil(np.log2(2.0 * n))))
        assert n * 2.0 ** -u <= 0.5 and u <= 16, (n, u)
        for s in range(S):
            blk[:, s] = 2.0 ** -u
            blk[em[rng.integers(len(em))], s] = 1.0 - (n - 1) * 2.0 ** -u
    elif kind == "sub_unit":
        assert n * SUB_UNIT[0] < 1.0
        for s in range(S):
            col = SUB_UNIT[((np.arange(n) + 5 * s) // SUB_UNIT_STRETCH) % 3]
            r = em[rng.integers(len(em))]
            col[r] = 0.0
            col[r] = 1.0 - col.sum()  # (multiples of 2**-19 below 1: exact in any order)
            blk[:, s] = col
    elif kind == "quantised":
        for s in range(S):
            col = np.floor(blk[:, s] * 2.0 ** 18) / 2.0 ** 18
            r = em[np.argmax(col[em])]
            col[r] += 1.0 - col.sum()
            blk[:, s] = col
    elif kind == "one_row":
        mid = n // 2
        circles = op.transition_type[b0 + mid] >= 0 and int(op.destination_level_id[b0 + mid]) in one_row_blocks
        for s in range(S):
            r = mid if (s % 2 == 0 and not circles) else em[len(em) // 2]
            blk[:, s] = 0.0
            blk[r, s] = 1.0
    elif kind in SCALES:
        for s in range(S):
            blk[:, s] *= SCALES[kind][s % 2]
    else:
        raise ValueError(kind)
    assert np.all(blk >= 0.0)
    return kind


# the blocks synthetic's "heavy" level sizes plant (lines per level: 33 / 96 / 99 / 192 / 300 / 2100 rows in macro-atom mode), each with a kind of its own:
# tie runs across row 32 of the block just past one window, exact 16-bit sums in the block of three whole windows, plateaus under the window search
PLANTED = {11: "sub_unit", 32: "dyadic_equal", 33: "one_row", 64: "continuous", 100: "scaled_up", 700: "zeros"}


def deal_kinds(op, rng):
    """Deal KINDS out by block-size rank (the longest block gets KINDS[0], the next KINDS[1], ...: every kind gets long and short blocks;
    the planted blocks as PLANTED says) and overwrite the blocks; returns the kind index written, per block."""
    sizes = np.diff(op.macro_block_edge_index)
    order = np.argsort(-sizes, kind="stable")
    want = np.empty(len(sizes), dtype=np.int64)
    want[order] = np.arange(len(sizes)) % len(KINDS)
    rows_per_line = len(op.transition_type) // len(op.line_list_nu)
    for lines, kind in PLANTED.items():  # (the first block of each planted size: the rotation above may hand several of them one kind)
        at = np.flatnonzero(sizes == lines * rows_per_line)
        if len(at):
            want[at[0]] = KINDS.index(kind)
    one_row = set(np.flatnonzero(want == KINDS.index("one_row")).tolist())
    got = np.empty(len(sizes), dtype=np.int64)
    for b in range(len(sizes)):
        got[b] = KINDS.index(apply_kind(op, b, KINDS[want[b]], rng, one_row))
    return got


# ---- (a) the family ---------------------------------------------------------------------------------------------------------------

def _degenerate_family(prob):
    prob.block_kinds = deal_kinds(prob.opacity_state, np.random.default_rng(71))
    prob.description += " degenerate macro-atom blocks"
    return prob


ktr.register_family("degenerate", _degenerate_family)


# ---- (b) the giant problem ---------------------------------------------------------------------------------------------------------

_problems = {}


def giant_problem(n_packets=6000, log_tau_mean=-5.6, seed=61):
    """Macro-atom mode, 2 shells, 66 000 lines.  Level A owns 21 846 lines (65 538 rows): every row 2**-17 except the last, row 65 537
    (past the 16-bit row limit of a hot sector), which takes the rest.  Level B owns 43 691 lines (131 073 rows): in shell 0 the first
    131 072 rows are 2**-17, in shell 1 every second row is 2**-16 and the others are 0; the last row is 0 in both (the sum is exactly 1,
    with a trailing zero row).  The other levels own 1 .. 8 lines with continuous probabilities; internal rows lead to random levels; one
    empty block, behind A, that no line and no row leads to.  Attributes `giant_a`, `giant_b`, `empty_block`: the block ids.  Computed once."""
    k = ("giant", n_packets, log_tau_mean, seed)
    if k in _problems:
        return _problems[k]
    prob = synthetic.make_problem(seed=seed, n_packets=n_packets, n_shells=2, n_lines=GIANT_LINES, line_interaction_type="macroatom", n_bins=500,
                                  log_tau_mean=log_tau_mean)
    rng = np.random.default_rng(seed + 1)
    sizes, left = [], GIANT_LINES - GIANT_A_LINES - GIANT_B_LINES
    while left > 0:
        g = int(min(left, rng.integers(1, 9)))
        sizes.append(g)
        left -= g
    a, b = len(sizes) // 3, 2 * len(sizes) // 3 + 2
    sizes[a:a] = [GIANT_A_LINES, 0]
    sizes.insert(b, GIANT_B_LINES)
    prob.giant_a, prob.empty_block, prob.giant_b = a, a + 1, b
    old = prob.opacity_state
    op = tables_from_sizes(rng, old, np.asarray(sizes), 3)
    edge, P = op.macro_block_edge_index, op.transition_probabilities
    A = P[edge[a]:edge[a + 1]]
    A[:] = 2.0 ** -17
    A[-1] = 1.0 - (len(A) - 1) * 2.0 ** -17
    B = P[edge[b]:edge[b + 1]]
    B[:, 0] = 2.0 ** -17
    B[0::2, 1] = 0.0
    B[1::2, 1] = 2.0 ** -16
    B[-1] = 0.0
    prob.opacity_state = op
    prob.block_kinds = np.full(len(sizes), KINDS.index("continuous"))
    prob.description += " two giant blocks"
    _problems[k] = prob
    return prob


def tables_from_sizes(rng, old, sizes, rows_per_line):
    """A copy of the opacity state `old` with macro-atom tables of levels that own sizes[i] lines (0: an empty block that nothing leads
    to), laid out as synthetic.make_opacity_state lays them out: the emission rows of a level's lines, then (rows_per_line = 3) their
    internal down and internal up rows, to random non-empty levels; continuous probabilities, normalised per block and shell."""
    L, S = old.tau_sobolev.shape
    assert sizes.sum() == L
    n_levels, T = len(sizes), rows_per_line * L
    perm = rng.permutation(L)
    level_of_line = np.empty(L, np.int64)
    ttype, dest, tline = np.empty(T, np.int64), np.empty(T, np.int64), np.empty(T, np.int64)
    edge = np.concatenate(([0], np.cumsum(rows_per_line * sizes))).astype(np.int64)
    P = rng.random((T, S)) + 0.05
    full = np.flatnonzero(sizes > 0)
    pos = 0
    for lvl, g in enumerate(sizes):
        ids = np.sort(perm[pos:pos + g])
        pos += g
        level_of_line[ids] = lvl
        row = edge[lvl]
        ttype[row:row + g], dest[row:row + g], tline[row:row + g] = -1, -99, ids
        for t in range(1, rows_per_line):
            r = row + t * g
            ttype[r:r + g], dest[r:r + g], tline[r:r + g] = t - 1, full[rng.integers(0, len(full), g)], ids
        if g:
            P[edge[lvl]:edge[lvl + 1]] /= P[edge[lvl]:edge[lvl + 1]].sum(axis=0, keepdims=True)
    return st.OpacityState(old.electron_density.copy(), old.t_electrons.copy(), old.line_list_nu.copy(), old.tau_sobolev.copy(), P, level_of_line,
                           edge, ttype, dest, tline)


# ---- (c) the chain problem ----------------------------------------------------------------------------------------------------------

CHAIN_PACKETS = {"macroatom": 26000, "downbranch": 80000}  # 9e5 and 8e5 jumps: about 2**-16 of them draw x = 65535


def chain_problem(mode, n_packets=None, log_tau_mean=-2.5, seed=67):
    """4 shells x 6000 lines, heavy-tailed blocks, `mode` "macroatom" or "downbranch"; the kinds dealt out by block-size rank.  In
    macro-atom mode the emission rows of every block are first scaled to 2 .. 5 % of the block (drawn per block and shell), so that walks
    are many jumps long; the kinds that put "the rest" on one row put it on an emission row (on an internal row the walks grow to 1e5
    jumps).  Computed once."""
    n_packets = CHAIN_PACKETS[mode] if n_packets is None else n_packets
    k = ("chain", mode, n_packets, log_tau_mean, seed)
    if k in _problems:
        return _problems[k]
    prob = synthetic.make_problem(seed=seed, n_packets=n_packets, n_shells=4, n_lines=6000, line_interaction_type=mode, level_sizes="heavy",
                                  n_bins=500, log_tau_mean=log_tau_mean)
    op = prob.opacity_state
    rng = np.random.default_rng(seed + 1)
    if mode == "macroatom":
        edge, P = op.macro_block_edge_index, op.transition_probabilities
        for b in range(len(edge) - 1):
            blk = P[edge[b]:edge[b + 1]]
            em = op.transition_type[edge[b]:edge[b + 1]] == -1
            f = rng.uniform(0.02, 0.05, P.shape[1])
            blk[em] *= f / blk[em].sum(axis=0)
            blk[~em] *= (1.0 - f) / blk[~em].sum(axis=0)
            blk /= blk.sum(axis=0, keepdims=True)
    prob.block_kinds = deal_kinds(op, rng)
    prob.description += " degenerate macro-atom blocks, long walks"
    _problems[k] = prob
    return prob


# ---- (d) the error problems ---------------------------------------------------------------------------------------------------------

ERROR_KINDS = ("sum_below_one", "empty_block", "unsupported_type")
ERROR_SHELL = 1


def error_problem(what, n_packets=3000):
    """The chain problem in macro-atom mode (a fresh copy), broken:
    sum_below_one     every 64th block x 0.75, in shell 1 only: a number drawn above the block's sum finds no row there;
    empty_block       one more level, of no rows (edge[b] == edge[b + 1]), and every 700th internal row leads to it: the reference examines
                      0 rows and raises;
    unsupported_type  every 900th row gets transition type -3."""
    base = chain_problem("macroatom", n_packets)
    old = base.opacity_state
    P, edge, ttype, dest = old.transition_probabilities.copy(), old.macro_block_edge_index.copy(), old.transition_type.copy(), old.destination_level_id.copy()
    if what == "sum_below_one":
        for b in range(0, len(edge) - 1, 64):
            P[edge[b]:edge[b + 1], ERROR_SHELL] *= 0.75
    elif what == "empty_block":
        edge = np.append(edge, edge[-1])
        internal = np.flatnonzero(ttype >= 0)
        dest[internal[::700]] = len(edge) - 2
    elif what == "unsupported_type":
        ttype[::900] = -3
    else:
        raise ValueError(what)
    op = st.OpacityState(old.electron_density.copy(), old.t_electrons.copy(), old.line_list_nu.copy(), old.tau_sobolev.copy(), P,
                         old.line2macro_level_upper.copy(), edge, ttype, dest, old.transition_line_id.copy())
    prob = synthetic.Problem(base.packet_collection, base.geometry, base.time_explosion, op, base.montecarlo_configuration,
                             base.spectrum_frequency_grid, base.description + " " + what)
    prob.block_kinds = np.append(base.block_kinds, KINDS.index("continuous"))[:len(edge) - 1]
    return prob


# ---- (e) rows of probability 0 -------------------------------------------------------------------------------------------------------

ZERO_ROW_COUNTS = (1, 7, 8, 31, 32, 33)


def insert_zero_rows(opacity_state, rng, n_sites=300):
    """(new state, old_of_new): after `n_sites` random rows (of random blocks) 1, 7, 8, 31, 32 or 33 rows of probability 0 in every shell
    are inserted, with the transition type, the destination and the line of the row in front of them.  A row of probability 0 adds +0.0
    to the running sum and cannot be selected.  old_of_new[j] is the old index of the new row j, -1 for an inserted one."""
    op = opacity_state
    T, S = op.transition_probabilities.shape
    extra = np.zeros(T, dtype=np.int64)
    sites = rng.choice(T, min(n_sites, T), replace=False)
    extra[sites] = rng.choice(np.asarray(ZERO_ROW_COUNTS), len(sites))
    counts = 1 + extra
    new_of_old = np.cumsum(counts) - counts  # (the row itself first, the zero rows behind it)
    old_of_new = np.full(int(counts.sum()), -1, dtype=np.int64)
    old_of_new[new_of_old] = np.arange(T)
    P = np.zeros((len(old_of_new), S))
    P[new_of_old] = op.transition_probabilities
    edge = np.append(new_of_old, len(old_of_new))[op.macro_block_edge_index]
    new = st.OpacityState(op.electron_density.copy(), op.t_electrons.copy(), op.line_list_nu.copy(), op.tau_sobolev.copy(), P,
                          op.line2macro_level_upper.copy(), edge, np.repeat(op.transition_type, counts), np.repeat(op.destination_level_id, counts),
                          np.repeat(op.transition_line_id, counts))
    return new, old_of_new


def zero_row_problems(mode):
    """(problem, problem with zero rows, old_of_new) on the chain problem of `mode`."""
    k = ("zero rows", mode)
    if k not in _problems:
        base = chain_problem(mode)
        op, old_of_new = insert_zero_rows(base.opacity_state, np.random.default_rng(101))
        twin = synthetic.Problem(base.packet_collection, base.geometry, base.time_explosion, op, base.montecarlo_configuration,
                                 base.spectrum_frequency_grid, base.description + " with zero rows")
        twin.block_kinds = base.block_kinds
        _problems[k] = (base, twin, old_of_new)
    return _problems[k]


# ---- the oracle's jump log ----------------------------------------------------------------------------------------------------------

def oracle_run(oracle, prob, packets=None, n_threads=1, track=True):
    return oracle.run(prob.packet_collection if packets is None else packets, prob.geometry, prob.time_explosion, prob.opacity_state,
                      prob.montecarlo_configuration, prob.spectrum_frequency_grid, math_mode=oracle.MATH_PORTABLE, n_threads=n_threads,
                      track_last_interaction=track)


def jump_log(oracle, prob, packets=None):
    """(oracle result, log): one serial, tracked oracle run with the jump log on.  log[j] = {shell, b0 of the block, selected row relative
    to b0 or -1 where the block ran out, bits of the number drawn}, jump by jump, packet by packet."""
    lib = oracle.lib()
    lib.oracle_set_jump_log.restype = None
    lib.oracle_set_jump_log.argtypes = [C.c_void_p, C.c_int64]
    lib.oracle_jump_log_count.restype = C.c_int64
    cap = 1 << 20
    while True:
        buf = np.zeros((cap, 4), dtype=np.int64)
        lib.oracle_set_jump_log(buf.ctypes.data, cap)
        try:
            ref = oracle_run(oracle, prob, packets)
            n = int(lib.oracle_jump_log_count())
        finally:
            lib.oracle_set_jump_log(None, 0)
        if n < cap:
            return ref, buf[:n].copy()
        cap *= 4


def first_packets(pc, n):
    """The first n packets of a collection, as a collection of its own."""
    return st.PacketCollection(pc.initial_radii[:n].copy(), pc.initial_nus[:n].copy(), pc.initial_mus[:n].copy(), pc.initial_energies[:n].copy(),
                               pc.packet_seeds[:n].copy(), pc.radiation_field_luminosity)


def events_of(log):
    return np.ascontiguousarray(log[:, 3]).view(np.float64)


# ---- (f) the census -----------------------------------------------------------------------------------------------------------------

def compact_starts(edge, sector_packing=1):
    """The compact index at which every block's 16-bit sums start (derive_opacity_tables): blocks padded to whole quads; with sector
    packing a block of at most one window that would straddle a 64-byte sector, and every longer block, starts on a sector boundary."""
    c0 = np.zeros(len(edge) - 1, dtype=np.int64)
    tc = 0
    for b in range(len(edge) - 1):
        n = (int(edge[b + 1] - edge[b]) + 7) // 8 * 8
        if sector_packing and n > 0:
            in_sector = tc & 31
            if in_sector != 0 and (n > 32 or in_sector + n > 32):
                tc += 32 - in_sector
        c0[b] = tc
        tc += n
    return c0


def _six_widest(w):
    """The rows walk_hot_kernel keeps of a block with the interval widths w (0: not eligible), in its list's order: rows are inserted in
    order into a list of six sorted by width; a row no wider than the sixth is passed over; an inserted row takes the place of the first
    entry it is wider than, and the displaced entry moves on down the list in the same way -- past entries of its OWN width, so among equal
    widths it is not the last-come row that drops out (in a block of equal rows with one wide row behind them, the second row does)."""
    wd, rows = [0] * HOT_ENTRIES, [-1] * HOT_ENTRIES
    for k in np.flatnonzero(w > 0):
        cw, ck = int(w[k]), int(k)
        if cw <= wd[-1]:
            continue
        for e in range(HOT_ENTRIES):
            if cw > wd[e]:
                wd[e], cw = cw, wd[e]
                rows[e], ck = ck, rows[e]
    return rows


class BlockTables:
    """What the device derives from one block, restated: cum[n, S] the running sums (serial, in the reference's order), c16[n, S] =
    min(65535, floor(cum 65536)), the six hot intervals [lo, hi) per shell with their rows and the total width `mass` (walk_hot_kernel:
    lo = c16 of the row in front + 1, or 0 for the first row; hi = c16; rows of a type below -1, rows >= 65535 and empty intervals are
    not eligible; the six widest as _six_widest restates the kernel's insertion)."""

    def __init__(self, P, ttype):
        n, S = P.shape
        self.n = n
        self.cum = np.cumsum(P, axis=0)
        t = self.cum * 65536.0
        self.c16 = np.where(t >= 65535.0, 65535.0, np.floor(t)).astype(np.int64)
        lo = np.zeros_like(self.c16)
        lo[1:] = self.c16[:-1] + 1
        ok = (self.c16 > lo) & (ttype >= -1)[:, None] & (np.arange(n) < HOT_ROW_LIMIT)[:, None]
        w = np.where(ok, self.c16 - lo, 0)
        top = np.stack([_six_widest(w[:, s]) for s in range(S)])                  # [S, 6], -1: an empty entry
        at = np.maximum(top, 0)
        self.hot_rows = top
        self.hot_lo = np.where(top >= 0, lo[at, np.arange(S)[:, None]], 1)
        self.hot_hi = np.where(top >= 0, self.c16[at, np.arange(S)[:, None]], 0)
        self.mass = np.where(top >= 0, w[at, np.arange(S)[:, None]], 0).sum(axis=1)
        zero = P == 0.0
        self.zeros_before = np.cumsum(zero, axis=0) - zero                        # rows of probability 0 in front of a row
        self.leading_zeros = np.where(zero.all(axis=0), n, np.argmin(zero, axis=0))


def block_tables(prob):
    """BlockTables of every block of the problem (None for an empty block); computed once per problem."""
    if getattr(prob, "_block_tables", None) is None:
        op = prob.opacity_state
        edge = op.macro_block_edge_index
        prob._block_tables = [BlockTables(op.transition_probabilities[edge[b]:edge[b + 1]], op.transition_type[edge[b]:edge[b + 1]])
                              if edge[b + 1] > edge[b] else None for b in range(len(edge) - 1)]
    return prob._block_tables


def hot_blocks(prob, walk_hot=-1, min_mass=800, min_mass_long=400):
    """The blocks entered through a hot sector (derive_opacity_tables): none (walk_hot 0), every block with rows (1), or those whose six
    intervals cover `min_mass` per mille of the block on average over the shells (`min_mass_long` for blocks of more than one window)."""
    tabs = block_tables(prob)
    hot = np.zeros(len(tabs), dtype=bool)
    if walk_hot == 0:
        return hot
    for b, t in enumerate(tabs):
        if t is None:
            continue
        m = float(t.mass.sum()) / (65536.0 * len(t.mass))
        hot[b] = walk_hot == 1 or m >= 1e-3 * float(min_mass_long if t.n > WINDOW else min_mass)
    return hot


def window_of(c16, x):
    """(first entry, end) of the window the walk reads for every number x of a block with the 16-bit sums c16 (padded here to whole quads
    with 0xffff): all of a block of at most 32 rows; else the binary search of propagate_wave.hpp on the quads' last entries -- q_lo
    rises past a quad whose last entry is below x -- until at most three quads are left, and four quads from there."""
    n = len(c16)
    nq_all = (n + 7) // 8
    pad = np.full(8 * nq_all, 65535, dtype=np.int64)
    pad[:n] = c16
    q_lo, q_hi = np.zeros(len(x), dtype=np.int64), np.full(len(x), nq_all, dtype=np.int64)
    if n > WINDOW:
        while True:
            on = q_hi - q_lo > 3
            if not on.any():
                break
            qm = q_lo + ((q_hi - q_lo) >> 1)
            below = pad[np.minimum(8 * qm + 7, len(pad) - 1)] < x
            q_lo = np.where(on & below, qm + 1, q_lo)
            q_hi = np.where(on & ~below, qm, q_hi)
    nq = np.minimum(4, nq_all - q_lo)
    return pad, 8 * q_lo, 8 * (q_lo + nq)


COUNTS = ("jumps", "ran out", "tie", "tie run >= 2", "tie run >= 8", "decided inside a run", "run crosses a quad", "run crosses the window",
          "run crosses a sector", "x = 65535", "x = 0", "behind a plateau", "behind leading zeros", "row >= 32", "row >= 65535",
          "long block", "saturated tail", "sum above 1", "sum below 1", "fp64 decided", "giant")


def census(prob, log, walk_hot_min_mass=800, walk_hot_min_mass_long=400, sector_packing=1):
    """What the jumps of `log` (the oracle's jump log of `prob`) exercise, counted from the tables alone.  With x = floor(number 65536):

    tie                      a row of the block has the 16-bit sum x ("tie run >= 2 / >= 8": that many rows have it);
    decided inside a run     the selected row has the 16-bit sum x and is not the first that has it;
    run crosses ...          a run of >= 2 such rows lies in two quads (8 entries) / reaches past the end of the window the walk reads /
                             lies in two 64-byte sectors of the compact table;
    behind a plateau         a row of probability 0 lies in front of the selected row, behind the block's first non-zero row;
    behind leading zeros     the block starts with rows of probability 0 (and a row is selected);
    long block               the block has more than 32 rows (device counter 16384 with walk_hot 0);
    saturated tail           at least two rows of the block have the 16-bit sum 65535;
    sum above 1 / below 1    the block's last running sum in this shell is > 1 / < 1 - 2**-20;
    fp64 decided             an entry of the WINDOW -- the 0xffff padding included -- equals x: the window predicate of the compact walk,
                             restated exactly (device counter 32768 with walk_hot 0);
    giant                    the block has more than 65 535 rows.

    "hot 1" / "hot auto": with every block / the automatic choice of blocks on hot sectors, the jumps out of such blocks ("jumps"), those
    whose x lies in one of the six intervals ("hits"; device counter 65536), the others ("misses"; 131072), and those on an interval's
    end unit, x = hi or x = lo - 1 ("end unit").  "kind": jumps per kind of block.  The census also checks the log against the tables:
    the selected row is the first whose running sum exceeds the number."""
    op = prob.opacity_state
    edge = op.macro_block_edge_index
    S = op.transition_probabilities.shape[1]
    tabs = block_tables(prob)
    c0 = compact_starts(edge, sector_packing)
    first_block_at = {}
    for b in range(len(edge) - 1):  # (an empty block shares its b0 with the block behind it: jumps out of it have row -1 and no rows)
        first_block_at.setdefault(int(edge[b]), []).append(b)
    hot = {"hot 1": hot_blocks(prob, 1), "hot auto": hot_blocks(prob, -1, walk_hot_min_mass, walk_hot_min_mass_long)}
    out = {k: 0 for k in COUNTS}
    for h in hot:
        out[h] = {"jumps": 0, "hits": 0, "misses": 0, "end unit": 0}
    out["kind"] = {k: 0 for k in KINDS}
    out["jumps"] = len(log)
    if len(log) == 0:
        return out
    ev_all = events_of(log)
    key = log[:, 1] * S + log[:, 0]
    order = np.argsort(key, kind="stable")
    bounds = np.flatnonzero(np.diff(key[order])) + 1
    for grp in np.split(order, bounds):
        s, b0 = int(log[grp[0], 0]), int(log[grp[0], 1])
        row, ev = log[grp, 2], ev_all[grp]
        x = np.floor(ev * 65536.0).astype(np.int64)
        cands = first_block_at[b0]
        out["x = 65535"] += int((x == 65535).sum())
        out["x = 0"] += int((x == 0).sum())
        out["ran out"] += int((row < 0).sum())
        real = [b for b in cands if tabs[b] is not None]
        if not real:
            continue  # jumps out of an empty block: no rows, no tables
        b = real[0]
        t = tabs[b]
        cum, c16, n = t.cum[:, s], t.c16[:, s], t.n
        if len(cands) > 1:  # an empty block in front of b, at the same b0: its jumps ran out on numbers that select a row of b
            keep = ~((row < 0) & (cum[-1] > ev))
            row, ev, x, grp = row[keep], ev[keep], x[keep], grp[keep]
            if len(grp) == 0:
                continue
        sel = row >= 0
        r = np.where(sel, row, 0)
        assert np.all(cum[r[sel]] > ev[sel]) and np.all((r[sel] == 0) | (cum[np.maximum(r[sel] - 1, 0)] <= ev[sel])), "the log is not of these tables"
        assert np.all(cum[-1] <= ev[~sel])
        left, right = np.searchsorted(c16, x, "left"), np.searchsorted(c16, x, "right")
        n_eq = right - left
        out["tie"] += int((n_eq > 0).sum())
        out["tie run >= 2"] += int((n_eq >= 2).sum())
        out["tie run >= 8"] += int((n_eq >= 8).sum())
        out["decided inside a run"] += int((sel & (row > left) & (row < right)).sum())
        pad, w0, w1 = window_of(c16, x)
        run = n_eq >= 2
        last = right - 1
        out["run crosses a quad"] += int((run & (left // QUAD != last // QUAD)).sum())
        out["run crosses the window"] += int((run & (last >= w1)).sum())
        out["run crosses a sector"] += int((run & ((c0[b] + left) // SECTOR != (c0[b] + last) // SECTOR)).sum())
        pl, pr = np.searchsorted(pad, x, "left"), np.searchsorted(pad, x, "right")
        out["fp64 decided"] += int((np.minimum(pr, w1) - np.maximum(pl, w0) > 0).sum())
        lead = int(t.leading_zeros[s])
        out["behind leading zeros"] += int(sel.sum()) if lead > 0 else 0
        out["behind a plateau"] += int((sel & (t.zeros_before[r, s] > lead)).sum())
        out["row >= 32"] += int((row >= 32).sum())
        out["row >= 65535"] += int((row >= 65535).sum())
        m = len(grp)
        out["long block"] += m if n > WINDOW else 0
        out["giant"] += m if n > HOT_ROW_LIMIT else 0
        out["saturated tail"] += m if n >= 2 and c16[-2] == 65535 else 0
        out["sum above 1"] += m if cum[-1] > 1.0 else 0
        out["sum below 1"] += m if cum[-1] < 1.0 - 2.0 ** -20 else 0
        out["kind"][KINDS[int(prob.block_kinds[b])]] += m
        lo, hi = t.hot_lo[s][None, :], t.hot_hi[s][None, :]
        hit = ((x[:, None] >= lo) & (x[:, None] < hi)).any(axis=1)
        end = ((hi > lo) & ((x[:, None] == hi) | (x[:, None] == lo - 1))).any(axis=1)
        for h, flags in hot.items():
            if flags[b]:
                d = out[h]
                d["jumps"] += m
                d["hits"] += int(hit.sum())
                d["misses"] += int((~hit).sum())
                d["end unit"] += int(end.sum())
    return out


def hot_sector_entries(prob, b):
    """Number of non-empty entries of block b's hot sector, per shell."""
    return (block_tables(prob)[b].hot_rows >= 0).sum(axis=1)
