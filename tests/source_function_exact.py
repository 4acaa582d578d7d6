"""Hand-built macro-atom tables for tardis_mc_source_function and an exact reference of its level solve, for
tests/test_source_function_exact_host.py and tests/test_source_function_exact_gpu.py.  A helper module, not a test file.

The builders make an opacity state from the number of lines of every level and a list of internal rows (source level, destination
level, probability per shell); every line gets one emission row.  `menu_lengths` deals out the CSR row lengths at which
tardis_amd/csrc/source_function.hpp changes its path: a row is summed by a group of G lanes (G = 1, 4, 16 from the index's mean row
length) or, beyond 32 G entries, by the whole wave.

The reference shares nothing with the device's summation order or stop rule:
  terms   norm_e (1 - exp(-tau)) Edotlu in fp64 with the roundings the header states (exp is the project's own, oracle.exp_array(x, 1));
  e       their EXACT sum per level (fractions.Fraction: doubles are dyadic rationals);
  C       the exact solution of (I - Q^T) C = e, per weakly connected component of the jump graph: substitution in Fractions where the
          component is acyclic, Gaussian elimination in Fractions for a cyclic component of at most EXACT_CYCLIC levels (no rounding at
          all), mpmath at 50 digits with the residual checked to 1e-30 of each component beyond that;
  B       (I - Q^T)^-1 C, the same way.

Bound of a level.  u = 2**-53, r the longest incoming row, n the most lines on a level, w = (r + n + 3) u.  All data are non-negative, so
every term of C_k = e_k + sum q C_src sees at most r + 2 roundings in any summation order, e_k at most n, and to first order the fp64
iteration at its fixed point lies within w B_k of C_k (the errors propagate through (I - Q^T)^-1 >= 0).  `level_bound` is
2 w B_k + 1e-14 C_k: the 2 covers the second-order terms, 1e-14 is the truncation the header used to promise, read per component.  A
level whose exact value is 0 must be exactly 0.  The condition of the derivation -- a serial fp64 iteration run until x no longer changes
stays within w B_k -- is checked on every case by the host tests (`serial_fixed_point`).

Given the device's own C, `close_bitwise` restates sf_close_kernel and sf_shell_kernel operation by operation.
"""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import oracle  # noqa: E402
from tardis_amd import state as st, synthetic  # noqa: E402

U = 2.0 ** -53
C_LIGHT = 2.99792458e10
LONG_STEPS = 32       # SF_LONG_STEPS
EXACT_CYCLIC = 8      # cyclic components up to this size are eliminated in Fractions
T_SIM = 1.3e-4


# ---- which path a CSR row takes -------------------------------------------------------------------------------------------------------

def group_width(nnz, n_rows):
    """sf_group_width, restated."""
    mean = nnz / n_rows if n_rows > 0 else 0.0
    return 1 if mean <= 4.0 else (4 if mean <= 16.0 else 16)


def row_paths(lengths):
    """(G, is_long[K]) for an index with these row lengths."""
    lengths = np.asarray(lengths)
    G = group_width(int(lengths.sum()), len(lengths))
    return G, lengths > LONG_STEPS * G


def menu_lengths(G, K, rng, fill_max):
    """K row lengths that make the index run with groups of G lanes and hold rows of 0, 1, G - 1, G, G + 1, 32 G (the longest a group
    takes) and 32 G + 1 entries (the shortest the wave takes), a second long row in the wave of the first, a long row in the last wave,
    which is partly filled, and a row count that fills no block (256 / G rows); the other rows hold 0 .. fill_max entries."""
    rows_per_wave, rows_per_block = 64 // G, 256 // G
    assert K % rows_per_wave != 0 and K % rows_per_block != 0 and K > rows_per_block
    base = sorted({0, 1, G - 1, G, G + 1, LONG_STEPS * G, LONG_STEPS * G + 1})
    lengths = rng.integers(0, fill_max + 1, K)
    lengths[:len(base)] = base
    a = len(base) - 1
    assert (a + 1) // rows_per_wave == a // rows_per_wave
    lengths[a + 1] = LONG_STEPS * G + 2
    lengths[K - 1] = LONG_STEPS * G + 1
    got, is_long = row_paths(lengths)
    assert got == G, (got, G, lengths.sum() / K)
    waves = np.arange(K) // rows_per_wave
    assert is_long[a] and is_long[a + 1] and waves[a] == waves[a + 1] and is_long[K - 1] and not is_long[a - 1]
    return lengths


# ---- the builders --------------------------------------------------------------------------------------------------------------------

class Case:
    """One hand-built problem: op (OpacityState), geometry, volume, t_sim, mode, j_blue / edotlu [L, S], and the table's description:
    lines_of_level [K], level_of_line [L], row_src / row_dst [R], row_q [R, S] (the internal rows in table order)."""

    def __init__(self, name, mode, lines_of_level, row_src, row_dst, row_q, S, seed, estimator_decades=3.0, edotlu=None, tau=None):
        rng = np.random.default_rng(seed)
        self.name, self.mode, self.S = name, mode, S
        self.lines_of_level = np.asarray(lines_of_level, dtype=np.int64)
        K, L = len(self.lines_of_level), int(self.lines_of_level.sum())
        self.K, self.L = K, L
        row_src, row_dst = np.asarray(row_src, dtype=np.int64), np.asarray(row_dst, dtype=np.int64)
        row_q = np.asarray(row_q, dtype=np.float64).reshape(len(row_src), S)
        order = np.argsort(row_src, kind="stable")  # (the rows of a block lie together)
        self.row_src, self.row_dst, self.row_q = row_src[order], row_dst[order], row_q[order]
        # lines are dealt to the levels at random: the counting sort of the level index has something to sort
        perm = rng.permutation(L)
        self.level_of_line = np.empty(L, dtype=np.int64)
        lines_of = []
        pos = 0
        for k, g in enumerate(self.lines_of_level):
            ids = np.sort(perm[pos:pos + g])
            pos += g
            self.level_of_line[ids] = k
            lines_of.append(ids)
        out_rows = np.bincount(self.row_src, minlength=K)
        sizes = self.lines_of_level + out_rows
        edge = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        T = int(edge[-1])
        ttype, dest, tline = np.full(T, -1, np.int64), np.full(T, -99, np.int64), np.zeros(T, np.int64)
        P = np.zeros((T, S))
        at = 0
        for k in range(K):
            g = int(self.lines_of_level[k])
            r0 = int(edge[k])
            tline[r0:r0 + g] = lines_of[k]
            P[r0:r0 + g] = rng.uniform(0.05, 1.0, (g, S)) / max(g, 1)
            n = int(out_rows[k])
            ttype[r0 + g:r0 + g + n] = 0
            dest[r0 + g:r0 + g + n] = self.row_dst[at:at + n]
            P[r0 + g:r0 + g + n] = self.row_q[at:at + n]
            at += n
        nu = np.sort(rng.uniform(1.0e14, 3.0e15, L))[::-1].copy()
        if tau is None:
            tau = 10.0 ** rng.uniform(-6.0, 2.0, (L, S))
            special = rng.permutation(L)[:min(L // 4, 12)]  # depths whose term is exactly 0 (tau 0 and 1e-20) or loses its exp (750)
            tau[special] = np.resize(np.array([0.0, 1.0e-20, 750.0]), len(special))[:, None]
        self.geometry = synthetic.make_geometry(S)
        self.time_explosion = self.geometry.time_explosion
        self.volume = self.geometry.volume
        self.t_sim = T_SIM
        rho = np.linspace(1.0, 0.3, S)
        self.op = st.OpacityState(1.0e9 * rho, np.full(S, 9000.0), nu, tau, P, self.level_of_line, edge, ttype, dest, tline)
        cfg = st.MonteCarloConfiguration()
        cfg.LINE_INTERACTION_TYPE = st.LINE_INTERACTION_TYPES[mode]
        self.config = cfg
        self.grid = synthetic.make_spectrum_grid(16)
        # estimators: different in every shell; `estimator_decades` on either side of 1e-6
        self.j_blue = 1.0e-8 * 10.0 ** rng.uniform(-estimator_decades, estimator_decades, (L, S))
        self.edotlu = 1.0e-6 * 10.0 ** rng.uniform(-estimator_decades, estimator_decades, (L, S)) if edotlu is None else np.asarray(edotlu, dtype=np.float64)
        self.j_blue[rng.permutation(L)[:max(1, L // 16)]] = 0.0
        self._exact = None

    # -- what the kernels' tuning sees
    def in_lengths(self):
        return np.bincount(self.row_dst, minlength=self.K) if self.mode == "macroatom" else np.zeros(self.K, dtype=np.int64)

    def widths(self):
        return {"level index": row_paths(self.lines_of_level), "incoming rows": row_paths(self.in_lengths())}

    def w(self):
        """(r + n + 3) u of this table."""
        return (int(self.in_lengths().max(initial=0)) + int(self.lines_of_level.max(initial=0)) + 3) * U


def norm_e(case):
    return 1 / (case.t_sim * case.volume)


def norm_j(case):
    """sf_shell_kernel: jblue_norm_num / (four_pi_tsim * volume), the two factors formed on the host."""
    return (C_LIGHT * case.time_explosion) / ((4 * 3.141592653589793 * case.t_sim) * case.volume)


def exp_tau(case):
    tau = case.op.tau_sobolev
    return oracle.exp_array(-tau.ravel(), 1).reshape(tau.shape)


def terms(case):
    """norm_e (1 - exp(-tau)) Edotlu [L, S], left to right, every product a rounding of its own."""
    return norm_e(case)[None, :] * (1 - exp_tau(case)) * case.edotlu


# ---- the exact solve -----------------------------------------------------------------------------------------------------------------

def exact_level_sums(case):
    """e[s][k] as Fractions."""
    t = terms(case)
    out = []
    for s in range(case.S):
        e = [Fraction(0)] * case.K
        for l in range(case.L):
            e[int(case.level_of_line[l])] += Fraction(float(t[l, s]))
        out.append(e)
    return out


def _components(K, src, dst):
    from scipy import sparse as sp
    from scipy.sparse.csgraph import connected_components
    g = sp.coo_matrix((np.ones(len(src)), (src, dst)), shape=(K, K))
    n, label = connected_components(g, directed=False)
    groups = [[] for _ in range(n)]
    for k in range(K):
        groups[label[k]].append(k)
    return groups


def _mp_solve(A, b):
    """x with (A x = b) by mpmath at 50 digits; the residual is checked, in that precision, to 1e-30 of every component."""
    import mpmath as mp
    from mpmath.libmp import to_rational
    with mp.workdps(50):
        n = len(b)
        f = lambda v: mp.mpf(v.numerator) / mp.mpf(v.denominator)
        Am = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                if A[i][j]:
                    Am[i, j] = f(A[i][j])
        bm = mp.matrix([f(v) for v in b])
        x = mp.lu_solve(Am, bm)
        r = Am * x - bm
        for i in range(n):
            assert abs(r[i]) <= mp.mpf("1e-30") * abs(x[i]), (i, r[i], x[i])
        out = []
        for i in range(n):
            p, q = to_rational(x[i]._mpf_)
            out.append(Fraction(int(p), int(q)))
        return out


def _gauss(A, b):
    """Gaussian elimination in Fractions (A is I - Q^T with a convergent Q >= 0: the pivots are positive)."""
    n = len(b)
    A = [row[:] for row in A]
    b = b[:]
    for c in range(n):
        assert A[c][c] > 0
        for r in range(c + 1, n):
            if A[r][c]:
                f = A[r][c] / A[c][c]
                for j in range(c, n):
                    A[r][j] -= f * A[c][j]
                b[r] -= f * b[c]
    x = [Fraction(0)] * n
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - sum(A[r][j] * x[j] for j in range(r + 1, n))) / A[r][r]
    return x


def solve_exact(K, src, dst, q, rhs, stats=None):
    """x with x_k = rhs_k + sum over the rows t with dst[t] == k of q[t] x[src[t]], exactly (see the module text).  Rows of probability 0
    do not exist for the structure.  stats (a dict) counts the components by the way they were solved."""
    keep = np.flatnonzero(np.asarray(q) != 0.0)
    src, dst, q = np.asarray(src)[keep], np.asarray(dst)[keep], [Fraction(float(v)) for v in np.asarray(q)[keep]]
    incoming = [[] for _ in range(K)]
    for t in range(len(src)):
        incoming[int(dst[t])].append((int(src[t]), q[t]))
    x = list(rhs)
    for comp in _components(K, src, dst):
        if len(comp) == 1 and not incoming[comp[0]]:
            continue
        inside = set(comp)
        # Kahn: a level is ready when every level that jumps into it is done
        waiting = {k: sum(1 for s_, _ in incoming[k]) for k in comp}
        outgoing = {k: [] for k in comp}
        for k in comp:
            for s_, _ in incoming[k]:
                assert s_ in inside
                outgoing[s_].append(k)
        ready = [k for k in comp if waiting[k] == 0]
        done = 0
        order = []
        while ready:
            k = ready.pop()
            order.append(k)
            done += 1
            for d in outgoing[k]:
                waiting[d] -= 1
                if waiting[d] == 0:
                    ready.append(d)
        if done == len(comp):
            for k in order:
                x[k] = rhs[k] + sum((qv * x[s_] for s_, qv in incoming[k]), Fraction(0))
            how = "acyclic"
        else:
            at = {k: i for i, k in enumerate(comp)}
            n = len(comp)
            A = [[Fraction(int(i == j)) for j in range(n)] for i in range(n)]
            for k in comp:
                for s_, qv in incoming[k]:
                    A[at[k]][at[s_]] -= qv
            b = [rhs[k] for k in comp]
            sol = _gauss(A, b) if n <= EXACT_CYCLIC else _mp_solve(A, b)
            how = "cyclic, Fractions" if n <= EXACT_CYCLIC else "cyclic, mpmath"
            for k in comp:
                x[k] = sol[at[k]]
        if stats is not None:
            stats[how] = stats.get(how, 0) + 1
    return x


def exact(case):
    """{"e", "C", "B": [S][K] Fractions, "how": how the components were solved}; computed once per case."""
    if case._exact is None:
        e = exact_level_sums(case)
        stats = {}
        if case.mode == "macroatom" and len(case.row_src):
            C = [solve_exact(case.K, case.row_src, case.row_dst, case.row_q[:, s], e[s], stats) for s in range(case.S)]
            B = [solve_exact(case.K, case.row_src, case.row_dst, case.row_q[:, s], C[s]) for s in range(case.S)]
        else:
            C, B = e, e
        case._exact = {"e": e, "C": C, "B": B, "how": stats}
    return case._exact


def level_bound(case, factor=2, truncation=1.0e-14):
    """[S][K] Fractions: factor w B_k + truncation C_k."""
    ex = exact(case)
    w = Fraction(case.w())
    return [[factor * w * ex["B"][s][k] + Fraction(truncation) * ex["C"][s][k] for k in range(case.K)] for s in range(case.S)]


def worst_ratio(case, c_levels, bound, want="C"):
    """max over (shell, level) of |c_levels[k, s] - exact| / bound, as a float, with where it is; a level whose exact value is 0 must be
    exactly 0 (ratio inf otherwise).  c_levels is [K, S], as the engine returns e_dot_u."""
    ex = exact(case)[want]
    worst, where = 0.0, None
    for s in range(case.S):
        for k in range(case.K):
            got, ref = float(c_levels[k, s]), ex[s][k]
            if not np.isfinite(got):
                ratio = float("inf")
            elif ref == 0:
                ratio = 0.0 if got == 0.0 else float("inf")
            else:
                ratio = float(abs(Fraction(got) - ref) / bound[s][k])
            if ratio > worst:
                worst, where = ratio, (s, k)
    return worst, where


def sum_bound(case):
    """[S][K]: (n_k + 1) u e_k, the bound of section (a) on a level's sum of n_k terms in any order."""
    e = exact(case)["e"]
    return [[Fraction(int(case.lines_of_level[k]) + 1) * Fraction(U) * e[s][k] for k in range(case.K)] for s in range(case.S)]


# ---- plain fp64 iterations -----------------------------------------------------------------------------------------------------------

def _csr_in(case, s):
    """Q^T of shell s in CSR with duplicate entries kept (every row of the table is a term of its own)."""
    from scipy import sparse as sp
    order = np.argsort(case.row_dst, kind="stable")
    ptr = np.concatenate(([0], np.cumsum(np.bincount(case.row_dst, minlength=case.K))))
    return sp.csr_matrix((case.row_q[order, s], case.row_src[order], ptr), shape=(case.K, case.K))


def serial_level_sums(case):
    """e [K, S] in fp64: the terms of a level added one after the other, ascending line ids, from 0.0."""
    t = terms(case)
    e = np.zeros((case.K, case.S))
    for l in range(case.L):
        e[case.level_of_line[l]] += t[l]
    return e


def serial_fixed_point(case, max_iterations=2_000_000):
    """(x [K, S], iterations [S]): x <- e + Q^T x from x = e in fp64, every sum serial, until x no longer changes in any component."""
    e = serial_level_sums(case)
    if case.mode != "macroatom" or not len(case.row_src):
        return e, [0] * case.S
    out, its = np.empty_like(e), []
    for s in range(case.S):
        QT = _csr_in(case, s)
        x = e[:, s].copy()
        for it in range(1, max_iterations + 1):
            x_new = e[:, s] + QT @ x
            same = np.array_equal(x_new, x)
            x = x_new
            if same:
                break
        else:
            raise RuntimeError("no fixed point")
        out[:, s] = x
        its.append(it)
    return out, its


def former_rule(QT, e, check_every=16, rtol=1.0e-14, max_iterations=1_000_000):
    """The stop rule the header stated before this module existed: x <- e + Q^T x from x = e, and every `check_every` iterations stop when
    max|dx| <= rtol max|x|.  Returns (x, iterations).  Kept as the record of what that rule accepts."""
    x = e.copy()
    for it in range(1, max_iterations + 1):
        x_new = e + QT @ x
        dx = np.abs(x_new - x).max()
        x = x_new
        if it % check_every == 0 and dx <= rtol * np.abs(x).max():
            return x, it
    raise RuntimeError("not converged")


def two_block_system(scale, p):
    """(Q^T dense [4, 4], e [4], exact solution as Fractions): a strong two-level block (jumps 0.3 / 0.2, e = (1, 0.5)) beside a weak one
    (jump p both ways, e = (scale, 0))."""
    QT = np.zeros((4, 4))
    QT[1, 0], QT[0, 1] = 0.3, 0.2   # level 0 -> 1 with 0.3, 1 -> 0 with 0.2
    QT[3, 2], QT[2, 3] = p, p
    e = np.array([1.0, 0.5, scale, 0.0])
    src, dst, q = [0, 1, 2, 3], [1, 0, 3, 2], [0.3, 0.2, p, p]
    return QT, e, solve_exact(4, src, dst, q, [Fraction(float(v)) for v in e])


# ---- the closing kernel, bit for bit ----------------------------------------------------------------------------------------------------

def close_bitwise(case, c_levels, wavelength_cm=None):
    """att_S_ul, Jred_lu, Jblue_lu [S * L] shell-major from the level rates c_levels [K, S]: sf_close_kernel's expressions in its order --
    a = wave * (p * c) * t_sim / (4 pi); jb = j_blue * norm_j; jred = jb * exp_tau + a, every operation a rounding of its own."""
    op = case.op
    emission = np.flatnonzero(op.transition_type == -1)
    row_of_line = np.empty(case.L, dtype=np.int64)
    row_of_line[op.transition_line_id[emission]] = emission
    wave = (C_LIGHT / op.line_list_nu) if wavelength_cm is None else np.asarray(wavelength_cm, dtype=np.float64)
    p = op.transition_probabilities[row_of_line]                      # [L, S]
    c = np.asarray(c_levels)[case.level_of_line]                      # [L, S]
    four_pi = 4 * 3.141592653589793
    a = wave[:, None] * (p * c) * case.t_sim / four_pi
    jb = case.j_blue * norm_j(case)[None, :]
    jred = jb * exp_tau(case) + a
    flat = lambda v: np.ascontiguousarray(v.T).ravel()
    return {"att_S_ul": flat(a), "Jred_lu": flat(jred), "Jblue_lu": flat(jb)}


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

SHAPES = {1: dict(K=300, fill_max=4), 4: dict(K=70, fill_max=8), 16: dict(K=21, fill_max=40)}  # rows of the index per group width
_cases = {}


def _cached(f):
    def g(*a):
        k = (f.__name__,) + a
        if k not in _cases:
            _cases[k] = f(*a)
        return _cases[k]
    return g


@_cached
def row_sum_case(G):
    """(a) downbranch, S = 3: the menu as lines per level; G = 0: the one-level table (K = 1, five lines)."""
    rng = np.random.default_rng(100 + G)
    lengths = np.array([5]) if G == 0 else menu_lengths(G, SHAPES[G]["K"], rng, SHAPES[G]["fill_max"])
    return Case(f"row sums G={G}", "downbranch", lengths, [], [], np.zeros((0, 3)), 3, seed=200 + G, estimator_decades=15.0)


def _ranks(K, rng, depth):
    """A rank 0 .. depth per level, the last level and the first ones low (they hold the long rows): jumps go to strictly lower ranks."""
    rank = rng.integers(0, depth + 1, K)
    rank[:10] = 0
    rank[K - 1] = 0
    rank[K // 2] = depth
    return rank


@_cached
def acyclic_case(G):
    """(b) macroatom, S = 3: the menu as incoming rows per level; sources are drawn among the levels of higher rank (ranks 0 .. 12, so no
    chain has more than 12 jumps), with repetition -- a level with 600 incoming rows out of 20 others sees every pair many times."""
    rng = np.random.default_rng(300 + G)
    K = SHAPES[G]["K"]
    in_len = menu_lengths(G, K, rng, SHAPES[G]["fill_max"])
    rank = _ranks(K, rng, 12)
    src, dst = [], []
    for k in range(K):
        higher = np.flatnonzero(rank > rank[k])
        if len(higher) == 0:
            in_len[k] = 0
            continue
        src += rng.choice(higher, int(in_len[k])).tolist()
        dst += [k] * int(in_len[k])
    in_len = np.bincount(np.asarray(dst), minlength=K)
    assert row_paths(in_len)[0] == G and in_len[K - 1] == LONG_STEPS * G + 1 and (in_len == 0).any()
    src, dst = np.asarray(src), np.asarray(dst)
    shuffle = rng.permutation(len(src))  # (table order is not index order)
    src, dst = src[shuffle], dst[shuffle]
    out_n = np.bincount(src, minlength=K)
    q = rng.uniform(0.2, 1.0, (len(src), 3)) * 0.9 / out_n[src][:, None]
    lines = rng.integers(0, 4, K)
    lines[rank == 12] = np.maximum(lines[rank == 12], 1)  # (the top of every chain has something to hand down)
    lines[:3] = 0
    case = Case(f"acyclic G={G}", "macroatom", lines, src, dst, q, 3, seed=400 + G, estimator_decades=15.0)
    pairs = set()
    assert any((a, b) in pairs or pairs.add((a, b)) for a, b in zip(case.row_src.tolist(), case.row_dst.tolist()))  # duplicates exist
    return case


STOP_K, STOP_S = 300, 5
STOP_TABLES = {"1e-6, 0.99": (1.0e-6, 0.99), "1e-8, 0.999": (1.0e-8, 0.999)}
STOP_POSITIONS = (0, 63, 64, 255, 256, STOP_K - 1)
STOP_SHELLS = (0, STOP_S // 2, STOP_S - 1)


@_cached
def stop_rule_case(table, position, shell):
    """(c) K = 300 levels in 150 independent two-level blocks, one line per level, S = 5.  Every block is strong (jumps about 0.3 / 0.2,
    e about (1, 0.5)) except, in `shell` only, the one whose first level is `position` (its partner is the next level; the level before
    for the last one): there it jumps with p both ways and has e = (scale, 0) -- the partner's line has an Edotlu of 0."""
    scale, p = STOP_TABLES[table]
    rng = np.random.default_rng(500 + 7 * position + shell)
    K, S = STOP_K, STOP_S
    partner = position + 1 if position + 1 < K else position - 1
    rest = [k for k in range(K) if k not in (position, partner)]
    pairs = [(position, partner)] + [(rest[i], rest[i + 1]) for i in range(0, len(rest), 2)]
    src, dst, q = [], [], []
    for i, (a, b) in enumerate(pairs):
        qa, qb = 0.3 * rng.uniform(0.9, 1.1, S), 0.2 * rng.uniform(0.9, 1.1, S)
        if i == 0:
            qa[shell] = qb[shell] = p
        src += [a, b]
        dst += [b, a]
        q += [qa, qb]
    # Edotlu that gives e_k of about the value wanted: e = norm_e (1 - exp(-tau)) Edotlu with tau = 1 on every line
    want = np.empty((K, S))
    for a, b in pairs:
        want[a], want[b] = rng.uniform(0.5, 1.5, S), 0.5 * rng.uniform(0.5, 1.5, S)
    want[position, shell], want[partner, shell] = scale, 0.0
    probe = Case("probe", "macroatom", np.ones(K, np.int64), src, dst, q, S, seed=600, tau=np.ones((K, S)))  # (the same seed deals the lines the same way)
    per_unit = norm_e(probe) * (1 - np.exp(-1.0))
    edotlu = (want / per_unit[None, :])[probe.level_of_line]
    return Case(f"stop rule {table} at level {position}, shell {shell}", "macroatom", np.ones(K, np.int64), src, dst, q, S, seed=600,
                edotlu=edotlu, tau=np.ones((K, S)))


@_cached
def mixed_case():
    """(c) the case the max-norm rule handled: 41 levels, every level jumps on to the next (a ring: irreducible) and to two random ones,
    with a total of 0.85 .. 0.92 per level and shell: contraction rate about 0.9.  One to three lines per level, S = 3."""
    rng = np.random.default_rng(700)
    K, S = 41, 3
    src, dst, q = [], [], []
    for k in range(K):
        total = rng.uniform(0.85, 0.92, S)
        split = rng.uniform(0.2, 1.0, (3, S))
        split *= total / split.sum(axis=0)
        for j, d in enumerate([(k + 1) % K] + rng.integers(0, K, 2).tolist()):
            src.append(k)
            dst.append(d)
            q.append(split[j])
    return Case("well mixed, rate 0.9", "macroatom", rng.integers(1, 4, K), src, dst, q, S, seed=701)


@_cached
def stride_case():
    """(e) S = 2, 262 144 + 257 lines on five levels (one without lines), a short acyclic chain of jumps: sf_close_kernel's grid stride wraps."""
    L = 262144 + 257
    lines = np.array([100000, 0, 62401, 99999, 1])
    assert lines.sum() == L
    rng = np.random.default_rng(800)
    src, dst = [4, 4, 3, 2, 2], [3, 1, 1, 0, 0]
    return Case("grid stride", "macroatom", lines, src, dst, rng.uniform(0.05, 0.2, (5, 2)), 2, seed=801)
