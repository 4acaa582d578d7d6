"""The yardstick of the photo-ionisation and heating estimators (csrc/bf_estimators.hpp): a NumPy restatement of the accumulate pass in
the operation order include/tardis_mc.h spells out -- every product, quotient and difference a rounding of its own, exp the
transport's own (plasma_update_ref.exp) -- on a list of segment records (nu, ed, shell).  The per-term values are formed in that
order; a cell's sum is math.fsum of its terms, the correctly rounded sum: the device adds the same non-negative terms in an
unspecified order, so it agrees with this to (terms - 1) 2^-53 relative, and the tests hold it to terms 2^-52.

The bracket of a frequency in a block is that of tests/continuum_ref.query: hi = clip(searchsorted(block, nu, "left"), 1, n - 1), so a
block's first frequency takes the first interval and gives x_sect[first]."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plasma_update_ref as ref  # noqa: E402

exp = ref.exp
K_BOLTZMANN, H_PLANCK = ref.K_BOLTZMANN, ref.H_PLANCK
TABLES = ("photo_ion", "stim_recomb", "bf_heating", "stim_recomb_cooling")


def terms(cd, t_electrons, nu, ed, shell):
    """Per continuum c: (the indices of the records at which c is current, inc, inc bfac, heat, heat bfac of those records)."""
    nu, ed = np.asarray(nu, dtype=np.float64), np.asarray(ed, dtype=np.float64)
    shell = np.asarray(shell, dtype=np.int64)
    edge = np.asarray(cd.block_edge, dtype=np.int64)
    grid, x_sect = np.asarray(cd.nu, dtype=np.float64), np.asarray(cd.x_sect, dtype=np.float64)
    beta_e = 1 / (K_BOLTZMANN * np.asarray(t_electrons, dtype=np.float64))
    bfac = exp((H_PLANCK * nu) * (-beta_e[shell])) if len(nu) else np.zeros(0)
    out = []
    for c in range(len(edge) - 1):
        a, b = int(edge[c]), int(edge[c + 1])
        blk, x = grid[a:b], x_sect[a:b]
        idx = np.flatnonzero((blk[0] <= nu) & (nu <= blk[-1]))
        v = nu[idx]
        hi = np.clip(np.searchsorted(blk, v, side="left"), 1, len(blk) - 1)
        lo = hi - 1
        interval, hw, lw = blk[hi] - blk[lo], v - blk[lo], blk[hi] - v
        x_c = ((x[hi] * hw) + (x[lo] * lw)) / interval
        ex = ed[idx] * x_c
        inc = ex / v
        heat = ex * (1.0 - blk[0] / v)
        out.append((idx, inc, inc * bfac[idx], heat, heat * bfac[idx]))
    return out


def tables(cd, t_electrons, n_shells, nu, ed, shell):
    """The five tables [NC, S] of the records: the four sums (math.fsum per cell) and the statistics (int64)."""
    shell = np.asarray(shell, dtype=np.int64)
    per = terms(cd, t_electrons, nu, ed, shell)
    NC, S = len(per), int(n_shells)
    out = {name: np.zeros((NC, S)) for name in TABLES}
    out["statistics"] = np.zeros((NC, S), dtype=np.int64)
    for c, (idx, *vals) in enumerate(per):
        s_of = shell[idx]
        for s in range(S):
            m = s_of == s
            out["statistics"][c, s] = int(m.sum())
            for name, v in zip(TABLES, vals):
                out[name][c, s] = math.fsum(v[m])
    return out


def add(a, b):
    """Two tables' worth of records accumulated: the statistics add; the sums are NOT the fsum of the union (two roundings), so this
    returns the pair's float sum -- within one rounding of it, which the tolerance of a cell (terms 2^-52) covers."""
    return {k: a[k] + b[k] for k in a}


def rates(tab, time_of_simulation, volume):
    """gamma_est, stim_est [NC, S]: norm[s] = 1.0 / ((time_of_simulation volume[s]) h), each table times norm."""
    norm = 1.0 / ((time_of_simulation * np.asarray(volume, dtype=np.float64)) * H_PLANCK)
    return {"gamma_est": tab["photo_ion"] * norm[None, :], "stim_est": tab["stim_recomb"] * norm[None, :]}


def shell_fsum(values, shell, n_shells):
    """math.fsum of ``values`` per shell."""
    values, shell = np.asarray(values, dtype=np.float64), np.asarray(shell, dtype=np.int64)
    return np.array([math.fsum(values[shell == s]) for s in range(int(n_shells))])
