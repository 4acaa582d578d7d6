"""The BLOCKED order of the NLTE solve (tardis_amd/csrc/nlte_excitation.hpp: nlte_panel_kernel / nlte_trailing_kernel /
nlte_backsolve_kernel) restated in NumPy, to be compared with the unblocked yardstick nlte_excitation_ref.lu_solve: a right-looking LU
in panels of NB columns.

Inside a panel the steps are serial, restricted to the panel's columns; the row swaps of a step also move the multipliers the panel has
already stored, which stay in place below the diagonal.  Then, per trailing column j (b is the last one): the panel's swaps in panel
order, the row block by the recurrence u_k = ((a_k - l_k0 u_0) - l_k1 u_1) - ..., and every entry below as acc = a_ij followed by
acc = acc - l_ik u_kj for the panel's k in ascending order.  NumPy rounds every product and every difference on its own, so each entry
sees the roundings of the unblocked order in the same order: x and the swap steps are array_equal.

`summed_first=True` is the re-association a matrix-product unit or a dot-product accumulator would make -- the NB products of an entry
summed, then subtracted once.  It is kept to show that the comparison can fail: its bits differ."""
import numpy as np

from nlte_excitation_ref import NlteSolveError

PANEL_COLUMNS = 32  # nlte::PANEL_COLUMNS (tests/test_nlte_blocked_plan.py reads the header's value)


def blocked_lu_solve(m, b, nb=PANEL_COLUMNS, summed_first=False):
    """x, and the steps at which two rows were swapped.  m and b are not modified."""
    n = len(b)
    a = np.empty((n, n + 1))  # b is one more trailing column
    a[:, :n], a[:, n] = m, b
    swaps = []
    with np.errstate(all="ignore"):
        for c0 in range(0, n, nb):
            c1 = min(n, c0 + nb)
            rows = []
            for k in range(c0, c1):  # the panel, serial in k, on columns c0 .. c1 - 1 only
                p = k + int(np.argmax(np.abs(a[k:, k])))
                rows.append(p)
                if p != k:
                    a[[k, p], c0:c1] = a[[p, k], c0:c1]  # (the multipliers of columns c0 .. k - 1 go with their rows)
                    swaps.append(k)
                pivot = a[k, k]
                if pivot == 0.0 or not np.isfinite(pivot):
                    raise NlteSolveError("zero or non-finite pivot", k)
                a[k + 1:, k] = a[k + 1:, k] / pivot
                a[k + 1:, k + 1:c1] = a[k + 1:, k + 1:c1] - a[k + 1:, k][:, None] * a[k, k + 1:c1][None, :]
            for k, p in zip(range(c0, c1), rows):  # the panel's swaps on the trailing columns, in panel order
                if p != k:
                    a[[k, p], c1:] = a[[p, k], c1:]
            for k in range(c0, c1):  # the row block: u_k from the rows above it, in ascending order
                for kk in range(c0, k):
                    a[k, c1:] = a[k, c1:] - a[k, kk] * a[kk, c1:]
            if summed_first:
                a[c1:, c1:] = a[c1:, c1:] - a[c1:, c0:c1] @ a[c0:c1, c1:]
            else:
                for k in range(c0, c1):  # the tile update, term by term
                    a[c1:, c1:] = a[c1:, c1:] - a[c1:, k][:, None] * a[k, c1:][None, :]
        rhs = a[:, n].copy()
        x = np.zeros(n)
        for j in range(n - 1, -1, -1):
            x[j] = rhs[j] / a[j, j]
            rhs[:j] = rhs[:j] - a[:j, j] * x[j]
    if not np.all(np.isfinite(x)):
        raise NlteSolveError("a population that is not finite", n)
    if x[0] == 0.0:
        raise NlteSolveError("x[0] == 0", n)
    return x, swaps


def random_systems(n, count, seed):
    """Seeded dense systems of order n: rows are swapped at nearly every step and the pivot row lies anywhere below the diagonal."""
    rng = np.random.default_rng([seed, n])
    return rng.standard_normal((count, n, n)), rng.standard_normal((count, n))
