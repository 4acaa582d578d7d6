"""The yardstick of the last-interaction decomposition (tardis_mc_packet_decomposition, include/tardis_mc.h): plain numpy on the
per-packet arrays that get_results returns (themselves pinned to the oracle).

Double cells: boolean masks as the header defines them, ``np.digitize`` for the bin (numpy.histogram's rule: left-closed bins, the
last one also closed on the right, nothing outside the grid), ``math.fsum`` over each cell's weights -- the correctly rounded sum --
and each cell's addend count ``n``.  Integer outputs: ``np.bincount`` and ``np.add.at``.

``assert_matches`` holds a result against it: integers exactly; a double cell within ``n * 2**-53 * fsum`` -- all addends are
non-negative, so any summation order of n of them errs by at most (n - 1) u relatively (u = 2**-53), the weight is the same single
IEEE division on both sides, and fsum itself is correctly rounded (u more) --; a cell with n = 0 exactly 0.
"""
import math

import numpy as np

LINE, ESCATTERING, NO_INTERACTION = 2, 4, -1
U = 2.0 ** -53
DOUBLE_KEYS = ("emission", "absorption", "no_interaction", "electron_scatter")
INT_KEYS = ("shell_packets", "line_emit_packets", "line_absorb_packets")
COUNT_KEYS = ("n_selected", "n_line", "n_electron_scatter", "n_no_interaction")


def bins_of(x, grid):
    """(inside, k): which values have a bin on ``grid``, and the bin of those."""
    B = len(grid) - 1
    inside = (x >= grid[0]) & (x <= grid[-1])
    k = np.digitize(x[inside], grid) - 1
    k[k == B] = B - 1  # x == grid[-1]: the last bin is closed on the right
    return inside, k


def _cells(rows, k, w, shape):
    """fsum of the weights of every (row, k) cell and the number of addends there."""
    total, count = np.zeros(shape), np.zeros(shape, dtype=np.int64)
    flat = rows * shape[-1] + k
    order = np.argsort(flat, kind="stable")
    flat, w = flat[order], w[order]
    cuts = np.flatnonzero(np.diff(flat)) + 1
    for cell, ws in zip(flat[np.r_[0, cuts]] if len(flat) else [], np.split(w, cuts)):
        total.flat[cell] = math.fsum(ws)
        count.flat[cell] = len(ws)
    return total, count


def decompose(output_nus, output_energies, time_of_simulation, grid, trackers, line_class, n_classes, n_shells, nu_start=0.0,
              nu_end=np.inf):
    """``trackers``: anything with the last-interaction arrays interaction_type, interaction_line_emit_id,
    interaction_line_absorb_id, before_nu, shell_id.  Returns (values, addend counts of the double cells)."""
    grid = np.asarray(grid, dtype=np.float64)
    cls = np.asarray(line_class, dtype=np.int64)
    C, B, S, L = int(n_classes), len(grid) - 1, int(n_shells), len(cls)
    assert C >= 1 and (L == 0 or (cls.min() >= 0 and cls.max() < C))
    nu, en = np.asarray(output_nus), np.asarray(output_energies)
    sel = (en >= 0) & (nu > nu_start) & (nu < nu_end)
    lum = en / time_of_simulation
    itype = np.asarray(trackers.interaction_type)
    line, es, none = sel & (itype == LINE), sel & (itype == ESCATTERING), sel & (itype == NO_INTERACTION)
    emit, absorb = np.asarray(trackers.interaction_line_emit_id)[line], np.asarray(trackers.interaction_line_absorb_id)[line]
    shell = np.asarray(trackers.shell_id)
    out, n = {}, {}
    inside, k = bins_of(nu[line], grid)
    out["emission"], n["emission"] = _cells(cls[emit[inside]], k, lum[line][inside], (C, B))
    inside, k = bins_of(np.asarray(trackers.before_nu)[line], grid)
    out["absorption"], n["absorption"] = _cells(cls[absorb[inside]], k, lum[line][inside], (C, B))
    for key, mask in (("no_interaction", none), ("electron_scatter", es)):
        inside, k = bins_of(nu[mask], grid)
        out[key], n[key] = _cells(np.zeros(len(k), dtype=np.int64), k, lum[mask][inside], (B,))
    sp = np.zeros((C + 1, S), dtype=np.int64)
    np.add.at(sp, (cls[emit], shell[line]), 1)
    np.add.at(sp, (np.full(int(es.sum()), C), shell[es]), 1)
    out["shell_packets"] = sp
    out["line_emit_packets"] = np.bincount(emit, minlength=L).astype(np.int64)
    out["line_absorb_packets"] = np.bincount(absorb, minlength=L).astype(np.int64)
    out.update(n_selected=int(sel.sum()), n_line=int(line.sum()), n_electron_scatter=int(es.sum()), n_no_interaction=int(none.sum()))
    return out, n


def within_bound(got, want, n):
    """|got - want| <= n u want per cell, and exactly 0 where n = 0."""
    got, want, n = np.asarray(got), np.asarray(want), np.asarray(n)
    return bool(np.all(np.abs(got - want) <= n * U * want) and np.all(got[n == 0] == 0))


def assert_matches(got, want, n, what=""):
    for key in COUNT_KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in INT_KEYS:
        assert got[key].dtype == np.int64 and got[key].shape == want[key].shape, (what, key)
        assert np.array_equal(got[key], want[key]), (what, key)
    for key in DOUBLE_KEYS:
        assert got[key].shape == want[key].shape, (what, key)
        err = np.abs(got[key] - want[key])
        worst = float(np.max(err / np.where(want[key] > 0, want[key] * U, 1.0))) if err.size else 0.0
        print(f"{what} {key}: cells {int((n[key] > 0).sum())}, most addends {int(n[key].max()) if n[key].size else 0}, "
              f"worst error {worst:.2f} u")
        assert within_bound(got[key], want[key], n[key]), (what, key, worst)
