"""Plain numpy / pandas / scipy restatement of the reference's ``make_source_function``
(tardis/spectrum/formal_integral/source_function.py), written the way the reference writes it: a group-by sum for
``e_dot_u``, a ``coo_matrix`` for the internal jumps and one linear solve per shell.  The checker of
tardis_mc_source_function (tests/test_source_function_gpu.py); a helper module, not a test file.

All 2-D inputs use the reference's [lines or transitions, shells] layout.  ``solver``: "dense" (numpy.linalg.solve of
(I - Q)^T per shell, for tables of at most about 3e3 levels), "fixed_point" (x <- e + Q^T x from x = e until
x no longer changes, the iteration the device runs, with a sparse matvec) or "none" (downbranch: C = e_dot_u).
"""
import numpy as np
import pandas as pd
from scipy import sparse as sp

C_LIGHT = 2.99792458e10  # the engine's speed of light (tardis/constants.py, CODATA 2010 cgs)


def jump_matrix(opacity_state, shell):
    """Q_s as the reference builds it: coo_matrix((probabilities, (source level, destination level))) over the rows with
    transition_type >= 0; duplicates add."""
    op = opacity_state
    edge = np.asarray(op.macro_block_edge_index)
    n_levels = len(edge) - 1
    ttype = np.asarray(op.transition_type)
    source_level = np.repeat(np.arange(n_levels), np.diff(edge))
    internal = ttype >= 0
    q = np.asarray(op.transition_probabilities)[internal, shell]
    return sp.coo_matrix((q, (source_level[internal], np.asarray(op.destination_level_id)[internal])),
                         shape=(n_levels, n_levels)).tocsr()


def fixed_point(Q, e, max_iterations=20000):
    """x <- e + Q^T x from x = e until an iteration changes no component (the device's rule; with e, Q >= 0 the iterates never decrease, so
    the iteration ends, at the fixed point of the rounded map); returns (x, iterations)."""
    QT = Q.T.tocsr()
    x = e.copy()
    for it in range(1, max_iterations + 1):
        x_new = e + QT @ x
        same = np.array_equal(x_new, x)
        x = x_new
        if same:
            return x, it
    raise RuntimeError(f"fixed point not converged after {max_iterations} iterations")


def level_rates(opacity_state, edotlu_estimator, time_of_simulation, volume):
    """e_dot_u [levels, S]: the normalised Edotlu summed over the lines of every upper level (pandas group-by, as the
    reference does it)."""
    op = opacity_state
    n_levels = len(op.macro_block_edge_index) - 1
    Edotlu_norm_factor = 1 / (time_of_simulation * np.asarray(volume, dtype=np.float64))
    exptau = 1 - np.exp(-np.asarray(op.tau_sobolev))
    Edotlu = Edotlu_norm_factor * exptau * np.asarray(edotlu_estimator)
    upper = np.asarray(op.line2macro_level_upper)
    return pd.DataFrame(Edotlu).groupby(upper).sum().reindex(np.arange(n_levels), fill_value=0.0).to_numpy()


def make_source_function(opacity_state, j_blue_estimator, edotlu_estimator, time_of_simulation, volume, time_explosion,
                         solver="dense", wavelength_cm=None, threads=1):
    """Returns a dict: att_S_ul, Jred_lu, Jblue_lu flat shell-major [S * L]; e_dot_u [levels, S] (C for a macro-atom
    solver); iterations (list per shell, fixed_point only).  ``threads``: shells solved side by side (the timing tool)."""
    op = opacity_state
    tau = np.asarray(op.tau_sobolev)
    L, S = tau.shape
    edge = np.asarray(op.macro_block_edge_index)
    n_levels = len(edge) - 1
    ttype = np.asarray(op.transition_type)
    prob = np.asarray(op.transition_probabilities)
    volume = np.asarray(volume, dtype=np.float64)

    e_dot_u = level_rates(op, edotlu_estimator, time_of_simulation, volume)

    iterations = []
    if solver == "none":
        C = e_dot_u
    else:
        if solver not in ("dense", "fixed_point"):
            raise ValueError(solver)

        def solve_shell(s):
            Q = jump_matrix(op, s)
            if solver == "dense":
                return np.linalg.solve((np.eye(n_levels) - Q.toarray()).T, e_dot_u[:, s]), None
            return fixed_point(Q, e_dot_u[:, s])

        if threads > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(threads) as pool:
                solved = list(pool.map(solve_shell, range(S)))
        else:
            solved = [solve_shell(s) for s in range(S)]
        C = np.stack([x for x, _ in solved], axis=1)
        iterations = [it for _, it in solved if it is not None]

    # emission rows: q_ul and the line each ends in
    emission = ttype == -1
    source_level = np.repeat(np.arange(n_levels), np.diff(edge))
    line_of_row = np.asarray(op.transition_line_id)[emission]
    if not np.array_equal(np.sort(line_of_row), np.arange(L)):
        raise ValueError("every line needs exactly one emission row")
    wave = (C_LIGHT / np.asarray(op.line_list_nu)) if wavelength_cm is None else np.asarray(wavelength_cm, dtype=np.float64)
    att_S_ul = np.empty((L, S))
    att_S_ul[line_of_row] = (wave[line_of_row][:, None] * (prob[emission] * C[source_level[emission]]) * time_of_simulation
                             / (4 * np.pi))

    Jbluelu = np.asarray(j_blue_estimator) * (C_LIGHT * time_explosion / (4 * np.pi * time_of_simulation * volume))
    Jredlu = Jbluelu * np.exp(-tau) + att_S_ul
    return {"att_S_ul": att_S_ul.T.ravel(), "Jred_lu": Jredlu.T.ravel(), "Jblue_lu": Jbluelu.T.ravel(), "e_dot_u": C,
            "iterations": iterations}
