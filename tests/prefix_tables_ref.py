"""Exact prefix sums of optical-depth rows, and the adversarial tables of tests/test_prefix_tables_host.py and tests/test_prefix_tables_gpu.py.

The v-packet screening (tardis_amd/csrc/tau_prefix.hpp) and the lane sweep's block skip (tardis_amd/csrc/sweep_skip.hpp) argue their margins from one claim:
every prefix sum the device holds lies within 2^-53 of the exact one, relatively.  `exact_prefix` is the yardstick of that claim: the sums accumulated as
`fractions.Fraction`, which holds every double exactly, so `float()` of an entry is the correctly rounded prefix sum.  No GPU, no engine."""
from fractions import Fraction

import numpy as np

from tardis_amd import state as st, synthetic

# the claim of tau_prefix.hpp, and what the low word's own roundings can add on top: a row of L doubles goes through at most L two-sums whose error terms are
# added in plain double, each addition within 2^-53 of a low word that is itself below L 2^-53 P -- L^2 2^-106 P, less than 2^-70 P for L < 2^15 (2^-76 P)
REL_BOUND = Fraction(1, 2 ** 53) + Fraction(1, 2 ** 70)
N_TABLE_SHELLS = 12
ROW_NAMES = ("lognormal", "ascending", "descending", "tenths", "giant-then-dust", "alternating", "single-one-at-the-end", "subnormals", "negative-zeros",
             "one-1e250", "powers-of-two", "blue-giants")
assert len(ROW_NAMES) == N_TABLE_SHELLS


def exact_prefix(row):
    """P[0 .. L] of a row of L doubles, exactly: P[i] = sum of row[:i]."""
    out, acc = [Fraction(0)], Fraction(0)
    for x in row:
        acc += Fraction(float(x))
        out.append(acc)
    return out


def check_row(p_hat, exact):
    """The entries of `p_hat` against the exact sums: (indices that miss REL_BOUND, largest error in units of 2^-53 P, entries that are not the correctly rounded sum)."""
    bad, worst, not_rounded = [], 0.0, 0
    for i, (h, e) in enumerate(zip(p_hat, exact)):
        h = float(h)
        err = abs(Fraction(h) - e)
        if err == 0:
            continue
        # (the correctly rounded sum is within 2^-53 P: a sum of doubles that lies below the normal range is itself a double, its error 0)
        if h != float(e):
            not_rounded += 1
            if not err <= REL_BOUND * abs(e):
                bad.append(i)
        worst = max(worst, float(err) / (abs(float(e)) * 2.0 ** -53) if e != 0 else float("inf"))
    return bad, worst, not_rounded


def adversarial_rows(n_lines: int, lognormal, seed: int = 11):
    """The twelve rows of ROW_NAMES, `n_lines` doubles each, as [12, n_lines]; `lognormal`: the generator's own row."""
    L = n_lines
    rng = np.random.default_rng(seed)
    rows = np.zeros((N_TABLE_SHELLS, L))
    base = np.asarray(lognormal, dtype=np.float64)
    assert base.shape == (L,)
    rows[0] = base
    rows[1] = np.sort(base)
    rows[2] = np.sort(base)[::-1]
    rows[3] = 0.1
    rows[4] = 1e-7
    rows[4, 0] = 1e10
    rows[5, 0::2] = 1e8
    rows[5, 1::2] = 1e-8
    rows[6, L - 1] = 1.0
    rows[7] = base
    rows[7, rng.choice(L, min(500, L), replace=False)] = 5e-324
    rows[8] = base
    rows[8, rng.choice(L, (L + 1) // 2, replace=False)] = -0.0
    rows[9] = base
    rows[9, L // 3] = 1e250
    rows[10] = 2.0 ** rng.integers(-60, 41, L)
    rows[10, :2] = (2.0 ** 40, 2.0 ** -60)[: min(2, L)]
    rows[11] = base
    rows[11, : min(200, L)] = 1e6 * (1.0 + rng.random(min(200, L)))
    return rows


def with_tau(op, tau_sobolev):
    """`op` with another [n_lines, n_shells] table of optical depths."""
    return st.OpacityState(op.electron_density, op.t_electrons, op.line_list_nu, tau_sobolev, op.transition_probabilities, op.line2macro_level_upper,
                           op.macro_block_edge_index, op.transition_type, op.destination_level_id, op.transition_line_id)


def table_problem(n_lines: int, n_packets: int, n_vpackets: int = 0):
    """A downbranch problem of 12 shells whose shell s carries row s of adversarial_rows; returns (problem, rows [12, n_lines])."""
    prob = synthetic.make_problem(seed=5, n_packets=n_packets, n_shells=N_TABLE_SHELLS, n_lines=n_lines, line_interaction_type="downbranch",
                                  n_vpackets=n_vpackets)
    rows = adversarial_rows(n_lines, np.array(prob.opacity_state.tau_sobolev[:, 0], dtype=np.float64, copy=True))
    prob.opacity_state = with_tau(prob.opacity_state, np.ascontiguousarray(rows.T))
    return prob, rows


def ssk_margin(n_lines: int, rowsum_max: float) -> float:
    """ssk::margin (tardis_amd/csrc/sweep_skip.hpp), operation for operation."""
    return rowsum_max * (1.02 * (float(n_lines) + 16.0) * 2.0 ** -53 + 2.0 ** -48)


# ---- the screening's margin, attacked: three scatter problems without electron scattering whose v-packets come within 1e-12 of the roulette threshold
THRESHOLDS = (10.0 * (1.0 - 1e-13), 10.0, 10.0 * (1.0 + 1e-13))
SCENARIOS = ("drift", "cancellation", "concentrated")
BLUE_FACTOR = 1.2  # lines bluer than this times the bluest packet: no packet and no v-packet ever reaches them


def blue_lines(prob):
    return np.asarray(prob.opacity_state.line_list_nu) > BLUE_FACTOR * prob.packet_collection.initial_nus.max()


def screening_problem(name: str):
    """drift: every tau = 0.1 on 30 shells x 30 000 lines -- a v-packet's depth is a long serial sum of an inexact term, the prefix sums round once.
    cancellation: the same with the blue lines, which nothing reaches, at 1e6 (1 + U): every prefix sum a v-packet reads is ~7e9, its ulp 1e-6.
    concentrated: 2000 lines of tau = 0.02 in a band of 6 % below 1e15 Hz on 20 shells: a crossing passes more than 43 lines, (n + 4) tau_shell > row sum."""
    if name == "concentrated":
        prob = synthetic.make_problem(seed=47, n_packets=1500, n_shells=20, n_lines=2000, line_interaction_type="scatter", n_vpackets=3)
        rng = np.random.default_rng(48)
        prob.opacity_state.line_list_nu[:] = np.sort(1e15 * (1.0 - 0.06 * rng.random(2000)))[::-1]
        prob.opacity_state.tau_sobolev[:, :] = 0.02
    else:
        prob = synthetic.make_problem(seed=47, n_packets=1500, n_shells=30, n_lines=30_000, line_interaction_type="scatter", n_vpackets=3)
        prob.opacity_state.tau_sobolev[:, :] = 0.1
        if name == "cancellation":
            blue = blue_lines(prob)
            rng = np.random.default_rng(49)
            prob.opacity_state.tau_sobolev[blue, :] = 1e6 * (1.0 + rng.random((int(blue.sum()), prob.opacity_state.tau_sobolev.shape[1])))
        else:
            assert name == "drift", name
    cfg = prob.montecarlo_configuration
    cfg.DISABLE_ELECTRON_SCATTERING = True
    cfg.ENABLE_VPACKET_TRACKING = True
    return prob


def lines_per_crossing(geometry, line_list_nu, nu, mu):
    """Lines a v-packet of lab frequency `nu` passes in each shell on its way out from the inner boundary with direction cosine `mu` >= 0 (partial
    relativity: comoving frequency nu (1 - mu r / (c t))) -- from the line list and the geometry alone."""
    r, t = float(geometry.r_inner[0]), float(geometry.time_explosion)
    asc = np.asarray(line_list_nu)[::-1]
    counts = []
    for r_out in geometry.r_outer:
        d = np.sqrt(r_out * r_out - r * r * (1.0 - mu * mu)) - r * mu
        comov_in = nu * (1.0 - mu * r / (st.C_SPEED_OF_LIGHT * t))
        mu = (mu * r + d) / r_out
        r = float(r_out)
        comov_out = nu * (1.0 - mu * r / (st.C_SPEED_OF_LIGHT * t))
        counts.append(int(np.searchsorted(asc, comov_in, side="right") - np.searchsorted(asc, comov_out, side="right")))
    return counts


# ---- the block skip on tables that make its margin M large
SKIP_TABLES = ("blue-giants", "sparse-giants", "one-shell-1e9")


def skip_table(name: str, tau_sobolev, seed: int = 21):
    """A copy of `tau_sobolev` [n_lines, n_shells] with: the 200 bluest lines at 1e6 (1 + U); 40 random lines at 10 ** U(4, 8); one shell times 1e9."""
    tau = np.array(tau_sobolev, dtype=np.float64, copy=True)
    L, S = tau.shape
    rng = np.random.default_rng(seed)
    if name == "blue-giants":
        tau[:200, :] = 1e6 * (1.0 + rng.random((200, S)))
    elif name == "sparse-giants":
        tau[rng.choice(L, 40, replace=False), :] = 10.0 ** rng.uniform(4.0, 8.0, (40, S))
    elif name == "one-shell-1e9":
        tau[:, S // 2] *= 1e9
    else:
        raise ValueError(name)
    return tau


# ---- non-finite and overflowing rows
SPECIAL_TABLES = ("one-inf", "two-1e308")


def special_table(name: str, tau_sobolev):
    """A copy of `tau_sobolev` with +inf on one line of one shell, or 1e308 on two lines of one shell (their row sum overflows)."""
    tau = np.array(tau_sobolev, dtype=np.float64, copy=True)
    L, S = tau.shape
    if name == "one-inf":
        tau[L // 3, S // 2] = np.inf
    elif name == "two-1e308":
        tau[L // 4, S // 2] = 1e308
        tau[(2 * L) // 3, S // 2] = 1e308
    else:
        raise ValueError(name)
    return tau
