"""Deterministic synthetic transport problems shaped like BASELINE.json's configs.

The reference's atomic data (kurucz_cd23_chianti_H_He) is fetched over the network and is not available
offline, so ``tardis_example.yml`` cannot be run literally.  ``make_problem`` builds opacity states with the
same *layout and statistics* the classic transport mode sees (sorted-descending line list, [L,S] Sobolev
optical depths, macro-atom block tables) on the tardis_example geometry (20 shells, 1.1e9-2.0e9 cm/s,
t_exp = 13 d; docs/tardis_example.yml:6,12-16).

The packet source is a host-side restatement of the reference's ``BlackBodySimpleSource``
(tardis/transport/montecarlo/packet_source/base.py:195-253, black_body.py:122-222): PCG64 stream seeded
with ``base_seed + iteration``; draw order = packet seeds, 5xP uniforms for the Carter-Cashwell Planck
sampler, P uniforms for mu = sqrt(z).
"""
from __future__ import annotations

from dataclasses import dataclass, replace as _dataclass_replace

import numpy as np

from . import state as st

DAY = 86400.0
ANGSTROM = 1e-8
DEFAULT_BASE_SEED = 23111963  # io/configuration/schemas/montecarlo.yml:12-15
MAX_SEED_VAL = 2**32 - 1  # packet_source/base.py:25


@dataclass
class Problem:
    packet_collection: st.PacketCollection
    geometry: st.HomologousRadial1DGeometry
    time_explosion: float
    opacity_state: st.OpacityState
    montecarlo_configuration: st.MonteCarloConfiguration
    spectrum_frequency_grid: np.ndarray
    description: str = ""


def black_body_packets(n_packets: int, radius: float, temperature: float, base_seed: int = DEFAULT_BASE_SEED,
                       seed_offset: int = 0, l_samples: int = 1000, legacy_random_state=None,
                       time_explosion: float | None = None) -> st.PacketCollection:
    """Sample a packet collection at the photosphere (see module docstring for the reference lines).

    ``time_explosion``: None is BlackBodySimpleSource; a number is BlackBodySimpleSourceRelativistic (black_body.py), what the
    reference builds under ``enable_full_relativity``: with beta = radius / time_explosion / c the directions follow
    p(mu) = 2 (mu + beta) / (2 beta + 1), mu = -beta + sqrt(beta^2 + 2 beta z + z), and every energy carries
    (2 beta + 1) / (1 - beta^2) / gamma.  Seeds, radii, nus and stream positions are the simple source's.

    ``legacy_random_state``: the reference's ``legacy_mode_enabled`` source (what its own integration test runs,
    tests/test_montecarlo_main_loop.py:14-60) draws the five Planck uniforms and the direction uniforms from NumPy's GLOBAL
    legacy stream (black_body.py:172,201), seeded once with ``base_seed`` when the source is constructed (base.py:48-59) and
    never re-seeded, so consecutive iterations continue it; only the packet seeds still come from PCG64(base_seed +
    iteration).  Pass one ``np.random.RandomState(base_seed)`` for the whole run to reproduce that."""
    rng = np.random.default_rng(base_seed + seed_offset)
    packet_seeds = rng.choice(MAX_SEED_VAL, n_packets, replace=True)
    radii = np.ones(n_packets) * radius
    # Planck sampler (Carter & Cashwell 1975 via Bjorkman & Wood 2001)
    l_array = np.cumsum(np.arange(1, l_samples, dtype=np.float64) ** -4)
    l_coef = np.pi**4 / 90.0
    draws = legacy_random_state.random_sample if legacy_random_state is not None else rng.random
    xis = draws((5, n_packets))
    l_min = l_array.searchsorted(xis[0] * l_coef) + 1.0
    x = -np.log(np.prod(xis[1:], 0)) / l_min
    nus = x * (st.K_BOLTZMANN * temperature) / st.H_PLANCK
    if time_explosion is None:
        mus = np.sqrt(draws(n_packets))
        energies = np.ones(n_packets) / n_packets
    else:  # squares as products and this parenthesisation: the device source restates it operation for operation
        r, t = float(radius), float(time_explosion)
        if not (np.isfinite(r) and r >= 0.0 and np.isfinite(t) and t > 0.0):
            raise ValueError(f"relativistic source: radius {r!r} must be finite and >= 0, time_explosion {t!r} finite and > 0")
        beta = (r / t) / st.C_SPEED_OF_LIGHT
        if not 0.0 <= beta < 1.0:
            raise ValueError(f"relativistic source: beta = radius / time_explosion / c = {beta!r} is not in [0, 1)")
        gamma = 1.0 / np.sqrt(1.0 - beta * beta)
        z = draws(n_packets)
        mus = (-beta) + np.sqrt(((beta * beta) + ((2.0 * beta) * z)) + z)
        energies = ((np.ones(n_packets) / n_packets) * ((2.0 * beta + 1.0) / (1.0 - beta * beta))) / gamma
    luminosity = 4 * np.pi * st.SIGMA_SB * radius**2 * temperature**4
    return st.PacketCollection(radii, nus, mus, energies, packet_seeds, luminosity)


def make_geometry(n_shells: int = 20, v_inner: float = 1.1e9, v_outer: float = 2.0e9,
                  time_explosion: float = 13 * DAY) -> st.HomologousRadial1DGeometry:
    v = np.linspace(v_inner, v_outer, n_shells + 1)
    r = v * time_explosion
    return st.HomologousRadial1DGeometry(r[:-1], r[1:], v[:-1], v[1:], time_explosion)


def make_opacity_state(seed: int, geometry: st.HomologousRadial1DGeometry, n_lines: int,
                       line_interaction_type: str, log_tau_mean: float = -4.0, log_tau_sigma: float = 2.0,
                       electron_density_0: float = 1e9,
                       shell_independent_probabilities: bool = False,
                       level_sizes: str = "uniform") -> st.OpacityState:
    rng = np.random.default_rng(seed)
    n_shells = len(geometry.r_inner)
    # lines: log-uniform in wavelength on [500 A, 20000 A]; frequency sorted descending
    lam = np.exp(rng.uniform(np.log(500.0), np.log(20000.0), n_lines)) * ANGSTROM
    line_list_nu = np.sort(st.C_SPEED_OF_LIGHT / lam)[::-1].copy()
    rho = (geometry.v_inner / geometry.v_inner[0]) ** -7.0
    tau0 = 10.0 ** rng.normal(log_tau_mean, log_tau_sigma, n_lines)
    tau_sobolev = tau0[:, None] * rho[None, :]
    electron_density = electron_density_0 * rho
    t_electrons = np.full(n_shells, 9000.0)

    if line_interaction_type == "scatter":
        # size-1 dummies, as opacity_state.py:199-209 does for scatter mode
        op = st.OpacityState(electron_density, t_electrons, line_list_nu, tau_sobolev,
                             np.zeros((1, n_shells)), np.zeros(1, np.int64), np.zeros(1, np.int64),
                             np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64))
        op.tau_factors = (tau0, rho)
        return op

    # macro-atom levels: every level owns 4-8 emission lines ("uniform"), lines assigned at random so that a
    # de-excitation can fluoresce to a far-away wavelength
    sizes = []
    left = n_lines
    if level_sizes == "heavy":
        # In the reference a block is ALL transitions out of one source level (macroatom_solver.py:383-428, 624-670):
        # with real Kurucz data most levels own a handful of lines, Fe-group levels hundreds to thousands.  Pareto(1.2)
        # line counts from 4 up (2 % of the levels > 100 lines, 0.1 % > 1000), capped at 6000 lines per level, behind a few
        # planted sizes that pin the edges of the device tables: 11 / 33 lines (33 / 99 rows in macroatom mode, 33 rows
        # in downbranch: just past one 32-entry window, not a multiple of 8), 32 and 64 (whole windows: no padding),
        # 100, 700 and -- on long line lists -- 6000 lines.
        for g in (11, 32, 33, 64, 100, 700, 6000):
            if left >= 2 * g:
                sizes.append(g)
                left -= g
        while left > 0:
            g = int(min(left, 6000, np.floor(4.0 * (1.0 - rng.random()) ** (-1.0 / 1.2))))
            sizes.append(g)
            left -= g
        order = rng.permutation(len(sizes))  # (planted blocks somewhere in the tables, not all at the front)
        sizes = [sizes[i] for i in order]
    elif level_sizes == "uniform":
        while left > 0:
            g = int(min(left, rng.integers(4, 9)))
            sizes.append(g)
            left -= g
    else:
        raise ValueError(level_sizes)
    sizes = np.asarray(sizes)
    n_levels = len(sizes)
    perm = rng.permutation(n_lines)
    level_of_line = np.empty(n_lines, np.int64)
    level_lines = []
    pos = 0
    for lvl, g in enumerate(sizes):
        ids = np.sort(perm[pos:pos + g])
        level_lines.append(ids)
        level_of_line[ids] = lvl
        pos += g

    if line_interaction_type == "downbranch":
        rows_per_line = 1
    elif line_interaction_type == "macroatom":
        rows_per_line = 3
    else:
        raise ValueError(line_interaction_type)
    n_trans = rows_per_line * n_lines
    transition_type = np.empty(n_trans, np.int64)
    destination_level_id = np.empty(n_trans, np.int64)
    transition_line_id = np.empty(n_trans, np.int64)
    block_edge = np.empty(n_levels + 1, np.int64)
    weights = rng.random((n_trans, 1 if shell_independent_probabilities else n_shells)) + 0.05
    if level_sizes == "heavy":
        # transition probabilities of a real block span many decades (A-values x Sobolev escape probabilities): most
        # rows of a long block are below 2**-16 of the block's sum, a few carry it
        weights *= 10.0 ** rng.normal(0.0, 2.0, (n_trans, 1))
    row = 0
    for lvl, ids in enumerate(level_lines):
        block_edge[lvl] = row
        g = len(ids)
        # emission rows (BB_EMISSION = -1; destination unused = -99 as in the reference)
        transition_type[row:row + g] = -1
        destination_level_id[row:row + g] = -99
        transition_line_id[row:row + g] = ids
        row += g
        if rows_per_line == 3:
            # internal down (0) and internal up (1) jumps to random other levels; emission rows keep
            # >= ~1/3 of the block probability so the walk terminates quickly
            for ttype in (0, 1):
                transition_type[row:row + g] = ttype
                destination_level_id[row:row + g] = rng.integers(0, n_levels, g)
                transition_line_id[row:row + g] = ids
                row += g
    block_edge[n_levels] = n_trans  # trailing sentinel (macroatom_solver.py:651-656)
    # normalise per block per shell
    for lvl in range(n_levels):
        a, b = block_edge[lvl], block_edge[lvl + 1]
        weights[a:b] /= weights[a:b].sum(axis=0, keepdims=True)
    if shell_independent_probabilities:
        weights = np.repeat(weights, n_shells, axis=1)
    op = st.OpacityState(electron_density, t_electrons, line_list_nu, tau_sobolev, weights, level_of_line,
                         block_edge, transition_type, destination_level_id, transition_line_id)
    op.tau_factors = (tau0, rho)  # tau_sobolev == tau0[:, None] * rho[None, :] exactly (compact fixtures)
    return op


def make_spectrum_grid(n_bins: int = 10000, lam_start: float = 500.0, lam_stop: float = 20000.0) -> np.ndarray:
    """Uniform-in-frequency ascending edge grid (spectrum/base.py:190-195; solver.py:305-309)."""
    return np.linspace(st.C_SPEED_OF_LIGHT / (lam_stop * ANGSTROM), st.C_SPEED_OF_LIGHT / (lam_start * ANGSTROM),
                       n_bins + 1)


def make_problem(seed: int = 1, n_packets: int = 10_000, n_shells: int = 20, n_lines: int = 30_000,
                 line_interaction_type: str = "downbranch", n_vpackets: int = 0,
                 enable_full_relativity: bool = False, disable_line_scattering: bool = False,
                 n_bins: int = 10_000, iteration: int = 0, temperature_inner: float = 1.0e4,
                 electron_density_0: float = 1e9, log_tau_mean: float = -4.0,
                 vpacket_spawn_range=None, shell_independent_probabilities: bool = False,
                 level_sizes: str = "uniform") -> Problem:
    geometry = make_geometry(n_shells)
    opacity = make_opacity_state(seed, geometry, n_lines, line_interaction_type,
                                 log_tau_mean=log_tau_mean, electron_density_0=electron_density_0,
                                 shell_independent_probabilities=shell_independent_probabilities,
                                 level_sizes=level_sizes)
    packets = black_body_packets(n_packets, geometry.r_inner[0], temperature_inner, seed_offset=iteration)
    cfg = st.MonteCarloConfiguration()
    cfg.LINE_INTERACTION_TYPE = st.LINE_INTERACTION_TYPES[line_interaction_type]
    cfg.NUMBER_OF_VPACKETS = n_vpackets
    cfg.TEMPORARY_V_PACKET_BINS = n_vpackets
    cfg.ENABLE_FULL_RELATIVITY = bool(enable_full_relativity)
    cfg.DISABLE_LINE_SCATTERING = bool(disable_line_scattering)
    cfg.MONTECARLO_SEED = DEFAULT_BASE_SEED
    if vpacket_spawn_range is not None:
        cfg.VPACKET_SPAWN_START_FREQUENCY, cfg.VPACKET_SPAWN_END_FREQUENCY = vpacket_spawn_range
    grid = make_spectrum_grid(n_bins)
    desc = (f"synthetic P={n_packets} S={n_shells} L={n_lines} {line_interaction_type} n_v={n_vpackets} "
            f"full_rel={int(enable_full_relativity)} seed={seed}" + (" heavy-tailed levels" if level_sizes == "heavy" else ""))
    return Problem(packets, geometry, geometry.time_explosion, opacity, cfg, grid, desc)


# BASELINE.json configs -> generator arguments
BASELINE_CONFIGS = {
    1: dict(n_packets=10_000, n_shells=20, n_lines=30_000, line_interaction_type="downbranch", n_vpackets=0),
    2: dict(n_packets=10_000_000, n_shells=20, n_lines=30_000, line_interaction_type="downbranch", n_vpackets=0),
    3: dict(n_packets=100_000_000, n_shells=20, n_lines=500_000, line_interaction_type="macroatom", n_vpackets=0),
    4: dict(n_packets=100_000_000, n_shells=20, n_lines=500_000, line_interaction_type="macroatom", n_vpackets=0),
    5: dict(n_packets=500_000_000, n_shells=100, n_lines=500_000, line_interaction_type="macroatom",
            n_vpackets=10),
}


# pi e^2 / (m_e c) [cm^2 / s], CODATA 2010 cgs: the plasma's TauSobolev.sobolev_coefficient
SOBOLEV_COEFFICIENT = np.pi * 4.80320450e-10**2 / (9.10938291e-28 * st.C_SPEED_OF_LIGHT)


@dataclass
class LineData:
    """Static line data of Engine.set_line_data plus one plasma state to feed Engine.update_opacity with."""
    f_lu: np.ndarray
    wavelength_cm: np.ndarray
    g_lower: np.ndarray
    g_upper: np.ndarray
    level_lower: np.ndarray
    level_upper: np.ndarray
    n_levels: int
    transition_probability_coef: np.ndarray | None
    sobolev_coefficient: float
    level_number_density: np.ndarray  # [n_levels, n_shells]
    electron_density: np.ndarray      # [n_shells]
    t_radiative: np.ndarray           # [n_shells]
    dilution_factor: np.ndarray       # [n_shells]


def make_line_data(seed: int, opacity_state: st.OpacityState, n_levels: int | None = None, level_sizes: str = "uniform",
                   time_explosion: float = 13 * DAY) -> LineData:
    """Atomic data and level populations for the device opacity update, on the topology of ``opacity_state`` (make_opacity_state):
    oscillator strengths log-uniform over three decades, wavelengths c / nu, statistical weights 2J + 1, every line between two of
    ``n_levels`` atomic levels (lower index < upper index), macro-atom coefficients per transition row (spread over many decades for
    ``level_sizes="heavy"``, as the probabilities of make_opacity_state are; internal-up rows carry 1e4, the inverse of a typical
    mean intensity) and populations that fall with the level index and the shell's density, with 1.5 dex of scatter -- enough for
    inverted pairs -- and a few levels empty in some shells.  The populations are scaled so that the median Sobolev optical depth at
    ``time_explosion`` is 1e-2: with their spread tau reaches both beyond 1e3 and below 1e-4, all three branches of beta."""
    rng = np.random.default_rng(seed + 7919)
    L = len(opacity_state.line_list_nu)
    S = len(opacity_state.electron_density)
    K = int(n_levels) if n_levels is not None else max(8, L // 10)
    if K < 2:
        raise ValueError("n_levels must be at least 2")
    f_lu = 10.0 ** rng.uniform(-3.0, 0.0, L)
    wavelength_cm = st.C_SPEED_OF_LIGHT / np.asarray(opacity_state.line_list_nu, dtype=np.float64)
    a, b = rng.integers(0, K, L), rng.integers(0, K - 1, L)
    b = np.where(b >= a, b + 1, b)  # (two different levels)
    level_lower, level_upper = np.minimum(a, b).astype(np.int64), np.maximum(a, b).astype(np.int64)
    g_level = 2.0 * rng.integers(0, 6, K) + 1.0
    g_lower, g_upper = g_level[level_lower], g_level[level_upper]
    rho = np.asarray(opacity_state.electron_density, dtype=np.float64) / float(opacity_state.electron_density[0])
    log_n = 4.0 - 8.0 * np.arange(K) / K + rng.normal(0.0, 1.5, K)
    n = 10.0 ** log_n[:, None] * rho[None, :] * 10.0 ** rng.normal(0.0, 0.2, (K, S))
    raw = SOBOLEV_COEFFICIENT * f_lu[:, None] * wavelength_cm[:, None] * time_explosion * n[level_lower]
    n *= 1e-2 / np.median(raw)
    empty = rng.choice(K, max(2, K // 50), replace=False)
    n[empty[0], :] = 0.0                 # a level empty everywhere
    n[empty[1:], rng.integers(0, S, len(empty) - 1)] = 0.0  # ... and some empty in one shell
    coef = None
    ttype = np.asarray(opacity_state.transition_type)
    if len(ttype) > 1:
        T = len(ttype)
        coef = rng.random(T) + 0.05
        if level_sizes == "heavy":
            coef *= 10.0 ** rng.normal(0.0, 2.0, T)
        coef[ttype == 1] *= 1e4
    S_idx = np.arange(S)
    t_rad = 10000.0 - 150.0 * S_idx
    w = 0.4 / (1.0 + 0.2 * S_idx)
    return LineData(f_lu, wavelength_cm, g_lower, g_upper, level_lower, level_upper, K, coef, float(SOBOLEV_COEFFICIENT), n,
                    np.asarray(opacity_state.electron_density, dtype=np.float64).copy(), t_rad, w)


EV = 1.602176565e-12  # erg (CODATA 2010)
# first ionization energies [eV] of the elements make_plasma_data draws from: (atomic number, I -> II, II -> III, ...), NIST ASD
_IONIZATION_EV = (
    (6, 11.260, 24.383, 47.888, 64.494, 392.09),
    (8, 13.618, 35.121, 54.936, 77.414, 113.90),
    (12, 7.646, 15.035, 80.144, 109.27, 141.33),
    (14, 8.152, 16.346, 33.493, 45.142, 166.77),
    (16, 10.360, 23.338, 34.86, 47.222, 72.59),
    (20, 6.113, 11.872, 50.913, 67.27, 84.34),
    (26, 7.902, 16.199, 30.651, 54.91, 75.0),
    (28, 7.640, 18.169, 35.19, 54.9, 76.06),
)
CHI_0_CA_II = 11.872 * EV  # the reference's chi_0: the ionization energy of Ca II


@dataclass
class PlasmaData:
    """Static plasma data of Engine.set_plasma_data plus one radiation field to feed Engine.update_plasma with."""
    level_energy: np.ndarray        # [K] erg
    level_g: np.ndarray             # [K]
    level_metastable: np.ndarray    # [K] 0 / 1
    ion_level_edge: np.ndarray      # [I+1]
    element_ion_edge: np.ndarray    # [E+1]
    ion_charge: np.ndarray          # [I]
    ionization_energy: np.ndarray   # [I] erg
    zeta_temperatures: np.ndarray   # [NT]
    zeta: np.ndarray                # [I, NT]
    number_density: np.ndarray      # [E, S]
    chi_0: float
    link_t_rad_t_electron: float
    atomic_number: np.ndarray       # [E]
    t_radiative: np.ndarray         # [S]
    dilution_factor: np.ndarray     # [S]


def make_plasma_data(seed: int, line_data: LineData, n_shells: int, n_elements: int = 6, ions_per_element: int = 5,
                     largest_ion: int | None = None, density_inner: float = 1e9) -> PlasmaData:
    """Atomic data and abundances for the device plasma update on the ``line_data.n_levels`` levels of make_line_data:
    ``n_elements`` elements of ``ions_per_element`` ions each (neutral upward) with their NIST ionization energies; the levels dealt
    to the ions with heavy-tailed counts -- an element's highest ion keeps a single level, like a closed shell or a bare nucleus,
    singly ionized iron-group ions take hundreds; ``largest_ion`` plants an ion of exactly that many levels --, level energies rising
    from 0 to below the ionization energy, weights 2J + 1, the ground and some low levels metastable, a smooth zeta table on
    2000 K .. 40000 K with rows of 1.0 for the ions the reference has no data for, and number densities that fall outward as
    (1 + 0.15 s)^-7."""
    rng = np.random.default_rng(seed + 104729)
    K, S, E = int(line_data.n_levels), int(n_shells), int(n_elements)
    per = int(ions_per_element)
    if not 2 <= per <= 6 or E < 1:
        raise ValueError("ions_per_element must be 2 .. 6, n_elements positive")
    I = E * per
    if K < I:
        raise ValueError("fewer levels than ions")
    rows = [_IONIZATION_EV[e % len(_IONIZATION_EV)] for e in range(E)]
    atomic_number = np.array([r[0] for r in rows], dtype=np.int64)
    ion_charge = np.tile(np.arange(per, dtype=np.float64), E)
    chi = np.array([[r[1 + j] if j < per - 1 else 0.0 for j in range(per)] for r in rows]).ravel() * EV
    # level counts: one per ion, the rest dealt by log-normal weights; the last ion of an element keeps its single level
    weight = 10.0 ** rng.normal(0.0, 0.8, I)
    weight[per - 1::per] = 0.0
    weight[1::per] *= 4.0  # (singly ionized species dominate a supernova's line list)
    extra = np.floor(weight / weight.sum() * (K - I)).astype(np.int64)
    big = int(np.argmax(weight))
    if largest_ion is not None:
        if not 1 <= largest_ion <= K - I + 1:
            raise ValueError("largest_ion does not fit")
        others = np.delete(np.arange(I), big)
        left = K - I - (largest_ion - 1)
        w = weight[others]
        extra[others] = np.floor(w / w.sum() * left).astype(np.int64) if w.sum() > 0 else 0
        extra[big] = largest_ion - 1
    rest = K - I - int(extra.sum())
    if largest_ion is None:
        extra[big] += rest
    else:
        second = int(np.argmax(np.where(np.arange(I) == big, -1.0, weight)))
        extra[second] += rest
    counts = 1 + extra
    ion_level_edge = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    element_ion_edge = (per * np.arange(E + 1)).astype(np.int64)
    level_energy, level_meta = np.zeros(K), np.zeros(K, dtype=np.int32)
    for i in range(I):
        a, b = ion_level_edge[i], ion_level_edge[i + 1]
        top = chi[i] if chi[i] > 0 else 50.0 * EV
        level_energy[a + 1:b] = np.sort(0.05 * top + 0.9 * top * rng.random(b - a - 1) ** 0.7)
        level_meta[a] = 1
        low = a + 1 + np.flatnonzero(rng.random(b - a - 1) < 3.0 / max(3, b - a))
        level_meta[low] = 1
    level_g = 2.0 * rng.integers(0, 6, K) + 1.0
    zeta_t = np.arange(2000.0, 40001.0, 2000.0)
    centre, width = rng.uniform(5000.0, 30000.0, I), rng.uniform(4000.0, 15000.0, I)
    zeta = 0.05 + 0.9 / (1.0 + np.exp((zeta_t[None, :] - centre[:, None]) / width[:, None]))
    zeta[rng.random(I) < 0.2] = 1.0
    abundance = rng.dirichlet(np.full(E, 2.0))
    total = density_inner * (1.0 + 0.15 * np.arange(S)) ** -7.0
    number_density = abundance[:, None] * total[None, :]
    t_rad = np.asarray(line_data.t_radiative, dtype=np.float64)
    w = np.asarray(line_data.dilution_factor, dtype=np.float64)
    if t_rad.shape != (S,):
        t_rad, w = 10000.0 - 150.0 * np.arange(S), 0.4 / (1.0 + 0.2 * np.arange(S))
    return PlasmaData(level_energy, level_g, level_meta, ion_level_edge, element_ion_edge, ion_charge, chi, zeta_t, zeta, number_density,
                      float(CHI_0_CA_II), 0.9, atomic_number, t_rad.copy(), w.copy())


HELIUM_IONIZATION_EV = (24.587387, 54.417763)  # He I -> He II, He II -> He III, NIST ASD


def make_helium_plasma_data(seed: int, line_data: LineData, n_shells: int, helium_levels=(19, 10), helium_abundance: float = 0.3,
                            **kwargs) -> PlasmaData:
    """make_plasma_data with helium in front: element 0 has atomic_number 2 and the three ions He I, He II, He III of
    ``helium_levels[0]``, ``helium_levels[1]`` and one level on the first levels of ``line_data``; the remaining levels are dealt to
    the other elements exactly as make_plasma_data(seed, ..., **kwargs) deals them.  He I has its ground level and two low metastable
    levels (the 2s states, at 0.806 and 0.839 of the ionisation energy); every other excited level of He I and He II lies between 0.78
    and 0.98 of its ion's ionisation energy, as helium's do.  Helium takes ``helium_abundance`` of every shell's number density, the
    other elements share the rest in make_plasma_data's proportions.  What Engine.set_ionization_options("recomb-nlte") needs."""
    n1, n2 = (int(n) for n in helium_levels)
    if n1 < 3 or n2 < 1:
        raise ValueError("He I needs at least three levels, He II one")
    KH = n1 + n2 + 1
    rest = make_plasma_data(seed, _dataclass_replace(line_data, n_levels=int(line_data.n_levels) - KH), n_shells, **kwargs)
    rng = np.random.default_rng(seed + 611953)
    chi = np.array(HELIUM_IONIZATION_EV + (0.0,)) * EV
    counts = np.array([n1, n2, 1])
    edge = np.concatenate(([0], np.cumsum(counts)))
    energy, meta = np.zeros(KH), np.zeros(KH, dtype=np.int32)
    for i in range(2):
        a, b = edge[i], edge[i + 1]
        energy[a + 1:b] = np.sort(0.78 * chi[i] + 0.2 * chi[i] * rng.random(b - a - 1))
        meta[a] = 1
    energy[1:3] = np.array([0.806, 0.839]) * chi[0]
    energy[1:n1] = np.sort(energy[1:n1])
    meta[1:3] = 1
    meta[edge[2]] = 1
    g = 2.0 * rng.integers(0, 6, KH) + 1.0
    I_rest, NT = len(rest.ion_charge), len(rest.zeta_temperatures)
    centre, width = rng.uniform(5000.0, 30000.0, 3), rng.uniform(4000.0, 15000.0, 3)
    zeta = 0.05 + 0.9 / (1.0 + np.exp((rest.zeta_temperatures[None, :] - centre[:, None]) / width[:, None]))
    total = rest.number_density.sum(axis=0)
    number_density = np.concatenate(((helium_abundance * total)[None, :], (1.0 - helium_abundance) * rest.number_density))
    assert zeta.shape == (3, NT) and I_rest == len(rest.ion_level_edge) - 1
    return PlasmaData(np.concatenate((energy, rest.level_energy)), np.concatenate((g, rest.level_g)), np.concatenate((meta, rest.level_metastable)),
                      np.concatenate((edge[:-1], rest.ion_level_edge + KH)).astype(np.int64),
                      np.concatenate(([0], rest.element_ion_edge + 3)).astype(np.int64), np.concatenate(([0.0, 1.0, 2.0], rest.ion_charge)),
                      np.concatenate((chi, rest.ionization_energy)), rest.zeta_temperatures, np.concatenate((zeta, rest.zeta)), number_density,
                      rest.chi_0, rest.link_t_rad_t_electron, np.concatenate(([2], rest.atomic_number)).astype(np.int64),
                      rest.t_radiative, rest.dilution_factor)


# 4 pi^2 e^2 / (h m_e c), CODATA 2010 cgs: B_lu = EINSTEIN_COEFFICIENT f_lu / nu (the atomic data's lines preparation)
EINSTEIN_COEFFICIENT = 4.0 * np.pi**2 * 4.80320450e-10**2 / (6.62606957e-27 * 9.10938291e-28 * st.C_SPEED_OF_LIGHT)


def lines_within_ions(seed: int, line_data: LineData, plasma_data: PlasmaData) -> LineData:
    """``line_data`` with every line moved between two levels of ONE ion of ``plasma_data``, as the lines of real atomic data are
    (make_line_data deals its lines over all levels, which is all the opacity update needs): per ion of n >= 2 levels first the n - 1
    lines of a ladder (k, k + 1), so that every level of an ion is reached, then the remaining lines dealt to the ions in proportion to
    their number of level pairs, each between two different levels drawn uniformly (lower index < upper index).  The statistical
    weights follow the plasma data's level_g; everything else is kept."""
    from dataclasses import replace
    rng = np.random.default_rng(seed + 15485863)
    edge = np.asarray(plasma_data.ion_level_edge, dtype=np.int64)
    n = np.diff(edge)
    L = len(line_data.f_lu)
    if L < int((n - 1).sum()):
        raise ValueError("fewer lines than the ladders of the ions need")
    lower = np.concatenate([np.arange(a, b - 1) for a, b in zip(edge[:-1], edge[1:])]).astype(np.int64)
    upper = lower + 1
    rest = L - len(lower)
    pairs = (n * (n - 1)).astype(np.float64)
    ion = rng.choice(len(n), rest, p=pairs / pairs.sum())
    a = rng.integers(0, n[ion])
    b = rng.integers(0, n[ion] - 1)
    b = np.where(b >= a, b + 1, b)
    lower = np.concatenate((lower, edge[ion] + np.minimum(a, b)))
    upper = np.concatenate((upper, edge[ion] + np.maximum(a, b)))
    order = rng.permutation(L)
    lower, upper = lower[order], upper[order]
    g = np.asarray(plasma_data.level_g, dtype=np.float64)
    return replace(line_data, level_lower=lower, level_upper=upper, g_lower=g[lower], g_upper=g[upper])


@dataclass
class NlteData:
    """The NLTE species of Engine.set_nlte_data: their ions, their lines in the line list and the lines' Einstein coefficients."""
    species_ion: np.ndarray         # [NS] indices into the plasma data's ions
    species_line_edge: np.ndarray   # [NS+1]
    line_id: np.ndarray             # [NL] indices into the line list
    A_ul: np.ndarray                # [NL]
    B_ul: np.ndarray                # [NL]
    B_lu: np.ndarray                # [NL]
    coronal_approximation: bool = False
    classical_nebular: bool = False


def make_nlte_data(seed: int, line_data: LineData, plasma_data: PlasmaData, species=None, coronal_approximation: bool = False,
                   classical_nebular: bool = False, untouched_level=None) -> NlteData:
    """The NLTE data of the ions ``species`` (indices into ``plasma_data``'s ions; None: the ion with the most levels): a species'
    lines are those of ``line_data`` whose two levels both lie in its ion (lines_within_ions makes every line such a line), in a
    seeded order, the first of several lines between the same two levels kept -- every pair is unique.  B_lu = C f_lu / nu with
    C = 4 pi^2 e^2 / (h m_e c), B_ul = B_lu g_lower / g_upper, A_ul = (2 h nu^3 / c^2) B_ul: with f_lu over three decades and nu
    over the line list the rates span the many orders of magnitude real ones do.  ``untouched_level`` = (position in species, local
    level) drops every line of that level, which makes the species' rate matrix exactly singular."""
    rng = np.random.default_rng(seed + 32452843)
    edge = np.asarray(plasma_data.ion_level_edge, dtype=np.int64)
    if species is None:
        species = [int(np.argmax(np.diff(edge)))]
    species = np.asarray(species, dtype=np.int64)
    lower, upper = np.asarray(line_data.level_lower, dtype=np.int64), np.asarray(line_data.level_upper, dtype=np.int64)
    ids, line_edge = [], [0]
    for pos, i in enumerate(species):
        k0, k1 = edge[i], edge[i + 1]
        own = np.flatnonzero((lower >= k0) & (lower < k1) & (upper >= k0) & (upper < k1) & (lower != upper))
        own = own[rng.permutation(len(own))]
        lo, hi = np.minimum(lower[own], upper[own]), np.maximum(lower[own], upper[own])
        _, first = np.unique(lo * (k1 - k0 + 1) * 2 + hi, return_index=True)
        own = own[np.sort(first)]
        if untouched_level is not None and untouched_level[0] == pos:
            k = k0 + int(untouched_level[1])
            own = own[(lower[own] != k) & (upper[own] != k)]
        ids.append(own)
        line_edge.append(line_edge[-1] + len(own))
    line_id = np.concatenate(ids).astype(np.int64) if ids else np.zeros(0, dtype=np.int64)
    nu = st.C_SPEED_OF_LIGHT / np.asarray(line_data.wavelength_cm, dtype=np.float64)[line_id]
    b_lu = EINSTEIN_COEFFICIENT * np.asarray(line_data.f_lu, dtype=np.float64)[line_id] / nu
    b_ul = b_lu * np.asarray(line_data.g_lower, dtype=np.float64)[line_id] / np.asarray(line_data.g_upper, dtype=np.float64)[line_id]
    a_ul = (2.0 * 6.62606957e-27 * nu**3 / st.C_SPEED_OF_LIGHT**2) * b_ul
    return NlteData(species, np.asarray(line_edge, dtype=np.int64), line_id, a_ul, b_ul, b_lu, bool(coronal_approximation), bool(classical_nebular))


K_BOLTZMANN = 1.3806488e-16  # erg / K, tardis/constants.py (CODATA 2010, cgs)


@dataclass
class NlteCollisionData:
    """The collision strengths of Engine.set_nlte_collision_data: per NLTE species, pairs of local levels with C_ul over a
    temperature grid (what ``collision_data`` is to the atomic data)."""
    collision_temperatures: np.ndarray  # [NT] kelvin, ascending
    species_pair_edge: np.ndarray       # [NS+1]; an empty range: the species has no collision data
    level_lower: np.ndarray             # [NP] local to the species' ion
    level_upper: np.ndarray             # [NP]
    delta_e: np.ndarray                 # [NP] kelvin
    g_ratio: np.ndarray                 # [NP] g_lower / g_upper
    C_ul: np.ndarray                    # [NP, NT]; NaN where the source has no value


def make_nlte_collision_data(seed: int, plasma_data: PlasmaData, nlte_data: NlteData, pair_fraction=1.0, n_temperatures: int = 12,
                             nan_fraction: float = 0.1, magnitude: float = 1e-8, reach_levels=(), t_min: float = 2000.0,
                             t_max: float = 40000.0) -> NlteCollisionData:
    """Collision data for the species of ``nlte_data``: of a species' n (n - 1) / 2 level pairs the share ``pair_fraction`` (a number
    for all species, or one per species; 1.0: dense, 0.0: an empty range, the species has no data), drawn with the seed and sorted
    by (lower, upper).  ``reach_levels`` = [(position in species, local level), ...] adds the pairs of that level with every other
    level of its ion, whatever the fraction -- the way to give rates to a level no line reaches.  delta_e = (E_upper - E_lower) /
    k_B and g_ratio = g_lower / g_upper from the plasma data.  C_ul = ``magnitude`` times a log-normal factor of one decade per
    pair, times (t / 1e4 K)^p with p in [-0.7, 0.3] per pair, on ``n_temperatures`` knots spaced geometrically from ``t_min`` to
    ``t_max``; a share ``nan_fraction`` of the pairs has NaN at its first one to three knots (the cool end, where Chianti's fits
    have none)."""
    rng = np.random.default_rng(seed + 49979687)
    edge = np.asarray(plasma_data.ion_level_edge, dtype=np.int64)
    species = np.asarray(nlte_data.species_ion, dtype=np.int64)
    NT = int(n_temperatures)
    if NT < 2:
        raise ValueError("n_temperatures must be at least 2")
    fraction = np.broadcast_to(np.asarray(pair_fraction, dtype=np.float64), species.shape)
    if np.any(fraction < 0) or np.any(fraction > 1):
        raise ValueError("pair_fraction lies in [0, 1]")
    temps = np.geomspace(float(t_min), float(t_max), NT)
    energy, g = np.asarray(plasma_data.level_energy, dtype=np.float64), np.asarray(plasma_data.level_g, dtype=np.float64)
    lower, upper, pair_edge = [], [], [0]
    for pos, i in enumerate(species):
        k0, n = int(edge[i]), int(edge[i + 1] - edge[i])
        lo, up = np.triu_indices(n, 1)
        keep = rng.random(len(lo)) < fraction[pos] if fraction[pos] < 1.0 else np.ones(len(lo), dtype=bool)
        for where, level in reach_levels:
            if where == pos:
                keep |= (lo == level) | (up == level)
        lower.append(lo[keep])  # (triu_indices is sorted by (lower, upper))
        upper.append(up[keep])
        pair_edge.append(pair_edge[-1] + int(keep.sum()))
    first = np.repeat(edge[species], np.diff(pair_edge))
    lower, upper = np.concatenate(lower).astype(np.int64), np.concatenate(upper).astype(np.int64)
    NP = len(lower)
    delta_e = (energy[first + upper] - energy[first + lower]) / K_BOLTZMANN
    g_ratio = g[first + lower] / g[first + upper]
    c_ul = magnitude * 10.0 ** rng.normal(0.0, 0.5, NP)[:, None] * (temps[None, :] / 1e4) ** rng.uniform(-0.7, 0.3, NP)[:, None]
    holes = np.flatnonzero(rng.random(NP) < nan_fraction)
    for q, m in zip(holes, rng.integers(1, min(3, NT - 1) + 1, len(holes))):
        c_ul[q, :m] = np.nan
    return NlteCollisionData(temps, np.asarray(pair_edge, dtype=np.int64), lower, upper, delta_e, g_ratio, c_ul)


H_PLANCK = 6.62606957e-27  # erg s, tardis/constants.py (CODATA 2010, cgs)


@dataclass
class ContinuumData:
    """The photo-ionisation cross-sections of Engine.set_continuum_data: per level that has a table, a block of (nu, x_sect)
    points (what ``photoionization_data`` is to the atomic data, with ``photo_ion_block_references`` as block_edge)."""
    level: np.ndarray        # [NC] indices into the plasma data's levels, strictly ascending
    block_edge: np.ndarray   # [NC+1]
    nu: np.ndarray           # [NP] Hz, ascending inside a block; a block's first nu is the threshold
    x_sect: np.ndarray       # [NP] cm^2


def make_continuum_data(seed: int, plasma_data: PlasmaData, n_continua: int, points=(2, 40), levels=None, lengths=None,
                        x_threshold: float = 6.3e-18, span=(1.5, 6.0)) -> ContinuumData:
    """Hydrogenic photo-ionisation blocks for ``n_continua`` levels of ``plasma_data``: a level's threshold is its distance to its
    ion's ionisation energy, nu_i = (chi_i - E_k) / h, and above it x_sect = x0 (nu_i / nu)^3 with x0 = ``x_threshold`` times a
    log-normal factor, on a geometric grid from nu_i to nu_i times a factor drawn from ``span``.  The levels are drawn (without
    repetition, then sorted) from those whose ion has an upper ion and that lie below the ionisation energy -- the ground levels of
    such ions first, so that every charge takes part --, or given as ``levels``; the block lengths are drawn uniformly from
    ``points`` = (shortest, longest), or given as ``lengths`` (one per continuum, in level order)."""
    rng = np.random.default_rng(seed + 86028121)
    edge = np.asarray(plasma_data.ion_level_edge, dtype=np.int64)
    elem = np.asarray(plasma_data.element_ion_edge, dtype=np.int64)
    chi = np.asarray(plasma_data.ionization_energy, dtype=np.float64)
    energy = np.asarray(plasma_data.level_energy, dtype=np.float64)
    ion = np.repeat(np.arange(len(edge) - 1), np.diff(edge))
    NC = int(n_continua)
    if levels is None:
        last = np.zeros(len(edge) - 1, dtype=bool)
        last[elem[1:] - 1] = True
        ok = ~last[ion] & (energy < 0.999 * chi[ion])
        ground = edge[:-1][~last]
        ground = ground[ok[ground]]
        rest = np.setdiff1d(np.flatnonzero(ok), ground)
        if NC < 1 or NC > len(ground) + len(rest):
            raise ValueError("n_continua does not fit the levels that can ionise")
        take = ground[:NC] if NC <= len(ground) else np.concatenate((ground, rng.choice(rest, NC - len(ground), replace=False)))
        levels = np.sort(take)
    levels = np.asarray(levels, dtype=np.int64)
    if len(levels) != NC:
        raise ValueError("levels must have n_continua entries")
    if lengths is None:
        lengths = rng.integers(int(points[0]), int(points[1]) + 1, NC)
    lengths = np.asarray(lengths, dtype=np.int64)
    if len(lengths) != NC or np.any(lengths < 2):
        raise ValueError("lengths must have n_continua entries of at least 2")
    nu, x = [], []
    for k, n in zip(levels, lengths):
        nu_i = (chi[ion[k]] - energy[k]) / H_PLANCK
        grid = nu_i * np.geomspace(1.0, rng.uniform(*span), int(n))
        grid[0] = nu_i
        x0 = x_threshold * 10.0 ** rng.normal(0.0, 0.3)
        nu.append(grid)
        x.append(x0 * (nu_i / grid) ** 3)
    return ContinuumData(levels, np.concatenate(([0], np.cumsum(lengths))).astype(np.int64), np.concatenate(nu), np.concatenate(x))


def comoving_frequency_range(problem: Problem) -> tuple[float, float]:
    """An interval that holds every comoving frequency a packet of ``problem`` can have on a move: a packet's frequency is its
    initial one or, after an interaction, a Doppler shift of a line's or of its own comoving one, and every Doppler factor lies
    within 1 -+ beta of the outer edge -- widened by three such factors on either side."""
    beta = float(problem.geometry.v_outer[-1]) / st.C_SPEED_OF_LIGHT
    nus = np.concatenate((np.asarray(problem.packet_collection.initial_nus, dtype=np.float64),
                          np.asarray(problem.opacity_state.line_list_nu, dtype=np.float64)))
    return float(nus.min() * (1.0 - beta) ** 3), float(nus.max() * (1.0 + beta) ** 3)


def make_covering_continuum_data(plasma_data: PlasmaData, blocks) -> ContinuumData:
    """Continuum blocks laid where the caller wants them -- e.g. over comoving_frequency_range(), so that some continua are current
    for a run's packets (the hydrogenic thresholds of make_continuum_data lie far above a 1e4-K photosphere's frequencies).
    ``blocks``: a sequence of (nu, x_sect) array pairs, nu ascending strictly; block c goes to the c-th level of ``plasma_data``,
    in level order, whose ion has an upper ion -- the frequencies then have nothing to do with the levels' energies: for the
    estimators of the transport, not for physics."""
    edge = np.asarray(plasma_data.ion_level_edge, dtype=np.int64)
    elem = np.asarray(plasma_data.element_ion_edge, dtype=np.int64)
    ion = np.repeat(np.arange(len(edge) - 1), np.diff(edge))
    last = np.zeros(len(edge) - 1, dtype=bool)
    last[elem[1:] - 1] = True
    levels = np.flatnonzero(~last[ion])[:len(blocks)]
    if len(levels) != len(blocks):
        raise ValueError("more blocks than levels that can ionise")
    nu = [np.asarray(b[0], dtype=np.float64) for b in blocks]
    x = [np.asarray(b[1], dtype=np.float64) for b in blocks]
    if any(a.ndim != 1 or len(a) < 2 or a.shape != b.shape or np.any(np.diff(a) <= 0) for a, b in zip(nu, x)):
        raise ValueError("a block is (nu, x_sect): two vectors of one length >= 2, nu ascending strictly")
    lengths = [len(a) for a in nu]
    return ContinuumData(levels.astype(np.int64), np.concatenate(([0], np.cumsum(lengths))).astype(np.int64), np.concatenate(nu), np.concatenate(x))
