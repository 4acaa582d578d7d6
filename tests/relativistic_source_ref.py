"""Plain-NumPy restatement of the reference's BlackBodySimpleSourceRelativistic (packet_source/black_body.py), the packet source
of a full-relativity run.  Independent of tardis_amd.synthetic: the constants are written out, the draws come straight from
np.random.default_rng(base_seed + seed_offset) in the reference's order (choice, random((5, n)), random(n)), and the squares
are products, so that libm's pow never enters.

    beta   = (radius / time_explosion) / c
    gamma  = 1 / sqrt(1 - beta*beta)
    energy = ((1 / n) * (2 beta + 1) / (1 - beta*beta)) / gamma
    mu     = -beta + sqrt(beta*beta + 2 beta z + z),   z = rng.random(n)
"""
from types import SimpleNamespace

import numpy as np

C_SPEED_OF_LIGHT = 2.99792458e10  # tardis/constants.py (CODATA 2010, cgs)
K_BOLTZMANN = 1.3806488e-16
H_PLANCK = 6.62606957e-27
BASE_SEED = 23111963              # io/configuration/schemas/montecarlo.yml
MAX_SEED_VAL = 2**32 - 1          # packet_source/base.py
DAY = 86400.0


def factors(radius, time_explosion, n):
    """(beta, energy) of an n-packet draw, in the reference's operation order."""
    beta = (radius / time_explosion) / C_SPEED_OF_LIGHT
    gamma = 1.0 / np.sqrt(1.0 - beta * beta)
    factor = (2.0 * beta + 1.0) / (1.0 - beta * beta)
    energy = ((1.0 / n) * factor) / gamma
    return float(beta), float(energy)


def mus_from_z(z, beta):
    return (-beta) + np.sqrt(((beta * beta) + ((2.0 * beta) * z)) + z)


def mu_mean_and_sigma(beta):
    """Mean and standard deviation of p(mu) = 2 (mu + beta) / (2 beta + 1) on [0, 1]."""
    mean = (2.0 / 3.0 + beta) / (2.0 * beta + 1.0)
    var = (0.5 + 2.0 * beta / 3.0) / (2.0 * beta + 1.0) - mean * mean
    return mean, np.sqrt(var)


def packets(n, radius, temperature, time_explosion, base_seed=BASE_SEED, seed_offset=0, max_seed_val=MAX_SEED_VAL, l_samples=1000):
    """The packets of BlackBodySimpleSourceRelativistic(radius, temperature, base_seed).create_packets(n, seed_offset);
    time_explosion=None gives BlackBodySimpleSource's.  `z` (the direction uniforms) is returned beside the packet arrays."""
    rng = np.random.default_rng(base_seed + seed_offset)
    seeds = rng.choice(max_seed_val, n, replace=True)
    xis = rng.random((5, n))
    z = rng.random(n)
    l_array = np.cumsum(np.arange(1, l_samples, dtype=np.float64) ** -4)
    l_min = l_array.searchsorted(xis[0] * (np.pi**4 / 90.0)) + 1.0
    x = -np.log(np.prod(xis[1:], 0)) / l_min
    nus = x * (K_BOLTZMANN * temperature) / H_PLANCK
    if time_explosion is None:
        beta, mus, energies = 0.0, np.sqrt(z), np.ones(n) / n
    else:
        beta = (radius / time_explosion) / C_SPEED_OF_LIGHT
        gamma = 1.0 / np.sqrt(1.0 - beta * beta)
        factor = (2.0 * beta + 1.0) / (1.0 - beta * beta)
        mus = mus_from_z(z, beta)
        energies = np.ones(n) / n * factor / gamma
    return SimpleNamespace(packet_seeds=seeds, initial_radii=np.ones(n) * radius, initial_nus=nus, initial_mus=mus,
                           initial_energies=energies, z=z, beta=beta)
