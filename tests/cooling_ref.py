"""The yardstick of the cooling sub-stage behind the continuum stage of tardis_mc_update_plasma and of tardis_mc_kpacket_sample: a
NumPy restatement of SpontRecombCoolingRateCoeff, FreeBoundEmissionCDF, FreeBoundCoolingRate, CollIonCooling, FreeFreeCoolingRate,
AdiabaticCoolingRate, the k-packet table and the three samplers in the operation order include/tardis_mc.h spells out, every product,
quotient, sum and difference a rounding of its own.  It runs on the output of continuum_ref.stage() and the solved plasma.  exp and log
are the transport's own (oracle.exp_array(x, 1), oracle.log_array(x, 1)); every sum is a serial sum from 0.0, added in Python order;
the samplers are scalar Python arithmetic.

One decision of the project that differs from the reference, as the header states it: where the last value E[b-1] of a block's
running trapezoid is not positive and finite, the block's CDF is 0.0 at every point but the last and 1.0 at the last, and the case is
counted; the reference produces NaN there.  Collisional-excitation cooling is not in the k-packet table."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import continuum_ref as cref  # noqa: E402
import plasma_update_ref as ref  # noqa: E402
from oracle import oracle  # noqa: E402

K_BOLTZMANN, H_PLANCK = ref.K_BOLTZMANN, ref.H_PLANCK
C0_FF = 1.426e-27
RATES = ("c_fb_sp", "cool_rate_fb", "cool_rate_coll_ion")
SHELL = ("cool_rate_ff", "cool_rate_adiabatic", "cool_rate_total")
TABLES = ("fb_emission_cdf", "k_cdf")
KIND_FF, KIND_ADIABATIC, KIND_FB, KIND_COLL_ION = 0, 1, 2, 3


def log(x):
    return float(oracle.log_array(np.array([x], dtype=np.float64), 1)[0])


def stage(pd, cd, sol, out, time_explosion):
    """The sub-stage on the solved plasma ``sol`` and ``out`` = continuum_ref.stage(...) of it: c_fb_sp, cool_rate_fb,
    cool_rate_coll_ion [NC, S]; cool_rate_ff, cool_rate_adiabatic, cool_rate_total [S]; fb_emission_cdf [NP, S]; k_cdf [2 + 2 NC, S];
    n_degenerate_fb_cdf; also "degenerate" [NC, S], "e_last" [NC, S], "y_cool", "y_em" [NP, S] and "rates" [2 + 2 NC, S], the entries
    of the k-packet table before the running sum (for the host tests)."""
    edge = np.asarray(cd.block_edge, dtype=np.int64)
    nu = np.asarray(cd.nu, dtype=np.float64)
    x_sect = np.asarray(cd.x_sect, dtype=np.float64)
    level = np.asarray(cd.level, dtype=np.int64)
    ion = ref.level_ion(pd)[level]
    charge = np.asarray(pd.ion_charge, dtype=np.float64)
    n_ion, n_e, t_e = sol["ion_number_density"], sol["electron_density"], out["t_electrons"]
    n_i, n_up = sol["level_number_density"][level], n_ion[ion + 1]
    NC, NP, S = len(level), len(nu), len(n_e)
    cont = np.repeat(np.arange(NC), np.diff(edge))
    nu_i = nu[edge[:-1]]
    nu_col = nu[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        y_cool = (out["y_sp"] * (H_PLANCK * nu_col)) * (1.0 - nu_i[cont][:, None] / nu_col)
        y_em = (((nu_col * nu_col) * nu_col) * x_sect[:, None]) * out["bfp"]
        t_cool = np.stack([cref.trapezoid(nu[a:b], y_cool[a:b]) for a, b in zip(edge[:-1], edge[1:])])
        c_fb_sp = t_cool * out["phi_ik"]
        cdf = np.zeros((NP, S))
        e_last = np.zeros((NC, S))
        degenerate = np.zeros((NC, S), dtype=bool)
        for c, (a, b) in enumerate(zip(edge[:-1], edge[1:])):
            run = np.zeros((b - a, S))
            for j in range(a, b - 1):
                run[j + 1 - a] = run[j - a] + ((nu[j + 1] - nu[j]) * (y_em[j + 1] + y_em[j])) / 2.0
            e_last[c] = run[-1]
            degenerate[c] = ~((run[-1] > 0.0) & np.isfinite(run[-1]))
            flat = np.zeros((b - a, S))
            flat[-1] = 1.0
            cdf[a:b] = np.where(degenerate[c][None, :], flat, run / run[-1][None, :])
        fb = (c_fb_sp * n_up) * n_e[None, :]
        coll = ((out["coll_ion"] * n_e[None, :]) * n_i) * (H_PLANCK * nu_i)[:, None]
        q = ref.serial_sum(n_ion * (charge * charge)[:, None])
        ff = ((C0_FF * n_e) * np.sqrt(t_e)) * q
        adiabatic = (((3.0 * n_e) * K_BOLTZMANN) * t_e) / time_explosion
        rates = np.concatenate((ff[None, :], adiabatic[None, :], fb, coll))
        running = np.zeros_like(rates)
        total = np.zeros(S)
        for j in range(len(rates)):
            total = total + rates[j]
            running[j] = total
        k_cdf = running / total[None, :]
    return {"c_fb_sp": c_fb_sp, "cool_rate_fb": fb, "cool_rate_coll_ion": coll, "cool_rate_ff": ff, "cool_rate_adiabatic": adiabatic,
            "cool_rate_total": total, "fb_emission_cdf": cdf, "k_cdf": k_cdf, "n_degenerate_fb_cdf": int(degenerate.sum()),
            "degenerate": degenerate, "e_last": e_last, "y_cool": y_cool, "y_em": y_em, "rates": rates}


def process(cool, n_continua, shell, z):
    """(kind, continuum) of a k-packet in ``shell`` at the random number z."""
    col = cool["k_cdf"][:, shell]
    j = min(int(np.searchsorted(col, z, side="right")), len(col) - 1)
    if j < 2:
        return j, -1
    return (KIND_FB, j - 2) if j < 2 + n_continua else (KIND_COLL_ION, j - 2 - n_continua)


def nu_free_bound(cd, cool, c, shell, z):
    a, b = int(cd.block_edge[c]), int(cd.block_edge[c + 1])
    cdf = cool["fb_emission_cdf"][a:b, shell]
    grid = np.asarray(cd.nu, dtype=np.float64)[a:b]
    hi = int(np.clip(np.searchsorted(cdf, z, side="right"), 1, b - a - 1))
    lo = hi - 1
    return float(grid[lo]) + ((float(z) - float(cdf[lo])) * (float(grid[hi]) - float(grid[lo]))) / (float(cdf[hi]) - float(cdf[lo]))


def nu_free_free(out, shell, z):
    with np.errstate(all="ignore"):
        return float(np.float64(-((K_BOLTZMANN * float(out["t_electrons"][shell])) / H_PLANCK)) * np.float64(log(z)))


def sample(cd, out, cool, shell, z_process, z_nu, force_kind=None, force_continuum=None):
    """tardis_mc_kpacket_sample on the tables of continuum_ref.stage() (``out``) and stage() (``cool``): kind, continuum (int64) and
    nu [n].  force_kind[q] == -1 samples the kind and the continuum with z_process[q]; 0 .. 3 sets the kind, and kinds 2 and 3 take
    force_continuum[q]."""
    n = len(shell)
    NC = len(cd.block_edge) - 1
    kind, cont, nu = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n)
    for q in range(n):
        fk = -1 if force_kind is None else int(force_kind[q])
        if fk < 0:
            k, c = process(cool, NC, int(shell[q]), float(z_process[q]))
        else:
            k, c = fk, (int(force_continuum[q]) if fk >= 2 else -1)
        kind[q], cont[q] = k, c
        if k == KIND_FF:
            nu[q] = nu_free_free(out, int(shell[q]), float(z_nu[q]))
        elif k == KIND_FB:
            nu[q] = nu_free_bound(cd, cool, c, int(shell[q]), float(z_nu[q]))
    return {"kind": kind, "continuum": cont, "nu": nu}


def process_batch(cool):
    """The hand-placed z of the kind sampler: per shell and per entry j with k_cdf[j] > k_cdf[j-1], z = k_cdf[j-1] (0.0 for j = 0) and
    z = nextafter(k_cdf[j], 0); plus 0.0 and 1 - 2**-53.  Returns (shell, z, entry expected)."""
    k_cdf = cool["k_cdf"]
    shell, z, entry = [], [], []
    for s in range(k_cdf.shape[1]):
        below = 0.0
        for j in range(k_cdf.shape[0]):
            if k_cdf[j, s] > below:
                shell += [s, s]
                z += [below, float(np.nextafter(k_cdf[j, s], 0.0))]
                entry += [j, j]
            below = max(below, float(k_cdf[j, s]))
        shell += [s, s]
        z += [0.0, 1.0 - 2.0 ** -53]
        entry += [-1, -1]
    return np.array(shell, dtype=np.int64), np.array(z), np.array(entry, dtype=np.int64)


def free_bound_batch(cd, cool, shells):
    """The hand-placed z_nu of the free-bound sampler: per continuum and per shell of ``shells``, every CDF grid value below 1, the
    midpoints between neighbouring grid values, 0.0 and 1 - 2**-53.  Returns (continuum, shell, z_nu)."""
    cont, shell, z = [], [], []
    for c in range(len(cd.block_edge) - 1):
        a, b = int(cd.block_edge[c]), int(cd.block_edge[c + 1])
        for s in shells:
            cdf = cool["fb_emission_cdf"][a:b, s]
            zs = [float(v) for v in cdf if v < 1.0] + [float(0.5 * (u + v)) for u, v in zip(cdf[:-1], cdf[1:])] + [0.0, 1.0 - 2.0 ** -53]
            zs = [v for v in zs if 0.0 <= v < 1.0]
            cont += [c] * len(zs)
            shell += [s] * len(zs)
            z += zs
    return np.array(cont, dtype=np.int64), np.array(shell, dtype=np.int64), np.array(z)
