"""The host side of the cooling sub-stage, without a GPU: the header's prototypes, and the restatement (tests/cooling_ref.py, the
yardstick of tests/test_cooling_gpu.py) on the planted model -- its CDFs and the k-packet table as distributions, every arm of the
arithmetic exercised in both population arms, and the samplers' properties."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import continuum_ref as cref  # noqa: E402
import cooling_ref as kref  # noqa: E402
import plasma_update_ref as ref  # noqa: E402
from tardis_amd import _abi, _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("nebular", "lte")


@pytest.fixture(scope="module")
def planted(oracle):
    pd, ld, prob, t_rad, w, cd, facts = cref.planted_continuum_model()
    arms = {}
    for arm in ARMS:
        sol = ref.solve(pd, t_rad, w, *(("lte", "lte") if arm == "lte" else ()))
        out = cref.stage(pd, cd, sol, t_rad, w)
        arms[arm] = (sol, out, kref.stage(pd, cd, sol, out, prob.time_explosion))
    return SimpleNamespace(pd=pd, cd=cd, t_rad=t_rad, w=w, facts=facts, arms=arms, NC=len(cd.level), S=len(t_rad))


def test_the_header_carries_the_prototypes_and_the_abi_version():
    header = open(os.path.join(ROOT, "include", "tardis_mc.h")).read()
    assert "#define TARDIS_MC_ABI_VERSION 2 " in header and _abi.ABI_VERSION == 2
    flat = re.sub(r"\s+", " ", header)
    for proto in ("int tardis_mc_get_cooling_rates(TardisMcContext *ctx, double *c_fb_sp, double *cool_rate_fb, double *cool_rate_coll_ion, "
                  "double *cool_rate_ff, double *cool_rate_adiabatic, double *cool_rate_total);",
                  "int tardis_mc_get_kpacket_tables(TardisMcContext *ctx, double *fb_emission_cdf, double *k_cdf, int64_t *n_degenerate_fb_cdf);",
                  "int tardis_mc_last_cooling_ms(TardisMcContext *ctx, double *out_points_ms, double *out_blocks_ms, double *out_table_ms);",
                  "int tardis_mc_kpacket_sample(TardisMcContext *ctx, const TardisMcKpacketQuery *query);",
                  "typedef struct TardisMcKpacketQuery {"):
        assert proto in flat, proto
    # the project's decisions and what is not covered are stated where a caller reads them
    for words in ("where E[b-1] is not positive and finite", "The reference produces NaN there", "collisional-excitation cooling is NOT in the table",
                  "C0_FF = 1.426e-27", "p_fb_deactivation", "the choice of the absorbing continuum", "NLTE ionisation",
                  "any reader of these tables in the propagation kernels"):
        assert words in flat, words
    assert _abi.C.sizeof(_abi.TardisMcKpacketQuery) == 9 * 8
    for name in ("tardis_mc_get_cooling_rates", "tardis_mc_get_kpacket_tables", "tardis_mc_last_cooling_ms", "tardis_mc_kpacket_sample"):
        assert name in _lib.SYMBOLS
    assert "1.426e-27" in open(os.path.join(ROOT, "tardis_amd", "csrc", "cooling_rates.hpp")).read() and kref.C0_FF == 1.426e-27


@pytest.mark.parametrize("arm", ARMS)
def test_the_tables_are_distributions(planted, arm):
    _, _, cool = planted.arms[arm]
    cdf, edge = cool["fb_emission_cdf"], planted.cd.block_edge
    for a, b in zip(edge[:-1], edge[1:]):
        assert np.all(cdf[a] == 0.0) and np.all(cdf[b - 1] == 1.0)
        assert np.all(np.diff(cdf[a:b], axis=0) >= 0.0)
    k_cdf = cool["k_cdf"]
    assert k_cdf.shape == (2 + 2 * planted.NC, planted.S)
    assert np.all(k_cdf[-1] == 1.0) and np.all(np.diff(k_cdf, axis=0) >= 0.0) and np.all(k_cdf[0] > 0.0)
    assert np.array_equal(cool["rates"][0], cool["cool_rate_ff"]) and np.array_equal(cool["rates"][1], cool["cool_rate_adiabatic"])


@pytest.mark.parametrize("arm", ARMS)
def test_the_planted_model_exercises_every_arm(planted, arm):
    _, out, cool = planted.arms[arm]
    NC = planted.NC
    # the degenerate CDF: bfp underflows on the whole block of continuum 9 in the cold shell
    assert cool["e_last"][9, 0] == 0.0 and cool["degenerate"][9, 0] and cool["n_degenerate_fb_cdf"] == int(cool["degenerate"].sum()) >= 1
    a, b = int(planted.cd.block_edge[9]), int(planted.cd.block_edge[10])
    assert not cool["fb_emission_cdf"][a:b - 1, 0].any() and cool["fb_emission_cdf"][b - 1, 0] == 1.0
    assert cool["cool_rate_fb"][9, 0] == 0.0                    # ... and it is never chosen
    # zero-width entries of k_cdf
    zero = int((cool["cool_rate_fb"] == 0.0).sum())
    assert cool["cool_rate_fb"].size == 48 and 13 <= zero <= 14, zero
    # no rate is non-finite although phi_ik comes close to the largest number
    assert out["phi_ik"].max() > 1e307
    for name in kref.RATES + kref.SHELL + kref.TABLES:
        assert np.all(np.isfinite(cool[name])), name
    # all four kinds have a positive rate in every shell
    r = cool["rates"]
    assert np.all(r >= 0.0)
    assert np.all(r[0] > 0.0) and np.all(r[1] > 0.0) and np.all(r[2:2 + NC].max(axis=0) > 0.0) and np.all(r[2 + NC:].max(axis=0) > 0.0)


@pytest.mark.parametrize("arm", ARMS)
def test_process_never_returns_an_entry_of_zero_rate(planted, arm):
    _, out, cool = planted.arms[arm]
    NC, r = planted.NC, cool["rates"]
    shell, z, entry = kref.process_batch(cool)
    rng = np.random.default_rng(11)
    shell = np.concatenate((shell, rng.integers(0, planted.S, 400)))
    z = np.concatenate((z, rng.random(400)))
    entry = np.concatenate((entry, np.full(400, -1)))
    seen = set()
    for s, v, want in zip(shell, z, entry):
        kind, c = kref.process(cool, NC, int(s), float(v))
        j = kind if kind < 2 else (2 + c if kind == 2 else 2 + NC + c)
        assert r[j, s] > 0.0, (s, v, j)
        assert (c == -1) == (kind < 2) and (kind < 2 or 0 <= c < NC)
        assert want < 0 or j == want, (s, v, j, want)
        seen.add(kind)
    assert seen == {0, 1, 2, 3}
    assert kref.process(cool, NC, 0, 0.0) == (0, -1)           # z = 0.0 takes the first entry: its rate is positive


@pytest.mark.parametrize("arm", ARMS)
def test_the_frequency_samplers(planted, arm):
    _, out, cool = planted.arms[arm]
    cd = planted.cd
    cont, shell, z = kref.free_bound_batch(cd, cool, range(planted.S))
    assert set(cont) == set(range(planted.NC)) and np.all((z >= 0.0) & (z < 1.0))
    got = kref.sample(cd, out, cool, shell, z, z, np.full(len(z), 2), cont)
    lo, hi = cd.nu[cd.block_edge[:-1]][cont], cd.nu[cd.block_edge[1:] - 1][cont]
    # inside the block: the weight (z - cdf[lo]) / (cdf[hi] - cdf[lo]) lies in [0, 1) before its three roundings and the sum adds a
    # fourth, so the upper end is the block's last frequency to 4 * 2^-53 of it
    assert np.all(np.isfinite(got["nu"])) and np.all((got["nu"] >= lo) & (got["nu"] <= hi * (1.0 + 2.0 ** -51)))
    # z = 0.0 gives the threshold where the first interval carries weight; in the degenerate block every z lands in the last interval
    a, b = int(cd.block_edge[9]), int(cd.block_edge[10])
    for v in (0.0, 0.5, 1.0 - 2.0 ** -53):
        assert cd.nu[b - 2] <= kref.nu_free_bound(cd, cool, 9, 0, v) <= cd.nu[b - 1] * (1.0 + 2.0 ** -51)
    assert kref.nu_free_bound(cd, cool, 0, 1, 0.0) == cd.nu[0]  # (the two-point block)
    # free-free: +inf at z = 0.0, k_B t_e / h at z = 1 / e to the rounding of log and a product, falling in z
    assert kref.nu_free_free(out, 0, 0.0) == np.inf
    scale = cref.K_BOLTZMANN * out["t_electrons"][2] / cref.H_PLANCK
    assert abs(kref.nu_free_free(out, 2, float(np.exp(-1.0))) - scale) <= 4 * 2.0 ** -52 * scale
    assert kref.nu_free_free(out, 2, 0.25) > kref.nu_free_free(out, 2, 0.5) > kref.nu_free_free(out, 2, 1.0 - 2.0 ** -53) > 0.0
