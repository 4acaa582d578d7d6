// cooling_rates.hpp -- the cooling sub-stage behind the continuum stage of tardis_mc_update_plasma (continuum_rates.hpp): the
// spontaneous-recombination cooling coefficient, the free-bound, collisional-ionisation, free-free and adiabatic cooling rates, the
// free-bound emission CDF of every continuum and the k-packet table.
//
// Restates SpontRecombCoolingRateCoeff, FreeBoundEmissionCDF, FreeBoundCoolingRate, CollIonCooling, FreeFreeCoolingRate and
// AdiabaticCoolingRate in the operation order include/tardis_mc.h spells out (fp64, -ffp-contract=off: every product, quotient, sum and
// difference a rounding of its own).  It reads bfp, y_sp, phi_ik and coll_ion of the continuum stage and the update's populations, and
// writes only its own tables; the samplers that read them are in kpacket_sample.hpp.
//
// Layout, as in the stage before it: everything per point -- the two integrands, fb_emission_cdf -- is [NP][S], the shell fastest, so
// that the lanes of the block kernel (lane = shell) read and write consecutive addresses while they walk a block and a sampler in shell
// s bisects a column; everything per continuum is [NC][S]; k_cdf is [2 + 2 NC][S].
//
// Three kernels, ONE form each.  cooling_point_kernel streams (point, shell) for y_cool and y_em.  cooling_block_kernel has a thread per
// (continuum, shell) and walks its block twice: the first walk forms T(y_cool) and the last value E[b-1] of the running trapezoid, the
// second repeats the running sum -- the same operations on the same values, hence the same bits -- and writes E[p] / E[b-1].  The CDF is
// so written once, normalised, from loads of the read-only y_em; the alternatives, a raw table with a streaming pass behind it or a
// second walk that reads back what the first wrote, cost a launch and an [NC][S] table, or a load that depends on a store.  The walk is
// three adds per point, as in continuum_rate_kernel, whose measured time (profiles/continuum.txt) is why no row-carried form for long
// blocks is built there or here (profiles/cooling_rates.txt has this kernel's).  cooling_table_kernel has a thread per shell: q, the two
// shell rates, then two walks over the 2 + 2 NC entries in the same way, the total first, the quotients second.  Its loads are issued
// eight ahead of the adds that depend on one another (cooling_walk): with a lane per shell the kernel is one or two waves of few live
// lanes and is bound by the latency of a load per entry; the plain loop measured 0.31 ms at NC = 400, S = 20, the batched one 0.12 ms,
// same bits (profiles/cooling_rates.txt).  The degenerate CDFs are counted per workgroup (continuum_block_count) and added on the
// host.  No atomics, nothing waits on another workgroup: two calls give identical bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "continuum_rates.hpp"

namespace mc {

constexpr double C0_FF = 1.426e-27;  // FreeFreeCoolingRate's constant, erg cm^3 s^-1 K^-1/2

struct CoolingArgs {
    int S, NC, I;
    long long K, NP;
    double h, k_b, time_explosion;
    const int *level;         // [NC]
    const int *level_ion;     // [NC]
    const int *block_edge;    // [NC+1]
    const int *point_cont;    // [NP]
    const double *nu;         // [NP]
    const double *x_sect;     // [NP]
    const double *charge;     // [I]
    const double *bfp, *y_sp; // [NP][S] the continuum stage's
    const double *phi_ik;     // [NC][S] rates[0]
    const double *coll_ion;   // [NC][S] rates[5]
    const double *t_e;        // [S]
    const double *n_t;        // [S][K]
    const double *n_ion;      // [I][S]
    const double *n_e;        // [S]
    double *y_cool, *y_em;    // [NP][S] out (point kernel)
    double *rates;            // [3][NC][S] out: c_fb_sp, cool_rate_fb, cool_rate_coll_ion
    double *fb_cdf;           // [NP][S] out
    double *shell;            // [3][S] out: cool_rate_ff, cool_rate_adiabatic, cool_rate_total
    double *k_cdf;            // [2 + 2 NC][S] out
    int *counts;              // [CONTINUUM_COUNT_BLOCKS] out: degenerate CDFs, per workgroup
};

// y_cool = (y_sp (h nu)) (1.0 - nu_i / nu);  y_em = (((nu nu) nu) x_sect) bfp
__global__ void __launch_bounds__(256) cooling_point_kernel(CoolingArgs a)
{
    const long long n = a.NP * a.S;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const long long p = e / a.S;
        const double nu = a.nu[p], nu_i = a.nu[a.block_edge[a.point_cont[p]]];
        a.y_cool[e] = (a.y_sp[e] * (a.h * nu)) * (1.0 - nu_i / nu);
        a.y_em[e] = (((nu * nu) * nu) * a.x_sect[p]) * a.bfp[e];
    }
}

// c_fb_sp, the two cooling rates and the normalised emission CDF of (continuum, shell)
__global__ void __launch_bounds__(256) cooling_block_kernel(CoolingArgs a)
{
    const long long n = (long long)a.NC * a.S;
    int degenerate = 0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e / a.S), s = (int)(e % a.S), S = a.S;
        const int k = a.level[c], i = a.level_ion[c];
        const int p0 = a.block_edge[c], p1 = a.block_edge[c + 1];
        double t_cool = 0.0, run = 0.0;
        double nu_lo = a.nu[p0];
        double cool_lo = a.y_cool[(long long)p0 * S + s], em_lo = a.y_em[(long long)p0 * S + s];
        for (int p = p0 + 1; p < p1; ++p) {
            const double nu_hi = a.nu[p];
            const double cool_hi = a.y_cool[(long long)p * S + s], em_hi = a.y_em[(long long)p * S + s];
            const double d = nu_hi - nu_lo;
            t_cool += (d * (cool_hi + cool_lo)) / 2.0;
            run += (d * (em_hi + em_lo)) / 2.0;
            nu_lo = nu_hi; cool_lo = cool_hi; em_lo = em_hi;
        }
        const double e_last = run;
        const bool ok = e_last > 0.0 && e_last < __builtin_huge_val();  // positive and finite (NaN fails both)
        if (!ok) ++degenerate;
        // the second walk: E[p] again, written as E[p] / E[b-1]
        run = 0.0;
        nu_lo = a.nu[p0];
        em_lo = a.y_em[(long long)p0 * S + s];
        a.fb_cdf[(long long)p0 * S + s] = ok ? run / e_last : 0.0;
        for (int p = p0 + 1; p < p1; ++p) {
            const double nu_hi = a.nu[p];
            const double em_hi = a.y_em[(long long)p * S + s];
            run += ((nu_hi - nu_lo) * (em_hi + em_lo)) / 2.0;
            a.fb_cdf[(long long)p * S + s] = ok ? run / e_last : (p == p1 - 1 ? 1.0 : 0.0);
            nu_lo = nu_hi; em_lo = em_hi;
        }
        const double c_fb_sp = t_cool * a.phi_ik[e];
        const double n_e = a.n_e[s];
        double *r = a.rates + e;
        r[0] = c_fb_sp;
        r[n] = (c_fb_sp * a.n_ion[(long long)(i + 1) * S + s]) * n_e;
        r[2 * n] = ((a.coll_ion[e] * n_e) * a.n_t[(long long)s * a.K + k]) * (a.h * a.nu[p0]);
    }
    continuum_block_count(degenerate, a.counts);
}

constexpr int COOLING_WALK_BATCH = 8;

// visit(j, col[j S]) for j = 0 .. n-1 in ascending j, the loads issued a batch ahead of the visits that depend on one another: with a
// lane per shell a wave has few live lanes and the walk is bound by the latency of its loads, not by their number
template <typename Visit>
__device__ __forceinline__ void cooling_walk(const double *col, int n, long long S, Visit &&visit)
{
    for (int j0 = 0; j0 < n; j0 += COOLING_WALK_BATCH) {
        double v[COOLING_WALK_BATCH];
#pragma unroll
        for (int u = 0; u < COOLING_WALK_BATCH; ++u) v[u] = j0 + u < n ? col[(long long)(j0 + u) * S] : 0.0;
#pragma unroll
        for (int u = 0; u < COOLING_WALK_BATCH; ++u)
            if (j0 + u < n) visit(j0 + u, v[u]);
    }
}

// cool_rate_ff, cool_rate_adiabatic, cool_rate_total and the k-packet table of a shell
__global__ void __launch_bounds__(64) cooling_table_kernel(CoolingArgs a)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const int S = a.S;
    const long long nc = (long long)a.NC * S;
    const double t_e = a.t_e[s], n_e = a.n_e[s];
    double q = 0.0;  // (the free-free sum of continuum_shell_kernel, formed again in its order)
    for (int i = 0; i < a.I; ++i) {
        const double z = a.charge[i];
        q += a.n_ion[(long long)i * S + s] * (z * z);
    }
    const double ff = ((C0_FF * n_e) * sqrt(t_e)) * q;
    const double adiabatic = (((3.0 * n_e) * a.k_b) * t_e) / a.time_explosion;
    const double *col = a.rates + nc + s;  // cool_rate_fb[0 .. NC) then cool_rate_coll_ion[0 .. NC) of this shell: 2 NC rows of stride S
    double total = 0.0;
    total += ff;
    total += adiabatic;
    cooling_walk(col, 2 * a.NC, S, [&](int, double v) { total += v; });
    a.shell[s] = ff;
    a.shell[S + s] = adiabatic;
    a.shell[2 * S + s] = total;
    // the second walk: R[j] again, written as R[j] / cool_rate_total
    double *out = a.k_cdf + s;
    double run = 0.0;
    run += ff;
    out[0] = run / total;
    run += adiabatic;
    out[S] = run / total;
    cooling_walk(col, 2 * a.NC, S, [&](int j, double v) {
        run += v;
        out[(long long)(2 + j) * S] = run / total;
    });
}

}  // namespace mc
