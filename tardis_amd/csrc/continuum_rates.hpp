// continuum_rates.hpp -- the continuum stage of tardis_mc_update_plasma: Saha factors, photo-ionisation / recombination / collisional
// ionisation rate coefficients in the dilute black body, the resident bound-free opacity table and the free-free factor.
//
// Restates SahaFactor, SpontRecombRateCoeff, PhotoIonRateCoeff (dilute Planckian field), StimRecombRateCoeff, CorrPhotoIonRateCoeff,
// CollIonRateCoeffSeaton, CollRecombRateCoeff, BoundFreeOpacity and ff_opacity_factor in the operation order include/tardis_mc.h spells
// out (fp64, -ffp-contract=off: every product, quotient, sum and difference a rounding of its own; exp is mcm::exp).
//
// Layout: everything per point -- bfp, the three integrands, chi_bf -- is [NP][S], the shell fastest: the layout tardis_mc_get_continuum_opacity
// hands out, the one in which the lanes of the rate kernel (lane = shell) read consecutive addresses while they walk a block, and the one
// the query of continuum_opacity.hpp reads two rows of per current continuum.  Everything per continuum is [NC][S].  The thermal
// Boltzmann factors lbf_e are [S][K] and their partition functions Z_e [I][S], because they are made by the kernels of
// plasma_update.hpp (plasma_boltzmann_kernel<false> on t_e, the two partition kernels): both forms of the partition kernel add in the
// same order.
//
// Four kernels here, ONE form each (continuum_plan.hpp says why).  continuum_shell_kernel, a thread per shell: t_e and the free-free
// factor.  continuum_point_kernel streams (point, shell).  continuum_rate_kernel has a thread per (continuum, shell): it forms phi_ik,
// walks its block serially (three running sums on loads that do not depend on them) and writes the seven [NC][S] outputs.
// continuum_chi_kernel streams (point, shell) again.  The two clamps are counted per workgroup in LDS and written to counts[blockIdx.x];
// the host adds the workgroups' counts.  No atomics, nothing waits on another workgroup: two calls give identical bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include "mc_device.hpp"
#include "mc_math.hpp"

namespace mc {

constexpr int CONTINUUM_COUNT_BLOCKS = 1024;  // upper bound on the workgroups of the two counting kernels (grid-stride beyond it)

struct ContinuumArgs {
    int S, NC, I;
    long long K, NP;
    double link, k_b, h, two_pi_me, hh;  // t_e = link t_rad; (2 pi) m_e and h h are rounded once, on the host
    double planck_coef, cc, eight_pi, four_pi, h_over_k;  // 2 h / (c c), c c, 8 pi, 4 pi, h / k_B: likewise
    const int *level;         // [NC]
    const int *level_ion;     // [NC]
    const int *block_edge;    // [NC+1]
    const int *point_cont;    // [NP] the continuum of a point
    const double *nu;         // [NP]
    const double *x_sect;     // [NP]
    const double *charge;     // [I]
    const double *chi;        // [I]
    const double *t_rad, *w;  // [S]
    const double *lbf_e;      // [S][K]
    const double *z_e;        // [I][S]
    const double *n_t;        // [S][K] the update's level populations
    const double *n_ion;      // [I][S]
    const double *n_e;        // [S] the solved electron density
    double *t_e, *ff;         // [S] out
    double *bfp, *y_sp, *y_g, *y_st;  // [NP][S] out (point kernel)
    double *rates;            // [7][NC][S] out: phi_ik, alpha_sp, gamma, alpha_stim, gamma_corr, coll_ion, coll_recomb
    double *chi_bf;           // [NP][S] out
    int *counts;              // [2][CONTINUUM_COUNT_BLOCKS] out: negative gamma_corr | negative chi_bf, per workgroup
    const double *gamma_est, *stim_est;  // [NC][S] option continuum_field 1: the transport's photo-ionisation estimators (bf_estimators.hpp); null: the dilute black body
};

// the sum of a workgroup's per-thread counts, written by thread 0 (integers: the order of the additions changes nothing)
__device__ __forceinline__ void continuum_block_count(int mine, int *out)
{
    __shared__ int part[256];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = part[0];
}

// t_e = link t_rad; q = the serial sum over all ion rows of N_i (charge_i charge_i); ff = (n_e q) / sqrt(t_e)
__global__ void __launch_bounds__(64) continuum_shell_kernel(ContinuumArgs a)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const double t_e = a.link * a.t_rad[s];
    double q = 0.0;
    for (int i = 0; i < a.I; ++i) {
        const double z = a.charge[i];
        q += a.n_ion[(long long)i * a.S + s] * (z * z);
    }
    a.t_e[s] = t_e;
    a.ff[s] = (a.n_e[s] * q) / sqrt(t_e);
}

// bfp and the integrands of the three rate integrals at every (point, shell)
__global__ void __launch_bounds__(256) continuum_point_kernel(ContinuumArgs a)
{
    const long long n = a.NP * a.S;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const long long p = e / a.S;
        const int s = (int)(e % a.S);
        const double t_rad = a.t_rad[s];
        const double beta_rad = 1 / (a.k_b * t_rad);
        const double beta_e = 1 / (a.k_b * (a.link * t_rad));
        const double nu = a.nu[p], x = a.x_sect[p];
        const double hnu = a.h * nu;
        const double bfp = mcm::exp(hnu * (-beta_e));
        const double j = a.w[s] * ((a.planck_coef * (nu * nu * nu)) / (mcm::exp(hnu * beta_rad) - 1));
        const double y_g = j * (((a.four_pi * x) / nu) / a.h);
        a.bfp[e] = bfp;
        a.y_sp[e] = (((a.eight_pi * x) * (nu * nu)) / a.cc) * bfp;
        a.y_g[e] = y_g;
        a.y_st[e] = y_g * bfp;
    }
}

// phi_ik, the three trapezoid sums over the continuum's block, the seven rate coefficients of (continuum, shell)
__global__ void __launch_bounds__(256) continuum_rate_kernel(ContinuumArgs a)
{
    const long long n = (long long)a.NC * a.S;
    int clamped = 0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(e / a.S), s = (int)(e % a.S), S = a.S;
        const int k = a.level[c], i = a.level_ion[c];
        const double t_e = a.link * a.t_rad[s];
        const double beta_e = 1 / (a.k_b * t_e);
        const double x = (a.two_pi_me / beta_e) / a.hh;
        const double g_ee = x * sqrt(x);
        const double z_lo = a.z_e[(long long)i * S + s], z_up = a.z_e[(long long)(i + 1) * S + s];
        double saha = (z_up / z_lo) * ((2 * g_ee) * mcm::exp(a.chi[i] * (-beta_e)));
        if (saha == 0.0) saha = DBL_MIN;
        const double phi = a.lbf_e[(long long)s * a.K + k] / (saha * z_lo);
        const int p0 = a.block_edge[c], p1 = a.block_edge[c + 1];
        double t_sp = 0.0, t_g = 0.0, t_st = 0.0;
        double nu_lo = a.nu[p0];
        double sp_lo = a.y_sp[(long long)p0 * S + s], g_lo = a.y_g[(long long)p0 * S + s], st_lo = a.y_st[(long long)p0 * S + s];
        for (int p = p0 + 1; p < p1; ++p) {
            const double nu_hi = a.nu[p];
            const double sp_hi = a.y_sp[(long long)p * S + s], g_hi = a.y_g[(long long)p * S + s], st_hi = a.y_st[(long long)p * S + s];
            const double d = nu_hi - nu_lo;
            t_sp += (d * (sp_hi + sp_lo)) / 2.0;
            t_g += (d * (g_hi + g_lo)) / 2.0;
            t_st += (d * (st_hi + st_lo)) / 2.0;
            nu_lo = nu_hi; sp_lo = sp_hi; g_lo = g_hi; st_lo = st_hi;
        }
        // (continuum_field 1: the field the packets carried instead of the two integrals over the dilute black body; everything else as before)
        const double alpha_sp = t_sp * phi, gamma = a.gamma_est ? a.gamma_est[e] : t_g, alpha_stim = (a.stim_est ? a.stim_est[e] : t_st) * phi;
        const double n_i = a.n_t[(long long)s * a.K + k], n_up = a.n_ion[(long long)(i + 1) * S + s], n_e = a.n_e[s];
        double gamma_corr = gamma;
        if (n_i != 0.0) gamma_corr = gamma - ((alpha_stim * n_up) * n_e) / n_i;
        if (gamma_corr < 0.0) { gamma_corr = 0.0; ++clamped; }
        const double u0 = (a.nu[p0] / t_e) * a.h_over_k;
        const double f = mcm::exp(-u0) / u0;
        const double z = a.charge[i];
        const double gbar = z == 0.0 ? 0.1 : (z == 1.0 ? 0.2 : 0.3);
        const double coll_ion = ((f * (1.55e13 * a.x_sect[p0])) / sqrt(t_e)) * gbar;
        double *r = a.rates + e;
        r[0] = phi; r[n] = alpha_sp; r[2 * n] = gamma; r[3 * n] = alpha_stim; r[4 * n] = gamma_corr; r[5 * n] = coll_ion; r[6 * n] = coll_ion * phi;
    }
    continuum_block_count(clamped, a.counts);
}

// chi_bf[p][s] = (n_i - ((phi_ik N_up) n_e) bfp) x_sect, a negative value 0.0 and counted
__global__ void __launch_bounds__(256) continuum_chi_kernel(ContinuumArgs a)
{
    const long long n = a.NP * a.S;
    int clamped = 0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const long long p = e / a.S;
        const int s = (int)(e % a.S), c = a.point_cont[p];
        const int k = a.level[c], i = a.level_ion[c];
        const double n_lte = (a.rates[(long long)c * a.S + s] * a.n_ion[(long long)(i + 1) * a.S + s]) * a.n_e[s];
        double chi = (a.n_t[(long long)s * a.K + k] - n_lte * a.bfp[e]) * a.x_sect[p];
        if (chi < 0.0) { chi = 0.0; ++clamped; }
        a.chi_bf[e] = chi;
    }
    continuum_block_count(clamped, a.counts + CONTINUUM_COUNT_BLOCKS);
}

}  // namespace mc
