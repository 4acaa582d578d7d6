// opacity_update.hpp -- the opacity tables of the next iteration, computed on the device from level populations.
//
// Restates StimulatedEmissionFactor, TauSobolev, BetaSobolev, JBluesDiluteBlackBody and calculate_transition_probabilities of the
// legacy plasma in their operation order (fp64, -ffp-contract=off keeps every product and sum a rounding of its own).  Per line l
// and shell s, with n_l / n_u the populations of the line's lower / upper level:
//   sef  = 1 - (g_lower n_u) / (g_upper n_l), 0 where n_l == 0 or the result is negative
//   tau  = ((((sobolev_coefficient f_lu) wavelength_cm) t_exp) n_l) sef
//   beta = 1 / tau (tau > 1e3), 1 - 0.5 tau (tau < 1e-4), (1 - exp(-tau)) / tau otherwise
//   j    = W (planck_coef nu^3 / (exp(h nu / (k_B t_rad)) - 1))   (dilute black body; the detailed j_blues come from radfield_jblue_kernel)
// and per transition row t of a block: p = coef[t] beta[line], times sef[line] j[line] for a type-1 row, divided by the block's
// serial left-to-right sum of p (0 where that sum is 0).
//
// Layout: everything shell-major, as the propagation reads it -- n_t[S][K] (the [K,S] upload transposed, so that a shell's gathers
// stay within one row), tau_t / beta_t / sef_t / j_t [S][L], prob_t[S][T].
//
// Two kernels.  opacity_line_kernel streams the lines of a shell (a 256-thread workgroup per tile, grid.y = shell).  The block kernel
// comes in two forms that add in the same order (opacity_update_plan.hpp chooses per block): a lane per (block, shell) for short
// blocks, and a 16-lane DPP row per (block, shell) for long ones -- lanes load consecutive rows and gather beta / sef / j, and the
// running sum is carried through the row with serial_prefix (propagate_group.hpp), then from step to step.  Either form first stores the
// unnormalised p into prob_t and then divides what it stored: the same lane writes and reads a row, no synchronisation is needed.
// No atomics: two calls give identical bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mc_device.hpp"
#include "mc_math.hpp"
#include "propagate_group.hpp"

namespace mc {

struct OpacityUpdateConsts { double coef_sobolev, t_exp, planck_coef, h, k_b; };

// j of the dilute black body, W (planck_coef nu^3 / (exp(h nu beta_rad) - 1)): one spelling for the line kernel below, the detailed j_blues'
// fallbacks and the NLTE rates (nlte_excitation.hpp), whose j have to be these bits
__device__ __forceinline__ double dilute_black_body_j(double ws, double planck_coef, double h, double nu, double beta_rad)
{
    return ws * (planck_coef * (nu * nu * nu) / (mcm::exp(h * nu * beta_rad) - 1));
}

// One detailed j_blue (radfield_jblue_kernel): the normalised estimator, the dilute black body outside the optical window, w_epsilon times it
// where the estimator is empty
__device__ __forceinline__ double detailed_j_blue(double estimator, double norm, double nu, double ws, double beta_rad, double planck_coef, double h,
                                                  double w_epsilon, double c_ang, int optical_window)
{
    const double est = estimator * norm;
    double value = est;
    bool outside = false;
    if (optical_window) {
        const double wav = c_ang / nu;  // Angstrom
        outside = !(wav > 2500.0 && wav < 10000.0);
    }
    if (est == 0.0 || outside) {
        const double planck = dilute_black_body_j(ws, planck_coef, h, nu, beta_rad);
        value = outside ? planck : value;
        if (est == 0.0) value = w_epsilon * planck;
    }
    return value;
}

// MODE0: j of the dilute black body is computed here; otherwise j_t already holds the detailed j_blues and is only read by the block kernel
template <bool MODE0>
__global__ void __launch_bounds__(256) opacity_line_kernel(const double *__restrict__ n_t, const int *__restrict__ level_lower,
                                                           const int *__restrict__ level_upper, const double *__restrict__ f_lu,
                                                           const double *__restrict__ wavelength_cm, const double *__restrict__ g_lower,
                                                           const double *__restrict__ g_upper, const double *__restrict__ nu_line,
                                                           const double *__restrict__ t_rad, const double *__restrict__ w, long long K, long long L,
                                                           OpacityUpdateConsts k, double *__restrict__ tau_t, double *__restrict__ beta_t,
                                                           double *__restrict__ sef_t, double *__restrict__ j_t)
{
    const long long s = blockIdx.y;
    const double *__restrict__ n = n_t + s * K;
    double beta_rad = 0.0, ws = 0.0;
    if (MODE0) { beta_rad = 1 / (k.k_b * t_rad[s]); ws = w[s]; }
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < L; l += (long long)gridDim.x * blockDim.x) {
        const double n_l = n[level_lower[l]], n_u = n[level_upper[l]];
        double sef = 0.0;
        if (n_l != 0.0) {
            sef = 1.0 - (g_lower[l] * n_u) / (g_upper[l] * n_l);
            if (sef < 0.0) sef = 0.0;
        }
        const double tau = ((((k.coef_sobolev * f_lu[l]) * wavelength_cm[l]) * k.t_exp) * n_l) * sef;
        double beta;
        if (tau > 1e3) beta = 1.0 / tau;
        else if (tau < 1e-4) beta = 1.0 - 0.5 * tau;
        else beta = (1.0 - mcm::exp(-tau)) / tau;
        const long long i = s * L + l;
        tau_t[i] = tau;
        beta_t[i] = beta;
        sef_t[i] = sef;
        if (MODE0) {
            const double nu = nu_line[l];
            j_t[i] = dilute_black_body_j(ws, k.planck_coef, k.h, nu, beta_rad);
        }
    }
}

// unnormalised probability of transition row t in one shell (the three tables are that shell's rows)
__device__ __forceinline__ double opacity_row_probability(long long t, const double *__restrict__ coef, const int *__restrict__ tline,
                                                          const int *__restrict__ ttype, const double *__restrict__ beta,
                                                          const double *__restrict__ sef, const double *__restrict__ j)
{
    const int line = tline[t];
    double p = coef[t] * beta[line];
    if (ttype[t] == 1) p = p * (sef[line] * j[line]);
    return p;
}

// Short blocks: one lane per (block, shell), consecutive lanes on consecutive blocks of a shell.  Blocks of long_rows rows or more
// are left to opacity_block_row_kernel.
__global__ void __launch_bounds__(256) opacity_block_lane_kernel(const int *__restrict__ block_edge, int n_blocks, long long T, long long L, int S,
                                                                 long long long_rows, const double *__restrict__ coef,
                                                                 const int *__restrict__ tline, const int *__restrict__ ttype,
                                                                 const double *__restrict__ beta_t, const double *__restrict__ sef_t,
                                                                 const double *__restrict__ j_t, double *__restrict__ prob_t)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n_blocks * S) return;
    const int b = (int)(i % n_blocks);
    const long long s = i / n_blocks;
    const int b0 = block_edge[b], b1 = block_edge[b + 1];
    if (b1 <= b0 || (long long)(b1 - b0) >= long_rows) return;
    const double *beta = beta_t + s * L, *sef = sef_t + s * L, *j = j_t + s * L;
    double *p = prob_t + s * T;
    double norm = 0.0;
    for (int k0 = b0; k0 < b1; k0 += 8) {  // (eight rows requested together; the additions stay one after the other)
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = k0 + q < b1 ? opacity_row_probability(k0 + q, coef, tline, ttype, beta, sef, j) : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (k0 + q < b1) {
                norm += v[q];
                p[k0 + q] = v[q];
            }
    }
    for (int k = b0; k < b1; ++k) p[k] = norm != 0.0 ? p[k] / norm : 0.0;
}

// Long blocks: a 16-lane DPP row per (listed block, shell); sixteen rows of lanes per 256-thread workgroup.  Lane q of the row takes
// transition rows b0 + q, b0 + 16 + q, ...; rows past the block's end add +0.0, which changes no sum.
__global__ void __launch_bounds__(256) opacity_block_row_kernel(const int *__restrict__ long_blocks, int n_long, const int *__restrict__ block_edge,
                                                                long long T, long long L, int S, const double *__restrict__ coef,
                                                                const int *__restrict__ tline, const int *__restrict__ ttype,
                                                                const double *__restrict__ beta_t, const double *__restrict__ sef_t,
                                                                const double *__restrict__ j_t, double *__restrict__ prob_t)
{
    const long long e = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;  // (whole DPP rows leave here together)
    if (e >= (long long)n_long * S) return;
    const int q = threadIdx.x & 15;
    const int b = long_blocks[e % n_long];
    const long long s = e / n_long;
    const int b0 = block_edge[b], b1 = block_edge[b + 1];
    const double *beta = beta_t + s * L, *sef = sef_t + s * L, *j = j_t + s * L;
    double *p = prob_t + s * T;
    double carry = 0.0;
    for (int k0 = b0; k0 < b1; k0 += 16) {
        const int t = k0 + q;
        const double v = t < b1 ? opacity_row_probability(t, coef, tline, ttype, beta, sef, j) : 0.0;
        if (t < b1) p[t] = v;
        const double acc = serial_prefix<16>(carry, v, q);
        carry = gbcast<16>(acc, 15);
    }
    const double norm = carry;
    for (int t = b0 + q; t < b1; t += 16) p[t] = norm != 0.0 ? p[t] / norm : 0.0;
}

}  // namespace mc
