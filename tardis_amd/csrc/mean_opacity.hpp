// mean_opacity.hpp -- the expansion opacity in frequency bins, and the Planck and Rosseland mean opacities and optical depths per shell,
// from the resident tau_t[S][L] (tardis_mc_mean_opacity; include/tardis_mc.h states the operation order, mean_opacity_plan.hpp the bins).
//
// fp64, -ffp-contract=off keeps every product, quotient and sum a rounding of its own; exp is mcm::exp.  Three kernels, no atomics:
//   mean_opacity_bin_kernel      a lane per (bin, shell), grid.y = shell.  The lane reads its m consecutive entries of the shell's row of tau_t
//                                backwards (the list is descending, the bins ascend), so a wave covers one contiguous run of 64 m entries;
//                                it adds 1 - exp(-tau) in member order and writes kexp_t[S][n_bins].
//   mean_opacity_reduce_*_kernel the four sums of a shell over its bins in ascending order -- pn = sum bd kexp, pd = sum bd,
//                                rn = sum ud / (kthom + kexp), rd = sum ud -- into sums[S][4].  Lane form: a lane per shell.  Row form: a wave per
//                                shell, its four 16-lane DPP rows carry one sum each through serial_prefix (propagate_group.hpp) and from step to
//                                step; slots past the last bin add +0.0, which changes no sum (a running sum from +0.0 is never -0.0).
//   mean_opacity_final_kernel    a lane per mean: kappa of every shell and the depths summed from the surface inward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mc_device.hpp"
#include "mc_math.hpp"
#include "propagate_group.hpp"

namespace mc {

struct MeanOpacityConsts { double ct, planck_coef, h, k_b, c, sigma_thomson; };

__global__ void __launch_bounds__(256) mean_opacity_bin_kernel(const double *__restrict__ tau_t, long long L, long long m, long long e, long long n_bins,
                                                               const double *__restrict__ bin_low, const double *__restrict__ bin_dnu, double ct,
                                                               double *__restrict__ kexp_t)
{
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bins) return;
    const long long s = blockIdx.y;
    const double *__restrict__ tau = tau_t + s * L;
    // member j of the padded sequence is line L + e - j of the descending list; j <= e (bin 0 only) is a pad of optical depth 0.0
    double x = 0.0;
    const long long j0 = b * m + 1, j1 = (b + 1) * m;
    for (long long j = j0; j <= j1; ++j) {
        const double q = j > e ? tau[L + e - j] : 0.0;
        x += 1.0 - mcm::exp(-q);
    }
    kexp_t[s * n_bins + b] = ((bin_low[b] / bin_dnu[b]) / ct) * x;
}

// The four addends of bin b in a shell of temperature t and Thomson opacity kthom: {bd kexp, bd, ud / (kthom + kexp), ud}; all 0.0 where
// exp(h nu / (k_B t)) overflows or equals 1
__device__ __forceinline__ void mean_opacity_terms(double nu, double dnu, double kexp, double t, double kthom, const MeanOpacityConsts &k, double (&out)[4])
{
    const double beta = 1 / (k.k_b * t);
    const double E = mcm::exp((k.h * nu) * beta);
    const double Em1 = E - 1;
    out[0] = out[1] = out[2] = out[3] = 0.0;
    if (!isfinite(E) || Em1 == 0.0) return;
    const double B = (k.planck_coef * (nu * nu * nu)) / Em1;
    const double cn = k.c / nu;
    const double U = (((B * E) * B) * (cn * cn)) / ((2 * k.k_b) * (t * t));
    const double bd = B * dnu, ud = U * dnu;
    out[0] = bd * kexp;
    out[1] = bd;
    out[2] = ud * (1.0 / (kthom + kexp));
    out[3] = ud;
}

__global__ void __launch_bounds__(64) mean_opacity_reduce_lane_kernel(const double *__restrict__ kexp_t, long long n_bins, int S,
                                                                      const double *__restrict__ bin_low, const double *__restrict__ bin_dnu,
                                                                      const double *__restrict__ t_rad, const double *__restrict__ n_e,
                                                                      MeanOpacityConsts k, double *__restrict__ sums)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double *__restrict__ kexp = kexp_t + (long long)s * n_bins;
    const double t = t_rad[s], kthom = n_e[s] * k.sigma_thomson;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long b = 0; b < n_bins; ++b) {
        double v[4];
        mean_opacity_terms(bin_low[b], bin_dnu[b], kexp[b], t, kthom, k, v);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += v[r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) sums[4 * s + r] = acc[r];
}

// A wave per shell (four shells per 256-thread workgroup); row r = lane / 16 of the wave carries sum r, lane q of a row takes bins q, 16 + q, ...
__global__ void __launch_bounds__(256) mean_opacity_reduce_row_kernel(const double *__restrict__ kexp_t, long long n_bins, int S,
                                                                      const double *__restrict__ bin_low, const double *__restrict__ bin_dnu,
                                                                      const double *__restrict__ t_rad, const double *__restrict__ n_e,
                                                                      MeanOpacityConsts k, double *__restrict__ sums)
{
    const int s = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);  // (whole waves leave here together)
    if (s >= S) return;
    const int q = threadIdx.x & 15, r = (threadIdx.x >> 4) & 3;
    const double *__restrict__ kexp = kexp_t + (long long)s * n_bins;
    const double t = t_rad[s], kthom = n_e[s] * k.sigma_thomson;
    double carry = 0.0;
    for (long long b0 = 0; b0 < n_bins; b0 += 16) {
        const long long b = b0 + q;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (b < n_bins) mean_opacity_terms(bin_low[b], bin_dnu[b], kexp[b], t, kthom, k, v);
        const double mine = r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : v[3];
        const double acc = serial_prefix<16>(carry, mine, q);
        carry = gbcast<16>(acc, 15);
    }
    if (q == 0) sums[4 * s + r] = carry;
}

// Lane 0: kappa_planck and tau_planck; lane 1: kappa_rosseland and tau_rosseland.  out: [4][S] = kappa_planck, kappa_rosseland, tau_planck, tau_rosseland
__global__ void __launch_bounds__(64) mean_opacity_final_kernel(const double *__restrict__ sums, int S, const double *__restrict__ n_e,
                                                                const double *__restrict__ r_inner, const double *__restrict__ r_outer,
                                                                double sigma_thomson, double *__restrict__ out)
{
    const int mean = threadIdx.x;
    if (blockIdx.x != 0 || mean > 1) return;
    double *__restrict__ kappa = out + (long long)mean * S, *__restrict__ tau = out + (long long)(2 + mean) * S;
    double below = 0.0;
    for (int s = S - 1; s >= 0; --s) {
        const double *a = sums + 4 * s;
        const double kap = mean == 0 ? n_e[s] * sigma_thomson + a[0] / a[1] : 1.0 / (a[2] / a[3]);
        const double d = kap * (r_outer[s] - r_inner[s]);
        const double depth = s == S - 1 ? d : below + d;
        kappa[s] = kap;
        tau[s] = depth;
        below = depth;
    }
}

}  // namespace mc
