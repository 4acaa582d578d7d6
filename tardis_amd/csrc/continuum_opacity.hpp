// continuum_opacity.hpp -- the continuum opacity at a frequency in a shell, from the resident tables of the continuum stage
// (continuum_rates.hpp): the __device__ function a transport kernel will call, and nothing transport-specific.
//
// Restates chi_continuum_calculator / chi_bf_interpolator / chi_ff_calculator in the operation order include/tardis_mc.h spells out.
// The continua that are current at nu are found by a walk over [nu_min[c], nu_max[c]] in ascending c (the reference's
// photo_ion_nu_threshold_mins / maxs); inside a current block the bracket is hi = clip(searchsorted(b, nu, "left"), 1, n - 1) -- the
// clip at 1 is this project's decision: the reference indexes [-1] when nu equals a block's first frequency.  chi_bf is read as
// chi_bf[p][s] of [NP][S].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mc_device.hpp"
#include "mc_math.hpp"

namespace mc {

// sqrt((2 pi) / ((3 m_e) k_B)) ((4 e^6) / (((3 m_e) h) c)), e = 4.80320451e-10 esu and e^6 = ((((e e) e) e) e) e, CODATA 2010 cgs,
// evaluated once in fp64 and recorded with 17 significant digits (tests/continuum_ref.py carries the same literal)
constexpr double FF_OPAC_CONST = 3.6923492443190485e+08;

struct ContinuumTables {
    int S, NC;
    double h, k_b;
    const int *block_edge;     // [NC+1]
    const double *nu;          // [NP]
    const double *x_sect;      // [NP]
    const double *nu_min;      // [NC] a block's first frequency
    const double *nu_max;      // [NC] a block's last frequency
    const double *chi_bf;      // [NP][S]
    const double *ff;          // [S] ff_opacity_factor
    const double *t_e;         // [S]
};

struct ContinuumOpacity {
    double chi_bf_tot, chi_ff;
    int n_current;
};

// The bracket of nu in a current block b[0 .. n): hi = clip(searchsorted(b, nu, "left"), 1, n - 1), lo = hi - 1, and the three differences of the linear
// interpolation; continuum_interpolate gives ((v_hi hw) + (v_lo lw)) / interval.  Shared by continuum_opacity below and the accumulate pass of the
// photo-ionisation estimators (bf_estimators.hpp).
struct ContinuumBracket {
    int hi;
    double hw, lw, interval;
};
__device__ __forceinline__ ContinuumBracket continuum_bracket(const double *b, int n, double nu)
{
    int lo_i = 0, hi_i = n;  // searchsorted(b, nu, side="left"): the first index with b[index] >= nu
    while (lo_i < hi_i) {
        const int mid = (lo_i + hi_i) >> 1;
        if (b[mid] < nu) lo_i = mid + 1; else hi_i = mid;
    }
    ContinuumBracket k;
    k.hi = lo_i < 1 ? 1 : (lo_i > n - 1 ? n - 1 : lo_i);
    const int lo = k.hi - 1;
    k.interval = b[k.hi] - b[lo]; k.hw = nu - b[lo]; k.lw = b[k.hi] - nu;
    return k;
}
__device__ __forceinline__ double continuum_interpolate(const ContinuumBracket &k, double v_hi, double v_lo) { return ((v_hi * k.hw) + (v_lo * k.lw)) / k.interval; }

// chi_bf_tot, chi_ff and the number of current continua at nu in shell s.  chi_each / x_each (either may be null) receive, with stride
// `each_stride` between continua, the contribution and the interpolated cross-section of every continuum, 0.0 where it is not current.
__device__ __forceinline__ ContinuumOpacity continuum_opacity(const ContinuumTables &t, double nu, int s, double *chi_each, double *x_each, long long each_stride)
{
    ContinuumOpacity out;
    out.chi_bf_tot = 0.0;
    out.n_current = 0;
    for (int c = 0; c < t.NC; ++c) {
        double chi_c = 0.0, x_c = 0.0;
        if (t.nu_min[c] <= nu && nu <= t.nu_max[c]) {
            const int p0 = t.block_edge[c], n = t.block_edge[c + 1] - p0;
            const ContinuumBracket k = continuum_bracket(t.nu + p0, n, nu);
            const int hi = k.hi, lo = hi - 1;
            chi_c = continuum_interpolate(k, t.chi_bf[(long long)(p0 + hi) * t.S + s], t.chi_bf[(long long)(p0 + lo) * t.S + s]);
            x_c = continuum_interpolate(k, t.x_sect[p0 + hi], t.x_sect[p0 + lo]);
            out.chi_bf_tot += chi_c;
            ++out.n_current;
        }
        if (chi_each) chi_each[(long long)c * each_stride] = chi_c;
        if (x_each) x_each[(long long)c * each_stride] = x_c;
    }
    const double beta_e = 1 / (t.k_b * t.t_e[s]);
    out.chi_ff = ((FF_OPAC_CONST * t.ff[s]) / (nu * nu * nu)) * (1 - mcm::exp((t.h * nu) * (-beta_e)));
    return out;
}

struct ContinuumQueryArgs {
    long long n;
    const double *nu;       // [n]
    const int *shell;       // [n]
    double *chi_bf_tot, *chi_ff;  // [n], may be null
    int *n_current;               // [n], may be null
    double *chi_each, *x_each;    // [n][NC], may be null
};

// tardis_mc_continuum_opacity: a thread per query
__global__ void __launch_bounds__(256) continuum_query_kernel(ContinuumTables t, ContinuumQueryArgs q)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= q.n) return;
    const ContinuumOpacity o = continuum_opacity(t, q.nu[e], q.shell[e], q.chi_each ? q.chi_each + e * t.NC : nullptr, q.x_each ? q.x_each + e * t.NC : nullptr, 1);
    if (q.chi_bf_tot) q.chi_bf_tot[e] = o.chi_bf_tot;
    if (q.chi_ff) q.chi_ff[e] = o.chi_ff;
    if (q.n_current) q.n_current[e] = o.n_current;
}

}  // namespace mc
