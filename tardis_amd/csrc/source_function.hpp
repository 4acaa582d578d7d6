// source_function.hpp -- the line source function of the formal integral on the device.
//
// Follows make_source_function (tardis/spectrum/formal_integral/source_function.py) on what is resident after
// set_opacity and propagate: the shell-major probabilities prob_t[S][T], the macro-atom index tables, tau_t[S][L] and
// the j_blue / Edotlu estimators [S][L].  Per shell s:
//   Edotlu[s][l]  = (1 / (t_sim vol[s])) (1 - exp(-tau[s][l])) Edotlu_est[s][l]
//   e_dot_u[s][k] = sum of Edotlu[s][l] over the lines whose upper level is k
//   C[s]          = e_dot_u[s] (downbranch), or the solution of (I - Q_s)^T C = e_dot_u[s] (macroatom), where Q_s[i][j]
//                   sums prob[s][t] over the internal rows t (type >= 0) of block i that end in level j
//   att_S_ul[s][l] = wave[l] (prob[s][t] C[s][k]) t_sim / (4 pi) for the one emission row t (type -1) of line l, in block k
//   Jblue_lu[s][l] = j_blue_est[s][l] (c t_exp / (4 pi t_sim vol[s])),  Jred_lu = Jblue_lu exp(-tau) + att_S_ul.
//
// Layout.  Two indices over the macro-atom tables are built once per set_opacity by counting sort, both in CSR form and
// shared by all shells: the lines of every upper level (ascending), and the internal rows that END in every level
// (ascending row ids) with the level each of them leaves.  A solve first gathers the probabilities of those rows into
// q[S][nnz] in index order, so that an iteration streams them instead of fetching 8 bytes from every 64-byte sector of
// prob_t.  The level vectors are x[S][levels].
//
// The solve is the fixed-point iteration x <- e + Q^T x from x = e, in gather form: one sum per (level, shell) over
// the incoming rows, ping-pong between two buffers, no atomics.  A CSR row is summed by a group of G lanes (1, 4 or 16,
// chosen per index from its mean row length: sf_group_width) -- lane i of the group takes entries i, i + G, ... in order,
// then a fixed butterfly adds the G partial sums; rows of more than SF_LONG_STEPS * G entries are left to the whole wave,
// which sums them the same way with G = 64.  The order of every sum is therefore a function of the index alone and
// results are bit-identical from run to run.
//
// Stop rule.  The host reads sf_convergence_kernel's {max |dx|, max |x|} per shell every 16 iterations and ends the solve when max |dx| == 0
// in every shell: the last iteration changed no level.  With non-negative e and q every operation of an iteration is monotone in x, x_1 >= x_0 = e,
// and so x_n never decreases in any component: the iteration cannot circle and ends exactly at the fixed point of the ROUNDED map, which lies
// within (r + n + 3) 2^-53 B_k of the exact C_k (r the longest incoming row, n the most lines on a level, B = (I - Q^T)^-1 C).  No
// norm over the levels enters the rule: a weak ion beside a strong one is converged relative to itself.  (Negative estimators, depths or
// probabilities void the argument; an iteration that then never settles ends at the bound on the iterations, as an error.)
// fp64 throughout; -ffp-contract=off keeps every product and sum a rounding of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mc_device.hpp"

namespace mc {

constexpr int SF_LONG_STEPS = 32;  // a group of G lanes sums CSR rows of up to SF_LONG_STEPS * G entries; longer ones go to the whole wave

// lanes per row for an index of n_rows rows and nnz entries (host): about four entries per lane at the mean row length
inline int sf_group_width(long long nnz, long long n_rows)
{
    const double mean = n_rows > 0 ? (double)nnz / (double)n_rows : 0.0;
    return mean <= 4.0 ? 1 : (mean <= 16.0 ? 4 : 16);
}

// every lane of a group of W lanes gets the same sum of the group's W values, added in the same order
template <int W>
__device__ __forceinline__ double sf_group_sum(double v)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// init + sum of term(j) over the CSR row [ptr[row], ptr[row + 1]) of this lane's group of G lanes (all of them get it); the whole
// wave must call it (rows past n_rows take no part in anything but the shuffles).
template <int G, typename Term>
__device__ __forceinline__ double sf_row_sum(const int *__restrict__ ptr, long long row, long long n_rows, double init, Term term)
{
    const int lane = threadIdx.x & 63, sub = lane & (G - 1);
    const bool valid = row < n_rows;
    const int b = valid ? ptr[row] : 0, e = valid ? ptr[row + 1] : 0;
    const bool is_long = e - b > SF_LONG_STEPS * G;
    double part = 0.0;
    if (!is_long)
        for (int j = b + sub; j < e; j += G) part += term(j);
    double acc = init + sf_group_sum<G>(part);
    unsigned long long todo = __ballot(is_long && sub == 0);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int bb = __shfl(b, src), ee = __shfl(e, src);
        const double init_src = __shfl(init, src);
        double p = 0.0;
        for (int j = bb + lane; j < ee; j += 64) p += term(j);
        p = sf_group_sum<64>(p);
        if ((lane & ~(G - 1)) == src) acc = init_src + p;
    }
    return acc;
}

// per-shell factors: norm_e = 1 / (t_sim vol), norm_j = c t_exp / (4 pi t_sim vol) -- the expression of radfield_shell_kernel
__global__ void sf_shell_kernel(const double *__restrict__ volume, int S, double t_sim, double jblue_norm_num, double four_pi_tsim,
                                double *__restrict__ norm_e, double *__restrict__ norm_j)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    norm_e[s] = 1 / (t_sim * volume[s]);
    norm_j[s] = jblue_norm_num / (four_pi_tsim * volume[s]);
}

// e_dot_u[s][k]: blockIdx.y = shell, G lanes per level (long levels: the wave)
template <int G>
__global__ void __launch_bounds__(256) sf_level_sums_kernel(const int *__restrict__ lvl_ptr, const int *__restrict__ lvl_line, int n_levels,
                                                            long long L, const double *__restrict__ exp_tau, const double *__restrict__ edot_t,
                                                            const double *__restrict__ norm_e, double *__restrict__ e_out)
{
    const int s = blockIdx.y;
    const long long k = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const double ne = norm_e[s];
    const double *__restrict__ et = exp_tau + (long long)s * L, *__restrict__ ed = edot_t + (long long)s * L;
    const double v = sf_row_sum<G>(lvl_ptr, k, n_levels, 0.0, [&](int j) {
        const int l = lvl_line[j];
        return ne * (1 - et[l]) * ed[l];
    });
    if (k < n_levels && (threadIdx.x & (G - 1)) == 0) e_out[(long long)s * n_levels + k] = v;
}

// q[s][j] = prob_t[s][in_row[j]]
__global__ void __launch_bounds__(256) sf_gather_q_kernel(const int *__restrict__ in_row, long long nnz, const double *__restrict__ prob_t,
                                                          long long T, double *__restrict__ q)
{
    const int s = blockIdx.y;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nnz; j += (long long)gridDim.x * blockDim.x)
        q[(long long)s * nnz + j] = prob_t[(long long)s * T + in_row[j]];
}

// one iteration x_new = e + Q^T x for all shells
template <int G>
__global__ void __launch_bounds__(256) sf_iterate_kernel(const int *__restrict__ in_ptr, const int *__restrict__ in_src, int n_levels, long long nnz,
                                                         const double *__restrict__ q, const double *__restrict__ e, const double *__restrict__ x,
                                                         double *__restrict__ x_new)
{
    const int s = blockIdx.y;
    const long long k = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const double *__restrict__ qs = q + (long long)s * nnz, *__restrict__ xs = x + (long long)s * n_levels;
    const double init = k < n_levels ? e[(long long)s * n_levels + k] : 0.0;
    const double v = sf_row_sum<G>(in_ptr, k, n_levels, init, [&](int j) { return qs[j] * xs[in_src[j]]; });
    if (k < n_levels && (threadIdx.x & (G - 1)) == 0) x_new[(long long)s * n_levels + k] = v;
}

// conv[2 s] = max |x_new - x|, conv[2 s + 1] = max |x_new| over the levels of shell s (NaN if any entry is); a block per shell
__global__ void __launch_bounds__(256) sf_convergence_kernel(const double *__restrict__ x, const double *__restrict__ x_new, int n_levels,
                                                             double *__restrict__ conv)
{
    __shared__ double sh[2][4];
    __shared__ int sh_bad[4];
    const int s = blockIdx.x;
    const double *__restrict__ a = x + (long long)s * n_levels, *__restrict__ b = x_new + (long long)s * n_levels;
    double md = 0.0, mx = 0.0;
    int bad = 0;
    for (int k = threadIdx.x; k < n_levels; k += blockDim.x) {
        const double v = b[k], d = fabs(v - a[k]);
        bad |= !(d == d);
        md = fmax(md, d);
        mx = fmax(mx, fabs(v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        md = fmax(md, __shfl_xor(md, o));
        mx = fmax(mx, __shfl_xor(mx, o));
        bad |= __shfl_xor(bad, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[0][w] = md; sh[1][w] = mx; sh_bad[w] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) { md = fmax(md, sh[0][i]); mx = fmax(mx, sh[1][i]); bad |= sh_bad[i]; }
        conv[2 * s] = bad ? __builtin_nan("") : md;
        conv[2 * s + 1] = mx;
    }
}

// steps 4-6: blockIdx.y = shell, grid-stride over the lines
__global__ void __launch_bounds__(256) sf_close_kernel(const int *__restrict__ emit_row, const int *__restrict__ emit_level, long long L, long long T,
                                                       int n_levels, const double *__restrict__ prob_t, const double *__restrict__ c_level,
                                                       const double *__restrict__ wavelength /* or null */, const double *__restrict__ nu_line,
                                                       const double *__restrict__ exp_tau, const double *__restrict__ jblue_t,
                                                       const double *__restrict__ norm_j, double t_sim, double four_pi,
                                                       double *__restrict__ att, double *__restrict__ jred, double *__restrict__ jblue)
{
    const int s = blockIdx.y;
    const double nj = norm_j[s];
    const double *__restrict__ ps = prob_t + (long long)s * T, *__restrict__ cs = c_level + (long long)s * n_levels;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < L; l += (long long)gridDim.x * blockDim.x) {
        const long long i = (long long)s * L + l;
        const double wave = wavelength ? wavelength[l] : C_LIGHT / nu_line[l];
        const double a = wave * (ps[emit_row[l]] * cs[emit_level[l]]) * t_sim / four_pi;
        const double jb = jblue_t[i] * nj;
        att[i] = a;
        jblue[i] = jb;
        jred[i] = jb * exp_tau[i] + a;
    }
}

}  // namespace mc
