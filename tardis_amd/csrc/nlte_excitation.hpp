// nlte_excitation.hpp -- NLTE excitation of selected species inside tardis_mc_update_plasma: the level Boltzmann factors of an NLTE species
// from the statistical equilibrium of its radiative and collisional bound-bound rates, solved per (species, shell) on the device.
//
// Restates LevelBoltzmannFactorNLTE._calculate_general / _main_nlte_calculation of the legacy plasma, collision matrix included (fp64,
// -ffp-contract=off keeps every product, quotient and difference a rounding of its own; the contract is spelled out in include/tardis_mc.h):
// per line of the species r_ul = (A_ul + B_ul j) beta and r_lu = (B_lu j) beta, a rate matrix with the destination as the row, the
// diagonal minus the serial column sum, the first row replaced by ones, b = e_0; M x = b by unblocked LU with partial pivoting and a
// column-oriented back substitution; lbf[k] = (x[k] g_0) / x[0].
//
// Two stages.  nlte_rates_kernel streams the NLTE lines of a shell (grid.y = shell) and writes r_ul / r_lu [S][NL]; its j comes from the
// device functions the line kernel and radfield_jblue_kernel evaluate (opacity_update.hpp), so it is the j the same update stores, bit for
// bit.  nlte_solve_kernel is one 256-thread workgroup per (species, shell): it zeroes the matrix, scatters the rates (one writer per
// entry: tardis_mc_set_nlte_data refuses a repeated pair), sums every column serially for the diagonal, eliminates and substitutes, and
// writes lbf_t, x and a status word.  The matrix is column-major with an odd leading dimension (nlte_plan.hpp): the rank-1 update and
// every column walk touch consecutive addresses, the row swap strides over 32 different bank pairs.  Its two forms differ only in
// where the working set lives -- the workgroup's dynamic LDS, or a slab of HBM per (species, shell) -- and run the same operations in
// the same order: same bits.  A species in HBM has a third form, the blocked one at the end of this file: the same roundings in the same
// order again, with the trailing update of a panel spread over the chip.
//
// An elimination step: every wave finds the pivot of column k for itself (a lane per 64 rows, then a butterfly over the wave that
// prefers the larger |value| and, among equals, the lower row: no arrival order enters); nothing the next phase writes lies in
// column k, so no barrier is needed before the row swap (a thread per column right of k) and the multipliers l_i (a thread per row,
// taken from the unswapped column with the swap applied on the fly; the pivot itself goes into a vector of its own); barrier; the
// rank-1 update (a wave per column, a lane per row) and b; barrier.  Two barriers per step, one per back-substitution step.  Every entry
// sees its updates in the order of k whatever the decomposition.  No workgroup waits on another, no atomics: two calls give identical bits.
//
// Collisional rates (atomic data with collision_data; tardis_mc_set_nlte_collision_data).  nlte_collision_kernel streams the pairs of a
// shell (grid.y = shell): t_e = link t_rad[s] and its bracket in the temperature grid are properties of the shell, so the first wave
// counts the knots below t_e with one ballot per 64 knots and hands hi to the workgroup through four bytes of LDS; C_ul is stored
// [NT][NP], so the two rows a shell reads are consecutive across lanes.  It writes c_ul / c_lu [S][NP], before the product with n_e.
// The solve kernel then has one more phase between the scatter of the line rates and the column sums: the species' pairs add
// c n_e[s] into M[l][u] and M[u][l] (one writer per entry: the set call refuses a repeated pair), behind a barrier of its own.  A
// species without pairs, and every species when no collision data are installed, skips the phase and its barrier on one
// workgroup-uniform branch.  Pairs sorted by (lower, upper) walk a row of M with consecutive upper levels: the odd leading dimension
// spreads them over 32 bank pairs, and the transposed entry is a walk down a column.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include "mc_device.hpp"
#include "mc_math.hpp"
#include "opacity_update.hpp"

namespace mc {

constexpr int NLTE_J_DILUTE = 0, NLTE_J_DETAILED = 1, NLTE_J_CORONAL = 2;

struct NlteRateArgs {
    int S;
    long long L, NL;
    const int *line_id;                      // [NL] into the line list
    const double *a_ul, *b_ul, *b_lu;        // [NL]
    const double *nu_line;                   // [L]
    const double *beta_t;                    // [S][L] of the previous update, or nullptr: 1.0
    const double *t_rad, *w;                 // [S] the field j is evaluated with (dilute: the call's; detailed: the estimators')
    const double *norm, *jblue_t;            // detailed: [S], [S][L]
    double planck_coef, h, k_b, w_epsilon, c_ang;
    int optical_window;
    double *r_ul_t, *r_lu_t;                 // [S][NL] out
};

template <int JMODE>
__global__ void __launch_bounds__(256) nlte_rates_kernel(NlteRateArgs a)
{
    const long long s = blockIdx.y;
    double beta_rad = 0.0, ws = 0.0, ns = 0.0;
    if (JMODE != NLTE_J_CORONAL) { beta_rad = 1 / (a.k_b * a.t_rad[s]); ws = a.w[s]; }
    if (JMODE == NLTE_J_DETAILED) ns = a.norm[s];
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < a.NL; q += (long long)gridDim.x * blockDim.x) {
        const long long l = a.line_id[q];
        double j = 0.0;
        if (JMODE == NLTE_J_DILUTE) j = dilute_black_body_j(ws, a.planck_coef, a.h, a.nu_line[l], beta_rad);
        if (JMODE == NLTE_J_DETAILED)
            j = detailed_j_blue(a.jblue_t[s * a.L + l], ns, a.nu_line[l], ws, beta_rad, a.planck_coef, a.h, a.w_epsilon, a.c_ang, a.optical_window);
        const double beta = a.beta_t ? a.beta_t[s * a.L + l] : 1.0;
        a.r_ul_t[s * a.NL + q] = (a.a_ul[q] + a.b_ul[q] * j) * beta;
        a.r_lu_t[s * a.NL + q] = (a.b_lu[q] * j) * beta;
    }
}

struct NlteCollisionArgs {
    int S, NT;
    long long NP;
    const double *temperatures;              // [NT] ascending
    const double *c_t;                       // [NT][NP] C_ul
    const double *delta_e, *inv_g_ratio;     // [NP]
    const double *t_rad;                     // [S] the call's
    double link;                             // link_t_rad_t_electron
    double *c_ul_t, *c_lu_t;                 // [S][NP] out
};

__global__ void __launch_bounds__(256) nlte_collision_kernel(NlteCollisionArgs a)
{
    __shared__ int hi_shared;
    const long long s = blockIdx.y;
    const double t_e = a.link * a.t_rad[s];
    // hi = clip(searchsorted(temperatures, t_e, side="left"), 1, NT - 1): the knots below t_e, counted by the first wave
    if (threadIdx.x < 64) {
        int below = 0;
        for (int base = 0; base < a.NT; base += 64) {
            const int i = base + (int)threadIdx.x;
            below += __popcll(__ballot(i < a.NT && a.temperatures[i] < t_e));
        }
        if (threadIdx.x == 0) hi_shared = below < 1 ? 1 : (below > a.NT - 1 ? a.NT - 1 : below);
    }
    __syncthreads();
    const int hi = hi_shared, lo = hi - 1;
    const double x_lo = a.temperatures[lo], dx = a.temperatures[hi] - x_lo, dt = t_e - x_lo;
    const double *y_lo = a.c_t + (long long)lo * a.NP, *y_hi = a.c_t + (long long)hi * a.NP;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < a.NP; q += (long long)gridDim.x * blockDim.x) {
        const double slope = (y_hi[q] - y_lo[q]) / dx;
        double c_ul = slope * dt + y_lo[q];
        if (c_ul != c_ul) c_ul = 0.0;  // (the reference zeroes NaN after interpolating)
        a.c_ul_t[s * a.NP + q] = c_ul;
        a.c_lu_t[s * a.NP + q] = (c_ul * mcm::exp(-a.delta_e[q] / t_e)) * a.inv_g_ratio[q];
    }
}

struct NlteSolveArgs {
    int S;
    long long K, NL, NX;
    const int *list;                         // the species of this launch
    const int *sp_k0, *sp_n, *sp_x0, *sp_line_edge;  // per species: first level, levels, first row of x, [NS+1] lines
    const int *lower, *upper;                // [NL] local levels
    const double *r_ul_t, *r_lu_t;           // [S][NL]
    const double *g;                         // [K] level_g
    double *lbf_t;                           // [S][K]: the species' levels are overwritten
    double *x_t;                             // [S][NX] out
    int *status;                             // [NS][S] out: 0, or 1 + the step of a bad pivot, n + 1 (x[0] == 0), n + 2 (x not finite)
    double *scratch;                         // global form: the slabs
    const long long *slab;                   // global form, per list entry: the offset (doubles) of shell 0's slab; shells follow each other
    // collisional rates; sp_pair_edge == nullptr: none installed
    long long NP;
    const int *sp_pair_edge;                 // [NS+1] pairs per species
    const int *pair_lower, *pair_upper;      // [NP] local levels, lower < upper
    const double *c_ul_t, *c_lu_t;           // [S][NP]
    const double *n_e;                       // [S] the resident electron density at entry to the call
};

__device__ __forceinline__ bool nlte_finite(double v) { return fabs(v) <= DBL_MAX; }

// is candidate (v, i) a better pivot than (best, bi)?  The larger |value|; NaN above everything (numpy.argmax); among equals the lower row
__device__ __forceinline__ bool nlte_better(double v, int i, double best, int bi)
{
    const bool vn = v != v, bn = best != best;
    if (vn != bn) return vn;
    if (!vn && v != best) return v > best;
    return i < bi;
}

template <bool LDS>
__global__ void __launch_bounds__(256) nlte_solve_kernel(NlteSolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double nlte_lds[];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = blockIdx.y;
    const int sp = a.list[e], n = a.sp_n[sp], ld = n | 1;
    const long long work = (long long)ld * n + 4LL * n;
    double *M = LDS ? nlte_lds : a.scratch + a.slab[e] + s * work;
    double *b = M + (long long)ld * n, *lv = b + n, *piv = lv + n, *x = piv + n;
    // assemble: zero, scatter, the diagonal from the serial column sums, the row of ones
    for (long long i = tid; i < (long long)ld * n; i += 256) M[i] = 0.0;
    for (int i = tid; i < n; i += 256) b[i] = i == 0 ? 1.0 : 0.0;
    __syncthreads();
    {
        const double *r_ul = a.r_ul_t + s * a.NL, *r_lu = a.r_lu_t + s * a.NL;
        for (int q = a.sp_line_edge[sp] + tid; q < a.sp_line_edge[sp + 1]; q += 256) {
            const int l = a.lower[q], u = a.upper[q];
            M[l + (long long)u * ld] = r_ul[q];
            M[u + (long long)l * ld] = r_lu[q];
        }
    }
    __syncthreads();
    {   // the collisional rates of the species' pairs on top: workgroup-uniform, so the barrier is met by all threads or by none
        const int p0 = a.sp_pair_edge ? a.sp_pair_edge[sp] : 0, p1 = a.sp_pair_edge ? a.sp_pair_edge[sp + 1] : 0;
        if (p0 < p1) {
            const double *c_ul = a.c_ul_t + s * a.NP, *c_lu = a.c_lu_t + s * a.NP;
            const double ne = a.n_e[s];
            for (int q = p0 + tid; q < p1; q += 256) {
                const int l = a.pair_lower[q], u = a.pair_upper[q];
                double *ul = M + l + (long long)u * ld, *lu = M + u + (long long)l * ld;
                *ul = *ul + c_ul[q] * ne;
                *lu = *lu + c_lu[q] * ne;
            }
            __syncthreads();
        }
    }
    for (int c = tid; c < n; c += 256) {
        double *col = M + (long long)c * ld;
        double sum = 0.0;
        for (int r = 0; r < n; ++r)
            if (r != c) sum += col[r];
        col[c] = -sum;
        col[0] = 1.0;
    }
    __syncthreads();
    int code = 0;
    for (int k = 0; k < n; ++k) {
        const double *colk = M + (long long)k * ld;
        // the pivot: every wave for itself
        double best = -1.0;
        int p = INT_MAX;
        for (int i = k + lane; i < n; i += 64) {
            const double v = fabs(colk[i]);
            if (nlte_better(v, i, best, p)) { best = v; p = i; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(p, off, 64);
            if (nlte_better(ov, oi, best, p)) { best = ov; p = oi; }
        }
        const double pv = colk[p], kk = colk[k];
        if (pv == 0.0 || !nlte_finite(pv)) { code = k + 1; break; }  // (the same in every thread)
        // the swap of rows k and p right of column k, the multipliers, the pivot
        if (p != k)
            for (int j = k + 1 + tid; j < n; j += 256) {
                double *col = M + (long long)j * ld;
                const double t = col[k];
                col[k] = col[p];
                col[p] = t;
            }
        for (int i = k + 1 + tid; i < n; i += 256) lv[i] = (i == p ? kk : colk[i]) / pv;
        if (tid == 0) {
            piv[k] = pv;
            const double t = b[k];
            b[k] = b[p];
            b[p] = t;
        }
        __syncthreads();
        for (int j = k + 1 + wave; j < n; j += 4) {
            double *col = M + (long long)j * ld;
            const double mkj = col[k];
            for (int i = k + 1 + lane; i < n; i += 64) col[i] = col[i] - lv[i] * mkj;
        }
        {
            const double bk = b[k];
            for (int i = k + 1 + tid; i < n; i += 256) b[i] = b[i] - lv[i] * bk;
        }
        __syncthreads();
    }
    if (code == 0) {
        for (int j = n - 1; j >= 0; --j) {
            const double xj = b[j] / piv[j];
            if (tid == 0) x[j] = xj;
            const double *col = M + (long long)j * ld;
            for (int i = tid; i < j; i += 256) b[i] = b[i] - col[i] * xj;
            __syncthreads();
        }
        bool bad = false;  // (every thread reads all of x: no vote, no static LDS beside the dynamic working set)
        for (int i = 0; i < n; ++i) bad = bad || !nlte_finite(x[i]);
        if (bad) code = n + 2;
        else if (x[0] == 0.0) code = n + 1;
    }
    if (code == 0) {
        const int k0 = a.sp_k0[sp], x0 = a.sp_x0[sp];
        const double g0 = a.g[k0], first = x[0];
        for (int i = tid; i < n; i += 256) {
            a.lbf_t[s * a.K + k0 + i] = (x[i] * g0) / first;
            a.x_t[s * a.NX + x0 + i] = x[i];
        }
    }
    if (tid == 0) a.status[(long long)sp * a.S + s] = code;
}

// ---- the blocked form: the elimination of a species in HBM spread over the chip ---------------------------------------------------------
// A right-looking blocked LU with the roundings of the unblocked one.  nlte_assemble_kernel builds the system in the slab and clears the
// status word; per panel of NLTE_NB columns nlte_panel_kernel (one workgroup per system) eliminates inside the panel, serially in k, and
// nlte_trailing_kernel (a workgroup per strip of NLTE_TN whole columns right of the panel, b being column n of the slab) applies the
// panel's row swaps to its columns, forms its part of the row block U by the recurrence u_k = a_k - l_k0 u_0 - ... in ascending order,
// and updates the rows below term by term, acc = acc - l_ik u_kj for k in panel order: every entry sees the products it sees in the
// unblocked kernel, rounded one by one, in the same order.  nlte_backsolve_kernel is the tail of nlte_solve_kernel.  The multipliers
// stay in place below the diagonal, swapped with their rows inside the panel (a panel's multipliers are not read again once its
// trailing launch is done, so earlier panels are left alone); the pivots are also in their vector, the pivot rows in pivrow [S][NX].
// Ordering is stream order; a system whose status word is set is skipped by every later launch before its first barrier.
constexpr int NLTE_NB = 32, NLTE_TN = 32, NLTE_TM = 128;

struct NlteSystem {
    int sp, n, ld;
    double *M, *b, *lv, *piv, *x;
    int *status;
};
__device__ __forceinline__ NlteSystem nlte_system(const NlteSolveArgs &a, int e, long long s)
{
    NlteSystem y;
    y.sp = a.list[e]; y.n = a.sp_n[y.sp]; y.ld = y.n | 1;
    y.M = a.scratch + a.slab[e] + s * ((long long)y.ld * y.n + 4LL * y.n);
    y.b = y.M + (long long)y.ld * y.n; y.lv = y.b + y.n; y.piv = y.lv + y.n; y.x = y.piv + y.n;
    y.status = a.status + (long long)y.sp * a.S + s;
    return y;
}

// the assembly of nlte_solve_kernel into the slab, in its order; grid (species of the launch, shells)
__global__ void __launch_bounds__(256) nlte_assemble_kernel(NlteSolveArgs a)
{
    const int tid = threadIdx.x;
    const long long s = blockIdx.y;
    const NlteSystem y = nlte_system(a, blockIdx.x, s);
    const int sp = y.sp, n = y.n, ld = y.ld;
    double *M = y.M, *b = y.b;
    for (long long i = tid; i < (long long)ld * n; i += 256) M[i] = 0.0;
    for (int i = tid; i < n; i += 256) b[i] = i == 0 ? 1.0 : 0.0;
    __syncthreads();
    {
        const double *r_ul = a.r_ul_t + s * a.NL, *r_lu = a.r_lu_t + s * a.NL;
        for (int q = a.sp_line_edge[sp] + tid; q < a.sp_line_edge[sp + 1]; q += 256) {
            const int l = a.lower[q], u = a.upper[q];
            M[l + (long long)u * ld] = r_ul[q];
            M[u + (long long)l * ld] = r_lu[q];
        }
    }
    __syncthreads();
    {
        const int p0 = a.sp_pair_edge ? a.sp_pair_edge[sp] : 0, p1 = a.sp_pair_edge ? a.sp_pair_edge[sp + 1] : 0;
        if (p0 < p1) {
            const double *c_ul = a.c_ul_t + s * a.NP, *c_lu = a.c_lu_t + s * a.NP;
            const double ne = a.n_e[s];
            for (int q = p0 + tid; q < p1; q += 256) {
                const int l = a.pair_lower[q], u = a.pair_upper[q];
                double *ul = M + l + (long long)u * ld, *lu = M + u + (long long)l * ld;
                *ul = *ul + c_ul[q] * ne;
                *lu = *lu + c_lu[q] * ne;
            }
            __syncthreads();
        }
    }
    for (int c = tid; c < n; c += 256) {
        double *col = M + (long long)c * ld;
        double sum = 0.0;
        for (int r = 0; r < n; ++r)
            if (r != c) sum += col[r];
        col[c] = -sum;
        col[0] = 1.0;
    }
    if (tid == 0) *y.status = 0;
}

// the panel of columns [c0, c0 + NLTE_NB): grid (species of the launch, shells).  The panel is worked on where it lies (L2): a panel
// of 1071 rows is 274 KB, more than a workgroup's LDS.  A step is that of nlte_solve_kernel restricted to the panel's columns -- the
// pivot search, the swap (here also of the multipliers in the panel's earlier columns), the multipliers through lv, barrier, the rank-1
// update -- and in that second phase column k, which no thread reads any more, receives the pivot and the multipliers in place.
__global__ void __launch_bounds__(256) nlte_panel_kernel(NlteSolveArgs a, int *pivrow, int c0)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const long long s = blockIdx.y;
    const NlteSystem y = nlte_system(a, blockIdx.x, s);
    const int n = y.n, ld = y.ld;
    if (c0 >= n || *y.status != 0) return;  // (the same in every thread, before any barrier)
    double *M = y.M, *lv = y.lv;
    int *prow = pivrow + s * a.NX + a.sp_x0[y.sp];
    const int c1 = c0 + NLTE_NB < n ? c0 + NLTE_NB : n;
    for (int k = c0; k < c1; ++k) {
        double *colk = M + (long long)k * ld;
        double best = -1.0;
        int p = INT_MAX;
        for (int i = k + lane; i < n; i += 64) {
            const double v = fabs(colk[i]);
            if (nlte_better(v, i, best, p)) { best = v; p = i; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(p, off, 64);
            if (nlte_better(ov, oi, best, p)) { best = ov; p = oi; }
        }
        const double pv = colk[p], kk = colk[k];
        if (pv == 0.0 || !nlte_finite(pv)) {  // (the same in every thread)
            if (tid == 0) *y.status = k + 1;
            return;
        }
        if (p != k)
            for (int j = c0 + tid; j < c1; j += 256) {
                if (j == k) continue;
                double *col = M + (long long)j * ld;
                const double t = col[k];
                col[k] = col[p];
                col[p] = t;
            }
        for (int i = k + 1 + tid; i < n; i += 256) lv[i] = (i == p ? kk : colk[i]) / pv;
        if (tid == 0) { y.piv[k] = pv; prow[k] = p; }
        __syncthreads();
        const int rows = n - k - 1, cols = c1 - k - 1;
        for (int idx = tid; idx < rows * cols; idx += 256) {
            const int i = k + 1 + idx % rows;
            double *col = M + (long long)(k + 1 + idx / rows) * ld;
            col[i] = col[i] - lv[i] * col[k];
        }
        for (int i = k + 1 + tid; i < n; i += 256) colk[i] = lv[i];
        if (tid == 0) colk[k] = pv;
        __syncthreads();
    }
}

// the trailing update of the panel at c0: grid (strips, species of the launch, shells); strip x owns the columns
// [c1 + x NLTE_TN, + NLTE_TN) of the slab up to column n, which is b, over their whole height.  Phase A, in LDS: the rows the panel's
// swaps touch (the panel's own rows and the pivot rows below it, a slot each) are loaded for the strip's columns, a thread per column
// applies the swaps in panel order and runs the recurrence of U on 32 registers against the panel's unit triangle, and the slots go
// back.  Phase B: blocks of NLTE_TM rows; L of the block and U of the strip in LDS, 4 x 4 entries per thread in registers, k innermost.
__global__ void __launch_bounds__(256) nlte_trailing_kernel(NlteSolveArgs a, const int *pivrow, int c0)
{
    constexpr int NB = NLTE_NB, TN = NLTE_TN, TM = NLTE_TM, SLOTS = 2 * NB, VLD = SLOTS + 1;
    static_assert(NB * NB + TN * VLD <= NB * TM && TM == 128 && TN == 32 && NB == 32, "the tile shape the thread layout is written for");
    __shared__ __attribute__((aligned(16))) double sh[NB * TM];  // phase A: the unit triangle [kk][k], then the slots [column][slot]; phase B: L [k][row]
    __shared__ __attribute__((aligned(16))) double Us[NB * TN];  // U [k][column]
    __shared__ int slot_row[SLOTS], swap_slot[NB];
    const int tid = threadIdx.x;
    const long long s = blockIdx.z;
    const NlteSystem y = nlte_system(a, blockIdx.y, s);
    const int n = y.n, ld = y.ld;
    if (c0 >= n) return;
    const int c1 = c0 + NB < n ? c0 + NB : n, nb = c1 - c0;
    const long long first = (long long)c1 + (long long)blockIdx.x * TN;
    if (first > n || *y.status != 0) return;  // (the same in every thread, before any barrier)
    const int j0 = (int)first, nj = n + 1 - j0 < TN ? n + 1 - j0 : TN;
    double *M = y.M;
    const int *prow = pivrow + s * a.NX + a.sp_x0[y.sp];
    double *L11 = sh, *V = sh + NB * NB;
    // the slot of row c0 + k is k; a pivot row below the panel gets slot NB + (the first step that names it)
    if (tid < NB) {
        int slot = -1, p = -1;
        if (tid < nb) {
            p = prow[c0 + tid];
            if (p < c1) slot = p - c0;
            else {
                slot = NB + tid;
                for (int q = tid - 1; q >= 0; --q)
                    if (prow[c0 + q] == p) slot = NB + q;
            }
            swap_slot[tid] = slot;
        }
        slot_row[tid] = tid < nb ? c0 + tid : -1;
        slot_row[NB + tid] = slot == NB + tid ? p : -1;
    }
    for (int idx = tid; idx < NB * NB; idx += 256) {
        const int kk = idx / NB, k = idx % NB;
        L11[idx] = (k < nb && kk < k) ? M[(c0 + k) + (long long)(c0 + kk) * ld] : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < TN * SLOTS; idx += 256) {
        const int c = idx / SLOTS, sl = idx % SLOTS, row = slot_row[sl];
        V[c * VLD + sl] = (c < nj && row >= 0) ? M[row + (long long)(j0 + c) * ld] : 0.0;
    }
    __syncthreads();
    if (tid < TN) {
        double *v = V + tid * VLD;
        for (int k = 0; k < nb; ++k) {
            const int sl = swap_slot[k];
            if (sl != k) { const double t = v[k]; v[k] = v[sl]; v[sl] = t; }
        }
        double u[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) u[k] = v[k];  // (slots from nb on hold 0.0 and meet multipliers of 0.0: never stored)
#pragma unroll
        for (int kk = 0; kk < NB; ++kk) {
#pragma unroll
            for (int k = kk + 1; k < NB; ++k) u[k] = u[k] - L11[kk * NB + k] * u[kk];
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) { v[k] = u[k]; Us[k * TN + tid] = u[k]; }
    }
    __syncthreads();
    for (int idx = tid; idx < TN * SLOTS; idx += 256) {
        const int c = idx / SLOTS, sl = idx % SLOTS, row = slot_row[sl];
        if (c < nj && row >= 0) M[row + (long long)(j0 + c) * ld] = V[c * VLD + sl];
    }
    const int rg = tid & 31, cg = tid >> 5;
    for (int i0 = c1; i0 < n; i0 += TM) {
        __syncthreads();  // (the slots are written back and sh is free; from the second block on: the L of the block before is used up)
        for (int idx = tid; idx < NB * TM; idx += 256) {
            const int k = idx / TM, r = idx % TM;
            sh[idx] = (k < nb && i0 + r < n) ? M[(i0 + r) + (long long)(c0 + k) * ld] : 0.0;
        }
        __syncthreads();
        double acc[4][4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = i0 + rg + 32 * rr, c = 4 * cg + cc;
                acc[cc][rr] = (i < n && c < nj) ? M[i + (long long)(j0 + c) * ld] : 0.0;
            }
        for (int k = 0; k < nb; ++k) {
            double l[4], u[4];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) l[rr] = sh[k * TM + rg + 32 * rr];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) u[cc] = Us[k * TN + 4 * cg + cc];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) acc[cc][rr] = acc[cc][rr] - l[rr] * u[cc];
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = i0 + rg + 32 * rr, c = 4 * cg + cc;
                if (i < n && c < nj) M[i + (long long)(j0 + c) * ld] = acc[cc][rr];
            }
    }
}

// the tail of nlte_solve_kernel on a factored slab: grid (species of the launch, shells)
__global__ void __launch_bounds__(256) nlte_backsolve_kernel(NlteSolveArgs a)
{
    const int tid = threadIdx.x;
    const long long s = blockIdx.y;
    const NlteSystem y = nlte_system(a, blockIdx.x, s);
    const int sp = y.sp, n = y.n, ld = y.ld;
    if (*y.status != 0) return;  // (the same in every thread, before any barrier)
    double *M = y.M, *b = y.b, *piv = y.piv, *x = y.x;
    for (int j = n - 1; j >= 0; --j) {
        const double xj = b[j] / piv[j];
        if (tid == 0) x[j] = xj;
        const double *col = M + (long long)j * ld;
        for (int i = tid; i < j; i += 256) b[i] = b[i] - col[i] * xj;
        __syncthreads();
    }
    int code = 0;
    bool bad = false;
    for (int i = 0; i < n; ++i) bad = bad || !nlte_finite(x[i]);
    if (bad) code = n + 2;
    else if (x[0] == 0.0) code = n + 1;
    if (code == 0) {
        const int k0 = a.sp_k0[sp], x0 = a.sp_x0[sp];
        const double g0 = a.g[k0], first = x[0];
        for (int i = tid; i < n; i += 256) {
            a.lbf_t[s * a.K + k0 + i] = (x[i] * g0) / first;
            a.x_t[s * a.NX + x0 + i] = x[i];
        }
    }
    if (tid == 0) *y.status = code;
}

}  // namespace mc
