// formal_interpolate.hpp -- the formal integral's `interpolate_shells`: the resident source function on the integrator's grid.
//
// Follows FormalIntegralSolver / interpolate_integrator_quantities (tardis/spectrum/formal_integral/): the S resident shells are
// replaced by S' = interpolate_shells - 1 equal ones between r_inner[0] and r_outer[S - 1]; att_S_ul, Jred_lu, Jblue_lu and the level
// rates e_dot_u are interpolated linearly over the shell midpoints (scipy interp1d, fill_value="extrapolate") and clipped at zero,
// tau_sobolev and the electron density take the value of the nearest midpoint (ties to the lower shell).  Per output shell j the
// host computes, in double and with the reference's expressions (fi_interpolation_grid), the source shells lo[j], hi[j] = lo[j] + 1
// and near[j] and the two abscissa differences x[hi] - x[lo] and xn[j] - x[lo]; a value is then
//   slope = (y[hi] - y[lo]) / (x[hi] - x[lo]);  v = slope * (xn - x[lo]) + y[lo];  max(v, 0)
// one division, one product, one sum, each rounded on its own (-ffp-contract=off): bit for bit what scipy returns.
//
// fi_interpolate_kernel is a pure stream over the output [S'][L], shell-major like the tables it reads: per output row two source
// rows of three tables and one row of exp(-tau) in (the same tau gives the same exp: a row gather), four rows out.  blockIdx.y is the
// output row, consecutive lanes take consecutive pairs of lines.  A row starts at s * L * 8 bytes, so with an odd L every other row
// is only 8-byte aligned: the pairs are laid so that the four STORES of a row are 16-byte aligned (one single line in front where the
// output row is not), and every source row is read 16 bytes at a time where its pairs fall on 16-byte boundaries and 8 bytes at a
// time where they do not (lo and hi = lo + 1 differ in that when L is odd).  The test is uniform over a block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace mc {

// the integrator's grid and the interpolation maps of steps 1-5 (host)
struct FiInterpolationGrid {
    std::vector<double> r_inner, r_outer;  // [S'] the new shells
    std::vector<int> lo, hi, near;         // [S'] source shells of the linear and the nearest interpolation
    std::vector<double> dx, dxn;           // [S'] x[hi] - x[lo], xn - x[lo]
};

inline FiInterpolationGrid fi_interpolation_grid(const std::vector<double> &r_in, const std::vector<double> &r_out, int n_points)
{
    const int S = (int)r_in.size(), Si = n_points - 1;
    std::vector<double> x((size_t)S), mid((size_t)S - 1), r((size_t)n_points);
    for (int s = 0; s < S; ++s) x[(size_t)s] = (r_in[(size_t)s] + r_out[(size_t)s]) / 2.0;
    for (int s = 0; s + 1 < S; ++s) mid[(size_t)s] = (x[(size_t)s + 1] + x[(size_t)s]) / 2.0;
    // numpy.linspace(start, stop, n): i * step + start, the last point is stop itself
    const double start = r_in[0], stop = r_out[(size_t)S - 1], step = (stop - start) / (double)(n_points - 1);
    for (int i = 0; i < n_points; ++i) r[(size_t)i] = (double)i * step + start;
    r[(size_t)n_points - 1] = stop;
    FiInterpolationGrid g;
    g.r_inner.assign(r.begin(), r.end() - 1);
    g.r_outer.assign(r.begin() + 1, r.end());
    g.lo.resize((size_t)Si); g.hi.resize((size_t)Si); g.near.resize((size_t)Si); g.dx.resize((size_t)Si); g.dxn.resize((size_t)Si);
    for (int j = 0; j < Si; ++j) {
        const double xn = (g.r_inner[(size_t)j] + g.r_outer[(size_t)j]) / 2.0;
        // searchsorted(side="left"): the first node that is not below xn
        const int at = (int)(std::lower_bound(x.begin(), x.end(), xn) - x.begin());
        const int hi = std::min(std::max(at, 1), S - 1), lo = hi - 1;
        g.lo[(size_t)j] = lo; g.hi[(size_t)j] = hi;
        g.dx[(size_t)j] = x[(size_t)hi] - x[(size_t)lo];
        g.dxn[(size_t)j] = xn - x[(size_t)lo];
        g.near[(size_t)j] = (int)(std::lower_bound(mid.begin(), mid.end(), xn) - mid.begin());
    }
    return g;
}

__device__ __forceinline__ double fi_interpolate_value(double y_lo, double y_hi, double dx, double dxn)
{
    const double slope = (y_hi - y_lo) / dx;
    const double v = slope * dxn + y_lo;
    return v < 0.0 ? 0.0 : v;  // (a NaN stays one, as under numpy's clip)
}

typedef double fi_v2d __attribute__((ext_vector_type(2)));

// lines l, l + 1 of a source row: one 16-byte load where they lie on a 16-byte boundary
__device__ __forceinline__ fi_v2d fi_load_pair(const double *__restrict__ p, bool aligned)
{
    if (aligned) return *reinterpret_cast<const fi_v2d *>(p);
    fi_v2d v;
    v.x = p[0]; v.y = p[1];
    return v;
}

__device__ __forceinline__ fi_v2d fi_interpolate_pair(fi_v2d y_lo, fi_v2d y_hi, double dx, double dxn)
{
    fi_v2d v;
    v.x = fi_interpolate_value(y_lo.x, y_hi.x, dx, dxn);
    v.y = fi_interpolate_value(y_lo.y, y_hi.y, dx, dxn);
    return v;
}

struct FiInterpolateArgs {
    long long L;
    const int *lo, *hi, *near;                           // [S']
    const double *dx, *dxn;                              // [S']
    const double *att, *jred, *jblue, *exp_tau;          // [S][L]
    double *att_i, *jred_i, *jblue_i, *exp_tau_i;        // [S'][L]
};

// grid (x, S'): the blocks of a row stride over its work items -- item k is the pair of lines {2 k - head, 2 k - head + 1}, cut to the row
__global__ void __launch_bounds__(256) fi_interpolate_kernel(FiInterpolateArgs a)
{
    const long long L = a.L, j = blockIdx.y;
    const long long lo = a.lo[j], hi = a.hi[j], near = a.near[j];
    const double dx = a.dx[j], dxn = a.dxn[j];
    const long long o_out = j * L, o_lo = lo * L, o_hi = hi * L, o_near = near * L;
    // every table starts on a 16-byte boundary, so element i of one is 16-byte aligned iff i is even
    const long long head = o_out & 1;
    const bool lo_al = ((o_lo + head) & 1) == 0, hi_al = ((o_hi + head) & 1) == 0, near_al = ((o_near + head) & 1) == 0;
    const long long items = (L + head + 1) / 2;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < items; k += (long long)gridDim.x * blockDim.x) {
        const long long l = 2 * k - head;
        if (l >= 0 && l + 1 < L) {
            const fi_v2d att = fi_interpolate_pair(fi_load_pair(a.att + o_lo + l, lo_al), fi_load_pair(a.att + o_hi + l, hi_al), dx, dxn);
            const fi_v2d jred = fi_interpolate_pair(fi_load_pair(a.jred + o_lo + l, lo_al), fi_load_pair(a.jred + o_hi + l, hi_al), dx, dxn);
            const fi_v2d jblue = fi_interpolate_pair(fi_load_pair(a.jblue + o_lo + l, lo_al), fi_load_pair(a.jblue + o_hi + l, hi_al), dx, dxn);
            const fi_v2d et = fi_load_pair(a.exp_tau + o_near + l, near_al);
            *reinterpret_cast<fi_v2d *>(a.att_i + o_out + l) = att;
            *reinterpret_cast<fi_v2d *>(a.jred_i + o_out + l) = jred;
            *reinterpret_cast<fi_v2d *>(a.jblue_i + o_out + l) = jblue;
            *reinterpret_cast<fi_v2d *>(a.exp_tau_i + o_out + l) = et;
        } else {  // the single line in front of the first pair or behind the last one
            const long long l1 = l < 0 ? 0 : l;
            a.att_i[o_out + l1] = fi_interpolate_value(a.att[o_lo + l1], a.att[o_hi + l1], dx, dxn);
            a.jred_i[o_out + l1] = fi_interpolate_value(a.jred[o_lo + l1], a.jred[o_hi + l1], dx, dxn);
            a.jblue_i[o_out + l1] = fi_interpolate_value(a.jblue[o_lo + l1], a.jblue[o_hi + l1], dx, dxn);
            a.exp_tau_i[o_out + l1] = a.exp_tau[o_near + l1];
        }
    }
}

// the level rates: e[S][K] (shell-major, as the source function keeps them) -> e_i[S'][K]; one thread per (output shell, level)
__global__ void __launch_bounds__(256) fi_interpolate_levels_kernel(const int *__restrict__ lo, const int *__restrict__ hi, const double *__restrict__ dx,
                                                                    const double *__restrict__ dxn, long long K, const double *__restrict__ e,
                                                                    double *__restrict__ e_i)
{
    const long long j = blockIdx.y;
    const long long o_lo = (long long)lo[j] * K, o_hi = (long long)hi[j] * K;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (long long)gridDim.x * blockDim.x)
        e_i[j * K + k] = fi_interpolate_value(e[o_lo + k], e[o_hi + k], dx[j], dxn[j]);
}

}  // namespace mc
