// plasma_update.hpp -- ion and level populations of the next iteration, solved on the device from (t_rad, W).
//
// Restates the legacy plasma's default configuration (ionization nebular or lte, excitation dilute-lte or lte; NLTE excitation: nlte_excitation.hpp; the continuum stage: continuum_rates.hpp) in its
// operation order: LevelBoltzmannFactorDiluteLTE / LTE, PartitionFunction, GElectron, PhiSahaLTE, PhiSahaNebular with
// RadiationFieldCorrection and the interpolated zeta, IonNumberDensity.calculate and LevelNumberDensity (fp64, -ffp-contract=off keeps
// every product and sum a rounding of its own; the formulas are spelled out in include/tardis_mc.h).
//
// Layout: lbf_t[S][K] and n_t[S][K] shell-major, as the opacity update's line kernel gathers the populations; everything per ion -- the
// partition functions Z, the Saha factors phi, the ion populations N -- ion-major [I][S], the layout tardis_mc_get_plasma hands out and
// the one in which the lane-per-shell iteration reads consecutive addresses.
//
// Four kernels.  plasma_boltzmann_kernel and plasma_population_kernel stream the levels of a shell (a 256-thread workgroup per tile,
// grid.y = shell).  The partition kernel comes in two forms that add in the same order (plasma_update_plan.hpp chooses per ion): a lane
// per (ion, shell) for short ions and a 16-lane DPP row per (ion, shell) for long ones, the running sum carried through the row with
// serial_prefix (propagate_group.hpp) and from step to step -- the pattern of opacity_block_row_kernel.  plasma_ionization_kernel is ONE
// workgroup with a lane per shell: a shell's state is private, the only thing the shells share is the vote "every shell has converged",
// taken with a workgroup barrier (__syncthreads_and / _or).  Nothing waits on another workgroup's memory.  No atomics: two calls give
// identical bits.
//
// The options of tardis_mc_set_ionization_options, both compile-time forms of plasma_ionization_kernel: delta_treatment puts a number
// in the place of delta in the phi prologue; helium_treatment recomb-nlte adds helium_relative_kernel (hp[K_He][S], shell fastest), a form whose
// lanes run three serial sums per pass over their column of hp, and helium_population_kernel behind the population kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include "mc_device.hpp"
#include "mc_math.hpp"
#include "propagate_group.hpp"

namespace mc {

constexpr int PLASMA_OK = 0, PLASMA_NAN = 1, PLASMA_BOUND = 2;  // status[0] of plasma_ionization_kernel; status[1] the passes

// lbf = g exp(E (-beta_rad)), times W for a non-metastable level when DILUTE
template <bool DILUTE>
__global__ void __launch_bounds__(256) plasma_boltzmann_kernel(const double *__restrict__ energy, const double *__restrict__ g,
                                                               const int *__restrict__ metastable, const double *__restrict__ t_rad,
                                                               const double *__restrict__ w, long long K, double k_b, double *__restrict__ lbf_t)
{
    const long long s = blockIdx.y;
    const double beta_rad = 1 / (k_b * t_rad[s]);
    const double nb = -beta_rad, ws = w[s];
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (long long)gridDim.x * blockDim.x) {
        double v = g[k] * mcm::exp(energy[k] * nb);
        if (DILUTE && !metastable[k]) v = v * ws;
        lbf_t[s * K + k] = v;
    }
}

// Short ions: one lane per (ion, shell), consecutive lanes on consecutive ions of a shell.  Ions of long_levels levels or more are left
// to plasma_partition_row_kernel.
__global__ void __launch_bounds__(256) plasma_partition_lane_kernel(const int *__restrict__ ion_edge, int n_ions, long long K, int S, long long long_levels,
                                                                    const double *__restrict__ lbf_t, double *__restrict__ z)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)n_ions * S) return;
    const int i = (int)(e % n_ions);
    const long long s = e / n_ions;
    const int k0 = ion_edge[i], k1 = ion_edge[i + 1];
    if ((long long)(k1 - k0) >= long_levels) return;
    const double *v = lbf_t + s * K;
    double sum = 0.0;
    for (int k = k0; k < k1; ++k) sum += v[k];
    z[(long long)i * S + s] = sum;
}

// Long ions: a 16-lane DPP row per (listed ion, shell); lane q takes levels k0 + q, k0 + 16 + q, ...; levels past the ion's end add +0.0,
// which changes no sum.
__global__ void __launch_bounds__(256) plasma_partition_row_kernel(const int *__restrict__ long_ions, int n_long, const int *__restrict__ ion_edge, long long K,
                                                                   int S, const double *__restrict__ lbf_t, double *__restrict__ z)
{
    const long long e = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;  // (whole DPP rows leave here together)
    if (e >= (long long)n_long * S) return;
    const int q = threadIdx.x & 15;
    const int i = long_ions[e % n_long];
    const long long s = e / n_long;
    const int k0 = ion_edge[i], k1 = ion_edge[i + 1];
    const double *v = lbf_t + s * K;
    double carry = 0.0;
    for (int k = k0; k < k1; k += 16) {
        const double x = k + q < k1 ? v[k + q] : 0.0;
        const double acc = serial_prefix<16>(carry, x, q);
        carry = gbcast<16>(acc, 15);
    }
    if (q == 0) z[(long long)i * S + s] = carry;
}

struct PlasmaIonArgs {
    int S, I, E, NT;
    int nebular;          // ionization_mode 0
    long long max_iter;
    double link, chi_0, k_b, two_pi_me, hh;  // t_e = link t_rad; (2 pi) m_e and h h are rounded once, on the host
    const int *element_edge;    // [E+1]
    const double *charge;       // [I]
    const double *chi;          // [I]
    const double *zeta_t;       // [NT]
    const double *zeta;         // [I][NT]
    const double *density;      // [E][S]
    const double *t_rad, *w;    // [S]
    const double *z;            // [I][S]
    double *phi;                // [I][S] scratch (the row of an element's last ion is not used)
    double *n_ion;              // [I][S] out
    double *n_e;                // [S] out: the electron density the last pass used
    int *status;                // [2] out: PLASMA_*, passes
    // tardis_mc_set_ionization_options (zero without options)
    double delta_treatment;     // FIXED_DELTA: delta for every ion and shell
    int he_element, he_ion;     // the helium form: helium's element row and its first ion a
    int he_n1, he_n2;           // levels of He I; of He I and He II together (He III is local level he_n2)
    const double *hp;           // [K_He][S] helium_relative_kernel's relative populations
    double *he_v;               // [K_He][S] out: the helium level populations of the pass whose n_e is handed out
};

// numpy.nan_to_num
__device__ __forceinline__ double plasma_nan_to_num(double x)
{
    if (x != x) return 0.0;
    if (x > DBL_MAX) return DBL_MAX;
    if (x < -DBL_MAX) return -DBL_MAX;
    return x;
}

// RadiationFieldCorrection with departure_coefficient 1 / W (fa = t_e / (((1 / W) W) t_rad))
__device__ __forceinline__ double plasma_delta(double chi, double chi_0, double fa, double beta_rad, double beta_e)
{
    if (chi >= chi_0) return fa * mcm::exp(chi * (beta_rad - beta_e));
    return (1 - mcm::exp(chi * beta_rad - beta_rad * chi_0)) + fa * mcm::exp(chi * beta_rad - beta_e * chi_0);
}

// zeta's bracket in the table: hi = clip(searchsorted(zeta_t, t_rad, side="left"), 1, NT - 1)
__device__ __forceinline__ int plasma_zeta_bracket(const double *__restrict__ zeta_t, int NT, double t_rad)
{
    int hi = 0;
    while (hi < NT && zeta_t[hi] < t_rad) ++hi;
    return hi < 1 ? 1 : (hi > NT - 1 ? NT - 1 : hi);
}

struct HeliumArgs {
    int S, NT;
    long long K;
    int k0, n1, n2;             // helium's first level; levels of He I; of He I and He II together (K_He = n2 + 1)
    int ion;                    // a, the row of He I
    int fixed_delta;
    double delta_treatment;
    double link, chi_0, k_b, two_pi_me, hh;
    const double *g;            // [K]
    const double *chi;          // [I]
    const double *zeta_t;       // [NT]
    const double *zeta;         // [I][NT]
    const double *t_rad, *w;    // [S]
    const double *lbf_t;        // [S][K]
    double *hp;                 // [K_He][S] out
};

// The populations of helium's levels relative to the He II ground level, before the electron density enters (HeliumNLTE): a thread
// per (helium level, shell), the shell fastest, so that the lanes of the ionisation kernel (lane = shell) read consecutive addresses.
__global__ void __launch_bounds__(256) helium_relative_kernel(HeliumArgs a)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)(a.n2 + 1) * a.S) return;
    const int s = (int)(e % a.S), k = (int)(e / a.S);
    const double t_rad = a.t_rad[s], w = a.w[s];
    const double beta_rad = 1 / (a.k_b * t_rad);
    const double x = (a.two_pi_me / beta_rad) / a.hh;
    const double g_e = x * sqrt(x);
    const double g1 = a.g[a.k0 + a.n1];
    const double lbf = a.lbf_t[(long long)s * a.K + a.k0 + k];
    double hp;
    if (k == 0) hp = 0.0;
    else if (k < a.n1) hp = (((lbf * (1 / (2 * g1))) * (1 / g_e)) * (1 / (w * w))) * mcm::exp(a.chi[a.ion] * beta_rad);
    else if (k == a.n1) hp = 1.0;
    else if (k < a.n2) hp = lbf * (1 / g1);
    else {
        const int i = a.ion + 1;
        const double g2 = a.g[a.k0 + a.n2], chi = a.chi[i];
        const double t_e = a.link * t_rad;
        const double beta_e = 1 / (a.k_b * t_e);
        const int hi = plasma_zeta_bracket(a.zeta_t, a.NT, t_rad), lo = hi - 1;
        const double x_lo = a.zeta_t[lo], dx = a.zeta_t[hi] - x_lo, dt = t_rad - x_lo;
        const double y_lo = a.zeta[(long long)i * a.NT + lo], y_hi = a.zeta[(long long)i * a.NT + hi];
        const double slope = (y_hi - y_lo) / dx;
        const double zeta = slope * dt + y_lo;
        const double fa = t_e / (((1 / w) * w) * t_rad);
        const double delta = a.fixed_delta ? a.delta_treatment : plasma_delta(chi, a.chi_0, fa, beta_rad, beta_e);  // (no exp for a fixed delta)
        hp = (((((2 * (g2 / g1)) * g_e) * mcm::exp(chi * (-beta_rad))) * w) * ((delta * zeta) + w * (1 - zeta))) * sqrt(t_e / t_rad);
    }
    a.hp[e] = hp;
}

// sum + the serial sum of a lane's u (or v) over helium's local levels k0 .. k1-1 of column s: u = hp n_e with NE (the levels of He I),
// hp without; times f with F.  The loads do not depend on the running sum: a batch of eight is issued ahead of its eight dependent
// adds, so a lane's chain is one add per level, not one round trip per level.
template <bool NE, bool F>
__device__ __forceinline__ double helium_serial_sum(const double *__restrict__ hp_s, int S, int k0, int k1, double n_e, double f, double sum)
{
    int k = k0;
    for (; k + 8 <= k1; k += 8) {
        double x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = hp_s[(long long)(k + j) * S];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            double u = NE ? x[j] * n_e : x[j];
            if (F) u = u * f;
            sum += u;
        }
    }
    for (; k < k1; ++k) {
        double u = NE ? hp_s[(long long)k * S] * n_e : hp_s[(long long)k * S];
        if (F) u = u * f;
        sum += u;
    }
    return sum;
}

// The Saha factors phi and IonNumberDensity.calculate.  One workgroup, lane s = shell s; lanes past S only take part in the votes.
// HELIUM (helium_treatment recomb-nlte): every pass forms the three helium ion rows from hp and the pass's n_e and puts them in the
// place of the Saha chain's, uncut.  FIXED_DELTA (delta_treatment): delta is the option's number, no exp is evaluated for it.
// <false, false> is the kernel of before: it reads none of the options' arguments.
template <bool HELIUM, bool FIXED_DELTA>
__global__ void __launch_bounds__(1024) plasma_ionization_kernel(PlasmaIonArgs a)
{
    const int s = threadIdx.x, S = a.S;
    const bool on = s < S;
    double n_e = 0.0;
    if (on) {
        const double t_rad = a.t_rad[s], w = a.w[s];
        const double beta_rad = 1 / (a.k_b * t_rad);
        const double t_e = a.link * t_rad;
        const double beta_e = 1 / (a.k_b * t_e);
        const double x = (a.two_pi_me / beta_rad) / a.hh;
        const double g_e2 = 2 * (x * sqrt(x));
        const double nb = -beta_rad;
        const int hi = plasma_zeta_bracket(a.zeta_t, a.NT, t_rad), lo = hi - 1;
        const double x_lo = a.zeta_t[lo], dx = a.zeta_t[hi] - x_lo, dt = t_rad - x_lo;
        const double fa = t_e / (((1 / w) * w) * t_rad);
        const double root = sqrt(t_e / t_rad);
        for (int e = 0; e < a.E; ++e) {
            const int i0 = a.element_edge[e], i1 = a.element_edge[e + 1];
            for (int i = i0; i + 1 < i1; ++i) {
                const double chi = a.chi[i];
                double phi = (a.z[(long long)(i + 1) * S + s] / a.z[(long long)i * S + s]) * (g_e2 * mcm::exp(chi * nb));
                if (a.nebular) {
                    const double y_lo = a.zeta[(long long)i * a.NT + lo], y_hi = a.zeta[(long long)i * a.NT + hi];
                    const double slope = (y_hi - y_lo) / dx;
                    const double zeta = slope * dt + y_lo;
                    const double delta = FIXED_DELTA ? a.delta_treatment : plasma_delta(chi, a.chi_0, fa, beta_rad, beta_e);
                    phi = ((phi * w) * ((zeta * delta) + w * (1 - zeta))) * root;
                }
                a.phi[(long long)i * S + s] = phi;
            }
        }
        for (int e = 0; e < a.E; ++e) n_e += a.density[(long long)e * S + s];
    }
    int status = PLASMA_BOUND, passes = 0;
    const double *hp_s = HELIUM ? a.hp + s : nullptr;  // (column s of hp[K_He][S])
    double he_f = 0.0;
    while (passes < a.max_iter) {
        double next = 0.0;
        if (on) {
            double he_0 = 0.0, he_1 = 0.0, he_2 = 0.0;
            if (HELIUM) {
                // nothing here depends on the other elements' populations of this pass, only on n_e: formed first, put in place below
                double total = helium_serial_sum<true, false>(hp_s, S, 0, a.he_n1, n_e, 0.0, 0.0);
                total = helium_serial_sum<false, false>(hp_s, S, a.he_n1, a.he_n2 + 1, n_e, 0.0, total);
                he_f = a.density[(long long)a.he_element * S + s] / total;
                he_0 = helium_serial_sum<true, true>(hp_s, S, 0, a.he_n1, n_e, he_f, 0.0);
                he_1 = helium_serial_sum<false, true>(hp_s, S, a.he_n1, a.he_n2, n_e, he_f, 0.0);
                he_2 = hp_s[(long long)a.he_n2 * S] * he_f;
            }
            for (int e = 0; e < a.E; ++e) {
                const int i0 = a.element_edge[e], i1 = a.element_edge[e + 1];
                if (HELIUM && e == a.he_element) {  // the Saha chain's three rows would be overwritten unread; no 1e-20 cut on these
                    a.n_ion[(long long)i0 * S + s] = he_0;
                    a.n_ion[(long long)(i0 + 1) * S + s] = he_1;
                    a.n_ion[(long long)(i0 + 2) * S + s] = he_2;
                    next += he_0 * a.charge[i0];
                    next += he_1 * a.charge[i0 + 1];
                    next += he_2 * a.charge[i0 + 2];
                    continue;
                }
                // the running products land in the rows they scale below: the same lane writes and reads them
                double cp = 1.0, sum = 0.0;
                for (int i = i0; i + 1 < i1; ++i) {
                    const double pe = plasma_nan_to_num(a.phi[(long long)i * S + s] / n_e);
                    cp = i == i0 ? pe : cp * pe;
                    sum += cp;
                    a.n_ion[(long long)(i + 1) * S + s] = cp;
                }
                double n0 = a.density[(long long)e * S + s] / (1 + sum);
                for (int i = i0; i < i1; ++i) {
                    double n = i == i0 ? n0 : n0 * a.n_ion[(long long)i * S + s];
                    if (n < 1e-20) n = 0.0;
                    a.n_ion[(long long)i * S + s] = n;
                    next += n * a.charge[i];
                }
            }
        }
        if (__syncthreads_or(on && next != next)) { status = PLASMA_NAN; break; }
        ++passes;
        const bool done = !on || fabs(next - n_e) / n_e < 0.05;
        if (__syncthreads_and(done)) { status = PLASMA_OK; break; }
        if (on) n_e = 0.5 * (next + n_e);
    }
    if (on) a.n_e[s] = n_e;
    if (HELIUM && on) {  // v of the last pass: n_e is the one it used, he_f its factor -- the same products, the same bits
        for (int k = 0; k <= a.he_n2; ++k) {
            const double h = hp_s[(long long)k * S];
            a.he_v[(long long)k * S + s] = (k < a.he_n1 ? h * n_e : h) * he_f;
        }
    }
    if (s == 0) { a.status[0] = status; a.status[1] = passes; }
}

// n = (lbf / Z[ion]) N[ion], written where the opacity update's line kernel reads the populations
__global__ void __launch_bounds__(256) plasma_population_kernel(const double *__restrict__ lbf_t, const int *__restrict__ level_ion,
                                                                const double *__restrict__ z, const double *__restrict__ n_ion, long long K, int S,
                                                                double *__restrict__ n_t)
{
    const long long s = blockIdx.y;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (long long)gridDim.x * blockDim.x) {
        const long long i = (long long)level_ion[k] * S + s;
        n_t[s * K + k] = (lbf_t[s * K + k] / z[i]) * n_ion[i];
    }
}

// helium's levels of n_t are the v of the iteration's last pass, not (lbf / Z) N: directly behind plasma_population_kernel
__global__ void __launch_bounds__(256) helium_population_kernel(const double *__restrict__ v, int k0, int levels, long long K, int S, double *__restrict__ n_t)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)levels * S) return;
    const long long s = e / levels, k = e % levels;
    n_t[s * K + k0 + k] = v[k * S + s];
}

}  // namespace mc
