// bf_estimators.hpp -- photo-ionisation and heating estimators from the transport's segment log.
//
// Restates update_bound_free_estimators in the operation order include/tardis_mc.h spells out (fp64, no contraction, exp is mcm::exp): a sum
// over the same segments as J, with a loop over the continua that are current at the segment's comoving frequency.  That loop does not run inside
// a propagation kernel: the FT instantiations of the lane kernel and of the wave-owner kernel log one 24-byte SegmentRecord per move of positive
// length (mc_device.hpp; appended through chunk_pool_claim, event_log.hpp), and this pass turns the log into the five [NC][S] tables:
//
//   bin_count_kernel / bin_scan_kernel / bin_scatter_kernel (estimator_log.hpp) group the record indices by shell (the keys are the shells);
//   bf_accumulate_kernel: a workgroup takes a (shell, slice of <= EST_SLICE records).  It stages batches of 256 records in LDS -- the staging thread
//     computes the record's bfac -- and every thread owns continua: with NC >= 256 thread t owns t, t + 256, ... in turn, a pass over the slice for
//     each (the records are staged, and bfac computed, ceil(NC / 256) times: the sums of one continuum per thread stay in registers, and the
//     staging is a small part of a pass in which 256 threads walk every record; profiles/bf_estimators.txt); with fewer, the 256 / NC threads that share a continuum walk every (256 / NC)-th record each.  A thread keeps its continuum's bounds and
//     its five sums in registers, reads the staged records by broadcast, bisects only in blocks that are current and adds its sums to the tables
//     once per slice with fp64 atomics.  No LDS atomics, no bound on NC.
//
// Every term is non-negative; the order of a cell's sum is not specified (atomics), the statistics are exact.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mc_device.hpp"
#include "mc_math.hpp"
#include "continuum_opacity.hpp"
#include "estimator_log.hpp"

namespace mc {

constexpr int BF_THREADS = 256;
constexpr int BF_TABLES = 5;  // photo_ion, stim_recomb, bf_heating, stim_recomb_cooling (doubles), statistics (int64): [NC][S] each, one allocation

struct BfAccumulateArgs {
    int S, NC;
    double h, k_b;
    const int *block_edge;            // [NC+1]
    const double *nu, *x_sect;        // [NP]
    const double *nu_min, *nu_max;    // [NC] a block's first (= nu_i) and last frequency
    const double *t_e;                // [S]
    const SegmentRecord *recs;        // the log's pool
    const unsigned *sorted_index;     // the slots of the records, grouped by shell
    const unsigned *bin_start;        // [S+1]
    const unsigned *slice_start;      // [S+1]
    double *tables;                   // [BF_TABLES][NC][S]
};

__global__ void __launch_bounds__(BF_THREADS) bf_accumulate_kernel(BfAccumulateArgs a)
{
    __shared__ double st_nu[BF_THREADS], st_ed[BF_THREADS], st_bfac[BF_THREADS];
    const unsigned n_slices = a.slice_start[a.S];
    const int t = threadIdx.x;
    const int width = a.NC < BF_THREADS ? a.NC : BF_THREADS;  // continua a pass over the records serves
    const int share = BF_THREADS / width;                     // threads that share a continuum
    const int ci = t % width, phase = t / width;
    const long long cells = (long long)a.NC * a.S;
    for (unsigned slice = blockIdx.x; slice < n_slices; slice += gridDim.x) {
        int lo = 0, hi = a.S;  // shell of this slice: the last s with slice_start[s] <= slice
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.slice_start[mid] <= slice) lo = mid; else hi = mid;
        }
        const int s = lo;
        const unsigned rec_first = a.bin_start[s] + (slice - a.slice_start[s]) * EST_SLICE;
        const unsigned rec_last = min(a.bin_start[s + 1], rec_first + EST_SLICE);
        const double beta_e = 1 / (a.k_b * a.t_e[s]);
        for (int c0 = 0; c0 < a.NC; c0 += width) {
            const int c = c0 + ci;
            const bool own = phase < share && c < a.NC;
            double c_min = 0.0, c_max = -1.0;  // (an empty interval: nothing is current for a thread without a continuum)
            int p0 = 0, n_pts = 0;
            if (own) { c_min = a.nu_min[c]; c_max = a.nu_max[c]; p0 = a.block_edge[c]; n_pts = a.block_edge[c + 1] - p0; }
            double photo = 0.0, stim = 0.0, heating = 0.0, cooling = 0.0;
            unsigned long long count = 0;
            for (unsigned base = rec_first; base < rec_last; base += BF_THREADS) {
                __syncthreads();  // (the previous batch has been walked)
                if (base + (unsigned)t < rec_last) {
                    const SegmentRecord rec = a.recs[a.sorted_index[base + (unsigned)t]];
                    st_nu[t] = rec.comov_nu;
                    st_ed[t] = rec.ed;
                    st_bfac[t] = mcm::exp((a.h * rec.comov_nu) * (-beta_e));
                }
                __syncthreads();
                const int m = (int)min((unsigned)BF_THREADS, rec_last - base);
                for (int j = phase; j < m; j += share) {
                    const double nu = st_nu[j];
                    if (c_min <= nu && nu <= c_max) {
                        const ContinuumBracket k = continuum_bracket(a.nu + p0, n_pts, nu);
                        const double x_c = continuum_interpolate(k, a.x_sect[p0 + k.hi], a.x_sect[p0 + k.hi - 1]);
                        const double ex = st_ed[j] * x_c, bfac = st_bfac[j];
                        const double inc = ex / nu;
                        const double heat = ex * (1.0 - c_min / nu);
                        photo += inc;
                        stim += inc * bfac;
                        heating += heat;
                        cooling += heat * bfac;
                        ++count;
                    }
                }
            }
            if (count) {
                double *cell = a.tables + (long long)c * a.S + s;
                atomic_add_f64(cell, photo);
                atomic_add_f64(cell + cells, stim);
                atomic_add_f64(cell + 2 * cells, heating);
                atomic_add_f64(cell + 3 * cells, cooling);
                atomicAdd(reinterpret_cast<unsigned long long *>(cell + 4 * cells), count);
            }
        }
    }
}

// totals[0] += the records the pass has just grouped, totals[1] += the records the call dropped
__global__ void bf_totals_kernel(const unsigned *grouped, const unsigned long long *dropped, unsigned long long *totals)
{
    totals[0] += *grouped;
    if (dropped) totals[1] += *dropped;
}

// norm[s] = 1.0 / ((time_of_simulation volume[s]) h); gamma_est = photo_ion norm, stim_est = stim_recomb norm: rates[2][NC][S]
__global__ void __launch_bounds__(256) bf_rates_kernel(int S, long long cells, double time_of_simulation, double h, const double *__restrict__ volume,
                                                       const double *__restrict__ tables, double *__restrict__ rates)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cells) return;
    const int s = (int)(e % S);
    const double norm = 1.0 / ((time_of_simulation * volume[s]) * h);
    rates[e] = tables[e] * norm;
    rates[cells + e] = tables[cells + e] * norm;
}

}  // namespace mc
