// kpacket_sample.hpp -- what a k-packet turns into and at which frequency it comes back, from the resident tables of the cooling
// sub-stage (cooling_rates.hpp): the __device__ functions a transport kernel will call per k-packet, and nothing transport-specific.
// They have no launch of their own; kpacket_query_kernel runs them a thread per query for tardis_mc_kpacket_sample, which pins their
// arithmetic before a kernel includes them.
//
// In the operation order include/tardis_mc.h spells out.  process: searchsorted(k_cdf[:, s], z, side="right"), so entry j is chosen iff
// k_cdf[j-1] <= z < k_cdf[j] and an entry of zero rate is never chosen.  nu_free_bound: numpy.interp on the continuum's block of
// fb_emission_cdf[:, s] against its frequencies.  nu_free_free: (-((k_B t_e) / h)) log(z) with mcm::log.  Both bisections read a column
// of a [rows][S] table: they stride by S.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mc_device.hpp"
#include "mc_math.hpp"

namespace mc {

struct KpacketTables {
    int S, NC;
    double h, k_b;
    const int *block_edge;     // [NC+1]
    const double *nu;          // [NP]
    const double *fb_cdf;      // [NP][S] fb_emission_cdf
    const double *k_cdf;       // [2 + 2 NC][S]
    const double *t_e;         // [S]
};

namespace kpacket {

constexpr int KIND_FF = 0, KIND_ADIABATIC = 1, KIND_FB = 2, KIND_COLL_ION = 3;

struct Choice {
    int kind, continuum;  // continuum: -1 for KIND_FF and KIND_ADIABATIC
};

// searchsorted(col[0 .. n), z, side="right") on a column of stride S: the first index with col[index] > z, n where there is none
__device__ __forceinline__ int upper_bound_strided(const double *col, int n, long long S, double z)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[(long long)mid * S] <= z) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the process a k-packet in shell s turns into at the random number z in [0, 1)
__device__ __forceinline__ Choice process(const KpacketTables &t, int s, double z)
{
    const int n = 2 + 2 * t.NC;
    int j = upper_bound_strided(t.k_cdf + s, n, t.S, z);
    if (j > n - 1) j = n - 1;
    Choice out;
    if (j < 2) { out.kind = j; out.continuum = -1; }
    else if (j < 2 + t.NC) { out.kind = KIND_FB; out.continuum = j - 2; }
    else { out.kind = KIND_COLL_ION; out.continuum = j - 2 - t.NC; }
    return out;
}

// the frequency of a free-bound emission of continuum c in shell s at the random number z in [0, 1)
__device__ __forceinline__ double nu_free_bound(const KpacketTables &t, int c, int s, double z)
{
    const int p0 = t.block_edge[c], n = t.block_edge[c + 1] - p0;
    const double *cdf = t.fb_cdf + (long long)p0 * t.S + s;
    const double *b = t.nu + p0;
    const int at = upper_bound_strided(cdf, n, t.S, z);
    const int hi = at < 1 ? 1 : (at > n - 1 ? n - 1 : at), lo = hi - 1;
    const double cdf_lo = cdf[(long long)lo * t.S], cdf_hi = cdf[(long long)hi * t.S];
    return b[lo] + ((z - cdf_lo) * (b[hi] - b[lo])) / (cdf_hi - cdf_lo);
}

// the frequency of a free-free emission in shell s at the random number z in [0, 1); z == 0.0 gives +inf
__device__ __forceinline__ double nu_free_free(const KpacketTables &t, int s, double z)
{
    return (-((t.k_b * t.t_e[s]) / t.h)) * mcm::log(z);
}

}  // namespace kpacket

struct KpacketQueryArgs {
    long long n;
    const int *shell;           // [n]
    const double *z_process;    // [n]
    const double *z_nu;         // [n]
    const int *force_kind;      // [n] -1: sample; null: sample all
    const int *force_continuum; // [n] read where force_kind is 2 or 3; null only with force_kind null
    int *kind, *continuum;      // [n], may be null
    double *nu;                 // [n], may be null
};

// tardis_mc_kpacket_sample: a thread per query
__global__ void __launch_bounds__(256) kpacket_query_kernel(KpacketTables t, KpacketQueryArgs q)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= q.n) return;
    const int s = q.shell[e];
    const int forced = q.force_kind ? q.force_kind[e] : -1;
    kpacket::Choice ch;
    if (forced < 0) ch = kpacket::process(t, s, q.z_process[e]);
    else { ch.kind = forced; ch.continuum = forced >= kpacket::KIND_FB ? q.force_continuum[e] : -1; }
    double nu = 0.0;
    if (ch.kind == kpacket::KIND_FF) nu = kpacket::nu_free_free(t, s, q.z_nu[e]);
    else if (ch.kind == kpacket::KIND_FB) nu = kpacket::nu_free_bound(t, ch.continuum, s, q.z_nu[e]);
    if (q.kind) q.kind[e] = ch.kind;
    if (q.continuum) q.continuum[e] = ch.continuum;
    if (q.nu) q.nu[e] = nu;
}

}  // namespace mc
