// vpacket_log.hpp -- the v-packet log of a propagate call, consolidated on the device (tardis_mc_get_vpacket_log,
// tardis_mc_vpacket_decomposition; include/tardis_mc.h).
//
// The propagation kernels append one entry per v-packet in the order the chip finishes them: {packet, seq, nu, energy, initial_mu,
// initial_r}, and with the option vpacket_last_interaction the spawning r-packet's last-interaction tracker at the time of the volley
// ({type, absorb line, emit line, shell} as 4 x int32 and before_nu as a double, 24 B; the radius of that interaction is the entry's
// initial_r, the volley is traced from where the interaction happened).  The reference consolidates per-packet lists in packet order
// (packet_collections.py:310-396).  `seq` is the entry's ordinal within its packet, so the position of an entry in that order is
// offsets[packet] + seq and nothing has to be sorted:
//   count    one atomic per entry: entries per source packet (int32 per packet);
//   scan     the event log's three scan kernels (event_log.hpp) turn the counts into offsets[n_packets + 1];
//   scatter  entry k goes to offsets[packet[k]] + seq[k] of packet-ordered SoA columns, the int32 fields widened to int64 -- the layout
//            packet_decomposition_kernel reads as it is.
// Every index is checked before it is used: the packet against [0, n_packets), seq against [0, count[packet]), the position against
// the capacity; an entry that fails is skipped and counted into an error word, which fails the call on the host.
#pragma once

#include "mc_device.hpp"

namespace mc {

__global__ void __launch_bounds__(256) vpacket_log_count_kernel(const long long *__restrict__ packet, long long n_entries, long long n_packets,
                                                                int *__restrict__ counts, unsigned long long *__restrict__ errors)
{
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n_entries; k += (long long)gridDim.x * blockDim.x) {
        const long long p = packet[k];
        if (p < 0 || p >= n_packets) { atomicAdd(errors, 1ull); continue; }
        atomicAdd(&counts[p], 1);
    }
}

// the raw log (append order) and the consolidated columns (packet order, then spawn order)
struct VpacketLogRaw {
    const long long *packet;
    const int *seq;
    const double *nu, *energy, *mu, *r;
    const int4 *li_ids;   // null: the call ran without vpacket_last_interaction
    const double *li_nu;
};
struct VpacketLogColumns {
    long long *source_packet;
    double *nu, *energy, *mu, *r;
    double *li_in_nu, *li_in_r;  // the six last-interaction columns: null with li_ids
    long long *li_type, *li_in_id, *li_out_id, *li_shell_id;
};

__global__ void __launch_bounds__(256) vpacket_log_scatter_kernel(VpacketLogRaw raw, long long n_entries, long long n_packets, long long capacity,
                                                                  const int *__restrict__ counts, const long long *__restrict__ offsets,
                                                                  VpacketLogColumns col, unsigned long long *__restrict__ errors)
{
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n_entries; k += (long long)gridDim.x * blockDim.x) {
        const long long p = raw.packet[k];
        if (p < 0 || p >= n_packets) { atomicAdd(errors, 1ull); continue; }
        const int s = raw.seq[k];
        if (s < 0 || s >= counts[p]) { atomicAdd(errors, 1ull); continue; }
        const long long j = offsets[p] + s;
        if (j < 0 || j >= capacity) { atomicAdd(errors, 1ull); continue; }
        col.source_packet[j] = p;
        col.nu[j] = raw.nu[k]; col.energy[j] = raw.energy[k]; col.mu[j] = raw.mu[k];
        const double r = raw.r[k];
        col.r[j] = r;
        if (raw.li_ids) {
            const int4 ids = raw.li_ids[k];  // {type, absorb line, emit line, shell}
            col.li_in_nu[j] = raw.li_nu[k];
            col.li_in_r[j] = ids.x == -1 ? __builtin_nan("") : r;  // (no interaction before the launch volley)
            col.li_type[j] = ids.x; col.li_in_id[j] = ids.y; col.li_out_id[j] = ids.z; col.li_shell_id[j] = ids.w;
        }
    }
}

}  // namespace mc
