// event_log.hpp -- full r-packet tracking: one row per trace_packet outcome, written on the device.
//
// A row is appended after its event has been processed (the interaction done, the shell crossed).  Rows go to a pool of
// equal chunks like the line-visit log's (EstimatorLog): a wave holds one open chunk, ranks its appending lanes inside it
// (ballot + mbcnt) and takes the next chunk from the pool -- one atomic per chunk -- when the append does not fit; the
// lanes past the end of the old chunk start the new one, so no chunk but a wave's last has empty slots.  Each packet's
// row count goes to counts[] when the packet ends.  Once the pool is empty rows are dropped (and counted); the counts stay
// exact, so the host learns the capacity a re-run needs.  After the call an exclusive scan of the counts gives each packet's
// first row and a scatter puts row (packet, event_id) at offsets[packet] + event_id of packet-major columns.
#pragma once
#include "mc_device.hpp"

namespace mc {

// 96 bytes, written as six 16-byte stores
struct __attribute__((aligned(16))) EventRow {
    double radius, before_nu;
    double before_mu, before_energy;
    double after_nu, after_mu;
    double after_energy;
    long long packet;
    int event_id, shell_id, after_shell_id, line_absorb_id;
    int line_emit_id, type_status, pad0, pad1;  // type_status: interaction_type | status << 8
};
static_assert(sizeof(EventRow) == 96, "event row layout");

// Per-wave state of the append (in LDS: lanes of a divergent wave append at different times): {open chunk, rows used}.
// chunk -1: none yet; -2: the pool is exhausted (no further claims).
__device__ __forceinline__ void event_log_wave_init(volatile int *ws)
{
    ws[0] = -1;
    ws[1] = 0;
}

// The slot of a record in a chunk pool (EventLog / SegmentLog: chunk_fill, pool_next, dropped, chunk_rows, n_chunks), shared by every appender.
// `mask`: the lanes that append now (all of them execute this call); `mine`: this lane is one of them; chunk / used: the wave's open chunk
// and the records in it, updated here (the same values in every lane).  Returns the slot, -1 for a lane that does not append or whose
// record is dropped because the pool is empty (counted in *dropped).
struct PoolSlot { long long slot; int chunk; unsigned used; };
template <typename Log>
__device__ __forceinline__ PoolSlot chunk_pool_claim(const Log &L, unsigned long long mask, bool mine, int chunk, unsigned used)
{
    const unsigned n = (unsigned)__popcll(mask);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    const int leader = __ffsll((long long)mask) - 1;
    const bool first = mine && rank == 0;
    const unsigned room = chunk >= 0 ? L.chunk_rows - used : 0u;
    int fresh = -2;
    if (n > room && chunk != -2) {
        int c = 0;
        if (first) {
            if (chunk >= 0) glob(L.chunk_fill)[chunk] = L.chunk_rows;
            c = (int)gatomic_add_u32(L.pool_next, 1u);
        }
        c = __shfl(c, leader);
        fresh = (unsigned)c < L.n_chunks ? c : -2;
    }
    PoolSlot out;
    out.slot = -1;
    if (mine) {
        if (rank < room) out.slot = (long long)chunk * L.chunk_rows + used + rank;
        else if (fresh >= 0) out.slot = (long long)fresh * L.chunk_rows + (rank - room);
    }
    const unsigned long long lost = __ballot(mine && out.slot < 0);
    if (first && lost) gatomic_add_u64(L.dropped, (unsigned long long)__popcll(lost));
    if (n > room) { out.chunk = fresh; out.used = fresh >= 0 ? n - room : 0u; }
    else { out.chunk = chunk; out.used = used + n; }
    return out;
}

// The lane kernel's appenders: the lanes of a divergent wave append at different times, so the wave's {open chunk, records used} live in LDS;
// every active lane appends.
template <typename Log>
__device__ __forceinline__ long long chunk_pool_claim_lds(const Log &L, volatile int *ws)
{
    const unsigned long long mask = __ballot(1);
    const PoolSlot s = chunk_pool_claim(L, mask, true, ws[0], (unsigned)ws[1]);
    if ((int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) { ws[0] = s.chunk; ws[1] = (int)s.used; }
    return s.slot;
}

__device__ __forceinline__ void event_row_store(EventRow *row, long long packet, int event_id, int type, int status, int shell, int after_shell,
                                                double radius, double b_nu, double b_mu, double b_e, double a_nu, double a_mu, double a_e, int absorb,
                                                int emit)
{
    double2 *d = reinterpret_cast<double2 *>(row);
    d[0] = make_double2(radius, b_nu);
    d[1] = make_double2(b_mu, b_e);
    d[2] = make_double2(a_nu, a_mu);
    d[3] = make_double2(a_e, __longlong_as_double(packet));
    int4 *q = reinterpret_cast<int4 *>(d + 4);
    q[0] = make_int4(event_id, shell, after_shell, absorb);
    q[1] = make_int4(emit, type | (status << 8), 0, 0);
}

// Append one row per active lane.  Called from one site per event, whatever the event's type.
__device__ __forceinline__ void event_log_append(const EventLog &L, volatile int *ws, long long packet, int event_id, int type,
                                                 int status, int shell, int after_shell, double radius, double b_nu,
                                                 double b_mu, double b_e, double a_nu, double a_mu, double a_e, int absorb,
                                                 int emit)
{
    const long long slot = chunk_pool_claim_lds(L, ws);
    if (slot >= 0) event_row_store(L.rows + slot, packet, event_id, type, status, shell, after_shell, radius, b_nu, b_mu, b_e, a_nu, a_mu, a_e, absorb, emit);
}

// The segment log of the photo-ionisation estimators: one record and its key
__device__ __forceinline__ void segment_record_store(const SegmentLog &L, long long slot, double comov_nu, double ed, int shell)
{
    SegmentRecord rec;
    rec.comov_nu = comov_nu; rec.ed = ed; rec.shell = shell; rec.pad = 0;
    gstore(L.recs + slot, rec);
    glob(L.keys)[slot] = (unsigned)shell;
}
__device__ __forceinline__ void segment_log_append(const SegmentLog &L, volatile int *ws, double comov_nu, double ed, int shell)
{
    const long long slot = chunk_pool_claim_lds(L, ws);
    if (slot >= 0) segment_record_store(L, slot, comov_nu, ed, shell);
}

// At the end of the kernel (wave converged): the fill of the wave's open chunk.
template <typename Log>
__device__ __forceinline__ void event_log_wave_close(const Log &L, volatile int *ws)
{
    if ((threadIdx.x & 63) == 0 && ws[0] >= 0) L.chunk_fill[ws[0]] = (unsigned)ws[1];
}

// ---- post pass: offsets[P + 1] = exclusive scan of counts[P] (three launches: tile sums, a scan of the tile sums, tiles)
constexpr int EV_SCAN_TILE = 1024;  // counts per tile (256 threads x 4)

__device__ __forceinline__ long long block_exclusive_scan_256(long long v, long long *lds, long long &total)
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        long long a = t >= off ? lds[t - off] : 0;
        __syncthreads();
        lds[t] += a;
        __syncthreads();
    }
    total = lds[255];
    long long ex = lds[t] - v;
    __syncthreads();
    return ex;
}

__global__ void __launch_bounds__(256) event_scan_tiles_kernel(const int *__restrict__ counts, long long n,
                                                              long long *__restrict__ tile_sums)
{
    __shared__ long long lds[256];
    const long long base = (long long)blockIdx.x * EV_SCAN_TILE + threadIdx.x * 4;
    long long s = 0;
    for (int k = 0; k < 4; ++k) if (base + k < n) s += counts[base + k];
    long long total;
    (void)block_exclusive_scan_256(s, lds, total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// one workgroup: tile_sums -> exclusive prefix in place, offsets[n] = total
__global__ void __launch_bounds__(256) event_scan_sums_kernel(long long *__restrict__ tile_sums, long long n_tiles,
                                                             long long *__restrict__ offsets, long long n)
{
    __shared__ long long lds[256];
    long long carry = 0;
    for (long long b = 0; b < n_tiles; b += 256) {
        const long long i = b + threadIdx.x;
        long long v = i < n_tiles ? tile_sums[i] : 0;
        long long total;
        long long ex = block_exclusive_scan_256(v, lds, total);
        if (i < n_tiles) tile_sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}

__global__ void __launch_bounds__(256) event_scan_apply_kernel(const int *__restrict__ counts, long long n,
                                                              const long long *__restrict__ tile_sums,
                                                              long long *__restrict__ offsets)
{
    __shared__ long long lds[256];
    const long long base = (long long)blockIdx.x * EV_SCAN_TILE + threadIdx.x * 4;
    int c[4];
    long long s = 0;
    for (int k = 0; k < 4; ++k) { c[k] = base + k < n ? counts[base + k] : 0; s += c[k]; }
    long long total;
    long long ex = block_exclusive_scan_256(s, lds, total) + tile_sums[blockIdx.x];
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) offsets[base + k] = ex;
        ex += c[k];
    }
}

// packet-major columns of the caller's TardisMcEventLog (int64 / float64, the ABI's dtypes)
struct EventColumns {
    long long *event_id, *interaction_type, *status, *shell_id, *after_shell_id, *line_absorb_id, *line_emit_id;
    double *radius, *before_nu, *before_mu, *before_energy, *after_nu, *after_mu, *after_energy;
};

__global__ void __launch_bounds__(256) event_scatter_kernel(const EventRow *__restrict__ rows,
                                                           const unsigned *__restrict__ chunk_fill, unsigned chunk_rows,
                                                           long long n_slots, const long long *__restrict__ offsets,
                                                           EventColumns col)
{
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += (long long)gridDim.x * blockDim.x) {
        const long long c = s / chunk_rows;
        if ((unsigned)(s - c * chunk_rows) >= chunk_fill[c]) continue;
        const double2 *d = reinterpret_cast<const double2 *>(rows + s);
        const double2 d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
        const int4 q0 = reinterpret_cast<const int4 *>(d + 4)[0], q1 = reinterpret_cast<const int4 *>(d + 4)[1];
        const long long packet = __double_as_longlong(d3.y);
        if (q0.x < 0 || q0.x >= offsets[packet + 1] - offsets[packet]) continue;  // (never for a complete call: the packet's count bounds its rows)
        const long long j = offsets[packet] + q0.x;
        col.radius[j] = d0.x; col.before_nu[j] = d0.y;
        col.before_mu[j] = d1.x; col.before_energy[j] = d1.y;
        col.after_nu[j] = d2.x; col.after_mu[j] = d2.y;
        col.after_energy[j] = d3.x;
        col.event_id[j] = q0.x; col.shell_id[j] = q0.y; col.after_shell_id[j] = q0.z; col.line_absorb_id[j] = q0.w;
        col.line_emit_id[j] = q1.x; col.interaction_type[j] = q1.y & 0xff; col.status[j] = q1.y >> 8;
    }
}

}  // namespace mc
