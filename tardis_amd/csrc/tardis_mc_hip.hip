// tardis_mc_hip.hip -- host side of libtardis_mc_hip.so: the C ABI of include/tardis_mc.h over the HIP kernels.
//
// One context = one HIP device + one stream.  Inputs are copied to HBM and re-laid shell-major once
// (tardis_mc_set_*), kernels run asynchronously on the context stream (tardis_mc_propagate), results are
// re-laid to the reference's [L,S] layout on the device and copied out (tardis_mc_get_results).
// RCCL is bound lazily with dlopen so that single-GPU users never map librccl.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <functional>
#include <numeric>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tardis_mc.h"
#include "mc_device.hpp"
#include "propagate_lane.hpp"
#include "event_log.hpp"
#include "bf_estimators.hpp"
#include "propagate_group.hpp"
#include "estimator_log.hpp"
#include "estimator_partition.hpp"
#include "propagate_wave.hpp"
#include "packet_source.hpp"
#include "formal_integral.hpp"
#include "formal_interpolate.hpp"
#include "source_function.hpp"
#include "tau_prefix.hpp"
#include "sweep_skip.hpp"
#include "propagate_plan.hpp"
#include "packet_decomposition.hpp"
#include "decomposition_plan.hpp"
#include "vpacket_log.hpp"
#include "opacity_update.hpp"
#include "opacity_update_plan.hpp"
#include "mean_opacity.hpp"
#include "mean_opacity_plan.hpp"
#include "plasma_update.hpp"
#include "plasma_update_plan.hpp"
#include "nlte_excitation.hpp"
#include "nlte_plan.hpp"
#include "continuum_rates.hpp"
#include "continuum_opacity.hpp"
#include "continuum_plan.hpp"
#include "cooling_rates.hpp"
#include "kpacket_sample.hpp"

static_assert(plan::DBG_WAVE_COUNTERS == mc::WV_DBG_FLAGS, "propagate_plan.hpp repeats the wave kernel's list of counter flags");

namespace {

thread_local std::string g_create_error;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap && p) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes ? bytes : 16;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};
// Function-local device scratch: a DevBuf that is freed when the function returns, on every path.  (The context's own buffers stay plain DevBufs
// with an explicit release(): tardis_mc_destroy has to select the device first.)
struct ScopedDevBuf : DevBuf {
    ScopedDevBuf() = default;
    ScopedDevBuf(const ScopedDevBuf &) = delete;
    ScopedDevBuf &operator=(const ScopedDevBuf &) = delete;
    ~ScopedDevBuf() { release(); }
};
// what the release() of a struct of the context is made of: each frees what it is given and nulls it
void release_buffer(DevBuf &b) { b.release(); }
template <size_t N> void release_buffer(DevBuf (&bufs)[N])
{
    for (DevBuf &b : bufs) b.release();
}
template <typename... Bufs> void release_buffers(Bufs &...bufs) { (release_buffer(bufs), ...); }
void destroy_event(hipEvent_t &e)
{
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
}
template <size_t N> void destroy_events(hipEvent_t (&ev)[N])
{
    for (hipEvent_t &e : ev) destroy_event(e);
}
void destroy_events(std::vector<hipEvent_t> &ev)
{
    for (hipEvent_t &e : ev) destroy_event(e);
    ev.clear();
}
void destroy_stream(hipStream_t &s)
{
    if (s) { (void)hipStreamDestroy(s); s = nullptr; }
}
template <typename T> void free_pinned(T *&p)
{
    if (p) { (void)hipHostFree(p); p = nullptr; }
}

// ---- RCCL, bound lazily
struct Id128 { char bytes[TARDIS_MC_UNIQUE_ID_BYTES]; };
struct Rccl {
    void *handle = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, /* ncclUniqueId by value: 128 bytes */ Id128, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;

bool load_rccl(std::string &err)
{
    if (g_rccl.handle) return true;
    const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void *h = nullptr;
    for (const char *n : names) { h = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (h) break; }
    if (!h) { err = std::string("dlopen(librccl.so) failed: ") + dlerror(); return false; }
    g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    g_rccl.AllReduce = reinterpret_cast<decltype(g_rccl.AllReduce)>(dlsym(h, "ncclAllReduce"));
    g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy) {
        err = "librccl.so lacks an expected nccl* symbol";
        dlclose(h);
        return false;
    }
    g_rccl.handle = h;
    return true;
}

}  // namespace

// The context: what several stages share at the top level, then one struct per stage -- its resources, the options that steer it, its flags, and a
// release() that names every resource of the struct.  A resource lives in exactly one struct; tardis_mc_destroy calls the release() of each.
struct TardisMcContext {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    std::vector<hipEvent_t> ev_chunk;  // group kernel: 4 per chunk (before seed / after seed / after propagate, twice); wave kernel: 5 per call (prep, launch, read-back)
    int chunks_timed = 0;
    bool timed = false;
    std::string err;
    hipDeviceProp_t prop{};
    double last_post_ms = 0.0;  // estimator passes (binning + accumulation) of the last propagate call
    double sum_seed_ms = 0.0, sum_prop_ms = 0.0, sum_post_ms = 0.0;
    int launches = 0;
    // state flags
    bool have_geometry = false, have_opacity = false, have_config = false, have_packets = false;
    // geometry
    int n_shells = 0;
    double t_exp = 0;
    DevBuf r_inner, r_outer;
    // problem shape of the resident opacity tables
    int n_lines = 0, n_trans = 0, n_levels = 0;
    // config
    TardisMcConfig cfg{};
    std::vector<double> grid_host;
    DevBuf grid;
    // scratch
    DevBuf staging, rng_state, counters, first_error, next_packet, problem_dev;
    mc::DeviceProblem problem_host{};
    long long chunk_packets = 16LL << 20;  // packets per seeded-state chunk (2496 B each) of the cooperative kernel
    // launch geometry
    int variant = -1;  // 0: lane-per-packet kernel; 1: group-per-packet kernel; 2: wave-owner kernel, group sweeps; 3: wave-owner kernel, lane sweeps; 4: wave-owner kernel with the volley queue; -1: automatic
    int blocks_per_cu = 16;
    int debug_flags = 0;
    int group_size = 0;  // 0: automatic (8 or 16 lanes per packet)
    long long vpk_wave_min_packets = 100000;  // option: calls with v-packets on fine grids take the wave kernel from this many packets on (the group kernel below)
    int vpk_wide_registers = 1;       // option: the two-waves-per-SIMD v-packet instantiation where LDS bounds the occupancy at eight waves per CU anyway
    int last_variant = -1;  // kernel of the last propagate call (see tardis_mc_last_variant)
    int table_offsets = -1;       // option: row offsets of the cooperative kernels, -1 64-bit where S x L or S x T reaches 2^28, 0 always 32-bit, 1 always 64-bit
    int last_table_offsets = -1;  // 32 / 64: row offsets of the last propagate call's kernel (see tardis_mc_last_table_offsets)
    int waves_per_simd = 4;  // register budget hint of the cooperative kernel (2: 256 VGPRs, 3: 168, 4: 128)
    int last_kernel_table = -1;   // the kernel-table row the last propagate call looked up: 0 lane, 1 group, 2 wave, -1 none ...
    int last_kernel_key[12] = {}; // ... and its key (see tardis_mc_last_kernel_key)
    void release()  // (the last of tardis_mc_destroy: the stages' buffers and events go before the stream they were used on)
    {
        release_buffers(r_inner, r_outer, grid, staging, rng_state, counters, first_error, next_packet, problem_dev);
        destroy_event(ev_start); destroy_event(ev_stop); destroy_events(ev_chunk);
        destroy_stream(stream);
    }
    // Opacity tables: what set_opacity uploads, re-laid shell-major, with the bucket index of the line list.  Per set_opacity: host copies of the five index
    // tables (line2macro_level_upper, macro_block_edge_index, transition_type, destination_level_id, transition_line_id; int32, the staging vectors of their
    // upload) and of the line list, from which derive_opacity_tables builds every table that depends on the probabilities, with or without the caller's pointers.
    struct OpacityTables {
        DevBuf nu_line, tau_t, n_e, prob_t, cum_t, trans_nu, line2level, block_edge, ttype, dest, tline, line_block, trans_rec, bucket_first;
        int bucket_shift = 0, bucket_n = 0;
        int bucket_lines_permille = 750;  // option: target lines per bucket x 1000 (takes effect in set_opacity)
        long long bucket_kmin = 0;
        bool lines_sorted = true;  // line_list_nu strictly usable by the index-based kernels (non-increasing, positive)
        bool prob_negative = false;  // a negative transition probability: the running sums are not monotone, no jump search
        std::vector<int> h_idx[5];
        std::vector<double> h_nu;
        bool h_macro = false;
        void release() { release_buffers(nu_line, tau_t, n_e, prob_t, cum_t, trans_nu, line2level, block_edge, ttype, dest, tline, line_block, trans_rec, bucket_first); }
    } ot;
    // Walk tables of the macro-atom walk (walk_tables.hpp), derived from the probabilities by derive_opacity_tables
    struct WalkTables {
        DevBuf cum16, rec16, quad_info, line_block_c;  // compact walk tables (walk_tables.hpp)
        DevBuf hot_sec, hot_mass, hot_flag, blk_tab;   // hot sectors of the macro-atom walk (walk_tables.hpp)
        bool have_hot = false;
        long long n_hot_blocks = 0;                    // blocks entered through a hot sector (diagnostic)
        int walk_hot = -1;                             // -1: blocks whose six widest intervals cover enough (walk_hot_min_mass); 0: none; 1: every block
        // per mille of a block's probability, mean over the shells; blocks of <= 32 / more rows.  Measured (profiles/r04_walk_hot_sectors.txt):
        // heavy-tailed blocks -11 % whatever the thresholds (95 % of their jumps are decided by the sector); blocks of 12-24 rows with
        // uniformly drawn probabilities (six intervals cover ~50-70 %) lose 2.5 % at 600 -- a missed probe costs a round of the walk
        int walk_hot_min_mass = 800, walk_hot_min_mass_long = 400;
        unsigned cum16_stride = 0;
        bool have_walk_tables = false;
        int walk_sector_packing = 1;  // compact walk tables: short blocks do not straddle 64-byte sectors (set before set_opacity; 0: packed at 16 bytes as in round 2)
        void release() { release_buffers(cum16, rec16, quad_info, line_block_c, hot_sec, hot_mass, hot_flag, blk_tab); }
    } wt;
    struct ScreeningTables {
        DevBuf tau_pfx, tau_rowsum, pfx_flag;          // v-packet screening tables (tau_prefix.hpp), built at the first SCREENING call after set_opacity (+ their negative-depth flag)
        bool pfx_valid = false, pfx_negative = false;
        int vpacket_screening = -1;  // v-packet screening on the prefix sums of tau (tau_prefix.hpp): -1 automatic, 0 off, 1 on
        void release() { release_buffers(tau_pfx, tau_rowsum, pfx_flag); }
    } sc;
    struct SweepTable {
        // Interleaved sweep table (round 6): nt_t[shell][line] = {nu_line, tau}, 16 bytes per line, rows on 128-byte boundaries -- the eight 16-byte loads of
        // a lane-sweep step come from one run of 128 bytes instead of two runs of 64 bytes in two tables.  Option sweep_table: 0 the separate tables,
        // 1 runs from the current line, 2 aligned runs (propagate_wave_kernel<..., NT>); built by the first propagate call after set_opacity that uses it.
        // -1 (default) = 1 -- measured (profiles/r06_sweep_table.txt): sixteen-wave instantiation, 1e8 packets of configs[2] -1.0 ... -1.5 %, 2e7 -4 %, 1.25e7 -6 %,
        // uniform levels -4.5 ... -6 %, configs[1] -1 ... -3 %; twelve-wave instantiation (with the lean proof) -1.7 ... -4.6 %; aligned runs (2) +2 ... +6 % on the
        // heavy-tailed tables (a trace's first step is shorter: 8 % more steps), -5 % on the uniform ones.
        int sweep_table = -1;
        DevBuf nt_t;
        bool nt_valid = false, nt_negative = false;  // (nt_negative: the table holds a negative / NaN optical depth -- the lean proof of the NT kernels does not apply)
        unsigned nt_stride = 0;
        // Block skip of the sixteen-wave and the twelve-wave lane sweep on this table (sweep_skip.hpp).  Option sweep_skip: -1 automatic, 0 off, 1 on where the plan allows it (plan::plan_sweep_skip).
        // Its tables lie behind the interleaved table in nt_t's allocation (the kernel reads all three from one base with 32-bit offsets): the coarse entries
        // ct[shell][block] = {nu_last, p_end}, rows of nt_stride / 8, 16 entries of slack; then pn[shell][0 .. L] = {frequency slot, prefix sum (tau_prefix_kernel)}.  Built by
        // the first propagate call after set_opacity that may use them (sk_valid falls with nt_valid); sk_negative: tau_prefix_kernel's flag; sk_margin: ssk::margin
        // of the largest row sum.  last_sweep_skip: what the last propagate call ran with (tardis_mc_last_sweep_skip)
        int sweep_skip = -1, last_sweep_skip = 0;
        // Option sweep_start_held (ssk::MODE_START_HELD: the walk's read of an emission line's frequency brings the start entry of the coming trace along): -1 automatic
        // (SWEEP_START_HELD_AUTO where the call's sweeps skip), 0 off, 1 on where the call's sweeps skip
        int sweep_start_held = -1;
        bool sk_valid = false, sk_negative = false;
        unsigned sk_ct_off = 0, sk_pn_off = 0;
        double sk_margin = 0.0;
        DevBuf sk_rowsum;
        void release() { release_buffers(nt_t, sk_rowsum); }
    } sw;
    struct Estimators {
        // estimators: one allocation [J | nubar | vhist | pad | jblue copy0 | edot copy0 | jblue copy1.. | edot copy1..]
        DevBuf est;
        size_t est_S = 0, est_L = 0, est_G = 0;
        int est_copies = 1;
        bool est_valid = false;
        bool est_propagated = false;  // a propagate call has added to the estimators since they were last zeroed (the detailed mode of tardis_mc_update_opacity)
        void release() { release_buffers(est); }
    } es;
    // packets and the per-packet results
    struct Packets {
        long long n_packets = 0;
        DevBuf r0, mu0, nu0, e0, seeds, out_nu, out_e;
        DevBuf li_f64[9], li_i64[5], li_rec;  // (li_rec: the wave kernel's 64-byte tracker records, unpacked into the arrays after the propagation)
        bool track = true;
        bool li_valid = false;  // the last-interaction arrays are those of the last propagate call's packets (tardis_mc_packet_decomposition)
        DevBuf dc_work;         // tardis_mc_packet_decomposition: the class table and the outputs of a call
        void release() { release_buffers(r0, mu0, nu0, e0, seeds, out_nu, out_e, li_f64, li_i64, li_rec, dc_work); }
    } pk;
    struct VpacketLog {
        DevBuf vlog_count, vlog_packet, vlog_seq, vlog_nu, vlog_energy, vlog_mu, vlog_r;
        long long vlog_capacity = 0;
        bool vlog_capacity_user = false;  // set through the vpacket_log_capacity option (otherwise sized per propagate call)
        // option vpacket_last_interaction: 24 B more per entry, behind vlog_r in its allocation (mc_device.hpp); the log consolidated on the device (vpacket_log.hpp): the per-packet
        // counts, their offsets, the scan's tile sums, the packet-ordered columns (five, or eleven with the last interaction), the error word
        bool vlog_li = false;
        DevBuf vl_counts, vl_offsets, vl_tiles, vl_cols, vl_errors;
        bool vl_valid = false;         // the last propagate call wrote a v-packet log and nothing has replaced its packets or its configuration since
        bool vl_li = false;            // ... with the last-interaction columns
        bool vl_consolidated = false;  // vl_cols holds that log
        long long vl_packets = 0, vl_capacity = 0, vl_count = 0;  // packets and device capacity of that call; entries it produced (once consolidated)
        void release() { release_buffers(vlog_count, vlog_packet, vlog_seq, vlog_nu, vlog_energy, vlog_mu, vlog_r, vl_counts, vl_offsets, vl_tiles, vl_cols, vl_errors); }
    } vl;
    struct EventLog {
        // full r-packet tracking (option track_full, event_log.hpp): runs on the wave kernel (variant 2) where that can run the call, else on the lane kernel; the row pool, its chunk fills, {pool_next, dropped},
        // the per-packet counts, and for tardis_mc_get_event_log the offsets, the tile sums of their scan and the packet-major columns
        bool track_full = false;
        long long evlog_capacity = 0;                    // option event_log_capacity: rows (0: automatic, 32 per packet)
        long long evlog_max_bytes = 16LL << 30;          // option event_log_max_bytes: the bound on the log's device memory
        DevBuf ev_rows, ev_fill, ev_state, ev_counts, ev_offsets, ev_tiles, ev_cols;
        bool ev_valid = false;                           // the last propagate call wrote an event log
        long long ev_packets = 0, ev_capacity = 0, ev_slots = 0;
        unsigned ev_chunk_rows = 128, ev_n_chunks = 0;
        void release() { release_buffers(ev_rows, ev_fill, ev_state, ev_counts, ev_offsets, ev_tiles, ev_cols); }
    } el;
    // What a call of the wave kernel runs on: the line-visit log sets, the epochs' saved lanes and waves, the compaction sets, the volley queue, the
    // second and the masked streams with their events, and the options that size or steer them
    struct WaveResources {
        bool walk_min_active_user = false, ls_min_active_user = false;  // (set through the options: no automatic choice then)
        int walk_min_active = 8;  // compact macro-atom walk: carry the longest chains over to the next pass once this few lanes still walk (-1: never)
        // last-interaction tracker of the lane sweeps without v-packets: 1 the record stays in LDS and is stored once, when the packet ends; 0 stored at every
        // interaction (propagate_wave.hpp, DEFER).  A problem whose shells or lines do not fit tracker_pack (mc_device.hpp) takes 0 whatever the option says;
        // tracker_pack_max_lines (tests): a lower bound on the lines that fit, 0 = the real one.  last_tracker_defer: what the last call ran with, -1 = no tracker
        // or another kernel
        int tracker_defer = 1, last_tracker_defer = -1;
        // rng_complete (lane sweeps without v-packets): the wave finishes a packet's MT19937 generation at the top of a pass, refills out of it only read
        int rng_complete = 1;
        long long tracker_pack_max_lines = 0;
        int ls_min_active = 8, ls_max_steps = 1 << 30;  // lane sweeps: when to leave the sweep phase (propagate_wave.hpp)
        int drain_split = 0;          // wave kernel: split the drain of a call off into a launch of its own (WaveCold::drain_split); measured: -4 % at 1e7 packets, +1.3 % at 1e8 -> off
        int log_tail_packets = 8;               // tail split: packets' worth of traces a lane in flight still logs after the supply has run out
        int log_tail_split = 1;                 // plan the epochs so that the last one holds only the drain of the call (see tardis_mc_propagate)
        int est_accumulate = 3;                 // accumulate kernel: 3 dyadic hierarchy of block sums, a lane per record (accumulate_dyadic_kernel<.., LOOP>), 2 the same with the blocks of 64 records spread over the lanes, 1 8-line block sums (accumulate_blocks_kernel), 0 one add per line visit (accumulate_kernel, index pipeline only)
        int est_pipeline = 1;                   // line-estimator passes: 1 two-level partition of the records (estimator_partition.hpp), 0 index sort + gather (estimator_log.hpp)
        DevBuf log_part;                        // est_pipeline 1: the scratch copy of one epoch's records, shared by both buffer sets
        long long log_chunk_records = 0;        // records per chunk of the line-visit log's pool (0: automatic, <= 4096; tests)
        long long log_capacity = 2500000000LL;  // upper bound of the line-visit records per epoch and buffer set of the wave kernel (24 B + 4 B + 4 B each)
        bool log_capacity_user = false;         // set through the log_capacity option (otherwise also bounded by the free device memory)
        // wave kernel: chunks alternate between two buffer sets / streams, so that seeding and the estimator passes of one
        // chunk overlap the propagation of its neighbours
        hipStream_t stream2 = nullptr;
        hipEvent_t ev_join = nullptr;
        // CU partition (option pass_cus: CUs per XCD set aside for the estimator passes, 0 = off): the propagation launches of a call of several
        // epochs run on a stream whose queue is masked to the other CUs, the passes of epoch k beside epoch k + 1 on a stream masked to these
        int pass_cus = 0, pass_cus_built = 0;
        hipStream_t stream_prop_m = nullptr, stream_pass_m = nullptr;
        hipEvent_t ev_fork_m = nullptr, ev_join_m = nullptr;
        DevBuf log_records[2], log_keys[2], log_cursor[2], log_bins[2], log_sorted[2], wave_cold_dev;
        DevBuf seed_chk, vp_scratch;       // wave kernel: the launch records of a call's packets | the v-packet results handed from worker to owner lanes
        DevBuf vp_park;                     // pooled volleys with carry-over: one parked v-packet per lane
        int vp_carry_min_active = 16;       // pooled volleys: leave the volley phase once nothing waits and this few lanes still trace (0: never).  16: -7 % on the
                                            // configs[4] shape, -5 % on the tardis_example shape + 10 v-packets, flat from 16 to 32 (profiles/r05_volley_carry.txt)
        // wave kernel: word 397 of every packet's init_genrand sequence (lazy MT19937 seeding)
        double traces_per_packet = 0.0;  // measured by the last propagate (sizes the line-visit log of the next one)
        double log_budget_per_packet = 128.0;  // log records reserved per packet
        unsigned long long *events_host = nullptr;  // pinned: {events counter of the last propagate, its packet count}
        hipEvent_t ev_events = nullptr;
        std::vector<mc::WaveCold> wave_cold_host;
        // wave kernel: a propagate call is a sequence of epochs over one packet supply (LaneSave, propagate_wave.hpp)
        DevBuf lane_save, wave_save, suspended_dev;
        // drain compaction (option drain_compact = T: waves suspend once the supply has run out and T or fewer of their lanes are left; the live lanes are packed into
        // full waves and the rest of the call is a launch of fewer waves, beside the estimator passes): the packed grid's buffers, two sets for repeated packing
        int drain_compact = 0;
        int drain_pack_lanes = 64;  // live lanes per packed wave
        int est_one_level = 1;      // the passes' partition in one pass where the (shell, tile) bins are few enough to be ranked in LDS at once (0: always two levels)
        DevBuf lane_save_c[2], wave_save_c[2], seeded_states_c[2], drain_census;
        int compactions = 0;  // of the last propagate call
        DevBuf vq_req, vq_items, vq_count, vq_jsave;  // volley queue (variant 4, propagate_wave.hpp: VolleyRequest)
        long long vq_min_items = -1;  // switch the queue off for the rest of a call once a launch requests fewer v-packets (-1: automatic)
        int vq_min_active = 8, vq_oversubscribe = 4, vq_tracer_waves_per_simd = 6;
        unsigned *suspended_host = nullptr;  // pinned
        hipEvent_t ev_post[4] = {nullptr, nullptr, nullptr, nullptr};  // start / end of the estimator passes on log buffer set 0 / 1
        bool wave_epoch_mode = false, post_pending[2] = {false, false}, prop_pending = false;
        int log_sets = 0;  // 2: the estimator passes of an epoch run beside the next launch (two log sets); 1: before it (one set); 0: 1 for calls of several epochs, 2 otherwise
        // Shell-sorted log (round 6; propagate_wave_kernel<..., SL>): every chunk of the line-visit log holds records of one shell, the estimator passes start with
        // the partition by bin.  1 / -1: where the kernel has it (the production lane-sweep instantiations, <= 64 shells, partition pipeline); 0 (default) off.
        // Measured (profiles/r06_shell_sorted_log.txt): the passes of an epoch of 2e9 records 86.5 -> 64.2 ms as priced -- and the propagation launches +4.3 %
        // (2773 -> 2891-2904 ms per 1e8 packets) whether the slots come from ballot ranks (+3 % instructions) or from one LDS atomic (+1.5 %): net +0.6 ... +1.3 % on
        // the headline, -2 ... -3 % only where a call's passes are not overlapped by anything (2e7 packets with log_sets 1; configs[1])
        int log_by_shell = 0;
        // Split launches (round 6): from the second epoch of a call on, the propagation grid is launched as TWO kernels -- the first half of the waves at once, on the
        // engine's stream; the second half on the passes' stream, behind the estimator passes of the previous epoch.  While those passes run, the chip holds eight
        // propagation waves per CU instead of none (the passes' 1024-thread workgroups need half a CU: they cannot be placed beside sixteen resident waves, and used to
        // run alone at every epoch boundary: 0.37 s of a 3.1-s step); when they are over the second half follows.  Nothing in the kernel changes: the second launch
        // gets a WaveCold whose per-wave pointers (MT19937 states, suspended lanes / waves, v-packet scratch) are offset by the first launch's wave count.
        // MEASURED, and a clear loss (profiles/r06_split_launch.txt): parity-green, but configs[2] at 1e8 packets 3 109 -> 4 107 ms -- the passes beside eight resident
        // waves per CU take three times as long as alone (their workgroups need 72 KB of CONTIGUOUS LDS and find it on few CUs), the second half of the grid idles
        // meanwhile.  Option epoch_split, default 0.
        int epoch_split = 0;
        hipEvent_t ev_split[3] = {nullptr, nullptr, nullptr};  // the first launch's inputs are in place | start / end of the second launch
        DevBuf seeded_states;
        void release()
        {
            release_buffers(log_part, log_records, log_keys, log_cursor, log_bins, log_sorted, wave_cold_dev, seed_chk, vp_scratch, vp_park, seeded_states);
            release_buffers(lane_save, wave_save, suspended_dev, lane_save_c, wave_save_c, seeded_states_c, drain_census, vq_req, vq_items, vq_count, vq_jsave);
            destroy_event(ev_join); destroy_event(ev_fork_m); destroy_event(ev_join_m); destroy_event(ev_events); destroy_events(ev_post); destroy_events(ev_split);
            destroy_stream(stream2); destroy_stream(stream_prop_m); destroy_stream(stream_pass_m);
            free_pinned(events_host); free_pinned(suspended_host);
        }
    } wv;
    struct LaneSweepTuner {
        // Two instantiations of the lane-sweep kernel: 128 VGPRs / sixteen waves per CU (A), and 168 VGPRs / twelve waves per CU (B).  On the interleaved table
        // (the default) both carry the block skip of sweep_skip.hpp, A at eight 16-byte loads per step, coarse or fine, B at ten (propagate_wave.hpp,
        // LS_SKIP_LOADS_16 / _12; profiles/sweep_skip_widths.txt): the tuner compares two kernels that skip.  On the separate tables A sweeps eight lines per
        // step and B twelve, neither skips.  A wins where the steady state dominates (1e8 packets of the configs[2] shape: B +3.8 %), B where the drain of a
        // call's longest packets does (1.25e7 packets: -11 %; 1e5-1e6 packets of the tardis_example shape: -6 %; profiles/r05_ls_instantiations.txt):
        // fewer steps per trace shorten the serial chain of a lone packet, and a mostly idle chip does not miss the four waves.  Option
        // ls_waves_per_simd: 4 = A, 3 = B, 0 (default) = the engine times both on the first calls of a given (packet count, tables) and keeps the
        // faster one -- a Monte Carlo iteration repeats the same call; per-packet results are bit-identical either way.
        int ls_waves_per_simd = 0;
        // (the tuner: calls 0-4 of a key run A untimed, A, B, A, B -- each timed call with the tuner's OWN event pair, recorded only when the call was
        // enqueued completely, so that neither another entry point's use of ev_start / ev_stop nor a failed call can leave a stale or unpaired
        // measurement behind -- and from call 5 on B only if the faster of its two calls beat the faster of A's by >= 3 %: boxes differ by more
        // than one noisy sample can tell apart)
        struct { long long n = -1; int lines = 0, shells = 0, mode = 0, table = 0, wide = 0, phase = 0, pending = -1, choice = 0; double ms[2][2] = {{-1.0, -1.0}, {-1.0, -1.0}}; } ls_tune;
        hipEvent_t ev_tune[2] = {nullptr, nullptr};
        void release() { destroy_events(ev_tune); }
    } lt;
    // result streaming (tardis_mc_stream_results): the caller's per-packet arrays, what has been copied to them while the call ran, and the packets that were
    // in flight when their range was copied (their results are sent again by get_results)
    struct ResultStream {
        bool armed = false;        // destinations registered for the next propagate
        bool valid = false;        // the last propagate streamed: [0, upto) + the late list are (about to be) in the caller's arrays
        void *dst[16] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        long long upto = 0;        // packets [0, upto) were copied at launch boundaries
        long long n_late = 0;      // entries of the late list (may hold a packet more than once)
        unsigned late_capacity = 0;
        DevBuf late, late_count, vals;
        hipStream_t stream = nullptr;
        hipEvent_t ev = nullptr;
        unsigned long long *next_host = nullptr;  // pinned: the packet counter after a launch
        long long min_packets = 1000000;  // a range worth sixteen copies of its own (option stream_min_packets; tests lower it)
        void release() { release_buffers(late, late_count, vals); destroy_event(ev); destroy_stream(stream); free_pinned(next_host); }
    } rs;
    // source function of the formal integral (source_function.hpp).  Per set_opacity: the CSR indices {lines of every upper level}, {internal rows
    // ending in every level, with the level each leaves}, every line's emission row and its block (topo_error: a line with none or several), and
    // the exp(-tau) table shared with the formal integral.  Per call: the level vectors e / x[2], the gathered probabilities q, the outputs.
    struct SourceFunction {
        DevBuf lvl_ptr, lvl_line, in_ptr, in_row, in_src, emit_row, emit_level;
        bool topo_valid = false;
        std::string topo_error;
        long long nnz = 0;
        DevBuf exp_tau, e, x[2], q, shell, conv, wave, att, jred, jblue;
        bool exp_valid = false;
        bool valid = false;                     // the resident att_S_ul / Jred_lu / Jblue_lu belong to the resident estimators and tables
        const double *c_level = nullptr;        // with valid: the level rates [S][levels] of that source function (e, or the x the solve ended in)
        double *conv_host = nullptr;            // pinned: {max |dx|, max |x|} per shell
        long long max_iterations = 20000;   // option: bound on the iterations of a solve
        int last_iterations = -1;
        void release()
        {
            release_buffers(lvl_ptr, lvl_line, in_ptr, in_row, in_src, emit_row, emit_level, exp_tau, e, x, q, shell, conv, wave, att, jred, jblue);
            free_pinned(conv_host);
        }
    } sf;
    // tardis_mc_progress (another host thread polls while propagate blocks): the running call's packet count, whether its kernel hands
    // packets out through next_packet over the whole call (wave kernel), whether it is complete; a stream and a pinned word of its own
    struct Progress {
        std::atomic<long long> progress_total{0};
        std::atomic<bool> progress_wave{false}, progress_done{true};
        std::mutex progress_mutex;
        hipStream_t stream_progress = nullptr;
        hipEvent_t ev_progress_reset = nullptr;  // recorded behind the reset of next_packet at the start of a call
        unsigned long long *progress_host = nullptr;
        void release() { destroy_event(ev_progress_reset); destroy_stream(stream_progress); free_pinned(progress_host); }
    } pg;
    // Opacity update (opacity_update.hpp).  Per set_opacity: the host copies of the index tables and of the line list (ot.h_idx, ot.h_nu).  Per set_line_data: the static
    // line data and the list of the blocks that take the row form.  Per update_opacity: n_t[S][K], the [S] inputs, beta_t / sef_t / j_t [S][L].
    struct OpacityUpdate {
        DevBuf f_lu, wave, g_lower, g_upper, level_lower, level_upper, coef, long_blocks;
        DevBuf n_t, shell, beta_t, sef_t, j_t;
        std::vector<int> h_lower, h_upper;  // host copies of the line data's levels: what set_nlte_data checks its lines against
        bool have = false, have_coef = false, valid = false;  // (have: line data installed; valid: beta_t / sef_t / j_t belong to the resident tau_t / prob_t)
        long long levels = 0, n_long = 0, long_rows_built = -1;
        long long long_rows = -1;  // option opacity_update_long_rows: -1 the rule of opacity_update_plan.hpp, else the threshold itself
        double sobolev_coefficient = 0.0;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // start | behind the line kernel | behind the block kernels | end of the last update (tardis_mc_last_opacity_update_ms)
        bool timed = false;
        void release() { release_buffers(f_lu, wave, g_lower, g_upper, level_lower, level_upper, coef, long_blocks, n_t, shell, beta_t, sef_t, j_t); destroy_events(ev); }
    } ou;
    // Mean opacities (mean_opacity.hpp): a reader of the resident tables that keeps nothing but its events -- its buffers are scratch of the call.
    struct MeanOpacity {
        long long long_bins = -1;  // option mean_opacity_long_bins: -1 the rule of mean_opacity_plan.hpp, else the threshold itself
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // start | behind the bin kernel | behind the reduction and the final kernel (tardis_mc_last_mean_opacity_ms)
        bool timed = false;
        void release() { destroy_events(ev); }
    } mo;
    // Plasma update (plasma_update.hpp).  Per set_plasma_data: the atomic data of the levels and ions, the map level -> ion, the list of the ions that
    // take the row form of the partition kernel.  Per update_plasma: lbf_t[S][K]; Z, phi, N [I][S]; the solved n_e [S]; {status, passes}.
    struct PlasmaUpdate {
        DevBuf energy, g, meta, level_ion, ion_edge, elem_edge, charge, chi, zeta_t, zeta, density, long_ions;
        DevBuf lbf_t, z, phi, n_ion, n_e, status;
        std::vector<int> h_ion_edge, h_elem_edge;
        std::vector<double> h_charge;  // (with the edges: what set_ionization_options checks the helium element against)
        double t_min = 0.0, t_max = 0.0, chi_0 = 0.0, link = 0.0;
        bool have = false, valid = false, timed = false;  // (have: plasma data installed; valid: Z / N / n_e belong to the resident n_t)
        int ions = 0, elements = 0, nt = 0, iterations = 0;
        long long n_long = 0, long_rows_built = -2;
        long long long_rows = -1;         // option plasma_update_long_rows: -1 the rule of plasma_update_plan.hpp, else the threshold itself
        long long max_iterations = 1000;  // option plasma_max_iterations: bound on the passes of the electron-density iteration
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // start | Boltzmann | partition | ionisation | populations (tardis_mc_last_plasma_update_ms)
        void release() { release_buffers(energy, g, meta, level_ion, ion_edge, elem_edge, charge, chi, zeta_t, zeta, density, long_ions, lbf_t, z, phi, n_ion, n_e, status); destroy_events(ev); }
    } pl;
    // NLTE excitation (nlte_excitation.hpp).  Per set_nlte_data: the species (first level, levels, first row of x, line edges), the lines (their id in
    // the line list, local levels, Einstein coefficients) and, per value of option nlte_lds_levels, the launches: the LDS form per size class, the
    // global form with its slab offsets.  Per update_plasma: r_ul / r_lu [S][NL], x [S][NX], the status words [NS][S], the slabs, (mode 1) the shell work.
    struct NlteExcitation {
        DevBuf line_id, a_ul, b_ul, b_lu, lower, upper, sp_k0, sp_n, sp_x0, sp_line_edge, list, slab;
        DevBuf r_ul, r_lu, x_t, status, scratch, work;
        // the blocked form (nlte::plan_blocked): the global launch's species as [one-workgroup | blocked] with their slab offsets, and the
        // pivot rows of the blocked systems [S][NX]
        DevBuf form_list, form_slab, pivrow;
        std::vector<int> h_n, h_ion, h_status;
        std::vector<nlte::Launch> launches;
        std::vector<nlte::BlockedStep> steps;
        int n_single = 0, n_blocked = 0;
        long long blocked_levels = -1, blocked_built = -2;  // option nlte_blocked_levels: -1 the rule of nlte_plan.hpp, else the threshold itself
        bool have = false, valid = false, timed = false, ran = false;  // (have: NLTE data installed; valid: lbf_t and x are those of the last successful update's NLTE stage)
        int coronal = 0, classical = 0;
        long long species = 0, lines = 0, nx = 0, scratch_doubles = 0;
        long long lds_levels = -1, lists_built = -2;  // option nlte_lds_levels: -1 the rule of nlte_plan.hpp, else the threshold itself
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // start | rates | solve (tardis_mc_last_nlte_ms)
        void release() { release_buffers(line_id, a_ul, b_ul, b_lu, lower, upper, sp_k0, sp_n, sp_x0, sp_line_edge, list, slab, r_ul, r_lu, x_t, status, scratch, work, form_list, form_slab, pivrow); destroy_events(ev); }
    } nl;
    // Collisional rates of the NLTE species (nlte_excitation.hpp).  Per set_nlte_collision_data: the temperature grid, C_ul as [NT][NP], delta_e,
    // 1 / g_ratio, the pairs' local levels and the species' pair edges.  Per update_plasma: c_ul / c_lu [S][NP] (tardis_mc_get_nlte_collision_rates).
    struct NlteCollisions {
        DevBuf temperatures, c_t, delta_e, inv_g, lower, upper, sp_pair_edge, c_ul, c_lu;
        bool have = false, valid = false;  // (have: collision data installed; valid: c_ul / c_lu are those of the last successful update)
        long long pairs = 0, nt = 0;
        double t_first = 0.0, t_last = 0.0;
        void release() { release_buffers(temperatures, c_t, delta_e, inv_g, lower, upper, sp_pair_edge, c_ul, c_lu); }
    } nc;
    // The options of the ionisation stage (plasma_update.hpp).  Per set_ionization_options: the two switches and where helium sits in the plasma data.
    // Per update_plasma with helium_treatment: hp and v, [K_He][S] each (tardis_mc_get_helium).
    struct IonizationOptions {
        DevBuf hp, v;
        bool have = false, valid = false, timed = false, ran = false;  // (have: options installed; valid: hp / v are those of the last successful update)
        int helium = 0, fixed_delta = 0;
        double delta = 0.0;
        int element = 0, ion = 0, k0 = 0, n1 = 0, n2 = 0;  // helium's element row and first ion; its first level; levels of He I; of He I and He II together
        hipEvent_t ev[2] = {nullptr, nullptr};  // around helium_relative_kernel (tardis_mc_last_helium_ms)
        void release() { release_buffers(hp, v); destroy_events(ev); }
    } he;
    // Continuum stage (continuum_rates.hpp, continuum_opacity.hpp).  Per set_continuum_data: the continua's levels and ions, the block edges, the
    // points' continuum, nu, x_sect and the blocks' first and last frequencies.  Per update_plasma: t_e and the free-free factor [S], lbf_e [S][K],
    // Z_e [I][S], bfp and the three integrands [NP][S], the seven rate tables [7][NC][S], chi_bf [NP][S], the workgroups' clamp counts.
    struct ContinuumStage {
        DevBuf level, level_ion, block_edge, point_cont, nu, x_sect, nu_min, nu_max;
        DevBuf t_e, ff, lbf_e, z_e, bfp, y_sp, y_g, y_st, rates, chi_bf, counts;
        bool have = false, valid = false, timed = false, ran = false;  // (have: continuum data installed; valid: the tables are those of the last successful update)
        long long continua = 0, points = 0;
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // start | thermal | points | rates | opacity (tardis_mc_last_continuum_ms)
        void release() { release_buffers(level, level_ion, block_edge, point_cont, nu, x_sect, nu_min, nu_max, t_e, ff, lbf_e, z_e, bfp, y_sp, y_g, y_st, rates, chi_bf, counts); destroy_events(ev); }
    } ct;
    // Cooling sub-stage behind the continuum stage (cooling_rates.hpp, kpacket_sample.hpp), per update_plasma: the two integrands and the emission CDF
    // [NP][S], c_fb_sp / cool_rate_fb / cool_rate_coll_ion [3][NC][S], cool_rate_ff / adiabatic / total [3][S], k_cdf [2 + 2 NC][S], the workgroups'
    // counts of degenerate CDFs.  It has no flags of its own: it runs whenever the continuum stage runs, and ct.valid / ct.timed speak for both.
    struct CoolingStage {
        DevBuf y_cool, y_em, fb_cdf, rates, shell, k_cdf, counts;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // start | points | blocks | table (tardis_mc_last_cooling_ms)
        void release() { release_buffers(y_cool, y_em, fb_cdf, rates, shell, k_cdf, counts); destroy_events(ev); }
    } ck;
    // Photo-ionisation and heating estimators (bf_estimators.hpp).  Per set_bf_estimators: t_e [S] and the zeroed tables [5][NC][S] with {records, dropped}.
    // Per propagate call with the option on: the segment log's pool (records, keys, chunk fills, {pool_next, dropped}) and the pass's grouping
    // (bin counts / starts / fills / slice starts, the sorted slots).  Per bf_estimator_rates: gamma_est | stim_est [2][NC][S].
    struct BfEstimators {
        bool on = false;                                 // option bf_estimators
        long long seg_capacity = 0;                      // option segment_log_capacity: records (0: automatic, 96 per packet)
        long long seg_max_bytes = 16LL << 30;            // option segment_log_max_bytes: the bound on the log's device memory
        bool seg_keep = false;                           // option segment_log_keep (tests): tardis_mc_get_segment_log may read the last call's records
        int continuum_field = 0;                         // option continuum_field: 0 the dilute black body, 1 the estimators' rates
        DevBuf t_e, tables, totals, rates;
        DevBuf seg_recs, seg_keys, seg_fill, seg_state, seg_sorted, seg_bins;
        bool have = false, rates_valid = false, seg_valid = false, timed = false;
        long long seg_slots = 0;
        unsigned seg_n_chunks = 0;
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // start | grouped | accumulated (tardis_mc_last_bf_estimator_ms)
        void release() { release_buffers(t_e, tables, totals, rates, seg_recs, seg_keys, seg_fill, seg_state, seg_sorted, seg_bins); destroy_events(ev); }
    } bf;
    // RCCL
    void *comm = nullptr;
    int rank = 0, world = 1;
};

namespace {

int fail(TardisMcContext *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                                      \
    do {                                                                                                        \
        hipError_t _e = (expr);                                                                                 \
        if (_e != hipSuccess)                                                                                   \
            return fail(ctx, TARDIS_MC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                        __LINE__);                                                                              \
    } while (0)

// [rows, cols] row-major -> [cols, rows] row-major (tile through LDS so both sides are coalesced)
__global__ void transpose_kernel(const double *__restrict__ in, double *__restrict__ out, long long rows, long long cols)
{
    __shared__ double tile[32][33];
    long long bx = (long long)blockIdx.x * 32, by = (long long)blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += 8) {
        long long r = by + j, c = bx + threadIdx.x;
        if (r < rows && c < cols) tile[j][threadIdx.x] = in[r * cols + c];
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8) {
        long long c = bx + j, r = by + threadIdx.x;
        if (r < rows && c < cols) out[c * rows + r] = tile[threadIdx.x][j];
    }
}

// nt[s * stride + l] = {nu_line[l], tau_t[s][l]} (the interleaved sweep table).  The frequency slot of the LAST line of the list, of the entries past a row's L
// lines and of the slack behind the last row holds -inf: the lane sweep's lean no-stop proof fails there (X = +inf) and hands the line to the exact evaluation,
// which never reads the last line's frequency (its distance is MISS_DISTANCE) -- so the sweep needs no per-line test for the end of the list.  `negative` is
// raised if an optical depth is negative or NaN: the lean proof assumes tau >= 0 (the host then keeps such tables on the separate-table kernels).
__global__ void __launch_bounds__(256) interleave_kernel(const double *__restrict__ nu_line, const double *__restrict__ tau_t, double2 *__restrict__ nt,
                                                         long long L, long long S, long long stride, long long total, int *negative)
{
    bool neg = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long s = i / stride, l = i - s * stride;
        const bool in = s < S && l < L;
        const double tau = in ? tau_t[s * L + l] : 0.0;
        neg |= !(tau >= 0.0);
        nt[i] = make_double2((in && l < L - 1) ? nu_line[l] : -__builtin_inf(), tau);
    }
    if (neg) atomicOr(negative, 1);
}

// The block-skip tables (sweep_skip.hpp) from the interleaved table and the prefix sums, which tau_prefix_kernel has left in the second halves of pn:
// pn[s * (L + 1) + l] = {frequency slot of line l (-inf from L - 1 on), pfx[s][l]}, l = 0 .. L;
// ct[s * (stride / 8) + b] = {frequency slot of the last entry of block b, pfx[s][min(8 b + 8, L)]}; the slack behind the last row: {-inf, the last prefix sum}
__global__ void __launch_bounds__(256) coarse_table_kernel(const double2 *__restrict__ nt, double2 *__restrict__ pn, double2 *__restrict__ ct, long long L,
                                                           long long S, long long stride, long long total)
{
    const long long rows = stride / 8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long s = i / rows, b = i - s * rows;
        if (s < S) {
            const long long e = 8 * b + 8 < L ? 8 * b + 8 : L;
            ct[i] = make_double2(nt[s * stride + 8 * b + 7].x, pn[s * (L + 1) + e].y);
        } else
            ct[i] = make_double2(-__builtin_inf(), pn[(S - 1) * (L + 1) + L].y);
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < S * (L + 1); i += (long long)gridDim.x * blockDim.x) {
        const long long s = i / (L + 1), l = i - s * (L + 1);
        pn[i].x = l < L - 1 ? nt[s * stride + l].x : -__builtin_inf();
    }
}

// Stores a launch-argument block into device memory.  The value travels in the kernel's argument buffer, which the runtime
// copies when the launch is enqueued -- unlike hipMemcpyAsync from pageable host memory, nothing on the host has to stay
// alive or unchanged afterwards, so back-to-back propagate calls need no stream synchronisation between them.
template <typename T>
__global__ void store_value_kernel(T *dst, const T v)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v;
}
template <typename T>
hipError_t store_value(hipStream_t st, T *dst, const T &v)
{
    static_assert(sizeof(T) <= 3584, "argument block too large for the kernel-argument buffer");
    hipLaunchKernelGGL(store_value_kernel<T>, dim3(1), dim3(64), 0, st, dst, v);
    return hipGetLastError();
}
struct FirstErrorInit { long long v[2]; };

// sum private copies into copy 0 (in place)
__global__ void reduce_copies_kernel(double *base, long long n, long long stride, int copies)
{
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long step = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += step) {
        double s = base[i];
        for (int c = 1; c < copies; ++c) { s += base[i + c * stride]; base[i + c * stride] = 0.0; }
        base[i] = s;
    }
}

// diagnostics: element-wise device arithmetic for the numerics parity tests
__global__ void debug_eval_kernel(int op, const double *x, const double *y, double *out, long long n, uint32_t *scratch)
{
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (op == 7) {  // MT19937 stream of seed (uint32)x[0]
        if (i == 0) {
            mc::Rng rng;
            rng.seed(scratch, (uint32_t)x[0]);
            for (long long k = 0; k < n; ++k) out[k] = rng.random();
        }
        return;
    }
    if (i >= n) return;
    double a = x[i], b = y ? y[i] : 0.0, r;
    switch (op) {
    case 0: r = a + b; break;
    case 1: r = a * b; break;
    case 2: r = a / b; break;
    case 3: r = sqrt(a); break;
    case 4: r = mcm::log(a); break;
    case 5: r = mcm::exp(a); break;
    case 6: r = a * b + a; break;  // must NOT be contracted into an fma
    case 8: r = floor(a); break;
    case 9: r = ((mc::mid_range(a) || a == 0.0) && mc::mid_range(b)) ? mc::exact_div<true>(a, b, 1.0 / b) : a / b; break;
    default: r = 0.0;
    }
    out[i] = r;
}

// ---- micro-benchmarks of the memory system (design input; not part of the product path)
// which: 0 random fp64 atomic add, agent scope; 1 same, workgroup scope inside a per-XCD private slice;
//        2 fp64 atomic add, 16 consecutive doubles per 16-lane group, agent scope; 3 same, workgroup scope/XCD slice;
//        4 random 8-byte loads; 5 16-lane-coalesced 8-byte loads;
//        6..9 every lane reads its own random, naturally aligned block of 16 / 32 / 64 / 128 bytes (dwordx4 loads);
//        10 dependent chain: the address of a lane's next random 8-byte load comes out of the loaded value (latency);
//        11 / 12 lane-private vs quad-shared 64-byte blocks (see below)
//        13 / 14 packet hand-over through binned queues, 128- / 64-byte records (see below)
__global__ void microbench_kernel(int which, double *table, long long n, int iters, double *sink)
{
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long st = 0x9E3779B97F4A7C15ull * (unsigned long long)(gtid + 1);
    const int lane16 = threadIdx.x & 15;
    const bool xcd_slice = (which == 1 || which == 3);
    long long span = n, base0 = 0;
    if (xcd_slice) { span = n / 8; base0 = span * (mc::xcc_id() & 7); }
    double acc = 0.0;
    if (which >= 6 && which <= 9) {
        typedef double v2d __attribute__((ext_vector_type(2)));
        const int quads = 1 << (which - 6);  // 16-byte pieces per block
        const unsigned long long n_blocks = (unsigned long long)n / (2ull * quads);
        for (int it = 0; it < iters; ++it) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            const v2d *b = reinterpret_cast<const v2d *>(table) + ((st >> 20) % n_blocks) * quads;
            v2d v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) if (q < quads) v[q] = b[q];
#pragma unroll
            for (int q = 0; q < 8; ++q) if (q < quads) acc += v[q].x + v[q].y;
        }
    } else if (which == 11 || which == 12) {
        // 11: every lane reads its own random 64-byte block with four 16-byte loads (the lane sweeps' pattern);
        // 12: the same blocks, but the four lanes of a quad read ONE block per instruction, lane j its j-th 16 bytes, four
        //     instructions for the quad's four blocks (same bytes, same lines; fewer distinct lines per instruction)
        typedef double v2d __attribute__((ext_vector_type(2)));
        const unsigned long long n_blocks = (unsigned long long)n / 8ull;
        const int lane = threadIdx.x & 63, j = lane & 3;
        for (int it = 0; it < iters; ++it) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            const unsigned long long mine = (st >> 20) % n_blocks;
            v2d v[4];
            if (which == 11) {
                const v2d *b = reinterpret_cast<const v2d *>(table) + mine * 4;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = b[q];
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned lo = (unsigned)__shfl((int)(unsigned)mine, (lane & ~3) + q, 64), hi = (unsigned)__shfl((int)(unsigned)(mine >> 32), (lane & ~3) + q, 64);
                    const unsigned long long blk = ((unsigned long long)hi << 32) | lo;
                    v[q] = (reinterpret_cast<const v2d *>(table) + blk * 4)[j];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc += v[q].x + v[q].y;
        }
    } else if (which == 13 || which == 14) {
        // packet hand-over through binned queues (what re-binning the lanes of a wave by (shell, line tile) would cost per event,
        // profiles/r04_locality.txt): a lane appends its packet -- a 128-byte (13) or 64-byte (14) record -- to the queue of a
        // random one of 4900 bins (one returning atomic on the bin's cursor, 16-byte stores), and takes over a packet from a
        // random slot of another bin (16-byte loads).  table = [4900 cursors | 4900 queues of `cap` records].
        typedef double v2d __attribute__((ext_vector_type(2)));
        const int rec_v2 = which == 13 ? 8 : 4;  // 16-byte pieces per record
        const unsigned long long n_bins = 4900ull;
        const unsigned long long cap = ((unsigned long long)n - 8192ull) / (n_bins * 2ull * (unsigned long long)rec_v2);
        unsigned long long *cursor = reinterpret_cast<unsigned long long *>(table);
        v2d *queues = reinterpret_cast<v2d *>(table + 8192);
        for (int it = 0; it < iters; ++it) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            const unsigned long long b_out = (st >> 20) % n_bins, b_in = (st >> 40) % n_bins;
            const unsigned long long slot = __hip_atomic_fetch_add(&cursor[b_out], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) % cap;
            v2d *dst = queues + (b_out * cap + slot) * rec_v2;
            const v2d rec = {acc, (double)it};
#pragma unroll
            for (int q = 0; q < 8; ++q) if (q < rec_v2) dst[q] = rec;
            const v2d *src = queues + (b_in * cap + (st >> 7) % cap) * rec_v2;
            v2d v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) if (q < rec_v2) v[q] = src[q];
#pragma unroll
            for (int q = 0; q < 8; ++q) if (q < rec_v2) acc += v[q].x + v[q].y;
        }
    } else if (which == 10) {
        unsigned long long r = st >> 20;
        for (int it = 0; it < iters; ++it) {
            const double v = table[(long long)(r % (unsigned long long)span)];
            r = r * 6364136223846793005ull + 1442695040888963407ull + (unsigned long long)__double_as_longlong(v);
            acc += v;
        }
    } else
    for (int it = 0; it < iters; ++it) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        unsigned long long r = st >> 20;
        long long idx;
        if (which == 2 || which == 3 || which == 5) {
            unsigned long long rg = __shfl(r, threadIdx.x & ~15, 64);  // group-uniform random base
            idx = base0 + (long long)((rg % (unsigned long long)(span / 16)) * 16) + lane16;
        } else
            idx = base0 + (long long)(r % (unsigned long long)span);
        if (which == 0 || which == 2) __hip_atomic_fetch_add(&table[idx], 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (which == 1 || which == 3) __hip_atomic_fetch_add(&table[idx], 1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else acc += table[idx];
    }
    if (acc == 123.456) sink[0] = acc;
}

// which = 15: the box's streaming rate -- a wide coalesced copy of the table's first half onto its second (16 bytes per lane and access, grid-stride):
// n_doubles x 8 bytes cross the memory interface per pass (half read, half written); bench.py reports it as roofline.peak_measured
__global__ void __launch_bounds__(256) stream_copy_kernel(double *table, long long n, int iters)
{
    typedef double v2d __attribute__((ext_vector_type(2)));
    const long long half = (n / 4) * 2;  // doubles per half, whole 16-byte pieces
    const v2d *__restrict__ src = reinterpret_cast<const v2d *>(table);
    v2d *__restrict__ dst = reinterpret_cast<v2d *>(table + half);
    const long long pieces = half / 2, step = (long long)gridDim.x * blockDim.x;
    for (int it = 0; it < iters; ++it) {
        long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
        for (; i + 3 * step < pieces; i += 4 * step) {  // four 16-byte pieces in flight per lane
            const v2d a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + step);
            const v2d c = __builtin_nontemporal_load(src + i + 2 * step), d = __builtin_nontemporal_load(src + i + 3 * step);
            __builtin_nontemporal_store(a, dst + i); __builtin_nontemporal_store(b, dst + i + step);
            __builtin_nontemporal_store(c, dst + i + 2 * step); __builtin_nontemporal_store(d, dst + i + 3 * step);
        }
        for (; i < pieces; i += step) dst[i] = src[i];
    }
}

// ---- real-packet spectrum and filtered luminosities from the resident per-packet outputs
// (SpectrumSolver.montecarlo_emitted/reabsorbed_luminosity, tardis/spectrum/base.py:140-159: np.histogram with the
//  spectrum_frequency_grid edges, weights = +/- output_energies / time_of_simulation split on output_energies >= 0
//  (montecarlo_transport_state.py:130-160); calculate_filtered_luminosity, tardis/spectrum/luminosity.py:5-30)
__global__ void spectrum_kernel(const double *__restrict__ out_nu, const double *__restrict__ out_e, long long n,
                                const double *__restrict__ edges, int n_edges, double t_sim, double nu_start, double nu_end,
                                double *hist_emitted, double *hist_reabsorbed, double *lum /* [2] */)
{
    const int B = n_edges - 1;
    const double e0 = edges[0], eN = edges[B];
    const double inv_delta = (double)B / (eN - e0);
    double lum_e = 0.0, lum_r = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double e = out_e[i], nu = out_nu[i];
        const bool emitted = e >= 0;
        const double l = emitted ? (e / t_sim) : -(e / t_sim);
        if (nu > nu_start && nu < nu_end) { if (emitted) lum_e += l; else lum_r += l; }
        const int k = mc::spectrum_bin(edges, B, e0, eN, inv_delta, nu);  // numpy.histogram's bin, -1 outside the grid
        if (k >= 0) mc::atomic_add_f64(emitted ? &hist_emitted[k] : &hist_reabsorbed[k], l);
    }
    // block reduction of the two luminosity sums
    __shared__ double sh[2][256];
    sh[0][threadIdx.x] = lum_e; sh[1][threadIdx.x] = lum_r;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { sh[0][threadIdx.x] += sh[0][threadIdx.x + s]; sh[1][threadIdx.x] += sh[1][threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { mc::atomic_add_f64(&lum[0], sh[0][0]); mc::atomic_add_f64(&lum[1], sh[1][0]); }
}

// ---- radiation-field update from the resident estimators (MCRadiationFieldPropertiesSolver.solve,
// tardis/transport/montecarlo/estimators/mc_rad_field_solver.py:37-144; intensity_black_body, tardis/util/base.py:279-302)
struct RadFieldConsts { double t_rad_const, four_sigma, jblue_norm_num, four_pi_tsim, tsim, planck_coef, h, k_b, w_epsilon, c_ang; };

__global__ void radfield_shell_kernel(const double *J, const double *nubar, const double *volume, int S, RadFieldConsts k,
                                      double *t_rad, double *w, double *norm)
{
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double t = k.t_rad_const * nubar[s] / J[s];
    t_rad[s] = t;
    const double t2 = t * t;
    w[s] = J[s] / (k.four_sigma * (t2 * t2) * k.tsim * volume[s]);
    norm[s] = k.jblue_norm_num / (k.four_pi_tsim * volume[s]);
}

__global__ void radfield_jblue_kernel(const double *__restrict__ jblue_t, const double *__restrict__ nu_line,
                                      const double *__restrict__ t_rad, const double *__restrict__ w,
                                      const double *__restrict__ norm, int S, long long L, RadFieldConsts k, int optical_window,
                                      double *__restrict__ out_t)
{
    const int s = blockIdx.y;
    const double beta = 1 / (k.k_b * t_rad[s]), ws = w[s], ns = norm[s];
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < L; l += (long long)gridDim.x * blockDim.x) {
        out_t[(long long)s * L + l] = mc::detailed_j_blue(jblue_t[(long long)s * L + l], ns, nu_line[l], ws, beta, k.planck_coef, k.h, k.w_epsilon, k.c_ang, optical_window);
    }
}

hipError_t launch_transpose(hipStream_t s, const double *in, double *out, long long rows, long long cols)
{
    dim3 block(32, 8), grid((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32));
    hipLaunchKernelGGL(transpose_kernel, grid, block, 0, s, in, out, rows, cols);
    return hipGetLastError();
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct EstLayout { size_t J, nubar, vhist, jblue, edot, copy_stride, reduce_elems, total; };
EstLayout est_layout(size_t S, size_t L, size_t G, int copies)
{
    EstLayout e;
    e.J = 0;
    e.nubar = S;
    e.vhist = 2 * S;
    size_t head = align_up(2 * S + G, 32);
    e.jblue = head;
    e.edot = head + S * L;
    e.copy_stride = 2 * S * L;             // distance between copy c and c+1 of the same table
    e.reduce_elems = head + 2 * S * L;     // contiguous range that is all-reduced (copy 0)
    e.total = head + (size_t)copies * 2 * S * L;
    return e;
}

int ensure_estimators(TardisMcContext *ctx)
{
    if (!ctx->have_opacity || !ctx->have_config) return TARDIS_MC_OK;
    size_t S = ctx->n_shells, L = ctx->n_lines, G = (size_t)ctx->cfg.n_spectrum_grid;
    if (ctx->es.est_valid && ctx->es.est_S == S && ctx->es.est_L == L && ctx->es.est_G == G) return TARDIS_MC_OK;
    EstLayout e = est_layout(S, L, G, ctx->es.est_copies);
    HIP_TRY(ctx, ctx->es.est.ensure(e.total * sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->es.est.p, 0, e.total * sizeof(double), ctx->stream));
    ctx->es.est_S = S; ctx->es.est_L = L; ctx->es.est_G = G;
    ctx->es.est_valid = true;
    ctx->es.est_propagated = false;
    return TARDIS_MC_OK;
}

template <typename T>
int upload(TardisMcContext *ctx, DevBuf &buf, const T *host, size_t n)
{
    HIP_TRY(ctx, buf.ensure(n * sizeof(T)));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return TARDIS_MC_OK;
}

// ---- boundary copies between the caller's (pageable) arrays and HBM: plain hipMemcpy.  (Round 6 measured a pipeline of its own -- four worker threads, each with a
// stream and two pinned 8-MB buffers -- against it: no gain, 29.7 vs 31.6 ms for the 1.28 GB of per-packet results of a 1e7-packet call, 10-26 vs 9.6 ms for the
// packet upload; the runtime's own staging already runs at ~40-50 GB/s once the destination pages exist.  What did cost 160 ms of that call was on the Python side:
// fresh tracker arrays allocated, page-faulted and copied once more into the caller's -- Engine.get_results now writes into the caller's arrays;
// profiles/r06_boundary.txt.)
struct CopyJob { void *host; void *dev; size_t bytes; };

hipError_t host_copy(TardisMcContext *ctx, const std::vector<CopyJob> &jobs, bool to_device)
{
    (void)ctx;
    for (const CopyJob &j : jobs) {
        if (!j.host || !j.dev || !j.bytes) continue;
        hipError_t e = to_device ? hipMemcpy(j.dev, j.host, j.bytes, hipMemcpyHostToDevice) : hipMemcpy(j.host, j.dev, j.bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// A table kept shell-major on the device, [S][rows], into the caller's [rows, S] through the staging buffer (host null: nothing to do)
int download_transposed(TardisMcContext *ctx, double *host, const double *table_t, size_t rows)
{
    if (!host) return TARDIS_MC_OK;
    const size_t S = (size_t)ctx->n_shells;
    HIP_TRY(ctx, ctx->staging.ensure(rows * S * sizeof(double)));
    HIP_TRY(ctx, launch_transpose(ctx->stream, table_t, ctx->staging.as<double>(), (long long)S, (long long)rows));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, host_copy(ctx, {{(void *)host, ctx->staging.p, rows * S * sizeof(double)}}, false));
    return TARDIS_MC_OK;
}

// the events of a stage: made on first use; read as the milliseconds between neighbours, out[k] (may be null) = ev[k] .. ev[k + 1] for k < n
template <size_t N>
int ensure_events(TardisMcContext *ctx, hipEvent_t (&ev)[N])
{
    for (hipEvent_t &e : ev)
        if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    return TARDIS_MC_OK;
}
int event_intervals_ms(TardisMcContext *ctx, const hipEvent_t *ev, int n, double *const *out)
{
    HIP_TRY(ctx, hipEventSynchronize(ev[n]));
    for (int k = 0; k < n; ++k) {
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        if (out[k]) *out[k] = ms;
    }
    return TARDIS_MC_OK;
}

// tardis/constants.py:1 (CODATA 2010, cgs), for the host side of the radiation field and of the opacity / plasma / NLTE updates; c is mc::C_LIGHT
constexpr double H_PLANCK = 6.62606957e-27, K_BOLTZMANN = 1.3806488e-16, M_ELECTRON = 9.10938291e-28;

// The resident stages of the plasma chain sit on a ladder of installed data: opacity state -> line data -> plasma data -> NLTE data -> collision data,
// every rung in the indices of the one above it.  Whoever replaces a rung (set_opacity: what the first rung sits on) drops it and every rung below it --
// what is installed (`have`) and what the last update computed from it (`valid`).  This is the only place that knows the order; a new stage adds its rung.
enum Rung { RUNG_LINE_DATA, RUNG_PLASMA_DATA, RUNG_NLTE_DATA, RUNG_COLLISION_DATA };
void drop_from(TardisMcContext *ctx, Rung rung)
{
    switch (rung) {
    case RUNG_LINE_DATA: ctx->ou.have = ctx->ou.valid = false; [[fallthrough]];
    case RUNG_PLASMA_DATA: ctx->pl.have = ctx->pl.valid = false; ctx->he.have = ctx->he.valid = false; ctx->ct.have = ctx->ct.valid = false; ctx->bf.have = ctx->bf.rates_valid = false; [[fallthrough]];  // (the ionisation options and the continuum data sit beside the NLTE data, on the plasma data; the photo-ionisation estimators on the continuum data)
    case RUNG_NLTE_DATA: ctx->nl.have = ctx->nl.valid = false; [[fallthrough]];
    case RUNG_COLLISION_DATA: ctx->nc.have = ctx->nc.valid = false;
    }
}

// The same for the transport side: which resident product is computed from which input.  Whoever replaces or changes an input names the cause, and every
// product computed from it loses its flag here and nowhere else; a flag is set where its product is built.
//   source function (sf.valid)                      <- geometry, opacity tables, estimators
//   its topology (sf.topo_valid)                    <- opacity topology
//   exp(-tau), screening prefix sums, sweep table   <- optical depths          (sf.exp_valid, sc.pfx_valid, sw.nt_valid: rebuilt lazily by their first user)
//   walk tables, hot sectors                        <- transition probabilities (wt.have_walk_tables, wt.have_hot: rebuilt by derive_opacity_tables itself)
//   per-packet results (pk.li_valid)                <- packets
//   v-packet log (vl.vl_valid, vl.vl_consolidated)  <- packets, configuration
//   event log, streamed results                     <- the propagate call that wrote them (el.ev_valid, rs.valid; the readers compare the packet count too)
enum Cause {
    GEOMETRY_REPLACED,          // tardis_mc_set_geometry
    OPACITY_TOPOLOGY_REPLACED,  // tardis_mc_set_opacity, before it validates: a refused call drops the source function too
    OPACITY_UPDATE_BEGINS,      // tardis_mc_update_opacity, the install stage of tardis_mc_update_plasma: tau_t / prob_t are about to be overwritten in place
    OPACITY_VALUES_REPLACED,    // derive_opacity_tables: set_opacity, update_opacity, update_plasma
    ESTIMATORS_CHANGED,         // tardis_mc_reset_estimators, tardis_mc_allreduce_estimators, the start of tardis_mc_source_function
    CONFIG_REPLACED,            // tardis_mc_set_config
    PACKETS_REPLACED,           // tardis_mc_set_packets, tardis_mc_create_blackbody_packets
    PROPAGATE_BEGINS            // tardis_mc_propagate
};
void drop_products(TardisMcContext *ctx, Cause cause)
{
    switch (cause) {
    case GEOMETRY_REPLACED:
    case OPACITY_UPDATE_BEGINS:
    case ESTIMATORS_CHANGED: ctx->sf.valid = false; break;
    case OPACITY_TOPOLOGY_REPLACED: ctx->sf.valid = ctx->sf.topo_valid = ctx->sf.exp_valid = false; break;
    case OPACITY_VALUES_REPLACED:
        ctx->sf.valid = ctx->sf.exp_valid = false;
        ctx->wt.have_walk_tables = ctx->wt.have_hot = false;
        ctx->sc.pfx_valid = false;  // (the prefix sums of the new tau table are built by the first propagate call that traces v-packets)
        ctx->sw.nt_valid = false;   // (likewise the interleaved sweep table: by the first call that sweeps on it)
        ctx->sw.sk_valid = false;   // (... and the block-skip tables behind it)
        break;
    case CONFIG_REPLACED: ctx->vl.vl_valid = ctx->vl.vl_consolidated = false; break;  // (the consolidated v-packet log belongs to the configuration it was written under)
    case PACKETS_REPLACED:
        ctx->pk.li_valid = false;  // (the resident results are no longer those of the resident packets)
        ctx->vl.vl_valid = ctx->vl.vl_consolidated = false;
        break;
    case PROPAGATE_BEGINS:
        ctx->el.ev_valid = ctx->pk.li_valid = ctx->sf.valid = ctx->rs.valid = ctx->bf.seg_valid = false;
        ctx->vl.vl_valid = ctx->vl.vl_consolidated = false;
        break;
    }
}

// the sixteen per-packet result arrays on the device / in a TardisMcResult, in one order: out_nu, out_e, nine tracker doubles, five tracker integers
void per_packet_device_arrays(TardisMcContext *ctx, void *dev[16])
{
    dev[0] = ctx->pk.out_nu.p; dev[1] = ctx->pk.out_e.p;
    for (int k = 0; k < 9; ++k) dev[2 + k] = ctx->pk.track ? ctx->pk.li_f64[k].p : nullptr;
    for (int k = 0; k < 5; ++k) dev[11 + k] = ctx->pk.track ? ctx->pk.li_i64[k].p : nullptr;
}
void per_packet_host_arrays(const TardisMcResult *r, void *host[16])
{
    host[0] = r->output_nus; host[1] = r->output_energies;
    double *f[] = {r->li_radius, r->li_nu, r->li_energy, r->li_before_nu, r->li_before_mu, r->li_before_energy, r->li_after_nu, r->li_after_mu, r->li_after_energy};
    for (int k = 0; k < 9; ++k) host[2 + k] = f[k];
    int64_t *g[] = {r->li_shell_id, r->li_interaction_type, r->li_line_absorb_id, r->li_line_emit_id, r->li_interactions_count};
    for (int k = 0; k < 5; ++k) host[11 + k] = g[k];
}

__global__ void __launch_bounds__(256) narrow_seeds_kernel(const long long *__restrict__ in, long long n, uint32_t *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t)in[i];
}

// whether the propagate call being set up writes the last-interaction columns of the v-packet log (option vpacket_last_interaction):
// such a call runs the VLI instantiations of the kernels
bool vlog_li_call(const TardisMcContext *ctx)
{
    return ctx->vl.vlog_li && ctx->cfg.enable_vpacket_tracking && ctx->cfg.number_of_vpackets > 0 && ctx->vl.vlog_capacity > 0;
}

mc::DeviceProblem make_device_problem(TardisMcContext *ctx)
{
    mc::DeviceProblem P{};
    P.n_packets = ctx->pk.n_packets;
    P.r0 = ctx->pk.r0.as<double>(); P.mu0 = ctx->pk.mu0.as<double>(); P.nu0 = ctx->pk.nu0.as<double>(); P.e0 = ctx->pk.e0.as<double>();
    P.seeds = ctx->pk.seeds.as<uint32_t>();
    P.out_nu = ctx->pk.out_nu.as<double>(); P.out_e = ctx->pk.out_e.as<double>();
    if (ctx->pk.track) {
        double **f[] = {&P.li_radius, &P.li_nu, &P.li_energy, &P.li_before_nu, &P.li_before_mu, &P.li_before_energy,
                        &P.li_after_nu, &P.li_after_mu, &P.li_after_energy};
        for (int k = 0; k < 9; ++k) *f[k] = ctx->pk.li_f64[k].as<double>();
        long long **g[] = {&P.li_shell_id, &P.li_interaction_type, &P.li_line_absorb_id, &P.li_line_emit_id,
                           &P.li_interactions_count};
        for (int k = 0; k < 5; ++k) *g[k] = ctx->pk.li_i64[k].as<long long>();
        P.li_rec = ctx->pk.li_rec.as<uint4>();
    }
    if (ctx->el.track_full || ctx->bf.on) P.li_rec = ctx->pk.li_rec.as<uint4>();  // (the tracked wave kernel counts rows with the tracker, TRACK on)
    P.n_shells = ctx->n_shells;
    P.r_inner = ctx->r_inner.as<double>(); P.r_outer = ctx->r_outer.as<double>();
    P.t_exp = ctx->t_exp;
    P.n_lines = ctx->n_lines; P.n_trans = ctx->n_trans;
    P.nu_line = ctx->ot.nu_line.as<double>(); P.tau_t = ctx->ot.tau_t.as<double>(); P.n_e = ctx->ot.n_e.as<double>();
    P.prob_t = ctx->ot.prob_t.as<double>();
    P.line2level = ctx->ot.line2level.as<int>(); P.block_edge = ctx->ot.block_edge.as<int>(); P.ttype = ctx->ot.ttype.as<int>();
    P.dest = ctx->ot.dest.as<int>(); P.tline = ctx->ot.tline.as<int>();
    EstLayout e = est_layout(ctx->es.est_S, ctx->es.est_L, ctx->es.est_G, ctx->es.est_copies);
    double *base = ctx->es.est.as<double>();
    P.J = base + e.J; P.nubar = base + e.nubar; P.vhist = base + e.vhist;
    P.jblue_t = base + e.jblue; P.edot_t = base + e.edot;
    P.est_copy_stride = (long long)e.copy_stride;
    P.n_est_copies = ctx->es.est_copies;
    const TardisMcConfig &c = ctx->cfg;
    P.line_interaction_type = c.line_interaction_type;
    P.disable_line_scattering = c.disable_line_scattering;
    P.n_vpackets = c.number_of_vpackets;
    P.survival_probability = c.survival_probability;
    P.tau_russian = c.vpacket_tau_russian;
    P.spawn_start = c.vpacket_spawn_start_frequency;
    P.spawn_end = c.vpacket_spawn_end_frequency;
    P.sigma_thomson = c.sigma_thomson;
    P.grid = ctx->grid.as<double>();
    P.n_grid = (int)c.n_spectrum_grid;
    if (c.n_spectrum_grid >= 2) {
        P.grid0 = ctx->grid_host[0];
        P.grid_last = ctx->grid_host[c.n_spectrum_grid - 1];
        P.delta_nu = ctx->grid_host[1] - ctx->grid_host[0];
    }
    if (c.enable_vpacket_tracking && c.number_of_vpackets > 0 && ctx->vl.vlog_capacity > 0) {
        P.vlog_count = ctx->vl.vlog_count.as<unsigned long long>();
        P.vlog_capacity = ctx->vl.vlog_capacity;
        P.vlog_packet = ctx->vl.vlog_packet.as<long long>(); P.vlog_seq = ctx->vl.vlog_seq.as<int>();
        P.vlog_nu = ctx->vl.vlog_nu.as<double>(); P.vlog_energy = ctx->vl.vlog_energy.as<double>();
        P.vlog_mu = ctx->vl.vlog_mu.as<double>(); P.vlog_r = ctx->vl.vlog_r.as<double>();
    }
    P.rng_state = ctx->rng_state.as<uint32_t>();
    P.counters = ctx->counters.as<unsigned long long>();
    P.first_error = ctx->first_error.as<long long>();
    P.next_packet = ctx->next_packet.as<unsigned long long>();
    P.debug_flags = ctx->debug_flags;
    return P;
}

// ---- The kernel tables: every instantiation of the three propagation kernels that exists, keyed by its template arguments (in their order).
// A call computes its key once and looks the kernel up; a key that is not in its table is a programming error, which the lookup reports.
struct LaneKernelKey { bool full, vpk, track, full_tracking, vli; };  // (vli: option vpacket_last_interaction; rows that leave it out: false)
struct GroupKernelKey { bool full, track; int width, block, occupancy; bool vpk, wide, vli; };
struct WaveKernelKey {
    bool full, track;
    int width;  // lanes per sweep worker
    bool vpk, lane_sweep, xwalk;
    int waves_per_simd, nt;  // the register budget | the interleaved sweep table: 0 none, 1 runs from the current line, 2 aligned runs
    bool shell_log, full_tracking, wide;  // (wide: 64-bit table offsets)
    bool vli;  // the v-packet log with last interactions (option vpacket_last_interaction)
};
bool operator==(const LaneKernelKey &a, const LaneKernelKey &b) { return a.full == b.full && a.vpk == b.vpk && a.track == b.track && a.full_tracking == b.full_tracking && a.vli == b.vli; }
bool operator==(const GroupKernelKey &a, const GroupKernelKey &b)
{
    return a.full == b.full && a.track == b.track && a.width == b.width && a.block == b.block && a.occupancy == b.occupancy && a.vpk == b.vpk && a.wide == b.wide && a.vli == b.vli;
}
bool operator==(const WaveKernelKey &a, const WaveKernelKey &b)
{
    return a.full == b.full && a.track == b.track && a.width == b.width && a.vpk == b.vpk && a.lane_sweep == b.lane_sweep && a.xwalk == b.xwalk &&
           a.waves_per_simd == b.waves_per_simd && a.nt == b.nt && a.shell_log == b.shell_log && a.full_tracking == b.full_tracking && a.wide == b.wide && a.vli == b.vli;
}
using LaneKernelFn = void (*)(mc::DeviceProblem);
using GroupKernelFn = void (*)(mc::GroupArgs, uint32_t *, long long, long long);
using WaveKernelFn = void (*)(mc::WaveHot, const mc::WaveCold *);
template <typename Key, typename Fn> struct KernelRow { Key key; Fn fn; };
template <typename Key, typename Fn, size_t N>
Fn find_kernel(const KernelRow<Key, Fn> (&table)[N], const Key &key)
{
    for (const auto &row : table)
        if (row.key == key) return row.fn;
    return nullptr;
}
#define KROW(KERNEL, ...) {{__VA_ARGS__}, mc::propagate_##KERNEL##_kernel<__VA_ARGS__>}
const KernelRow<LaneKernelKey, LaneKernelFn> LANE_KERNELS[] = {  // FULL, VPK, TRACK, FT
    // (the second half: full r-packet tracking)
    KROW(lane, 0, 0, 0, 0), KROW(lane, 0, 0, 1, 0), KROW(lane, 0, 1, 0, 0), KROW(lane, 0, 1, 1, 0),
    KROW(lane, 1, 0, 0, 0), KROW(lane, 1, 0, 1, 0), KROW(lane, 1, 1, 0, 0), KROW(lane, 1, 1, 1, 0),
    KROW(lane, 0, 0, 0, 1), KROW(lane, 0, 0, 1, 1), KROW(lane, 0, 1, 0, 1), KROW(lane, 0, 1, 1, 1),
    KROW(lane, 1, 0, 0, 1), KROW(lane, 1, 0, 1, 1), KROW(lane, 1, 1, 0, 1), KROW(lane, 1, 1, 1, 1),
    // the v-packet log with last interactions (vpacket_last_interaction): v-packets and a tracker -- TRACK, or full tracking
    KROW(lane, 0, 1, 1, 0, 1), KROW(lane, 1, 1, 1, 0, 1), KROW(lane, 0, 1, 0, 1, 1), KROW(lane, 0, 1, 1, 1, 1), KROW(lane, 1, 1, 0, 1, 1), KROW(lane, 1, 1, 1, 1, 1),
};
const KernelRow<GroupKernelKey, GroupKernelFn> GROUP_KERNELS[] = {  // FULL, TRACK, G, BLOCK, OCC, VPK, WIDE
    // (the second half: 64-bit table offsets)
    KROW(group, 0, 0, 8, 256, 4, 0, 0), KROW(group, 0, 1, 8, 256, 4, 0, 0), KROW(group, 1, 0, 8, 256, 4, 0, 0), KROW(group, 1, 1, 8, 256, 4, 0, 0),
    KROW(group, 0, 0, 16, 256, 4, 0, 0), KROW(group, 0, 1, 16, 256, 4, 0, 0), KROW(group, 1, 0, 16, 256, 4, 0, 0), KROW(group, 1, 1, 16, 256, 4, 0, 0),
    KROW(group, 0, 0, 8, 256, 4, 1, 0), KROW(group, 0, 1, 8, 256, 4, 1, 0), KROW(group, 1, 0, 8, 256, 4, 1, 0), KROW(group, 1, 1, 8, 256, 4, 1, 0),
    KROW(group, 0, 0, 16, 256, 4, 1, 0), KROW(group, 0, 1, 16, 256, 4, 1, 0), KROW(group, 1, 0, 16, 256, 4, 1, 0), KROW(group, 1, 1, 16, 256, 4, 1, 0),
    KROW(group, 0, 0, 8, 256, 4, 0, 1), KROW(group, 0, 1, 8, 256, 4, 0, 1), KROW(group, 1, 0, 8, 256, 4, 0, 1), KROW(group, 1, 1, 8, 256, 4, 0, 1),
    KROW(group, 0, 0, 16, 256, 4, 0, 1), KROW(group, 0, 1, 16, 256, 4, 0, 1), KROW(group, 1, 0, 16, 256, 4, 0, 1), KROW(group, 1, 1, 16, 256, 4, 0, 1),
    KROW(group, 0, 0, 8, 256, 4, 1, 1), KROW(group, 0, 1, 8, 256, 4, 1, 1), KROW(group, 1, 0, 8, 256, 4, 1, 1), KROW(group, 1, 1, 8, 256, 4, 1, 1),
    KROW(group, 0, 0, 16, 256, 4, 1, 1), KROW(group, 0, 1, 16, 256, 4, 1, 1), KROW(group, 1, 0, 16, 256, 4, 1, 1), KROW(group, 1, 1, 16, 256, 4, 1, 1),
    // the v-packet log with last interactions (vpacket_last_interaction): the tracked v-packet instantiations again
    KROW(group, 0, 1, 8, 256, 4, 1, 0, 1), KROW(group, 1, 1, 8, 256, 4, 1, 0, 1), KROW(group, 0, 1, 16, 256, 4, 1, 0, 1), KROW(group, 1, 1, 16, 256, 4, 1, 0, 1), KROW(group, 0, 1, 8, 256, 4, 1, 1, 1), KROW(group, 1, 1, 8, 256, 4, 1, 1, 1), KROW(group, 0, 1, 16, 256, 4, 1, 1, 1), KROW(group, 1, 1, 16, 256, 4, 1, 1, 1),
};
const KernelRow<WaveKernelKey, WaveKernelFn> WAVE_KERNELS[] = {  // FULL, TRACK, G, VPK, LS, XWALK, WPE, NT, SL, FT, WIDE
    // (XWALK: the instantiations with the macro-atom walks on the fp64 running sums compiled in -- only launched when the compact
    // walk tables are not used: debug flags 128 / 8192, tables too large; the production ones are 22 % shorter without them)
    // group sweeps, sweep width 4 / 8 / 16; XWALK: with the macro-atom walks on the fp64 running sums compiled in (cross-checks, no compact walk tables)
    KROW(wave, 0, 0, 4, 0, 0, 0, 4, 0, 0, 0, 0), KROW(wave, 0, 1, 4, 0, 0, 0, 4, 0, 0, 0, 0), KROW(wave, 1, 0, 4, 0, 0, 0, 4, 0, 0, 0, 0), KROW(wave, 1, 1, 4, 0, 0, 0, 4, 0, 0, 0, 0),
    KROW(wave, 0, 0, 8, 0, 0, 0, 4, 0, 0, 0, 0), KROW(wave, 0, 1, 8, 0, 0, 0, 4, 0, 0, 0, 0), KROW(wave, 1, 0, 8, 0, 0, 0, 4, 0, 0, 0, 0), KROW(wave, 1, 1, 8, 0, 0, 0, 4, 0, 0, 0, 0),
    KROW(wave, 0, 0, 16, 0, 0, 0, 4, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 0, 0, 0, 4, 0, 0, 0, 0), KROW(wave, 1, 0, 16, 0, 0, 0, 4, 0, 0, 0, 0), KROW(wave, 1, 1, 16, 0, 0, 0, 4, 0, 0, 0, 0),
    KROW(wave, 0, 0, 4, 1, 0, 0, 3, 0, 0, 0, 0), KROW(wave, 0, 1, 4, 1, 0, 0, 3, 0, 0, 0, 0), KROW(wave, 1, 0, 4, 1, 0, 0, 3, 0, 0, 0, 0), KROW(wave, 1, 1, 4, 1, 0, 0, 3, 0, 0, 0, 0),
    KROW(wave, 0, 0, 8, 1, 0, 0, 3, 0, 0, 0, 0), KROW(wave, 0, 1, 8, 1, 0, 0, 3, 0, 0, 0, 0), KROW(wave, 1, 0, 8, 1, 0, 0, 3, 0, 0, 0, 0), KROW(wave, 1, 1, 8, 1, 0, 0, 3, 0, 0, 0, 0),
    KROW(wave, 0, 0, 16, 1, 0, 0, 3, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 1, 0, 0, 3, 0, 0, 0, 0), KROW(wave, 1, 0, 16, 1, 0, 0, 3, 0, 0, 0, 0), KROW(wave, 1, 1, 16, 1, 0, 0, 3, 0, 0, 0, 0),
    KROW(wave, 0, 0, 4, 0, 0, 1, 4, 0, 0, 0, 0), KROW(wave, 0, 1, 4, 0, 0, 1, 4, 0, 0, 0, 0), KROW(wave, 1, 0, 4, 0, 0, 1, 4, 0, 0, 0, 0), KROW(wave, 1, 1, 4, 0, 0, 1, 4, 0, 0, 0, 0),
    KROW(wave, 0, 0, 8, 0, 0, 1, 4, 0, 0, 0, 0), KROW(wave, 0, 1, 8, 0, 0, 1, 4, 0, 0, 0, 0), KROW(wave, 1, 0, 8, 0, 0, 1, 4, 0, 0, 0, 0), KROW(wave, 1, 1, 8, 0, 0, 1, 4, 0, 0, 0, 0),
    KROW(wave, 0, 0, 16, 0, 0, 1, 4, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 0, 0, 1, 4, 0, 0, 0, 0), KROW(wave, 1, 0, 16, 0, 0, 1, 4, 0, 0, 0, 0), KROW(wave, 1, 1, 16, 0, 0, 1, 4, 0, 0, 0, 0),
    KROW(wave, 0, 0, 4, 1, 0, 1, 3, 0, 0, 0, 0), KROW(wave, 0, 1, 4, 1, 0, 1, 3, 0, 0, 0, 0), KROW(wave, 1, 0, 4, 1, 0, 1, 3, 0, 0, 0, 0), KROW(wave, 1, 1, 4, 1, 0, 1, 3, 0, 0, 0, 0),
    KROW(wave, 0, 0, 8, 1, 0, 1, 3, 0, 0, 0, 0), KROW(wave, 0, 1, 8, 1, 0, 1, 3, 0, 0, 0, 0), KROW(wave, 1, 0, 8, 1, 0, 1, 3, 0, 0, 0, 0), KROW(wave, 1, 1, 8, 1, 0, 1, 3, 0, 0, 0, 0),
    KROW(wave, 0, 0, 16, 1, 0, 1, 3, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 1, 0, 1, 3, 0, 0, 0, 0), KROW(wave, 1, 0, 16, 1, 0, 1, 3, 0, 0, 0, 0), KROW(wave, 1, 1, 16, 1, 0, 1, 3, 0, 0, 0, 0),
    // lane sweeps (partial relativity only; the sweep width is that of the cross-check walks)
    KROW(wave, 0, 0, 16, 0, 1, 0, 4, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 0, 1, 0, 4, 0, 0, 0, 0), KROW(wave, 0, 0, 16, 1, 1, 0, 3, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 1, 1, 0, 3, 0, 0, 0, 0),
    KROW(wave, 0, 0, 16, 0, 1, 1, 4, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 0, 1, 1, 4, 0, 0, 0, 0), KROW(wave, 0, 0, 16, 1, 1, 1, 3, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 1, 1, 1, 3, 0, 0, 0, 0),
    // v-packets with the register budget of two waves per SIMD (vpk_wide_registers)
    KROW(wave, 0, 0, 8, 1, 0, 0, 2, 0, 0, 0, 0), KROW(wave, 0, 1, 8, 1, 0, 0, 2, 0, 0, 0, 0), KROW(wave, 1, 0, 8, 1, 0, 0, 2, 0, 0, 0, 0), KROW(wave, 1, 1, 8, 1, 0, 0, 2, 0, 0, 0, 0),
    KROW(wave, 0, 0, 16, 1, 0, 0, 2, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 1, 0, 0, 2, 0, 0, 0, 0), KROW(wave, 1, 0, 16, 1, 0, 0, 2, 0, 0, 0, 0), KROW(wave, 1, 1, 16, 1, 0, 0, 2, 0, 0, 0, 0),
    KROW(wave, 0, 0, 16, 1, 1, 0, 2, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 1, 1, 0, 2, 0, 0, 0, 0),
    // lane sweeps at three waves per SIMD (ls_waves_per_simd: B); the interleaved sweep table (sweep_table) at three and four
    KROW(wave, 0, 0, 16, 0, 1, 0, 3, 0, 0, 0, 0), KROW(wave, 0, 1, 16, 0, 1, 0, 3, 0, 0, 0, 0), KROW(wave, 0, 0, 16, 0, 1, 0, 3, 1, 0, 0, 0), KROW(wave, 0, 1, 16, 0, 1, 0, 3, 1, 0, 0, 0),
    KROW(wave, 0, 0, 16, 0, 1, 0, 4, 1, 0, 0, 0), KROW(wave, 0, 1, 16, 0, 1, 0, 4, 1, 0, 0, 0), KROW(wave, 0, 0, 16, 0, 1, 0, 4, 2, 0, 0, 0), KROW(wave, 0, 1, 16, 0, 1, 0, 4, 2, 0, 0, 0),
    // the shell-sorted log (log_by_shell)
    KROW(wave, 0, 0, 16, 0, 1, 0, 3, 0, 1, 0, 0), KROW(wave, 0, 1, 16, 0, 1, 0, 3, 0, 1, 0, 0), KROW(wave, 0, 0, 16, 0, 1, 0, 4, 1, 1, 0, 0), KROW(wave, 0, 1, 16, 0, 1, 0, 4, 1, 1, 0, 0),
    // full r-packet tracking (track_full)
    KROW(wave, 0, 1, 16, 0, 0, 0, 4, 0, 0, 1, 0), KROW(wave, 1, 1, 16, 0, 0, 0, 4, 0, 0, 1, 0), KROW(wave, 0, 1, 16, 1, 0, 0, 3, 0, 0, 1, 0), KROW(wave, 1, 1, 16, 1, 0, 0, 3, 0, 0, 1, 0),
    // 64-bit table offsets (table_offsets): group sweeps of width 8 / 16, lane sweeps, full tracking
    KROW(wave, 0, 0, 8, 0, 0, 0, 4, 0, 0, 0, 1), KROW(wave, 0, 1, 8, 0, 0, 0, 4, 0, 0, 0, 1), KROW(wave, 1, 0, 8, 0, 0, 0, 4, 0, 0, 0, 1), KROW(wave, 1, 1, 8, 0, 0, 0, 4, 0, 0, 0, 1),
    KROW(wave, 0, 0, 16, 0, 0, 0, 4, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 0, 0, 0, 4, 0, 0, 0, 1), KROW(wave, 1, 0, 16, 0, 0, 0, 4, 0, 0, 0, 1), KROW(wave, 1, 1, 16, 0, 0, 0, 4, 0, 0, 0, 1),
    KROW(wave, 0, 0, 8, 1, 0, 0, 3, 0, 0, 0, 1), KROW(wave, 0, 1, 8, 1, 0, 0, 3, 0, 0, 0, 1), KROW(wave, 1, 0, 8, 1, 0, 0, 3, 0, 0, 0, 1), KROW(wave, 1, 1, 8, 1, 0, 0, 3, 0, 0, 0, 1),
    KROW(wave, 0, 0, 16, 1, 0, 0, 3, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 1, 0, 0, 3, 0, 0, 0, 1), KROW(wave, 1, 0, 16, 1, 0, 0, 3, 0, 0, 0, 1), KROW(wave, 1, 1, 16, 1, 0, 0, 3, 0, 0, 0, 1),
    KROW(wave, 0, 0, 16, 1, 1, 0, 3, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 1, 1, 0, 3, 0, 0, 0, 1), KROW(wave, 0, 0, 16, 0, 1, 0, 3, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 0, 1, 0, 3, 0, 0, 0, 1),
    KROW(wave, 0, 0, 16, 0, 1, 0, 4, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 0, 1, 0, 4, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 0, 0, 0, 4, 0, 0, 1, 1), KROW(wave, 1, 1, 16, 0, 0, 0, 4, 0, 0, 1, 1),
    KROW(wave, 0, 1, 16, 1, 0, 0, 3, 0, 0, 1, 1), KROW(wave, 1, 1, 16, 1, 0, 0, 3, 0, 0, 1, 1),
    // the v-packet log with last interactions (vpacket_last_interaction): every tracked v-packet instantiation above again, with VLI
    KROW(wave, 0, 1, 4, 1, 0, 0, 3, 0, 0, 0, 0, 1), KROW(wave, 1, 1, 4, 1, 0, 0, 3, 0, 0, 0, 0, 1), KROW(wave, 0, 1, 8, 1, 0, 0, 3, 0, 0, 0, 0, 1), KROW(wave, 1, 1, 8, 1, 0, 0, 3, 0, 0, 0, 0, 1),
    KROW(wave, 0, 1, 16, 1, 0, 0, 3, 0, 0, 0, 0, 1), KROW(wave, 1, 1, 16, 1, 0, 0, 3, 0, 0, 0, 0, 1), KROW(wave, 0, 1, 4, 1, 0, 1, 3, 0, 0, 0, 0, 1), KROW(wave, 1, 1, 4, 1, 0, 1, 3, 0, 0, 0, 0, 1),
    KROW(wave, 0, 1, 8, 1, 0, 1, 3, 0, 0, 0, 0, 1), KROW(wave, 1, 1, 8, 1, 0, 1, 3, 0, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 1, 0, 1, 3, 0, 0, 0, 0, 1), KROW(wave, 1, 1, 16, 1, 0, 1, 3, 0, 0, 0, 0, 1),
    KROW(wave, 0, 1, 16, 1, 1, 0, 3, 0, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 1, 1, 1, 3, 0, 0, 0, 0, 1), KROW(wave, 0, 1, 8, 1, 0, 0, 2, 0, 0, 0, 0, 1), KROW(wave, 1, 1, 8, 1, 0, 0, 2, 0, 0, 0, 0, 1),
    KROW(wave, 0, 1, 16, 1, 0, 0, 2, 0, 0, 0, 0, 1), KROW(wave, 1, 1, 16, 1, 0, 0, 2, 0, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 1, 1, 0, 2, 0, 0, 0, 0, 1), KROW(wave, 0, 1, 16, 1, 0, 0, 3, 0, 0, 1, 0, 1),
    KROW(wave, 1, 1, 16, 1, 0, 0, 3, 0, 0, 1, 0, 1), KROW(wave, 0, 1, 8, 1, 0, 0, 3, 0, 0, 0, 1, 1), KROW(wave, 1, 1, 8, 1, 0, 0, 3, 0, 0, 0, 1, 1), KROW(wave, 0, 1, 16, 1, 0, 0, 3, 0, 0, 0, 1, 1),
    KROW(wave, 1, 1, 16, 1, 0, 0, 3, 0, 0, 0, 1, 1), KROW(wave, 0, 1, 16, 1, 1, 0, 3, 0, 0, 0, 1, 1), KROW(wave, 0, 1, 16, 1, 0, 0, 3, 0, 0, 1, 1, 1), KROW(wave, 1, 1, 16, 1, 0, 0, 3, 0, 0, 1, 1, 1),
};
#undef KROW

// A key as integers, in the order of its row's template arguments (the unused tail zero): what tardis_mc_kernel_table_row and
// tardis_mc_last_kernel_key report, and what the "no such instantiation" errors print
constexpr int KERNEL_KEY_FIELDS = 12;
int key_fields(const LaneKernelKey &k, int out[KERNEL_KEY_FIELDS])
{
    const int f[] = {k.full, k.vpk, k.track, k.full_tracking, k.vli};
    std::fill(out, out + KERNEL_KEY_FIELDS, 0);
    std::copy(std::begin(f), std::end(f), out);
    return (int)(std::end(f) - std::begin(f));
}
int key_fields(const GroupKernelKey &k, int out[KERNEL_KEY_FIELDS])
{
    const int f[] = {k.full, k.track, k.width, k.block, k.occupancy, k.vpk, k.wide, k.vli};
    std::fill(out, out + KERNEL_KEY_FIELDS, 0);
    std::copy(std::begin(f), std::end(f), out);
    return (int)(std::end(f) - std::begin(f));
}
int key_fields(const WaveKernelKey &k, int out[KERNEL_KEY_FIELDS])
{
    const int f[] = {k.full, k.track, k.width, k.vpk, k.lane_sweep, k.xwalk, k.waves_per_simd, k.nt, k.shell_log, k.full_tracking, k.wide, k.vli};
    static_assert(sizeof f / sizeof f[0] == KERNEL_KEY_FIELDS, "the wave kernel's key fills the reported key");
    std::copy(std::begin(f), std::end(f), out);
    return KERNEL_KEY_FIELDS;
}
template <typename Key> std::string key_text(const Key &key)  // "(0, 1, 16, ...)"
{
    int f[KERNEL_KEY_FIELDS];
    const int n = key_fields(key, f);
    std::string s = "(";
    for (int i = 0; i < n; ++i) s += (i ? ", " : "") + std::to_string(f[i]);
    return s + ")";
}
template <typename Key> void record_kernel(TardisMcContext *ctx, int table, const Key &key)  // (-> tardis_mc_last_kernel_key)
{
    ctx->last_kernel_table = table;
    key_fields(key, ctx->last_kernel_key);
}
template <typename Key, typename Fn, size_t N>
int kernel_table_row(const KernelRow<Key, Fn> (&table)[N], int row, int *key)
{
    if (key && row >= 0 && row < (int)N) key_fields(table[row].key, key);
    return (int)N;
}

size_t wave_kernel_lds(const WaveKernelKey &k, int n_shells)  // dynamic LDS of an instantiation of the wave kernel
{
    if (k.shell_log) return mc::wave_kernel_lds_bytes<false, false, true, true>(n_shells);
    if (k.lane_sweep) return k.vpk ? mc::wave_kernel_lds_bytes<false, true, true>(n_shells) : mc::wave_kernel_lds_bytes<false, false, true>(n_shells);
    return k.vpk ? (k.full ? mc::wave_kernel_lds_bytes<true, true>(n_shells) : mc::wave_kernel_lds_bytes<false, true>(n_shells))
                 : (k.full ? mc::wave_kernel_lds_bytes<true, false>(n_shells) : mc::wave_kernel_lds_bytes<false, false>(n_shells));
}

int launch_lane(TardisMcContext *ctx, const mc::DeviceProblem &P, int blocks, size_t lds)
{
    const bool ft = P.evlog.rows != nullptr || P.seglog.recs != nullptr;  // full r-packet tracking and / or the segment log: 8 ints of LDS per workgroup and log for the waves' append state
    const LaneKernelKey key{ctx->cfg.enable_full_relativity != 0, ctx->cfg.number_of_vpackets > 0, ctx->pk.track, ft, vlog_li_call(ctx)};
    const LaneKernelFn k = find_kernel(LANE_KERNELS, key);
    if (!k) return fail(ctx, TARDIS_MC_ERR_STATE, "propagate: no such instantiation of the lane kernel: FULL, VPK, TRACK, FT, VLI = %s", key_text(key).c_str());
    record_kernel(ctx, 0, key);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), lds + (ft ? 64 : 0), ctx->stream, P);
    HIP_TRY(ctx, hipGetLastError());
    return TARDIS_MC_OK;
}

// Full r-packet tracking: size the row pool of this call (rows the caller asked for, plus one chunk per wave for the
// partly filled last chunks), bound its device memory, clear the counts and the chunk fills, and point P at it.
int setup_event_log(TardisMcContext *ctx, mc::DeviceProblem &P, long long n_waves)
{
    const long long n = ctx->pk.n_packets;
    const long long row_bytes = (long long)sizeof(mc::EventRow), col_bytes = 14 * 8;  // pool row; the fourteen int64 / float64 columns
    long long cap = ctx->el.evlog_capacity;
    const long long fixed = n * (4 + 8) + 64;  // counts, offsets
    if (cap <= 0) {  // automatic: 32 rows per packet, within the bound (a re-run with the exact count fixes an overflow)
        const long long fit = (ctx->el.evlog_max_bytes - fixed) / (row_bytes + col_bytes) - n_waves * (long long)ctx->el.ev_chunk_rows;
        cap = std::max<long long>(1024, std::min<long long>(32 * std::max<long long>(n, 1), fit));
    }
    const long long chunks = (cap + ctx->el.ev_chunk_rows - 1) / ctx->el.ev_chunk_rows + n_waves;
    const long long slots = chunks * (long long)ctx->el.ev_chunk_rows;
    const long long need = slots * row_bytes + cap * col_bytes + fixed;
    if (need > ctx->el.evlog_max_bytes || chunks >= (1LL << 31))
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT,
                    "full r-packet tracking: an event log of %lld rows for %lld packets needs %.2f GiB of device memory, more than the "
                    "bound of %.2f GiB (option event_log_max_bytes); propagate fewer packets per call or raise the bound",
                    cap, n, need / 1073741824.0, ctx->el.evlog_max_bytes / 1073741824.0);
    HIP_TRY(ctx, ctx->el.ev_rows.ensure((size_t)slots * row_bytes));
    HIP_TRY(ctx, ctx->el.ev_fill.ensure((size_t)chunks * sizeof(unsigned)));
    HIP_TRY(ctx, ctx->el.ev_state.ensure(2 * sizeof(unsigned long long)));
    HIP_TRY(ctx, ctx->el.ev_counts.ensure((size_t)std::max<long long>(n, 1) * sizeof(int)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->el.ev_fill.p, 0, (size_t)chunks * sizeof(unsigned), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->el.ev_state.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->el.ev_counts.p, 0, (size_t)std::max<long long>(n, 1) * sizeof(int), ctx->stream));
    P.evlog.rows = ctx->el.ev_rows.as<mc::EventRow>();
    P.evlog.chunk_fill = ctx->el.ev_fill.as<unsigned>();
    P.evlog.pool_next = ctx->el.ev_state.as<unsigned>();
    P.evlog.dropped = ctx->el.ev_state.as<unsigned long long>() + 1;
    P.evlog.counts = ctx->el.ev_counts.as<int>();
    P.evlog.chunk_rows = ctx->el.ev_chunk_rows;
    P.evlog.n_chunks = (unsigned)chunks;
    ctx->el.ev_packets = n;
    ctx->el.ev_capacity = cap;
    ctx->el.ev_slots = slots;
    ctx->el.ev_n_chunks = (unsigned)chunks;
    return TARDIS_MC_OK;
}

// The segment log of the photo-ionisation estimators (option bf_estimators): sized like the event log -- the records the caller asked for (automatic: 96 per
// packet) plus one chunk per wave and launch for the partly filled last chunks -- with a key and a sorted slot per record for the pass.  The grouping
// kernels index the slots in 32 bits and keep a histogram of the shells in LDS.
int setup_segment_log(TardisMcContext *ctx, mc::DeviceProblem &P, long long n_waves)
{
    const long long n = ctx->pk.n_packets, chunk_rows = (long long)ctx->el.ev_chunk_rows;
    const long long slot_bytes = (long long)sizeof(mc::SegmentRecord) + 2 * (long long)sizeof(unsigned);  // record, key, sorted slot
    const long long cap = ctx->bf.seg_capacity > 0 ? ctx->bf.seg_capacity : std::max<long long>(1024, 96 * std::max<long long>(n, 1));
    const long long chunks = (cap + chunk_rows - 1) / chunk_rows + n_waves;
    const long long slots = chunks * chunk_rows;
    const long long need = slots * slot_bytes + chunks * (long long)sizeof(unsigned);
    if (need > ctx->bf.seg_max_bytes)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT,
                    "photo-ionisation estimators: a segment log of %lld records for %lld packets needs %.2f GiB of device memory, more than the bound of "
                    "%.2f GiB (option segment_log_max_bytes); propagate fewer packets per call or raise the bound",
                    cap, n, need / 1073741824.0, ctx->bf.seg_max_bytes / 1073741824.0);
    if (slots >= (1LL << 32))  // (with it: fewer than 2^31 chunks, of at least 64 records each)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT,
                    "photo-ionisation estimators: a segment log of %lld records for %lld packets has %lld slots, and the pass indexes the slots in 32 bits; "
                    "propagate fewer packets per call", cap, n, slots);
    if (ctx->n_shells > mc::EST_MAX_BINS)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "photo-ionisation estimators: more than %d shells (the pass groups the records by shell in LDS)", mc::EST_MAX_BINS);
    HIP_TRY(ctx, ctx->bf.seg_recs.ensure((size_t)slots * sizeof(mc::SegmentRecord)));
    HIP_TRY(ctx, ctx->bf.seg_keys.ensure((size_t)slots * sizeof(unsigned)));
    HIP_TRY(ctx, ctx->bf.seg_sorted.ensure((size_t)slots * sizeof(unsigned)));
    HIP_TRY(ctx, ctx->bf.seg_fill.ensure((size_t)chunks * sizeof(unsigned)));
    HIP_TRY(ctx, ctx->bf.seg_state.ensure(2 * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->bf.seg_fill.p, 0, (size_t)chunks * sizeof(unsigned), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->bf.seg_state.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
    P.seglog.recs = ctx->bf.seg_recs.as<mc::SegmentRecord>();
    P.seglog.keys = ctx->bf.seg_keys.as<unsigned>();
    P.seglog.chunk_fill = ctx->bf.seg_fill.as<unsigned>();
    P.seglog.pool_next = ctx->bf.seg_state.as<unsigned>();
    P.seglog.dropped = ctx->bf.seg_state.as<unsigned long long>() + 1;
    P.seglog.chunk_rows = (unsigned)chunk_rows;
    P.seglog.n_chunks = (unsigned)chunks;
    ctx->problem_host.seglog = P.seglog;  // (what the pass behind the call and tardis_mc_get_segment_log read)
    ctx->bf.seg_slots = slots;
    ctx->bf.seg_n_chunks = (unsigned)chunks;
    return TARDIS_MC_OK;
}

// The accumulate pass of the photo-ionisation estimators (bf_estimators.hpp) on a pool of records -- a call's segment log, or the one chunk of
// tardis_mc_debug_bf_accumulate -- into the resident tables: the slots grouped by shell, the slices accumulated, the two totals advanced.
int bf_accumulate_pass(TardisMcContext *ctx, const mc::SegmentRecord *recs, const unsigned *keys, const unsigned *chunk_fill, int n_chunks, unsigned chunk_rows,
                       const unsigned long long *dropped)
{
    const int S = ctx->n_shells;
    int rc;
    if ((rc = ensure_events(ctx, ctx->bf.ev))) return rc;
    HIP_TRY(ctx, ctx->bf.seg_sorted.ensure((size_t)n_chunks * chunk_rows * sizeof(unsigned)));
    HIP_TRY(ctx, ctx->bf.seg_bins.ensure(4 * ((size_t)S + 1) * sizeof(unsigned)));
    unsigned *bin_count = ctx->bf.seg_bins.as<unsigned>(), *bin_start = bin_count + (S + 1), *bin_fill = bin_start + (S + 1), *slice_start = bin_fill + (S + 1);
    unsigned *sorted = ctx->bf.seg_sorted.as<unsigned>();
    const unsigned blocks = (unsigned)std::max(1, std::min(n_chunks, 1024));
    const size_t hist = (size_t)S * sizeof(unsigned);
    HIP_TRY(ctx, hipEventRecord(ctx->bf.ev[0], ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(bin_count, 0, ((size_t)S + 1) * sizeof(unsigned), ctx->stream));
    hipLaunchKernelGGL(mc::bin_count_kernel, dim3(blocks), dim3(256), hist, ctx->stream, keys, chunk_fill, n_chunks, chunk_rows, S, bin_count);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(mc::bin_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, (const unsigned *)bin_count, S, bin_start, bin_fill, slice_start);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(mc::bin_scatter_kernel, dim3(blocks), dim3(256), hist, ctx->stream, keys, chunk_fill, n_chunks, chunk_rows, S, bin_fill, sorted);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->bf.ev[1], ctx->stream));
    mc::BfAccumulateArgs a{};
    a.S = S; a.NC = (int)ctx->ct.continua; a.h = H_PLANCK; a.k_b = K_BOLTZMANN;
    a.block_edge = ctx->ct.block_edge.as<int>(); a.nu = ctx->ct.nu.as<double>(); a.x_sect = ctx->ct.x_sect.as<double>();
    a.nu_min = ctx->ct.nu_min.as<double>(); a.nu_max = ctx->ct.nu_max.as<double>(); a.t_e = ctx->bf.t_e.as<double>();
    a.recs = recs; a.sorted_index = sorted; a.bin_start = bin_start; a.slice_start = slice_start; a.tables = ctx->bf.tables.as<double>();
    // (a workgroup per slice, grid-stride beyond: the slices are at most records / EST_SLICE + S)
    const long long max_slices = ((long long)n_chunks * chunk_rows) / mc::EST_SLICE + S;
    const int cus = ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256;
    hipLaunchKernelGGL(mc::bf_accumulate_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>(max_slices, 8LL * cus))), dim3(mc::BF_THREADS), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(mc::bf_totals_kernel, dim3(1), dim3(1), 0, ctx->stream, (const unsigned *)(bin_start + S), dropped, ctx->bf.totals.as<unsigned long long>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->bf.ev[2], ctx->stream));
    ctx->bf.timed = true;
    return TARDIS_MC_OK;
}

// ---- tardis_mc_propagate: what the entry point hands to the runner of its call (run_lane_kernel / run_group_kernel / run_wave_kernel)
struct PropagateCall {
    plan::Plan plan;
    int cus;
    bool vpk, full;
    bool rs_armed;      // result streaming was armed for this call (tardis_mc_stream_results holds for one call)
    int tune_pending;   // the lane-sweep tuner: whether the previous propagate call was one of its timed ones: 2 * instantiation + sample, else -1
    int tune_slot;      // this call is a timed one of the tuner (becomes ls_tune.pending once it has been enqueued completely)
};

plan::PlanInput plan_input(const TardisMcContext *ctx)
{
    const TardisMcConfig &c = ctx->cfg;
    plan::PlanInput in{};
    in.n_shells = ctx->n_shells; in.n_lines = ctx->n_lines; in.n_trans = ctx->n_trans; in.n_packets = ctx->pk.n_packets;
    in.number_of_vpackets = c.number_of_vpackets; in.survival_probability = c.survival_probability;
    in.enable_full_relativity = c.enable_full_relativity; in.line_interaction_type = c.line_interaction_type;
    in.lines_sorted = ctx->ot.lines_sorted; in.prob_negative = ctx->ot.prob_negative; in.have_walk_tables = ctx->wt.have_walk_tables;
    in.variant = ctx->variant; in.table_offsets = ctx->table_offsets; in.vpacket_screening = ctx->sc.vpacket_screening;
    in.vpk_wave_min_packets = ctx->vpk_wave_min_packets; in.track_full = ctx->el.track_full; in.debug_flags = ctx->debug_flags;
    in.bf_estimators = ctx->bf.on;
    in.pfx_valid = ctx->sc.pfx_valid; in.pfx_negative = ctx->sc.pfx_negative;
    return in;
}

// the v-packet screening tables (tau_prefix.hpp): built by the first v-packet call after set_opacity that screens; a launch and a read-back of the negative-depth flag
int build_screening_tables(TardisMcContext *ctx)
{
    if (ctx->sc.pfx_valid) return TARDIS_MC_OK;
    const size_t S = (size_t)ctx->n_shells, L = (size_t)ctx->n_lines;
    HIP_TRY(ctx, ctx->sc.tau_pfx.ensure((S * (L + 1) + 8) * sizeof(double)));  // (+8: the four-entry windows of the screening)
    HIP_TRY(ctx, ctx->sc.tau_rowsum.ensure(S * sizeof(double)));
    HIP_TRY(ctx, ctx->sc.pfx_flag.ensure(sizeof(int)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->sc.pfx_flag.p, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(mc::tau_prefix_kernel, dim3((unsigned)S), dim3(256), 0, ctx->stream, ctx->ot.tau_t.as<double>(), (int)L,
                       ctx->sc.tau_pfx.as<double>(), ctx->sc.tau_rowsum.as<double>(), ctx->sc.pfx_flag.as<int>());
    HIP_TRY(ctx, hipGetLastError());
    int neg = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&neg, ctx->sc.pfx_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->sc.pfx_negative = neg != 0;
    ctx->sc.pfx_valid = true;
    return TARDIS_MC_OK;
}

// what option sweep_start_held = -1 stands for (profiles/sweep_start_held.txt)
constexpr int SWEEP_START_HELD_AUTO = 1;

// bytes of the block-skip tables (sweep_skip.hpp) behind the interleaved table: coarse entries with their slack, {frequency, prefix sum} entries
// (the slack: a coarse step of N loads reads N - 1 coarse entries from the block of its current line on; a trace that starts behind the last line of a list of
// 8 r lines starts at block r, so the last row's step reads N - 1 entries past the table: 7 and 9 at the widths compiled, 11 at the widest the host test runs,
// of 16.  A fine step of up to twelve lines from line L reads 12 entries of the interleaved table's 32.)
size_t skip_table_bytes(const TardisMcContext *ctx)
{
    const size_t stride = ((size_t)ctx->n_lines + 7) & ~(size_t)7;
    return ((stride / 8) * (size_t)ctx->n_shells + 16) * 16 + ((size_t)ctx->n_shells * ((size_t)ctx->n_lines + 1) + 1) * 16;
}

// the interleaved sweep table (option sweep_table): built by the first propagate call after set_opacity that uses it; like the screening tables a launch and a
// read-back (nt_negative: the lean proof of the NT kernels does not apply).  Tables whose padded rows reach 2^28 entries have none.
// (`skip_room`: with room for the block-skip tables behind it -- the caller's plan says the call may use them)
int build_sweep_table(TardisMcContext *ctx, bool skip_room)
{
    const unsigned long long stride = ((unsigned long long)ctx->n_lines + 7ull) & ~7ull;
    if (ctx->sw.nt_valid || stride * (unsigned long long)ctx->n_shells + 32ull >= (1ull << 28)) return TARDIS_MC_OK;
    const long long total = (long long)(stride * (unsigned long long)ctx->n_shells) + 32;  // (+ the slack of a step's loads behind the last row)
    HIP_TRY(ctx, ctx->sw.nt_t.ensure((size_t)total * 16 + (skip_room ? skip_table_bytes(ctx) : 0)));
    ctx->sw.sk_valid = false;
    HIP_TRY(ctx, ctx->sc.pfx_flag.ensure(sizeof(int)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->sc.pfx_flag.p, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(interleave_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 65536)), dim3(256), 0, ctx->stream, ctx->ot.nu_line.as<double>(),
                       ctx->ot.tau_t.as<double>(), ctx->sw.nt_t.as<double2>(), (long long)ctx->n_lines, (long long)ctx->n_shells, (long long)stride, total,
                       ctx->sc.pfx_flag.as<int>());
    HIP_TRY(ctx, hipGetLastError());
    int neg = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&neg, ctx->sc.pfx_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->sw.nt_negative = neg != 0;
    ctx->sw.nt_stride = (unsigned)stride;
    ctx->sw.nt_valid = true;
    return TARDIS_MC_OK;
}

// the block-skip tables (sweep_skip.hpp): built behind a valid interleaved table by the first propagate call that may use them; two launches and a read-back of
// the row sums and the negative-depth flag
int build_skip_tables(TardisMcContext *ctx)
{
    if (ctx->sw.sk_valid || !ctx->sw.nt_valid) return TARDIS_MC_OK;
    const size_t S = (size_t)ctx->n_shells, L = (size_t)ctx->n_lines, stride = ctx->sw.nt_stride;
    const size_t nt_total = stride * S + 32, ct_rows = stride / 8, ct_total = ct_rows * S + 16;
    if (ctx->sw.nt_t.cap < nt_total * 16 + skip_table_bytes(ctx)) {  // (the table was built by a call that could not use them: again, with room)
        ctx->sw.nt_valid = false;
        int rc = build_sweep_table(ctx, true);
        if (rc) return rc;
        if (!ctx->sw.nt_valid) return TARDIS_MC_OK;
    }
    double2 *nt = ctx->sw.nt_t.as<double2>();
    double2 *ct = nt + nt_total;
    double2 *pn = ct + ct_total;
    HIP_TRY(ctx, ctx->sw.sk_rowsum.ensure(S * sizeof(double)));
    HIP_TRY(ctx, ctx->sc.pfx_flag.ensure(sizeof(int)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->sc.pfx_flag.p, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(mc::tau_prefix_kernel, dim3((unsigned)S), dim3(256), 0, ctx->stream, ctx->ot.tau_t.as<double>(), (int)L, reinterpret_cast<double *>(pn),
                       ctx->sw.sk_rowsum.as<double>(), ctx->sc.pfx_flag.as<int>(), 2, 1);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(coarse_table_kernel, dim3((unsigned)std::min<size_t>((S * (L + 1) + 255) / 256, 65536)), dim3(256), 0, ctx->stream, (const double2 *)nt,
                       pn, ct, (long long)L, (long long)S, (long long)stride, (long long)ct_total);
    HIP_TRY(ctx, hipGetLastError());
    int neg = 0;
    std::vector<double> rowsum(S);
    HIP_TRY(ctx, hipMemcpyAsync(&neg, ctx->sc.pfx_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(rowsum.data(), ctx->sw.sk_rowsum.p, S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double r_max = 0.0;
    bool finite = true;
    for (double r : rowsum) { finite = finite && r >= 0.0 && r < 1e300; if (r > r_max) r_max = r; }
    ctx->sw.sk_negative = neg != 0 || !finite;
    ctx->sw.sk_margin = ssk::margin((int)L, r_max);
    ctx->sw.sk_ct_off = (unsigned)nt_total;
    ctx->sw.sk_pn_off = (unsigned)(nt_total + ct_total);
    ctx->sw.sk_valid = true;
    return TARDIS_MC_OK;
}

// The lane-sweep tuner (see ls_waves_per_simd and ls_tune in the context): which of the two production lane-sweep instantiations this call runs -- A (four waves per
// SIMD) or B (three: *ls3) -- forced by the option, or timed on the first calls of this key; call.tune_slot says which timed slot this call is, if any.
int lane_sweep_tuner(TardisMcContext *ctx, PropagateCall &call, bool *ls3)
{
    auto &tn = ctx->lt.ls_tune;
    const bool w64 = call.plan.w64;
    const int mode = ctx->cfg.line_interaction_type;
    *ls3 = false;
    // (a call that does not even fill the grid's lanes four times over is nothing but the drain of its longest packets: B, measured -6 % on
    // 1e5 - 1e6-packet calls of the tardis_example shape, without spending five calls of a 20-iteration run on finding that out)
    const bool all_drain = ctx->pk.n_packets < 4LL * 64 * 16 * call.cus;
    if (ctx->lt.ls_waves_per_simd == 3 || (ctx->lt.ls_waves_per_simd == 0 && all_drain)) *ls3 = true;
    else if (ctx->lt.ls_waves_per_simd == 0 && ctx->wv.pass_cus == 0) {
        if (tn.n != ctx->pk.n_packets || tn.lines != ctx->n_lines || tn.shells != ctx->n_shells || tn.mode != mode || tn.table != ctx->sw.sweep_table || tn.wide != (int)w64) {
            tn.n = ctx->pk.n_packets; tn.lines = ctx->n_lines; tn.shells = ctx->n_shells; tn.mode = mode; tn.table = ctx->sw.sweep_table;
            tn.wide = (int)w64;
            tn.phase = 0; tn.choice = 0;
            tn.ms[0][0] = tn.ms[0][1] = tn.ms[1][0] = tn.ms[1][1] = -1.0;
        } else if (call.tune_pending >= 0) {  // the previous call of this key was a timed one: its duration (propagation + passes)
            float ms = 0.f;
            HIP_TRY(ctx, hipEventSynchronize(ctx->lt.ev_tune[1]));
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->lt.ev_tune[0], ctx->lt.ev_tune[1]));
            tn.ms[call.tune_pending >> 1][call.tune_pending & 1] = ms;
        } else if (tn.phase >= 2 && tn.phase <= 5)
            tn.phase -= 1;  // the previous phase was a timed call and left no measurement (the call failed half-way): again
        // call 0: A, not timed (first-call allocations, the log sized from a guess); calls 1 / 3: A; calls 2 / 4: B; from call 5 on: the choice
        if (tn.phase == 0) *ls3 = false;
        else if (tn.phase <= 4) { *ls3 = (tn.phase & 1) == 0; call.tune_slot = 2 * (*ls3 ? 1 : 0) + ((tn.phase - 1) >> 1); }
        else {
            if (tn.phase == 5) {
                const bool all = tn.ms[0][0] > 0.0 && tn.ms[0][1] > 0.0 && tn.ms[1][0] > 0.0 && tn.ms[1][1] > 0.0;
                tn.choice = (all && std::min(tn.ms[1][0], tn.ms[1][1]) < 0.97 * std::min(tn.ms[0][0], tn.ms[0][1])) ? 1 : 0;
            }
            *ls3 = tn.choice == 1;
        }
        if (tn.phase < 6) ++tn.phase;
        if (call.tune_slot >= 0)
            for (int k = 0; k < 2; ++k)
                if (!ctx->lt.ev_tune[k]) HIP_TRY(ctx, hipEventCreate(&ctx->lt.ev_tune[k]));
    }
    return TARDIS_MC_OK;
}

// ---- the wave kernel of a call: its key, computed once from the plan and the options before anything is launched, and what the host decided on the way
struct WaveChoice {
    WaveKernelKey key;
    WaveKernelFn fn;
    size_t lds;
    int waves_per_cu;      // what the LDS and option waves_per_simd allow (the instantiation's own bound comes on top: max_waves_per_cu)
    int max_waves_per_cu;
    bool compact_walk, ls3;
    int sweep_skip;        // WaveCold::sweep_skip of the call's launches (plan::plan_sweep_skip)
    int tiles, n_bins;     // tiles of EST_TILE lines per shell, (shell, tile) bins of the line-visit log
    bool partition;        // est_pipeline 1 (estimator_partition.hpp): the records are grouped by shell, then by bin
};

int choose_wave_kernel(TardisMcContext *ctx, PropagateCall &call, mc::GroupArgs &P, WaveChoice &w)
{
    const TardisMcConfig &c = ctx->cfg;
    const bool vpk = call.vpk, full = call.full, w64 = call.plan.w64, vq = call.plan.variant == 4;
    WaveKernelKey &k = w.key;
    k = WaveKernelKey{};
    k.full = full; k.track = ctx->pk.track; k.vpk = vpk;
    k.lane_sweep = call.plan.variant == 3 && !full;  // (the bounds of the lane sweep are those of partial relativity)
    k.waves_per_simd = vpk ? 3 : 4;
    if (wave_kernel_lds(k, ctx->n_shells) > 64 * 1024) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "n_shells too large for the LDS J/nu_bar accumulator");
    w.waves_per_cu = std::max(1, std::min(ctx->waves_per_simd > 0 ? 4 * ctx->waves_per_simd : 16, (int)((160 * 1024) / wave_kernel_lds(k, ctx->n_shells))));
    // macro-atom jumps of the wave kernel (macroatom chains and the single jump of downbranch alike): per-lane walk on the
    // compact tables (walk_tables.hpp); debug flag 8192 keeps the cooperative group scan of the fp64 running sums (macroatom) /
    // the fp64 search (downbranch), 128 the per-lane search in them (both for cross-checks)
    w.compact_walk = c.line_interaction_type != 0 && ctx->wt.have_walk_tables && !(ctx->debug_flags & plan::DBG_FP64_WALKS);
    // (flag 1048576: the long instantiations, for A/B; the flags that read the kernel's profiling / test counters: those are only compiled into the long ones)
    k.xwalk = (c.line_interaction_type != 0 && !w.compact_walk) || (ctx->debug_flags & (plan::DBG_LONG_INSTANTIATIONS | plan::DBG_WAVE_COUNTERS)) != 0;
    if (w64 && k.xwalk) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "the fp64 macro-atom walks have no 64-bit table offsets");
    // (sweep-worker width of the wave kernel: 8 lanes for sparse line lists, 16 for long ones, like the group kernel; the lane-sweep
    // instantiations only use it in the cross-check walks: one width)
    const int GW = ctx->group_size ? ctx->group_size : (ctx->n_lines <= 100000 ? 8 : 16);
    k.width = k.lane_sweep ? 16 : GW;
    // v-packets on a grid so fine that the per-shell LDS arrays leave room for at most eight waves per CU (two per SIMD): the
    // instantiation compiled for two waves per SIMD -- 239 VGPRs, no spills -- costs no occupancy there (built for the sweep widths G = 16 and
    // G = 8, without the cross-check walks; option vpk_wide_registers 0 keeps the 168-VGPR one)
    // Measured (profiles/r05_vpk_wide_registers.txt): 3727-3766 vs 4442-4450 ms per 1e7 packets of the configs[4] shape (-16 %).  Option 2 forces
    // it (then eight waves per CU whatever the LDS allows), 0 keeps the 168-VGPR instantiation.
    // (with lane sweeps: variant 3 under partial relativity)
    if (vpk && !k.xwalk && !w64 && !ctx->el.track_full && !ctx->bf.on && (k.lane_sweep || GW == 16 || GW == 8) &&
        ((ctx->vpk_wide_registers == 1 && w.waves_per_cu <= 8) || ctx->vpk_wide_registers == 2))
        k.waves_per_simd = 2;
    // which lane-sweep instantiation (see ls_waves_per_simd in the context), and whether on the interleaved sweep table: the production lane-sweep instantiations only
    w.ls3 = false;
    if (k.lane_sweep && !vpk && !k.xwalk) {
        int rc = lane_sweep_tuner(ctx, call, &w.ls3);
        if (rc) return rc;
        if (w.ls3) k.waves_per_simd = 3;
        if (!w64 && ctx->sw.sweep_table != 0) {
            // (room for the block-skip tables only where this call may end up using them: what is known of its instantiation so far, the rest assumed in favour)
            plan::SkipInput room{};
            room.sweep_skip = ctx->sw.sweep_skip; room.lane_sweep = true; room.full_relativity = full; room.full_tracking = ctx->el.track_full || ctx->bf.on;
            room.waves_per_simd = k.waves_per_simd; room.nt = (ctx->sw.sweep_table == 2 && !w.ls3) ? 2 : 1; room.line_scattering = !c.disable_line_scattering;
            room.twelve_wave_skip = TMC_SWEEP_SKIP_12 != 0;
            rc = build_sweep_table(ctx, plan::plan_sweep_skip(room));
            if (rc) return rc;
            if (ctx->sw.nt_valid && !ctx->sw.nt_negative) {
                k.nt = (ctx->sw.sweep_table == 2 && !w.ls3) ? 2 : 1;
                P.nt_t = ctx->sw.nt_t.as<double>(); P.nt_stride = ctx->sw.nt_stride;
            }
        }
    }
    w.max_waves_per_cu = k.waves_per_simd == 2 ? 8 : (w.ls3 ? 12 : 16);
    w.tiles = std::max((ctx->n_lines + mc::EST_TILE - 1) / mc::EST_TILE, 1);
    w.n_bins = ctx->n_shells * w.tiles;
    // est_pipeline 1 (estimator_partition.hpp): needs a shell's bins and all shells to fit the partition kernel's local buckets
    w.partition = ctx->wv.est_pipeline == 1 && w.tiles <= mc::PART_LOCAL_BUCKETS && ctx->n_shells <= mc::PART_LOCAL_BUCKETS;
    // the shell-sorted log: instantiated for the two production lane-sweep kernels (sixteen waves on the interleaved table, twelve on the separate ones)
    k.shell_log = k.lane_sweep && !vpk && !k.xwalk && !w64 && !vq && w.partition && ctx->wv.log_by_shell != 0 && ctx->n_shells <= 64 &&
                  ((!w.ls3 && k.nt == 1) || (w.ls3 && k.nt == 0));
    // the block skip of the lane sweeps (sweep_skip.hpp): where the plan allows it; its tables are built here, and a negative optical depth in them plans again
    w.sweep_skip = 0;
    if (TMC_SWEEP_SKIP != 0) {  // (a build without the kernel's code reports off)
        plan::SkipInput si{};
        si.sweep_skip = ctx->sw.sweep_skip; si.lane_sweep = k.lane_sweep; si.vpk = vpk; si.full_relativity = full; si.wide = w64; si.cross_check = k.xwalk;
        si.shell_log = k.shell_log; si.full_tracking = ctx->el.track_full || ctx->bf.on; si.waves_per_simd = k.waves_per_simd; si.nt = k.nt;
        si.line_scattering = !c.disable_line_scattering; si.nt_negative = ctx->sw.nt_negative; si.pfx_negative = false;
        si.twelve_wave_skip = TMC_SWEEP_SKIP_12 != 0;
        if (plan::plan_sweep_skip(si)) {
            int rc = build_skip_tables(ctx);
            if (rc) return rc;
            // (a table built without room for them has been built again in a larger allocation: the address taken above is gone)
            P.nt_t = ctx->sw.nt_t.as<double>(); P.nt_stride = ctx->sw.nt_stride;
            si.pfx_negative = !ctx->sw.sk_valid || ctx->sw.sk_negative;
            if (plan::plan_sweep_skip(si)) w.sweep_skip = (ctx->debug_flags & plan::DBG_SKIP_FALLBACK) ? 2 : 1;
        }
        ctx->sw.last_sweep_skip = w.sweep_skip ? 1 : 0;
    }
    if (ctx->el.track_full || ctx->bf.on) {  // the tracked instantiations: group sweeps of 16 lanes, compact walks, default register budget
        k.full_tracking = true; k.track = true; k.width = 16;
    }
    // 64-bit row offsets: the production shapes above without the interleaved sweep table, the shell-sorted log and the two-waves-per-SIMD
    // v-packet form (those keep 32-bit offsets); sweep width 4 runs as 8 (per-packet results do not depend on the width)
    if (w64) { k.wide = true; if (k.width == 4) k.width = 8; }
    k.vli = vlog_li_call(ctx);
    w.fn = find_kernel(WAVE_KERNELS, k);
    if (!w.fn)
        return fail(ctx, TARDIS_MC_ERR_STATE, "propagate: no such instantiation of the wave kernel: FULL, TRACK, G, VPK, LS, XWALK, WPE, NT, SL, FT, WIDE, VLI = %s",
                    key_text(k).c_str());
    record_kernel(ctx, 2, k);
    w.lds = wave_kernel_lds(k, ctx->n_shells);
    return TARDIS_MC_OK;
}

// ---- The line-visit log (estimator_log.hpp): how much device memory it may take.  What is free plus what the log holds already (a context is cached: the
// buffers of an earlier call are reused or replaced); known = false when the runtime does not say.
struct LogMemory { bool known; double avail, total; };
LogMemory log_memory(const TardisMcContext *ctx)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return LogMemory{false, 0.0, 0.0};
    const double have = (double)(ctx->wv.log_records[0].cap + ctx->wv.log_records[1].cap + ctx->wv.log_keys[0].cap + ctx->wv.log_keys[1].cap +
                                 ctx->wv.log_sorted[0].cap + ctx->wv.log_sorted[1].cap + ctx->wv.log_part.cap);
    return LogMemory{true, (double)free_b + have, (double)total_b};
}
// bytes per record of a set's capacity: every set holds the record and its key, and its own index (the sort) or a share of the one scratch copy (the partition)
constexpr double LOG_RECORD_BYTES = (double)(sizeof(mc::LineVisitRecord) + sizeof(unsigned));
double log_bytes_per_record(int sets, bool partition)
{
    return partition ? sets * LOG_RECORD_BYTES + (double)sizeof(mc::LineVisitRecord) : sets * (LOG_RECORD_BYTES + (double)sizeof(unsigned));
}
constexpr double LOG_MEMORY_SHARE = 0.6;  // never take more than 60 % of what is free, counting what the log holds already

struct LogSizing {
    bool one_set;
    int n_sets;
    unsigned region_capacity;    // records per chunk
    unsigned long long n_chunks;
    size_t set_records;
    double tail_records;
    bool tail_plan, tail_possible, want_split, want_compact, set1_inside;
};

// Two buffer sets, one region per wave; an epoch ends when the regions are full.  Sized for the whole call when that fits log_capacity (1.2x the traces
// per packet measured in the last call, 128 per packet before anything was measured), else log_capacity.
int size_line_log(TardisMcContext *ctx, const PropagateCall &call, const WaveChoice &w, long long n, int waves, bool cu_split, LogSizing &s)
{
    const bool vpk = call.vpk, vq = call.plan.variant == 4, partition = w.partition, shell_log = w.key.shell_log;
    long long log_capacity = ctx->wv.log_capacity;
    // One log set or two.  Two let the passes of an epoch run on a second stream beside the next launch -- but they do not fit beside sixteen resident waves per CU,
    // so "beside" means: contending with the next launch's first 0.1 s, both slower for it.  Measured at 1e8 packets (profiles/r06_log_sets.txt): the passes before
    // the next launch, alone on the chip, are faster in total, and one set leaves room for epochs half as many again (three launches instead of five): -0.5 %.
    // So a call of many epochs uses one set; shorter calls keep two (the passes of the bulk run beside the drain of the last launch).
    s.one_set = ctx->wv.log_sets == 1;
    if (ctx->wv.log_sets == 0 && partition && !vq && !vpk && ctx->wv.drain_split == 0 && ctx->wv.drain_compact == 0 && ctx->wv.epoch_split == 0 && ctx->wv.pass_cus == 0) {
        double two_set_capacity = (double)ctx->wv.log_capacity;
        if (!ctx->wv.log_capacity_user) {
            const LogMemory m = log_memory(ctx);
            if (m.known) two_set_capacity = std::min(two_set_capacity, LOG_MEMORY_SHARE * m.avail / log_bytes_per_record(2, true));
        }
        // (four epochs or more with two sets; at two or three the passes of the first epochs still find room beside the last launch's drain: 4e7 packets
        // 1 292 - 1 308 ms with two sets, 1 320 - 1 351 with one)
        const double per_packet = ctx->wv.traces_per_packet > 0.0 ? 1.05 * ctx->wv.traces_per_packet : ctx->wv.log_budget_per_packet;
        s.one_set = (double)n * per_packet > 3.0 * two_set_capacity;
    }
    if (s.one_set && !ctx->wv.log_capacity_user) {
        // (the second set of an earlier, smaller call is given back first)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->wv.stream2) HIP_TRY(ctx, hipStreamSynchronize(ctx->wv.stream2));
        ctx->wv.log_records[1].release(); ctx->wv.log_keys[1].release(); ctx->wv.log_sorted[1].release(); ctx->wv.log_bins[1].release(); ctx->wv.log_cursor[1].release();
        log_capacity = 4000000000LL;
    }
    LogMemory m{false, 0.0, 0.0};
    bool asked = false;
    if (!ctx->wv.log_capacity_user) {
        // (fewer, longer epochs are faster -- 25.8 vs 24.5 Mpkt/s at 1e8 packets with 2.5e9 instead of 1.5e9 records per set
        // -- but two sets of 2.5e9 records are 160 GB)
        m = log_memory(ctx);
        asked = true;
        if (m.known) log_capacity = std::min<long long>(log_capacity, (long long)(LOG_MEMORY_SHARE * m.avail / log_bytes_per_record(s.one_set ? 1 : 2, partition)));
    }
    unsigned long long cap = std::min<unsigned long long>((unsigned long long)log_capacity,
                                                          (unsigned long long)((double)n * ctx->wv.log_budget_per_packet) + 64ull * (unsigned long long)waves + 65536ull);
    if (w.n_bins > mc::EST_MAX_BINS) cap = 0;  // too many tiles for the LDS histogram: the kernel adds its terms directly
    cap = std::min<unsigned long long>(cap, 0xfffffff0ull);
    // The log is a pool of chunks the waves take one after the other (EstimatorLog, mc_device.hpp): chunks of up to 4096 records
    // (~90 passes of a wave: one pool atomic per 7 ms), at least four per wave on average so that the pool runs dry for all
    // waves at nearly the same time, never fewer than one per wave; a chunk holds >= 256 records (a pass appends up to 64).
    s.region_capacity = 0;
    s.n_chunks = 0;
    if (cap > 0) {
        // (shell-sorted log: a wave holds an open chunk for every shell -- the pool needs a few more chunks per wave than there are shells; chunks of
        // 2048 records are what the partition kernel stages at a time.  A caller's own log_capacity (tests) is respected: with fewer chunks than that
        // the waves that find the pool empty suspend at once and the call takes more epochs)
        const unsigned long long per_wave = shell_log ? (unsigned long long)(ctx->n_shells + 4) : 4ull;
        s.region_capacity = ctx->wv.log_chunk_records > 0 ? (unsigned)ctx->wv.log_chunk_records : (shell_log ? 2048u : 4096u);
        while (s.region_capacity > 256 && (unsigned long long)s.region_capacity * per_wave * (unsigned long long)waves > cap) s.region_capacity >>= 1;
        s.region_capacity &= ~1u;  // even: a chunk of 24-byte records then starts on a 16-byte boundary (partition_kernel stages with 16-byte loads)
        s.n_chunks = std::max<unsigned long long>(cap / s.region_capacity, (unsigned long long)waves * ((shell_log && !ctx->wv.log_capacity_user) ? per_wave : 1ull));
        if (s.n_chunks * s.region_capacity > 0xfffffff0ull) s.n_chunks = 0xfffffff0ull / s.region_capacity;
    }
    // Memory check: the tables are resident (set_opacity), what is left must hold the smallest log this grid runs with -- one chunk of 256 records per wave,
    // in one set
    if (s.region_capacity > 0) {
        if (!asked) m = log_memory(ctx);
        const double least = (double)waves * 256.0 * log_bytes_per_record(1, partition);
        if (m.known && least > m.avail)
            return fail(ctx, TARDIS_MC_ERR_HIP, "device memory: the tables leave %.3f GiB of %.1f GiB free, the smallest line-visit log of this call needs "
                                                "%.3f GiB", m.avail / 1073741824.0, m.total / 1073741824.0, least / 1073741824.0);
    }
    const unsigned region_capacity = s.region_capacity;
    const unsigned long long n_chunks = s.n_chunks;
    // a second buffer set (the estimator passes of an epoch overlap the next epoch) only when the call may need several epochs
    // ... or splits off its drain (WaveCold::drain_split): worth a second launch once the call is long enough for a drain to form
    s.want_split = ctx->wv.drain_split && !vq && !s.one_set && region_capacity > 0 && n >= 64LL * waves * 4;
    // Tail split: the last epoch of a call should hold only the DRAIN (the ~4 % of the records the longest-lived packets log
    // after the packet supply has run out, on a mostly idle chip), so that the passes over everything before it run beside the
    // drain and only the passes of the tail -- milliseconds -- are left for after the call.  The host knows the call's records
    // from the last call's traces per packet and hands the second-to-last epoch a pool of exactly "what is left minus the
    // tail"; with the chunk pool that epoch ends for all waves at once.  Also for calls whose log fits ONE epoch (their passes
    // were not overlapped with anything before).  A wrong estimate only moves the boundary.
    // (the tail: what the packets in flight when the supply runs out still log -- lanes x ~8 packets' worth of traces, the mean
    // residual life of a heavy-tailed population; only for calls whose passes are worth a second launch: >= 5e8 records)
    s.tail_records = (double)ctx->wv.log_tail_packets * ctx->wv.traces_per_packet * 64.0 * (double)waves;
    // Measured (profiles/r04_tail_split.txt): calls whose log fits one epoch -3 ... -5 % (1e7 - 2e7 packets: their passes ran
    // after the call before); calls of several epochs +0.5 % (their passes overlap the next epoch already, the extra launch
    // costs) -- so only the former.
    const bool one_epoch = (double)region_capacity * (double)n_chunks >= (double)n * ctx->wv.traces_per_packet * 1.05;
    s.tail_plan = ctx->wv.log_tail_split && !vq && !s.one_set && region_capacity > 0 && ctx->wv.traces_per_packet > 0.0 && one_epoch &&
                  (double)n * ctx->wv.traces_per_packet >= 5e8 && (double)n * ctx->wv.traces_per_packet > 2.0 * s.tail_records;
    // (the second buffer set is allocated as soon as a tail split MAY be planned -- the first call of a context has no estimate yet
    // -- so that no later call of the same size allocates tens of GB in the middle of an iteration)
    s.tail_possible = ctx->wv.log_tail_split && !vq && !s.one_set && region_capacity > 0 && (double)n * std::max(ctx->wv.traces_per_packet, 16.0) >= 5e8;
    // ... or packs the drain's live lanes into fewer waves (drain_compact): the passes of the launch before run beside the packed drain
    s.want_compact = ctx->wv.drain_compact > 0 && !vq && !vpk && !cu_split && !shell_log && !s.one_set && region_capacity > 0 && n > 64LL * (waves - 1) && waves >= 8;
    const bool several_epochs = region_capacity > 0 && (unsigned long long)region_capacity * n_chunks < (unsigned long long)((double)n * ctx->wv.log_budget_per_packet);
    s.n_sets = (s.one_set || vq) ? 1 : ((s.tail_plan || s.tail_possible || s.want_split || s.want_compact || several_epochs) ? 2 : 1);
    s.set_records = (size_t)std::max<unsigned long long>((unsigned long long)region_capacity * n_chunks, 1);
    // (a two-set call on a context whose first set was sized by a larger one-set call: both sets lie in the first set's buffers -- a second allocation of
    // tens of GB costs ~1 s the first time, the memory is cleared)
    s.set1_inside = s.n_sets == 2 && !ctx->wv.log_records[1].p && ctx->wv.log_records[0].cap >= 2 * s.set_records * sizeof(mc::LineVisitRecord) &&
                    ctx->wv.log_keys[0].cap >= 2 * s.set_records * sizeof(unsigned) && (partition || ctx->wv.log_sorted[0].cap >= 2 * s.set_records * sizeof(unsigned));
    return TARDIS_MC_OK;
}

// ---- The wave kernel's call: epochs over one packet supply (see LaneSave).  What is fixed for the call, and below it what the epochs change.
struct WaveCall {
    const PropagateCall *call;
    const WaveChoice *w;
    const LogSizing *log;
    mc::GroupArgs P;
    mc::WaveHot hot;
    int sweep_skip = 0; // the call's lane sweeps clear whole blocks on the coarse table (WaveCold::sweep_skip: 1, or 2 under debug flag 536870912)
    int trk_defer = 0;  // the call keeps the tracker record in LDS and stores it once per packet (WaveCold::trk_defer)
    long long n;
    int waves;
    bool vq, may_suspend, cu_masked, streaming;
    hipStream_t st;  // the stream of the propagation launches
    // -- state of the epoch loop
    int waves_cur;   // (the grid of the next launch: smaller after a compaction)
    mc::LaneSave *cur_save; mc::WaveSave *cur_wsave; uint32_t *cur_states;
    bool split_armed, compact_armed;
    bool vq_on;      // volley queue: on for the bulk of a call (see wave_epoch_tail_volley_queue)
    bool call_complete;
    int log_gen;     // (volley queue: the chunk pool of the shared log is reset after every run of the estimator passes)
    double records_done;  // (tail split: what the call has logged so far)
    long long rs_pending_lo, rs_pending_hi;  // result streaming: a range whose unpacking is queued and whose copy the host still has to issue
    unsigned long long pool_chunks;  // chunks in the pool of the running epoch
    double split_w2;                 // share of the grid in the second launch of a split epoch
};

template <typename T> T *log_set_ptr(const LogSizing &s, const DevBuf (&buf)[2], int b) { return s.set1_inside ? buf[0].as<T>() + (size_t)b * s.set_records : buf[b].as<T>(); }

// the accumulate kernel of the estimator passes (option est_accumulate); BINNED: the records lie in bin order (partition pipeline), else `index` does (index sort)
template <bool FULL, bool BINNED, typename... Args>
void launch_accumulate_as(int est_accumulate, int cus, hipStream_t es, Args... args)
{
    if (est_accumulate == 3)  // the dyadic hierarchy, a lane per record (accumulate_dyadic_kernel<.., LOOP>: 73 KB of LDS, two workgroups per CU)
        hipLaunchKernelGGL((mc::accumulate_dyadic_kernel<FULL, BINNED, true>), dim3(cus * 2), dim3(64 * mc::ACCD_WAVES), 0, es, args...);
    else if (est_accumulate == 2)  // the dyadic hierarchy of block sums (accumulate_dyadic_kernel): one workgroup per CU
        hipLaunchKernelGGL((mc::accumulate_dyadic_kernel<FULL, BINNED>), dim3(cus), dim3(64 * mc::ACCD_WAVES), 0, es, args...);
    else if (BINNED || est_accumulate == 1)  // one add per aligned block of 8 lines (accumulate_blocks_kernel)
        hipLaunchKernelGGL((mc::accumulate_blocks_kernel<FULL, BINNED>), dim3(cus * 2), dim3(64 * mc::ACCB_WAVES), 0, es, args...);
    else if constexpr (!BINNED)  // one add per line visit (index pipeline only)
        hipLaunchKernelGGL(mc::accumulate_kernel<FULL>, dim3(cus * 3), dim3(64 * mc::ACC_WAVES), 0, es, args...);
}
hipError_t launch_accumulate(bool full, bool binned, int est_accumulate, int cus, hipStream_t es, const mc::LineVisitRecord *records, const unsigned *index, const unsigned *bin_start,
                             const unsigned *slice_start, int n_bins, int tiles_per_shell, int n_lines, const double *nu_line, double *jblue_t, double *edot_t)
{
    if (full) {
        if (binned) launch_accumulate_as<true, true>(est_accumulate, cus, es, records, index, bin_start, slice_start, n_bins, tiles_per_shell, n_lines, nu_line, jblue_t, edot_t);
        else launch_accumulate_as<true, false>(est_accumulate, cus, es, records, index, bin_start, slice_start, n_bins, tiles_per_shell, n_lines, nu_line, jblue_t, edot_t);
    } else {
        if (binned) launch_accumulate_as<false, true>(est_accumulate, cus, es, records, index, bin_start, slice_start, n_bins, tiles_per_shell, n_lines, nu_line, jblue_t, edot_t);
        else launch_accumulate_as<false, false>(est_accumulate, cus, es, records, index, bin_start, slice_start, n_bins, tiles_per_shell, n_lines, nu_line, jblue_t, edot_t);
    }
    return hipGetLastError();
}

// binning + accumulation of one epoch's line-visit log (estimator_log.hpp): buffer set b, on stream es
hipError_t estimator_passes(TardisMcContext *ctx, const WaveCall &E, const mc::EstimatorLog &lg, int b, hipStream_t es)
{
    if (lg.region_capacity == 0) return hipSuccess;
    const int cus = E.call->cus, n_bins = E.w->n_bins;
    const bool full = E.call->full, shell_log = E.w->key.shell_log;
    unsigned *bin_count = ctx->wv.log_bins[b].as<unsigned>(), *bin_start = bin_count + (n_bins + 1),
             *bin_fill = bin_start + (n_bins + 1), *slice_start = bin_fill + (n_bins + 1);
    hipError_t e = hipMemsetAsync(bin_count, 0, (size_t)(n_bins + 1) * sizeof(unsigned), es);
    if (e != hipSuccess) return e;
    const size_t hist_lds = (size_t)n_bins * sizeof(unsigned);
    if (hist_lds > 64 * 1024) {  // more than the default dynamic-LDS limit: BASELINE config 5 has 100 shells x 245 tiles
        e = hipFuncSetAttribute((const void *)mc::bin_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds);
        if (e != hipSuccess) return e;
        e = hipFuncSetAttribute((const void *)mc::bin_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds);
        if (e != hipSuccess) return e;
    }
    const int bin_blocks = cus * 8;
    hipLaunchKernelGGL(mc::bin_count_kernel, dim3(bin_blocks), dim3(256), hist_lds, es, lg.keys, lg.region_count, lg.n_regions,
                       lg.region_capacity, n_bins, bin_count);
    hipLaunchKernelGGL(mc::bin_scan_kernel, dim3(1), dim3(256), 0, es, bin_count, n_bins, bin_start, bin_fill, slice_start);
    if (!E.w->partition) {  // index sort: the accumulate kernel gathers the records through the sorted index
        unsigned *sorted = log_set_ptr<unsigned>(*E.log, ctx->wv.log_sorted, b);
        hipLaunchKernelGGL(mc::bin_scatter_kernel, dim3(bin_blocks), dim3(256), hist_lds, es, lg.keys, lg.region_count, lg.n_regions,
                           lg.region_capacity, n_bins, bin_fill, sorted);
        return launch_accumulate(full, false, ctx->wv.est_accumulate, cus, es, lg.records, sorted, bin_start, slice_start, n_bins, lg.tiles_per_shell, ctx->n_lines, E.P.nu_line,
                                 E.P.jblue_t, E.P.edot_t);
    }
    // estimator_partition.hpp: by shell into the scratch copy, by bin back into the set's own buffer
    unsigned *shell_fill = slice_start + (n_bins + 2);
    mc::LineVisitRecord *scratch = ctx->wv.log_part.as<mc::LineVisitRecord>();
    auto bits_of = [](int n) { int b = 0; while ((1 << b) < n) ++b; return b; };
    const mc::LineVisitRecord *binned = lg.records;  // what the accumulate kernel reads
    const int part_blocks = cus * 2;
    if (!shell_log && ctx->wv.est_one_level != 0 && n_bins <= mc::PART_LOCAL_BUCKETS) {
        // few bins (short line lists: 300 on the tardis_example tables): ONE partition pass, log chunks -> scratch copy by bin.  (partition_kernel<2> with
        // "one shell of n_bins tiles": every chunk's first bucket is bin 0, a staged segment ranks over all bins)
        hipLaunchKernelGGL(mc::partition_kernel<2>, dim3(part_blocks), dim3(mc::PART_THREADS), 0, es, lg.records, lg.keys, lg.region_count, lg.n_regions,
                           lg.region_capacity, (const unsigned *)nullptr, n_bins, ctx->n_lines, bits_of(n_bins), bin_fill, scratch);
        binned = scratch;
    } else if (shell_log) {  // the chunks hold one shell each: straight to the partition by bin, into the scratch copy
        hipLaunchKernelGGL(mc::partition_kernel<2>, dim3(part_blocks), dim3(mc::PART_THREADS), 0, es, lg.records, lg.keys, lg.region_count, lg.n_regions,
                           lg.region_capacity, (const unsigned *)nullptr, lg.tiles_per_shell, ctx->n_lines, bits_of(mc::PART_LOCAL_BUCKETS), bin_fill, scratch);
        binned = scratch;
    } else {
        hipLaunchKernelGGL(mc::partition_shell_fill_kernel, dim3(1), dim3(256), 0, es, bin_start, lg.tiles_per_shell, ctx->n_shells, shell_fill);
        hipLaunchKernelGGL(mc::partition_kernel<1>, dim3(part_blocks), dim3(mc::PART_THREADS), 0, es, lg.records, lg.keys, lg.region_count,
                           lg.n_regions, lg.region_capacity, (const unsigned *)nullptr, lg.tiles_per_shell, ctx->n_lines, bits_of(ctx->n_shells),
                           shell_fill, scratch);
        hipLaunchKernelGGL(mc::partition_kernel<0>, dim3(part_blocks), dim3(mc::PART_THREADS), 0, es, scratch, (const unsigned *)nullptr,
                           (const unsigned *)nullptr, 0, 0u, bin_start + n_bins, lg.tiles_per_shell, ctx->n_lines, bits_of(mc::PART_LOCAL_BUCKETS),
                           bin_fill, lg.records);
    }
    return launch_accumulate(full, true, ctx->wv.est_accumulate, cus, es, binned, nullptr, bin_start, slice_start, n_bins, lg.tiles_per_shell, ctx->n_lines, E.P.nu_line, E.P.jblue_t,
                             E.P.edot_t);
}

// the host's part of a streamed range: sixteen copies into the caller's arrays, beside the running launch
hipError_t rs_copy_pending(TardisMcContext *ctx, WaveCall &E)
{
    if (E.rs_pending_hi <= E.rs_pending_lo) return hipSuccess;
    hipError_t e = hipStreamWaitEvent(ctx->rs.stream, ctx->rs.ev, 0);
    void *dev[16];
    per_packet_device_arrays(ctx, dev);
    const size_t off = (size_t)E.rs_pending_lo * 8, bytes = (size_t)(E.rs_pending_hi - E.rs_pending_lo) * 8;
    for (int a = 0; a < 16 && e == hipSuccess; ++a)
        if (ctx->rs.dst[a] && dev[a]) e = hipMemcpyAsync((char *)ctx->rs.dst[a] + off, (char *)dev[a] + off, bytes, hipMemcpyDeviceToHost, ctx->rs.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->rs.stream);
    ctx->rs.upto = E.rs_pending_hi;
    E.rs_pending_lo = E.rs_pending_hi = 0;
    return e;
}

// the argument block of an epoch's launch, stored at wc_dev
int fill_wave_cold(TardisMcContext *ctx, const WaveCall &E, int epoch, const mc::EstimatorLog &lg, mc::WaveCold *wc_dev)
{
    const bool vq = E.vq, vpk = E.call->vpk;
    mc::WaveCold &wc = ctx->wv.wave_cold_host[epoch & 1];
    wc.P = E.P; wc.D = ctx->problem_host; wc.log = lg; wc.seeded_states = E.cur_states;
    wc.chunk_first = 0; wc.chunk_count = E.n;
    wc.launch = ctx->wv.seed_chk.as<mc::LaunchRec>();
    wc.vp_scratch = ctx->wv.vp_scratch.as<mc::VpResult>();
    wc.vp_park = (vpk && !E.vq_on && ctx->wv.vp_carry_min_active > 0) ? ctx->wv.vp_park.as<mc::VpPark>() : nullptr;
    wc.vp_carry_min_active = ctx->wv.vp_carry_min_active; wc.trk_defer = E.trk_defer;
    wc.save = E.may_suspend ? E.cur_save : nullptr;
    wc.wsave = E.may_suspend ? E.cur_wsave : nullptr;
    wc.resume = epoch > 0 ? 1 : 0;
    wc.drain_split = E.split_armed ? 64 : (E.compact_armed ? ctx->wv.drain_compact : 0);  // (the most live lanes a wave whose supply has run out suspends with)
    wc.suspended = ctx->wv.suspended_dev.as<unsigned>();
    wc.vq_req = E.vq_on ? ctx->wv.vq_req.as<mc::VolleyRequest>() : nullptr;
    wc.vq_items = E.vq_on ? ctx->wv.vq_items.as<unsigned>() : nullptr;
    wc.vq_count = vq ? ctx->wv.vq_count.as<unsigned>() : nullptr;
    wc.vq_jsave = vq ? ctx->wv.vq_jsave.as<double>() : nullptr;
    wc.log_continue = vq ? 1 : 0;
    wc.log_gen = E.log_gen;
    wc.rng_complete = ctx->wv.rng_complete;
    wc.sweep_start_held = (E.sweep_skip && (ctx->sw.sweep_start_held < 0 ? SWEEP_START_HELD_AUTO : ctx->sw.sweep_start_held)) ? 1 : 0;
    wc.sweep_skip = E.sweep_skip; wc.sk_ct_off = ctx->sw.sk_ct_off; wc.sk_pn_off = ctx->sw.sk_pn_off; wc.sk_margin = ctx->sw.sk_margin;
    HIP_TRY(ctx, store_value(E.st, wc_dev, wc));
    return TARDIS_MC_OK;
}

// Split launch (see epoch_split): the same epoch for waves [waves1, waves) on the passes' stream es, behind the estimator passes of the previous epoch
int launch_second_half(TardisMcContext *ctx, WaveCall &E, int epoch, int waves1, hipStream_t es, mc::WaveCold *wc_dev)
{
    const mc::WaveCold &wc = ctx->wv.wave_cold_host[epoch & 1];
    mc::WaveCold wc2 = wc;  // every per-wave array starts waves1 waves further on
    wc2.seeded_states = wc.seeded_states + (size_t)waves1 * 64 * mc::WV_STATE_STRIDE;
    if (wc.save) wc2.save = wc.save + (size_t)waves1 * 64;
    if (wc.wsave) wc2.wsave = wc.wsave + waves1;
    if (wc.vp_scratch) wc2.vp_scratch = wc.vp_scratch + (size_t)waves1 * 64 * mc::VP_ROUND;
    if (wc.vp_park) wc2.vp_park = wc.vp_park + (size_t)waves1 * 64;
    HIP_TRY(ctx, hipStreamWaitEvent(es, ctx->wv.ev_split[0], 0));
    HIP_TRY(ctx, store_value(es, wc_dev + 1, wc2));
    HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_split[1], es));
    hipLaunchKernelGGL(E.w->fn, dim3(E.waves - waves1), dim3(64), E.w->lds, es, E.hot, (const mc::WaveCold *)(wc_dev + 1));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_split[2], es));
    HIP_TRY(ctx, hipStreamWaitEvent(E.st, ctx->wv.ev_split[2], 0));  // (what follows on the engine's stream -- the read-back, the next epoch -- follows both)
    E.split_w2 = (double)(E.waves - waves1) / (double)E.waves;
    return TARDIS_MC_OK;
}

// Volley queue, the rest of an epoch: the estimator passes run when a wave reports a full log region, and once at the end of the call.  The queue is on for the
// bulk of a call; once a launch requests fewer v-packets than keep the tracer's lanes busy the launches are bound by their longest v-packet, not by work -- the
// rest of the call (the drain of the longest-lived packets) runs in ONE launch with the wave kernel's own pooled volleys
int wave_epoch_tail_volley_queue(TardisMcContext *ctx, WaveCall &E, const mc::EstimatorLog &lg)
{
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_chunk[4]));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_chunk[2], ctx->ev_chunk[3]));
    ctx->sum_prop_ms += ms;
    const bool last = ctx->wv.suspended_host[0] == 0;
    if (last || ctx->wv.suspended_host[1] > 0) {
        HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_post[0], E.st));
        HIP_TRY(ctx, estimator_passes(ctx, E, lg, 0, E.st));
        HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_post[1], E.st));
        HIP_TRY(ctx, hipMemsetAsync(lg.region_count, 0, (size_t)(E.log->n_chunks + 1) * sizeof(unsigned), E.st));
        ++E.log_gen;
        HIP_TRY(ctx, hipEventSynchronize(ctx->wv.ev_post[1]));
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->wv.ev_post[0], ctx->wv.ev_post[1]));
        ctx->sum_post_ms += ms;
    }
    if (last) { E.call_complete = true; return TARDIS_MC_OK; }
    const long long vq_min_items = ctx->wv.vq_min_items >= 0 ? ctx->wv.vq_min_items : (long long)E.call->cus * 4 * 64 * 8;
    if (E.vq_on && (long long)ctx->wv.suspended_host[4] < vq_min_items) E.vq_on = false;
    return TARDIS_MC_OK;
}

// CU partition, the rest of an epoch: the host first learns whether this was the last epoch.  If not, its passes run on the pass stream's CUs beside
// the next epoch; the last epoch's passes take the propagation stream (its CUs are idle now) -- after the passes still
// running on the pass stream, with which they share the scratch copy of the records
int wave_epoch_tail_cu_partition(TardisMcContext *ctx, WaveCall &E, const mc::EstimatorLog &lg, int b)
{
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_chunk[4]));
    float pms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&pms, ctx->ev_chunk[2], ctx->ev_chunk[3]));
    ctx->sum_prop_ms += pms;
    const bool last = *ctx->wv.suspended_host == 0;
    hipStream_t ps = ctx->wv.stream_pass_m;
    if (last) {
        HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_join, ctx->wv.stream_pass_m));
        HIP_TRY(ctx, hipStreamWaitEvent(E.st, ctx->wv.ev_join, 0));
        ps = E.st;
    } else HIP_TRY(ctx, hipStreamWaitEvent(ps, ctx->ev_chunk[3], 0));
    HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_post[2 * b], ps));
    HIP_TRY(ctx, estimator_passes(ctx, E, lg, b, ps));
    HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_post[2 * b + 1], ps));
    ctx->wv.post_pending[b] = true;
    if (last) { E.call_complete = true; return TARDIS_MC_OK; }
    E.records_done += (double)std::min<unsigned long long>((unsigned long long)ctx->wv.suspended_host[6], E.pool_chunks) * (double)E.log->region_capacity;
    if (ctx->wv.suspended_host[2] > 0) E.split_armed = false;
    return TARDIS_MC_OK;
}

// Drain compaction (drain_compact): some waves have suspended with few live lanes -- what is left on the grid?  Packed into full waves when nothing is left to
// hand out and it frees more than half of the grid
int compact_drain(TardisMcContext *ctx, WaveCall &E)
{
    hipStream_t st = E.st;
    unsigned *cen = ctx->wv.drain_census.as<unsigned>();
    HIP_TRY(ctx, hipMemsetAsync(cen, 0, 8 * sizeof(unsigned), st));
    hipLaunchKernelGGL(mc::drain_census_kernel, dim3(E.waves_cur), dim3(64), 0, st, E.cur_save, E.cur_wsave, E.waves_cur, E.n, cen);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->wv.suspended_host + 8, cen, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const unsigned live = ctx->wv.suspended_host[8], reserved = ctx->wv.suspended_host[9], waiting = ctx->wv.suspended_host[11];
    const unsigned density = (unsigned)ctx->wv.drain_pack_lanes;
    const int packed = (int)((live + density - 1u) / density);
    if (!(reserved == 0 && waiting == 0 && live > 0 && 2 * packed <= E.waves_cur)) return TARDIS_MC_OK;
    const int g = ctx->wv.compactions & 1;
    HIP_TRY(ctx, ctx->wv.lane_save_c[g].ensure((size_t)packed * 64 * sizeof(mc::LaneSave)));
    HIP_TRY(ctx, ctx->wv.wave_save_c[g].ensure((size_t)packed * sizeof(mc::WaveSave)));
    HIP_TRY(ctx, ctx->wv.seeded_states_c[g].ensure((size_t)packed * 64 * mc::WV_STATE_STRIDE * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMemsetAsync(cen + 4, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(mc::drain_compact_kernel, dim3(E.waves_cur), dim3(64), 0, st, (const mc::LaneSave *)E.cur_save, (const mc::WaveSave *)E.cur_wsave,
                       (const uint32_t *)E.cur_states, E.waves_cur, ctx->wv.lane_save_c[g].as<mc::LaneSave>(), ctx->wv.seeded_states_c[g].as<uint32_t>(), cen + 4, density);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(mc::drain_compact_finish_kernel, dim3((unsigned)((packed * 64 + 255) / 256)), dim3(256), 0, st, ctx->wv.lane_save_c[g].as<mc::LaneSave>(),
                       ctx->wv.wave_save_c[g].as<mc::WaveSave>(), (const unsigned *)(cen + 4), E.n, density);
    HIP_TRY(ctx, hipGetLastError());
    E.cur_save = ctx->wv.lane_save_c[g].as<mc::LaneSave>(); E.cur_wsave = ctx->wv.wave_save_c[g].as<mc::WaveSave>(); E.cur_states = ctx->wv.seeded_states_c[g].as<uint32_t>();
    E.waves_cur = packed;
    ctx->wv.compactions += 1;
    if (packed < 2 * E.call->cus || (int)density <= 2 * ctx->wv.drain_compact) E.compact_armed = false;  // (nothing left worth freeing / the packed waves would suspend again at once)
    return TARDIS_MC_OK;
}

// Result streaming, at a launch boundary: packets [0, handed) have been handed out; those of them still in flight (suspended lanes, reserved blocks) go on the late
// list, the range [upto, handed) is unpacked now -- in front of the next launch on the same stream -- and copied by the host beside that launch
int stream_range(TardisMcContext *ctx, WaveCall &E)
{
    const long long handed = (long long)std::min<unsigned long long>(*ctx->rs.next_host, (unsigned long long)E.n);
    if (handed - ctx->rs.upto < ctx->rs.min_packets) return TARDIS_MC_OK;
    hipLaunchKernelGGL(mc::late_list_kernel, dim3(E.waves_cur), dim3(64), 0, E.st, (const mc::LaneSave *)E.cur_save, (const mc::WaveSave *)E.cur_wsave, E.waves_cur, ctx->rs.upto, handed,
                       ctx->rs.late.as<unsigned>(), ctx->rs.late_count.as<unsigned>(), ctx->rs.late_capacity);
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->pk.track) {
        const long long cnt = handed - ctx->rs.upto;
        hipLaunchKernelGGL(mc::tracker_unpack_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, E.st, ctx->problem_host, ctx->rs.upto, cnt, (const unsigned *)nullptr);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->rs.ev, E.st));
    E.rs_pending_lo = ctx->rs.upto; E.rs_pending_hi = handed;
    return TARDIS_MC_OK;
}

// Result streaming, after the last launch: what was streamed is [0, upto) minus the late list, whose entries are gathered for get_results.  The list's length is
// read back here (the call has synchronised with every launch already).  *unpack_from: the first packet whose tracker records are still to be unpacked.
int gather_late_results(TardisMcContext *ctx, long long *unpack_from)
{
    unsigned n_late = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_late, ctx->rs.late_count.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_late > ctx->rs.late_capacity) return TARDIS_MC_OK;  // (the list overflowed -- get_results copies everything)
    ctx->rs.valid = true;
    ctx->rs.n_late = n_late;
    *unpack_from = ctx->rs.upto;
    if (n_late == 0) return TARDIS_MC_OK;
    if (ctx->pk.track) {
        hipLaunchKernelGGL(mc::tracker_unpack_kernel, dim3((n_late + 255) / 256), dim3(256), 0, ctx->stream, ctx->problem_host, 0LL, (long long)n_late, ctx->rs.late.as<unsigned>());
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, ctx->rs.vals.ensure((size_t)16 * n_late * 8));
    void *dev[16];
    per_packet_device_arrays(ctx, dev);
    for (int a = 0; a < 16; ++a)
        if (ctx->rs.dst[a] && dev[a]) {
            hipLaunchKernelGGL(mc::gather64_kernel, dim3((n_late + 255) / 256), dim3(256), 0, ctx->stream, (const unsigned long long *)dev[a],
                               ctx->rs.late.as<unsigned>(), (long long)n_late, ctx->rs.vals.as<unsigned long long>() + (size_t)a * n_late);
            HIP_TRY(ctx, hipGetLastError());
        }
    return TARDIS_MC_OK;
}

// One epoch: the pool of this epoch's log, the launch (or the two of a split epoch), the read-back of what is suspended, the estimator passes, and what the
// modes of the call do between two launches.  Sets E.call_complete when nothing is left suspended.
int run_wave_epoch(TardisMcContext *ctx, WaveCall &E, int epoch)
{
    const LogSizing &s = *E.log;
    const int cus = E.call->cus, waves = E.waves;
    const bool vq = E.vq;
    hipStream_t st = E.st;
    const int b = s.n_sets == 2 ? (epoch & 1) : 0;
    hipStream_t es = s.n_sets == 2 ? ctx->wv.stream2 : st;  // the estimator passes of an epoch run beside the next epoch
    if (ctx->wv.post_pending[b]) {  // this buffer set was used two epochs ago: its estimator passes must be over
        float ms = 0.f;
        HIP_TRY(ctx, hipEventSynchronize(ctx->wv.ev_post[2 * b + 1]));
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->wv.ev_post[2 * b], ctx->wv.ev_post[2 * b + 1]));
        ctx->sum_post_ms += ms;
        ctx->wv.post_pending[b] = false;
    }
    mc::EstimatorLog lg{};
    lg.tiles_per_shell = E.w->tiles;
    lg.records = log_set_ptr<mc::LineVisitRecord>(s, ctx->wv.log_records, b);
    lg.keys = log_set_ptr<unsigned>(s, ctx->wv.log_keys, b);
    E.pool_chunks = s.n_chunks;
    if (s.tail_plan) {
        const double records_est = (double)E.n * ctx->wv.traces_per_packet;  // (what the call will log, by the last call's measure)
        const double bulk = records_est - E.records_done - s.tail_records;  // what is left before the tail
        if (bulk > 0.0 && bulk <= (double)s.n_chunks * (double)s.region_capacity)
            E.pool_chunks = std::min<unsigned long long>(s.n_chunks, std::max<unsigned long long>((unsigned long long)waves * (E.w->key.shell_log ? (unsigned long long)(ctx->n_shells + 4) : 1ull),
                                                                                                  (unsigned long long)(bulk / (double)s.region_capacity) + 1ull));
    }
    lg.n_regions = (int)E.pool_chunks;
    lg.region_capacity = s.region_capacity;
    lg.region_count = ctx->wv.log_cursor[b].as<unsigned>();
    lg.pool_next = lg.region_count + s.n_chunks;
    // (volley queue: the launches of a call go on appending to the same log regions until one of them is full)
    if (!vq || epoch == 0) HIP_TRY(ctx, hipMemsetAsync(lg.region_count, 0, (size_t)(s.n_chunks + 1) * sizeof(unsigned), st));
    HIP_TRY(ctx, hipMemsetAsync(ctx->wv.suspended_dev.p, 0, 4 * sizeof(unsigned), st));
    if (vq) HIP_TRY(ctx, hipMemsetAsync(ctx->wv.vq_count.p, 0, 2 * sizeof(unsigned), st));
    mc::WaveCold *wc_dev = ctx->wv.wave_cold_dev.as<mc::WaveCold>() + 2 * (epoch & 1);
    int rc = fill_wave_cold(ctx, E, epoch, lg, wc_dev);
    if (rc) return rc;
    // split launch (see epoch_split): the estimator passes of the previous epoch are queued (or running) on the second stream
    // (not the drain launch of a tail-split call: its lanes are the call's critical path, half of them would start behind the bulk's passes)
    const bool split = ctx->wv.epoch_split && !s.want_compact && !vq && !E.cu_masked && !s.tail_plan && s.n_sets == 2 && epoch > 0 && es != st && ctx->wv.post_pending[b ^ 1] && waves >= 8 * cus;
    const int waves1 = split ? waves / 2 : E.waves_cur;
    if (split) HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_split[0], st));  // (pool, counters and argument block of this epoch are in place)
    HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[2], st));
    hipLaunchKernelGGL(E.w->fn, dim3(waves1), dim3(64), E.w->lds, st, E.hot, (const mc::WaveCold *)wc_dev);
    HIP_TRY(ctx, hipGetLastError());
    E.split_w2 = 0.0;
    if (split && (rc = launch_second_half(ctx, E, epoch, waves1, es, wc_dev))) return rc;
    if (E.vq_on) {  // the v-packets this launch requested (the item count is read on the device: an empty list costs a launch)
        const size_t geo_lds = (size_t)4 * (size_t)ctx->n_shells * sizeof(double);
        const int tracer_waves = cus * 4 * ctx->wv.vq_tracer_waves_per_simd;
        if (E.call->full) hipLaunchKernelGGL(mc::vpacket_trace_kernel<true>, dim3(tracer_waves), dim3(64), geo_lds, st, (const mc::WaveCold *)wc_dev);
        else hipLaunchKernelGGL(mc::vpacket_trace_kernel<false>, dim3(tracer_waves), dim3(64), geo_lds, st, (const mc::WaveCold *)wc_dev);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[3], st));
    if (E.may_suspend) {  // (read back before the estimator passes are queued: the host learns early whether another epoch follows)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->wv.suspended_host, ctx->wv.suspended_dev.p, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        if (vq) HIP_TRY(ctx, hipMemcpyAsync(ctx->wv.suspended_host + 4, ctx->wv.vq_count.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        if (s.region_capacity > 0) HIP_TRY(ctx, hipMemcpyAsync(ctx->wv.suspended_host + 6, lg.pool_next, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        if (E.streaming) HIP_TRY(ctx, hipMemcpyAsync(ctx->rs.next_host, ctx->next_packet.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[4], st));
    }
    ctx->launches += 1;
    if (vq) return wave_epoch_tail_volley_queue(ctx, E, lg);
    if (E.cu_masked) return wave_epoch_tail_cu_partition(ctx, E, lg, b);
    if (es != st) HIP_TRY(ctx, hipStreamWaitEvent(es, ctx->ev_chunk[3], 0));
    HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_post[2 * b], es));
    HIP_TRY(ctx, estimator_passes(ctx, E, lg, b, es));
    HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_post[2 * b + 1], es));
    ctx->wv.post_pending[b] = true;
    ctx->wv.prop_pending = true;
    if (!E.may_suspend) { E.call_complete = true; return TARDIS_MC_OK; }  // (no log: the kernel adds its terms directly and never suspends; the call stays asynchronous)
    // (result streaming: the range unpacked before this launch is copied to the caller's arrays now, while the launch runs)
    if (E.streaming) HIP_TRY(ctx, rs_copy_pending(ctx, E));
    // is anything suspended?  (the only host synchronisation of a call: once per epoch)
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_chunk[4]));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_chunk[2], ctx->ev_chunk[3]));
    if (E.split_w2 > 0.0) {  // a split epoch counts with the wave-weighted duration of its two launches (= the time a launch of the whole grid stands for)
        float ms2 = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms2, ctx->wv.ev_split[1], ctx->wv.ev_split[2]));
        ms = (float)((1.0 - E.split_w2) * (double)ms + E.split_w2 * (double)ms2);
    }
    ctx->sum_prop_ms += ms;
    ctx->wv.prop_pending = false;
    if (*ctx->wv.suspended_host == 0) { E.call_complete = true; return TARDIS_MC_OK; }
    E.records_done += (double)std::min<unsigned long long>((unsigned long long)ctx->wv.suspended_host[6], E.pool_chunks) * (double)s.region_capacity;
    if (ctx->wv.suspended_host[2] > 0) E.split_armed = false;  // (the drain has been split off: the next launch runs to the end)
    if (E.compact_armed && ctx->wv.suspended_host[2] > 0 && (rc = compact_drain(ctx, E))) return rc;
    if (E.streaming) return stream_range(ctx, E);
    return TARDIS_MC_OK;
}

// The wave kernel (variants 2 / 3 / 4): one packet supply for the whole call, launched in epochs (see LaneSave)
int run_wave_kernel(TardisMcContext *ctx, PropagateCall &call, mc::GroupArgs &P)
{
    const bool vpk = call.vpk, full = call.full, vq = call.plan.variant == 4;
    const int cus = call.cus;
    const long long n = ctx->pk.n_packets;
    const mc::DeviceProblem &F = ctx->problem_host;
    if (n >= (1LL << 31)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "more than 2^31 packets per propagate call");
    WaveChoice w{};
    int rc = choose_wave_kernel(ctx, call, P, w);
    if (rc) return rc;
    if (w.compact_walk) {
        P.cum16 = ctx->wt.cum16.as<unsigned short>(); P.rec16 = ctx->wt.rec16.as<mc::WalkRec>(); P.quad_info = ctx->wt.quad_info.as<int2>();
        P.cum16_stride = ctx->wt.cum16_stride;
        P.line_block = ctx->wt.line_block_c.as<int2>();
        P.hot_sec = ctx->wt.have_hot ? ctx->wt.hot_sec.as<unsigned>() : nullptr;
        P.blk_tab = ctx->wt.blk_tab.as<int2>();
        P.hot_stride = (unsigned)(16u * (unsigned)ctx->n_levels);
    }
    ctx->pg.progress_wave = true;  // (one packet supply for the whole call: next_packet counts the packets handed out)
    // (volley queue: more waves than the chip holds at once -- a wave that suspends frees its slot, and the more packets are
    // in flight the more v-packets every tracer launch has to spread over its lanes)
    // CU partition (pass_cus): only for calls long enough to run as several epochs -- the passes of an epoch then have the next one to hide behind
    const int n_xcd = 8;  // gfx950: 8 XCDs x 32 CUs; the bits of a queue's CU mask are interleaved over the XCDs (bit k -> XCD k % 8)
    const bool cu_split = ctx->wv.pass_cus > 0 && !vq && ctx->wv.log_sets != 1 && cus == 32 * n_xcd && n >= 30000000LL;
    const int cus_prop = cu_split ? cus - n_xcd * ctx->wv.pass_cus : cus;
    const int waves = (int)std::max<long long>(1, std::min<long long>((n + 63) / 64, (long long)cus_prop * std::min(w.waves_per_cu, w.max_waves_per_cu) * (vq ? ctx->wv.vq_oversubscribe : 1)));
    if (ctx->el.track_full) {  // (a wave leaves a partly filled chunk behind at every launch it takes part in: room for four launches)
        rc = setup_event_log(ctx, ctx->problem_host, 4LL * waves);
        if (rc) return rc;
    }
    if (ctx->bf.on && (rc = setup_segment_log(ctx, ctx->problem_host, 4LL * waves))) return rc;
    if (ctx->wv.events_host && ctx->wv.ev_events && hipEventQuery(ctx->wv.ev_events) == hipSuccess && ctx->wv.events_host[1] > 0)
        ctx->wv.traces_per_packet = (double)ctx->wv.events_host[0] / (double)ctx->wv.events_host[1];
    if (1.1 * ctx->wv.traces_per_packet > ctx->wv.log_budget_per_packet) ctx->wv.log_budget_per_packet = 1.3 * ctx->wv.traces_per_packet;
    LogSizing s{};
    rc = size_line_log(ctx, call, w, n, waves, cu_split, s);
    if (rc) return rc;
    WaveCall E{};
    E.call = &call; E.w = &w; E.log = &s; E.n = n; E.waves = waves; E.vq = vq;
    E.may_suspend = s.region_capacity > 0 || vq;  // (waves take chunks dynamically: every launch can suspend)
    E.split_armed = s.want_split && !s.want_compact;
    E.compact_armed = s.want_compact;
    E.waves_cur = waves;
    ctx->wv.compactions = 0;
    for (int b = 0; b < s.n_sets; ++b) {
        if (!(s.set1_inside && b == 1)) {
            HIP_TRY(ctx, ctx->wv.log_records[b].ensure(s.set_records * sizeof(mc::LineVisitRecord)));
            HIP_TRY(ctx, ctx->wv.log_keys[b].ensure(s.set_records * sizeof(unsigned)));
            if (!w.partition) HIP_TRY(ctx, ctx->wv.log_sorted[b].ensure(s.set_records * sizeof(unsigned)));
        }
        HIP_TRY(ctx, ctx->wv.log_bins[b].ensure((size_t)(4 * (w.n_bins + 2) + ctx->n_shells + 2) * sizeof(unsigned)));
        HIP_TRY(ctx, ctx->wv.log_cursor[b].ensure((size_t)(s.n_chunks + 2) * sizeof(unsigned)));  // chunk counts | pool counter
    }
    if (w.partition) HIP_TRY(ctx, ctx->wv.log_part.ensure(s.set_records * sizeof(mc::LineVisitRecord)));
    if (s.n_sets == 2 && !ctx->wv.stream2) {
        int prio_lo = 0, prio_hi = 0;  // (the estimator passes' stream: highest priority, their workgroups are dispatched first)
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->wv.stream2, hipStreamNonBlocking, prio_hi));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->wv.ev_join, hipEventDisableTiming));
    }
    E.cu_masked = cu_split && s.n_sets == 2;
    if (E.cu_masked && ctx->wv.pass_cus_built != ctx->wv.pass_cus) {
        if (ctx->wv.stream_prop_m) { HIP_TRY(ctx, hipStreamSynchronize(ctx->wv.stream_prop_m)); HIP_TRY(ctx, hipStreamDestroy(ctx->wv.stream_prop_m)); ctx->wv.stream_prop_m = nullptr; }
        if (ctx->wv.stream_pass_m) { HIP_TRY(ctx, hipStreamSynchronize(ctx->wv.stream_pass_m)); HIP_TRY(ctx, hipStreamDestroy(ctx->wv.stream_pass_m)); ctx->wv.stream_pass_m = nullptr; }
        uint32_t m_prop[8] = {0, 0, 0, 0, 0, 0, 0, 0}, m_pass[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int bit = 0; bit < cus; ++bit) {  // the first cus_prop bits = (32 - pass_cus) CUs of every XCD
            if (bit < cus_prop) m_prop[bit >> 5] |= 1u << (bit & 31);
            else m_pass[bit >> 5] |= 1u << (bit & 31);
        }
        HIP_TRY(ctx, hipExtStreamCreateWithCUMask(&ctx->wv.stream_prop_m, 8, m_prop));
        HIP_TRY(ctx, hipExtStreamCreateWithCUMask(&ctx->wv.stream_pass_m, 8, m_pass));
        if (!ctx->wv.ev_fork_m) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->wv.ev_fork_m, hipEventDisableTiming));
        if (!ctx->wv.ev_join_m) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->wv.ev_join_m, hipEventDisableTiming));
        ctx->wv.pass_cus_built = ctx->wv.pass_cus;
    }
    for (int k = 0; k < 4; ++k)
        if (!ctx->wv.ev_post[k]) HIP_TRY(ctx, hipEventCreate(&ctx->wv.ev_post[k]));
    // ---- per-lane MT19937 state buffers, launch records, suspended lanes
    HIP_TRY(ctx, ctx->wv.seeded_states.ensure((size_t)waves * 64 * mc::WV_STATE_STRIDE * sizeof(uint32_t)));
    HIP_TRY(ctx, ctx->wv.seed_chk.ensure((size_t)std::max<long long>(n, 1) * sizeof(mc::LaunchRec)));
    HIP_TRY(ctx, ctx->wv.lane_save.ensure((size_t)waves * 64 * sizeof(mc::LaneSave)));
    HIP_TRY(ctx, ctx->wv.wave_save.ensure((size_t)waves * sizeof(mc::WaveSave)));
    HIP_TRY(ctx, ctx->wv.suspended_dev.ensure(4 * sizeof(unsigned)));
    E.cur_save = ctx->wv.lane_save.as<mc::LaneSave>(); E.cur_wsave = ctx->wv.wave_save.as<mc::WaveSave>(); E.cur_states = ctx->wv.seeded_states.as<uint32_t>();
    if (s.want_compact) HIP_TRY(ctx, ctx->wv.drain_census.ensure(8 * sizeof(unsigned)));
    if (!ctx->wv.suspended_host) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->wv.suspended_host, 16 * sizeof(unsigned), hipHostMallocDefault));
    if (vq) {
        HIP_TRY(ctx, ctx->wv.vq_req.ensure((size_t)waves * 64 * sizeof(mc::VolleyRequest)));
        HIP_TRY(ctx, ctx->wv.vq_items.ensure((size_t)waves * 64 * mc::VP_ROUND * sizeof(unsigned)));
        HIP_TRY(ctx, ctx->wv.vq_count.ensure(2 * sizeof(unsigned)));
        HIP_TRY(ctx, ctx->wv.vq_jsave.ensure((size_t)waves * 2 * (size_t)ctx->n_shells * sizeof(double)));
        if ((size_t)waves * 64 >= (1u << 29)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "too many lanes for the volley queue's item words");
    }
    if (vpk) HIP_TRY(ctx, ctx->wv.vp_scratch.ensure((size_t)waves * 64 * mc::VP_ROUND * sizeof(mc::VpResult)));
    if (vpk && ctx->wv.vp_carry_min_active > 0) HIP_TRY(ctx, ctx->wv.vp_park.ensure((size_t)waves * 64 * sizeof(mc::VpPark)));
    HIP_TRY(ctx, ctx->wv.wave_cold_dev.ensure(4 * sizeof(mc::WaveCold)));  // (per epoch parity: the launch's block and the second launch's of a split epoch)
    ctx->wv.wave_cold_host.resize(2);
    for (hipEvent_t &e : ctx->wv.ev_split)
        if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_start, st));
    if (call.tune_slot >= 0) HIP_TRY(ctx, hipEventRecord(ctx->lt.ev_tune[0], st));
    if (E.cu_masked) {  // everything of this call runs on the masked stream from here on; it is joined to the engine's stream at the end
        HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_fork_m, ctx->stream));
        st = ctx->wv.stream_prop_m;
        HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->wv.ev_fork_m, 0));
    }
    E.st = st;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[0], st));
    if (n > 0) {
        // lazy seeding: only word 397 of every start state is precomputed; the refills continue the init_genrand chains
        mc::LaunchPrepArgs la{};
        la.r0 = F.r0; la.mu0 = F.mu0; la.nu0 = F.nu0; la.e0 = F.e0; la.nu_line = P.nu_line;
        la.seeds = ctx->pk.seeds.as<uint32_t>();
        la.bucket_first = P.bucket_first; la.bucket_shift = P.bucket_shift; la.bucket_n = P.bucket_n; la.n_lines = P.n_lines;
        la.bucket_kmin = P.bucket_kmin; la.t_exp = P.t_exp;
        la.out = ctx->wv.seed_chk.as<mc::LaunchRec>(); la.first = 0; la.count = n;
        if (full) hipLaunchKernelGGL(mc::launch_prep_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, la);
        else hipLaunchKernelGGL(mc::launch_prep_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, la);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[1], st));
    E.P = P;
    mc::WaveHot &hot = E.hot;
    hot.nu_line = P.nu_line; hot.tau_t = w.key.nt ? P.nt_t : P.tau_t; hot.n_lines = P.n_lines; hot.n_shells = P.n_shells;
    hot.disable_line_scattering = P.disable_line_scattering; hot.debug_flags = P.debug_flags;
    hot.t_exp = P.t_exp;
    // cut-offs of the sweep / walk phases (lanes still busy when the wave moves on): 8 / 8 by default.  Where most blocks are
    // entered through hot sectors the event phase is shorter and later cut-offs pay: 12 / 12 measured -2.5 % on the heavy-tailed
    // configs[2] tables, +2 % on the uniform ones (profiles/r04_cutoffs.txt) -- hence only there, and never against an option
    const bool mostly_hot = ctx->wt.have_hot && 2 * ctx->wt.n_hot_blocks > (long long)ctx->n_levels;
    hot.ls_min_active = (!ctx->wv.ls_min_active_user && mostly_hot) ? 12 : ctx->wv.ls_min_active;
    hot.ls_max_steps = ctx->wv.ls_max_steps;
    hot.walk_min_active = (!ctx->wv.walk_min_active_user && mostly_hot) ? 16 : ctx->wv.walk_min_active;  // (12 until round 6; with the leaner sweep 16: -1.2 %, profiles/r06_cutoffs.txt)
    hot.vq_min_active = ctx->wv.vq_min_active;
    {   // the deferred tracker record: only where the instantiation has it and the packed word holds every shell and line of the problem
        const WaveKernelKey &k = w.key;
        const bool has_defer = k.track && k.lane_sweep && !k.vpk && !k.full_tracking && !k.xwalk;
        const bool fits = mc::tracker_pack_fits(P.n_shells, P.n_lines) && (ctx->wv.tracker_pack_max_lines <= 0 || P.n_lines <= ctx->wv.tracker_pack_max_lines);
        E.sweep_skip = w.sweep_skip;
        E.trk_defer = (has_defer && ctx->wv.tracker_defer && fits) ? 1 : 0;  // (-> WaveCold::trk_defer of every launch of the call)
        ctx->wv.last_tracker_defer = has_defer ? E.trk_defer : -1;
    }
    hot.line_block = P.line_interaction_type != 0 ? P.line_block : nullptr;
    ctx->wv.post_pending[0] = ctx->wv.post_pending[1] = false;
    ctx->wv.prop_pending = false;
    // result streaming: only the plain epoch loop (no volley queue, no CU partition), with the tracker unpacking it needs done per range
    E.streaming = call.rs_armed && !vq && !E.cu_masked && E.may_suspend && n >= ctx->rs.min_packets;
    if (E.streaming) {
        ctx->rs.late_capacity = (unsigned)std::min<long long>(n, (long long)waves * 64 * 16);
        HIP_TRY(ctx, ctx->rs.late.ensure((size_t)ctx->rs.late_capacity * sizeof(unsigned)));
        HIP_TRY(ctx, ctx->rs.late_count.ensure(sizeof(unsigned)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->rs.late_count.p, 0, sizeof(unsigned), st));
        if (!ctx->rs.stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->rs.stream, hipStreamNonBlocking));
        if (!ctx->rs.ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->rs.ev, hipEventDisableTiming));
        if (!ctx->rs.next_host) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->rs.next_host, sizeof(unsigned long long), hipHostMallocDefault));
    }
    const int max_epochs = 1 << 20;
    E.vq_on = vq;
    E.call_complete = n <= 0;
    for (int epoch = 0; n > 0 && epoch < max_epochs && !E.call_complete; ++epoch)
        if ((rc = run_wave_epoch(ctx, E, epoch))) return rc;
    if (E.streaming && E.call_complete) HIP_TRY(ctx, rs_copy_pending(ctx, E));  // (a range queued before the last launch)
    if (!E.call_complete)  // (packets would be left suspended in lane_save, outputs and estimators silently incomplete)
        return fail(ctx, TARDIS_MC_ERR_STATE, "propagate: %d launches did not finish the call (waves still suspended)", max_epochs);
    if (E.cu_masked) {  // both masked streams join the engine's stream
        HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_join, ctx->wv.stream_pass_m));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->wv.ev_join, 0));
        HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_join_m, st));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->wv.ev_join_m, 0));
    } else if (s.n_sets == 2 && (ctx->wv.post_pending[0] || ctx->wv.post_pending[1])) {
        HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_join, ctx->wv.stream2));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->wv.ev_join, 0));
    }
    ctx->wv.wave_epoch_mode = true;
    ctx->pg.progress_done = true;  // (every packet has been handed out and has ended: the host read "nothing suspended")
    long long unpack_from = 0;
    if (E.streaming && ctx->rs.upto > 0 && (rc = gather_late_results(ctx, &unpack_from))) return rc;
    if (ctx->pk.track && n > unpack_from) {  // the wave kernel's tracker records -> the boundary's arrays
        hipLaunchKernelGGL(mc::tracker_unpack_kernel, dim3((unsigned)((n - unpack_from + 255) / 256)), dim3(256), 0, ctx->stream, F, unpack_from, n - unpack_from,
                           (const unsigned *)nullptr);
        HIP_TRY(ctx, hipGetLastError());
    }
    return TARDIS_MC_OK;
}

// The group kernel (variant 1), in chunks: the MT19937 states are seeded per chunk by a lane-per-packet kernel
int run_group_kernel(TardisMcContext *ctx, const PropagateCall &call, const mc::GroupArgs &P)
{
    const bool vpk = call.vpk;
    const int cus = call.cus;
    ctx->wv.wave_epoch_mode = false;
    long long chunk = std::min<long long>(std::max<long long>(ctx->pk.n_packets, 1), ctx->chunk_packets);
    HIP_TRY(ctx, ctx->wv.seeded_states.ensure((size_t)chunk * mc::WV_STATE_STRIDE * sizeof(uint32_t)));
    // group size: 8 lanes per packet pays off when the sweeps between events are short (sparse line lists)
    const int G = ctx->group_size == 8 ? 8 : (ctx->group_size == 16 ? 16 : ((ctx->n_lines <= 100000 && !vpk) ? 8 : 16));
    const int block = 256;
    const size_t lds = G == 8 ? mc::group_kernel_lds_bytes<8, 256>(ctx->n_shells) : mc::group_kernel_lds_bytes<16, 256>(ctx->n_shells);
    if (lds > 160 * 1024) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "n_shells too large for the LDS J/nu_bar accumulator");
    const int blocks_per_cu = std::max(1, std::min(std::min(ctx->blocks_per_cu, 8), (int)((160 * 1024) / lds)));
    const GroupKernelKey key{call.full, ctx->pk.track, G, block, 4, vpk, call.plan.w64, vlog_li_call(ctx)};
    const GroupKernelFn k = find_kernel(GROUP_KERNELS, key);
    if (!k)
        return fail(ctx, TARDIS_MC_ERR_STATE, "propagate: no such instantiation of the group kernel: FULL, TRACK, G, BLOCK, OCC, VPK, WIDE, VLI = %s", key_text(key).c_str());
    record_kernel(ctx, 1, key);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_start, st));
    uint32_t *seeded = ctx->wv.seeded_states.as<uint32_t>();
    for (long long first = 0; first < ctx->pk.n_packets; first += chunk) {
        const long long count = std::min(chunk, ctx->pk.n_packets - first);
        const int ci = ctx->chunks_timed;
        while ((int)ctx->ev_chunk.size() < 4 * (ci + 1)) {
            hipEvent_t e;
            HIP_TRY(ctx, hipEventCreate(&e));
            ctx->ev_chunk.push_back(e);
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[4 * ci], st));
        hipLaunchKernelGGL(mc::seed_states_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st,
                           ctx->pk.seeds.as<uint32_t>(), seeded, first, count, mc::MT_N);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemsetAsync(ctx->next_packet.p, 0, sizeof(unsigned long long), st));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[4 * ci + 1], st));
        const int groups_per_block = block / G;
        long long want_blocks = (count + groups_per_block - 1) / groups_per_block;
        int blocks = (int)std::max<long long>(1, std::min<long long>(want_blocks, (long long)cus * blocks_per_cu));
        // (the group kernel updates the line estimators with atomics: logging its traces was measured and is a loss
        // there -- the record bookkeeping costs its redundant-lane event loop more than the deferred atomics do)
        hipLaunchKernelGGL(k, dim3(blocks), dim3(block), lds, st, P, seeded, first, count);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[4 * ci + 2], st));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_chunk[4 * ci + 3], st));
        ctx->chunks_timed = ci + 1;
    }
    return TARDIS_MC_OK;
}

// The cooperative kernels (variants 1 - 4): the problem on the device and the argument block both kernels take by value, then the runner of the plan's variant
int run_cooperative(TardisMcContext *ctx, PropagateCall &call)
{
    const bool wave_kernel = call.plan.variant == 2 || call.plan.variant == 3 || call.plan.variant == 4;
    ctx->problem_host = make_device_problem(ctx);
    const mc::DeviceProblem &F = ctx->problem_host;
    HIP_TRY(ctx, ctx->problem_dev.ensure(sizeof(mc::DeviceProblem)));
    HIP_TRY(ctx, store_value(ctx->stream, ctx->problem_dev.as<mc::DeviceProblem>(), ctx->problem_host));
    mc::GroupArgs P{};
    P.cold = ctx->problem_dev.as<mc::DeviceProblem>();
    P.n_shells = F.n_shells; P.n_lines = F.n_lines; P.n_trans = F.n_trans;
    P.line_interaction_type = F.line_interaction_type; P.disable_line_scattering = F.disable_line_scattering;
    P.debug_flags = F.debug_flags; P.n_est_copies = F.n_est_copies;
    P.t_exp = F.t_exp; P.sigma_thomson = F.sigma_thomson;
    P.tc = F.t_exp * mc::C_LIGHT; P.rcp_tc = 1.0 / P.tc;
    P.r_inner = F.r_inner; P.r_outer = F.r_outer; P.nu_line = F.nu_line; P.tau_t = F.tau_t; P.n_e = F.n_e; P.prob_t = F.prob_t;
    P.line_block = ctx->ot.line_block.as<int2>(); P.trans_rec = ctx->ot.trans_rec.as<int4>();
    P.cum_t = ctx->ot.cum_t.as<double>(); P.trans_nu = ctx->ot.trans_nu.as<double>();
    P.jblue_t = F.jblue_t; P.edot_t = F.edot_t; P.est_copy_stride = F.est_copy_stride;
    P.next_packet = F.next_packet;
    P.n_vpackets = F.n_vpackets; P.survival_probability = F.survival_probability; P.tau_russian = F.tau_russian;
    P.spawn_start = F.spawn_start; P.spawn_end = F.spawn_end; P.grid0 = F.grid0; P.grid_last = F.grid_last;
    P.delta_nu = F.delta_nu; P.vhist = F.vhist;
    P.bucket_first = ctx->ot.bucket_first.as<int>(); P.bucket_shift = ctx->ot.bucket_shift; P.bucket_n = ctx->ot.bucket_n;
    P.bucket_kmin = ctx->ot.bucket_kmin;
    P.tau_pfx = call.plan.screen_on ? ctx->sc.tau_pfx.as<double>() : nullptr;
    P.tau_rowsum = call.plan.screen_on ? ctx->sc.tau_rowsum.as<double>() : nullptr;
    while ((int)ctx->ev_chunk.size() < 8) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreate(&e));
        ctx->ev_chunk.push_back(e);
    }
    ctx->chunks_timed = 0;
    ctx->sum_seed_ms = ctx->sum_prop_ms = ctx->sum_post_ms = 0.0;
    ctx->launches = 0;
    return wave_kernel ? run_wave_kernel(ctx, call, P) : run_group_kernel(ctx, call, P);
}

// The lane kernel (variant 0): lane-per-packet, persistent-ish grid, static round-robin packet assignment
int run_lane_kernel(TardisMcContext *ctx, const PropagateCall &call)
{
    // (the context is cached: the timing queries must not report the epochs of an earlier wave-kernel call)
    ctx->wv.wave_epoch_mode = false;
    ctx->wv.post_pending[0] = ctx->wv.post_pending[1] = false;
    ctx->wv.prop_pending = false;
    ctx->sum_seed_ms = ctx->sum_prop_ms = ctx->sum_post_ms = 0.0;
    ctx->launches = 0;
    long long want_blocks = (ctx->pk.n_packets + 255) / 256;
    int blocks = (int)std::max<long long>(1, std::min<long long>(want_blocks, (long long)call.cus * ctx->blocks_per_cu));
    HIP_TRY(ctx, ctx->rng_state.ensure((size_t)blocks * 256 * mc::MT_N * sizeof(uint32_t)));
    mc::DeviceProblem P = make_device_problem(ctx);
    const size_t lds = 2 * (size_t)ctx->n_shells * sizeof(double);
    if (lds + ((ctx->el.track_full || ctx->bf.on) ? 64 : 0) > 64 * 1024) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "n_shells too large for the LDS J/nu_bar accumulator");
    if (ctx->el.track_full) {
        int rc = setup_event_log(ctx, P, (long long)blocks * 4);
        if (rc) return rc;
    }
    if (ctx->bf.on) {
        int rc = setup_segment_log(ctx, P, (long long)blocks * 4);
        if (rc) return rc;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    ctx->chunks_timed = 0;
    return ctx->pk.n_packets > 0 ? launch_lane(ctx, P, blocks, lds) : TARDIS_MC_OK;
}

}  // namespace

extern "C" {

int tardis_mc_abi_version(void) { return TARDIS_MC_ABI_VERSION; }

int tardis_mc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int tardis_mc_create(int device_id, TardisMcContext **out_ctx)
{
    if (!out_ctx) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, TARDIS_MC_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
    if (device_id < 0 || device_id >= n)
        return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "device_id %d out of range [0,%d)", device_id, n);
    TardisMcContext *ctx = new TardisMcContext();
    ctx->device = device_id;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&ctx->prop, device_id)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&ctx->ev_start)) != hipSuccess || (e = hipEventCreate(&ctx->ev_stop)) != hipSuccess) {
        int rc = fail(nullptr, TARDIS_MC_ERR_HIP, "context creation failed: %s", hipGetErrorString(e));
        delete ctx;
        return rc;
    }
    if (const char *v = getenv("TARDIS_MC_VARIANT")) ctx->variant = atoi(v);
    if (const char *v = getenv("TARDIS_MC_BLOCKS_PER_CU")) ctx->blocks_per_cu = std::max(1, atoi(v));
    if (const char *v = getenv("TARDIS_MC_DEBUG_FLAGS")) ctx->debug_flags = atoi(v);
    if (const char *v = getenv("TARDIS_MC_EST_PIPELINE")) ctx->wv.est_pipeline = atoi(v) ? 1 : 0;
    if (const char *v = getenv("TARDIS_MC_EST_COPIES")) ctx->es.est_copies = std::max(1, std::min(8, atoi(v)));
    *out_ctx = ctx;
    return TARDIS_MC_OK;
}

void tardis_mc_destroy(TardisMcContext *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(ctx->comm);
    ctx->ot.release(); ctx->wt.release(); ctx->sc.release(); ctx->sw.release(); ctx->es.release(); ctx->pk.release(); ctx->vl.release(); ctx->el.release();
    ctx->wv.release(); ctx->lt.release(); ctx->rs.release(); ctx->sf.release(); ctx->pg.release();
    ctx->ou.release(); ctx->pl.release(); ctx->nl.release(); ctx->nc.release(); ctx->he.release(); ctx->ct.release(); ctx->ck.release(); ctx->bf.release(); ctx->mo.release();
    ctx->release();
    delete ctx;
}

const char *tardis_mc_last_error(const TardisMcContext *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int tardis_mc_set_option(TardisMcContext *ctx, const char *name, long long value)
{
    if (!ctx || !name) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    std::string n(name);
    if (n == "variant") ctx->variant = (int)value;
    else if (n == "blocks_per_cu") ctx->blocks_per_cu = std::max(1, (int)value);
    else if (n == "track_last_interaction") ctx->pk.track = value != 0;
    else if (n == "estimator_copies") { ctx->es.est_copies = std::max(1, std::min(8, (int)value)); ctx->es.est_valid = false; }
    else if (n == "vpacket_log_capacity") { ctx->vl.vlog_capacity = value; ctx->vl.vlog_capacity_user = value > 0; }
    else if (n == "track_full") ctx->el.track_full = value != 0;
    else if (n == "vpacket_last_interaction") ctx->vl.vlog_li = value != 0;
    else if (n == "event_log_capacity") ctx->el.evlog_capacity = std::max<long long>(0, value);
    else if (n == "event_log_max_bytes") ctx->el.evlog_max_bytes = std::max<long long>(1LL << 20, value);
    else if (n == "bf_estimators") ctx->bf.on = value != 0;
    else if (n == "segment_log_capacity") ctx->bf.seg_capacity = std::max<long long>(0, value);
    else if (n == "segment_log_max_bytes") ctx->bf.seg_max_bytes = std::max<long long>(1LL << 20, value);
    else if (n == "segment_log_keep") ctx->bf.seg_keep = value != 0;
    else if (n == "continuum_field") {
        if (value != 0 && value != 1) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "option continuum_field is 0 (the dilute black body) or 1 (the estimators' rates)");
        ctx->bf.continuum_field = (int)value;
    }
    else if (n == "debug_flags") ctx->debug_flags = (int)value;
    else if (n == "drain_split") ctx->wv.drain_split = value ? 1 : 0;
    else if (n == "drain_compact") ctx->wv.drain_compact = (int)std::max<long long>(0, std::min<long long>(48, value));
    else if (n == "est_one_level") ctx->wv.est_one_level = value ? 1 : 0;
    else if (n == "drain_pack_lanes") ctx->wv.drain_pack_lanes = (int)std::max<long long>(1, std::min<long long>(64, value));
    else if (n == "walk_sector_packing") ctx->wt.walk_sector_packing = value ? 1 : 0;
    else if (n == "walk_hot") ctx->wt.walk_hot = value < 0 ? -1 : (value ? 1 : 0);  // (like walk_sector_packing: before set_opacity)
    else if (n == "walk_hot_min_mass") ctx->wt.walk_hot_min_mass = (int)std::max<long long>(0, std::min<long long>(value, 1001));
    else if (n == "walk_hot_min_mass_long") ctx->wt.walk_hot_min_mass_long = (int)std::max<long long>(0, std::min<long long>(value, 1001));
    else if (n == "vpacket_screening") ctx->sc.vpacket_screening = value < 0 ? -1 : (value ? 1 : 0);
    else if (n == "waves_per_simd") ctx->waves_per_simd = (int)value;
    else if (n == "lane_sweep_min_active") {  // (< 0: the automatic choice again)
        ctx->wv.ls_min_active_user = value >= 0;
        ctx->wv.ls_min_active = value >= 0 ? (int)std::min<long long>(value, 63) : 8;
    }
    else if (n == "lane_sweep_max_steps") ctx->wv.ls_max_steps = (int)std::max<long long>(1, value);
    else if (n == "vq_oversubscribe") ctx->wv.vq_oversubscribe = (int)std::max<long long>(1, std::min<long long>(value, 64));
    else if (n == "vq_tracer_waves_per_simd") ctx->wv.vq_tracer_waves_per_simd = (int)std::max<long long>(1, std::min<long long>(value, 16));
    else if (n == "vq_min_items") ctx->wv.vq_min_items = value;
    else if (n == "vq_min_active") ctx->wv.vq_min_active = (int)std::max<long long>(0, std::min<long long>(value, 63));
    else if (n == "log_tail_split") ctx->wv.log_tail_split = value ? 1 : 0;
    else if (n == "est_pipeline") ctx->wv.est_pipeline = value ? 1 : 0;
    else if (n == "pass_cus") ctx->wv.pass_cus = (int)std::max<long long>(0, std::min<long long>(value, 16));
    else if (n == "vpk_wave_min_packets") ctx->vpk_wave_min_packets = std::max<long long>(0, value);
    else if (n == "ls_waves_per_simd") { ctx->lt.ls_waves_per_simd = (value == 3 || value == 4) ? (int)value : 0; ctx->lt.ls_tune.n = -1; }
    else if (n == "epoch_split") ctx->wv.epoch_split = value ? 1 : 0;
    else if (n == "log_by_shell") ctx->wv.log_by_shell = value < 0 ? -1 : (value ? 1 : 0);
    else if (n == "stream_min_packets") ctx->rs.min_packets = std::max<long long>(64, value);
    else if (n == "sweep_table") ctx->sw.sweep_table = (int)std::max<long long>(-1, std::min<long long>(value, 2));
    else if (n == "table_offsets") ctx->table_offsets = value < 0 ? -1 : (value ? 1 : 0);
    else if (n == "vpk_wide_registers") ctx->vpk_wide_registers = (int)std::max<long long>(0, std::min<long long>(value, 2));
    else if (n == "bucket_lines_permille") ctx->ot.bucket_lines_permille = (int)std::max<long long>(50, std::min<long long>(value, 16000));
    else if (n == "vp_carry_min_active") ctx->wv.vp_carry_min_active = (int)std::max<long long>(0, std::min<long long>(value, 63));
    else if (n == "est_accumulate") ctx->wv.est_accumulate = (int)std::max<long long>(0, std::min<long long>(value, 3));
    else if (n == "log_tail_packets") ctx->wv.log_tail_packets = (int)std::max<long long>(0, std::min<long long>(value, 1000));
    else if (n == "log_chunk_records") ctx->wv.log_chunk_records = value <= 0 ? 0 : std::max<long long>(256, std::min<long long>(value, 1 << 20));
    else if (n == "walk_min_active") {  // (-1: never carry a walk over; < -1: the automatic choice again)
        ctx->wv.walk_min_active_user = value >= -1;
        ctx->wv.walk_min_active = value >= -1 ? (int)std::min<long long>(value, 63) : 8;
    }
    else if (n == "tracker_defer") ctx->wv.tracker_defer = value ? 1 : 0;
    else if (n == "rng_complete") ctx->wv.rng_complete = value ? 1 : 0;
    else if (n == "sweep_skip") ctx->sw.sweep_skip = (int)std::max<long long>(-1, std::min<long long>(value, 1));
    else if (n == "sweep_start_held") ctx->sw.sweep_start_held = (int)std::max<long long>(-1, std::min<long long>(value, 1));
    else if (n == "tracker_pack_max_lines") ctx->wv.tracker_pack_max_lines = std::max<long long>(0, value);
    else if (n == "group_size") ctx->group_size = (value == 4 || value == 8 || value == 16) ? (int)value : 0;
    else if (n == "pipeline_chunks") {}  // (round 1: chunks on two streams; a call of the wave kernel now runs as epochs -- accepted, ignored)
    else if (n == "log_capacity") { ctx->wv.log_capacity = std::max<long long>(0, value); ctx->wv.log_capacity_user = true; }
    else if (n == "log_sets") ctx->wv.log_sets = (value == 1 || value == 2) ? (int)value : 0;  // 1: the estimator passes of an epoch run before the next epoch, not beside it; 0: automatic
    else if (n == "source_max_iterations") ctx->sf.max_iterations = std::max<long long>(1, value);
    else if (n == "chunk_packets") ctx->chunk_packets = std::max<long long>(1024, value);
    else if (n == "opacity_update_long_rows") ctx->ou.long_rows = value < 0 ? -1 : value;
    else if (n == "plasma_update_long_rows") ctx->pl.long_rows = value < 0 ? -1 : value;
    else if (n == "mean_opacity_long_bins") ctx->mo.long_bins = value < 0 ? -1 : value;
    else if (n == "plasma_max_iterations") ctx->pl.max_iterations = std::max<long long>(1, value);
    else if (n == "nlte_lds_levels") ctx->nl.lds_levels = value < 0 ? -1 : value;
    else if (n == "nlte_blocked_levels") ctx->nl.blocked_levels = value < 0 ? -1 : value;
    else return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "unknown option '%s'", name);
    return TARDIS_MC_OK;
}

int tardis_mc_set_geometry(TardisMcContext *ctx, const TardisMcGeometry *g)
{
    if (!ctx || !g || g->n_shells <= 0 || !g->r_inner || !g->r_outer)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid geometry");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drop_products(ctx, GEOMETRY_REPLACED);
    if ((int)g->n_shells != ctx->n_shells) ctx->bf.have = ctx->bf.rates_valid = false;  // (the photo-ionisation estimators' tables are [NC][S])
    int rc;
    if ((rc = upload(ctx, ctx->r_inner, g->r_inner, (size_t)g->n_shells))) return rc;
    if ((rc = upload(ctx, ctx->r_outer, g->r_outer, (size_t)g->n_shells))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->n_shells = (int)g->n_shells;
    ctx->t_exp = g->time_explosion;
    ctx->have_geometry = true;
    return TARDIS_MC_OK;
}

// Every table that depends on the resident probabilities prob_t[S][T] -- the running sums cum_t, the negative-probability flag, the choice of the hot
// sectors, rec16 / line_block_c / cum16 -- and the invalidation of what is built lazily from the opacity state (the prefix sums of tau, the interleaved
// sweep table, the source function with its exp(-tau)).  Shared by tardis_mc_set_opacity and tardis_mc_update_opacity: it reads the context's host
// copies of the index tables and of the line list, not the caller's pointers.
static int derive_opacity_tables(TardisMcContext *ctx, const size_t L, const size_t S, const size_t T, const std::function<void(const char *)> &tmark)
{
    const std::vector<int> &l2l = ctx->ot.h_idx[0], &edge = ctx->ot.h_idx[1], &ttype = ctx->ot.h_idx[2], &dest = ctx->ot.h_idx[3], &tline = ctx->ot.h_idx[4];
    const std::vector<double> &nu = ctx->ot.h_nu;
    const bool macro = ctx->ot.h_macro;
    const size_t E = macro ? edge.size() : 1;
    int rc;
    drop_products(ctx, OPACITY_VALUES_REPLACED);
    {   // running sums of the transition probabilities within their blocks (macro_cumulative_kernel)
        HIP_TRY(ctx, ctx->ot.cum_t.ensure((T * S + 8) * sizeof(double)));  // (+8: the jump search reads eight entries at a time)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->ot.cum_t.p, ctx->ot.prob_t.p, T * S * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        ctx->ot.prob_negative = false;
        if (macro && E > 1) {
            HIP_TRY(ctx, ctx->sc.pfx_flag.ensure(sizeof(int)));  // (a flag word the context keeps: no hipMalloc / hipFree per opacity state)
            int *flag = ctx->sc.pfx_flag.as<int>();
            HIP_TRY(ctx, hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
            const long long n = (long long)(E - 1) * (long long)S;
            hipLaunchKernelGGL(mc::macro_cumulative_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ot.prob_t.as<double>(),
                               ctx->ot.cum_t.as<double>(), ctx->ot.block_edge.as<int>(), (int)(E - 1), (long long)T, (int)S, flag);
            int neg = 0;
            hipError_t e1 = hipGetLastError();
            hipError_t e2 = hipMemcpyAsync(&neg, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
            hipError_t e3 = hipStreamSynchronize(ctx->stream);
            HIP_TRY(ctx, e1); HIP_TRY(ctx, e2); HIP_TRY(ctx, e3);
            ctx->ot.prob_negative = neg != 0;
        }
    }
    tmark("running sums");
    ctx->wt.n_hot_blocks = 0;
    if (macro && E > 1 && !ctx->ot.prob_negative) {
        // compact tables of the per-lane macro-atom walk (walk_tables.hpp): blocks at 16-byte aligned compact offsets.  The walk is
        // bound by the number of memory requests, and a block's window of running sums is fetched in 64-byte sectors: a block of
        // up to 32 entries (one window) that would straddle a sector boundary starts at the next boundary instead (the skipped
        // quads are padding no block owns), longer blocks start on a boundary -- one request per jump instead of 1.5.
        const size_t n_levels = E - 1;
        std::vector<long long> c0(n_levels + 1);
        long long tc = 0;
        for (size_t b = 0; b < n_levels; ++b) {
            const long long len = (edge[b + 1] - edge[b] + 7) / 8 * 8;
            if (ctx->wt.walk_sector_packing && len > 0) {
                const long long in_sector = tc & 31;  // (32 entries of 2 bytes per 64-byte sector)
                if (in_sector != 0 && (len > 32 || in_sector + len > 32)) tc += 32 - in_sector;
            }
            c0[b] = tc;
            tc += len;
        }
        c0[n_levels] = tc;
        const long long n_quads = tc / 8;
        const unsigned long long stride = ((unsigned long long)tc + 31ull) / 32ull * 32ull + mc::WALK_SLACK;  // (rows start on sector boundaries)
        if (tc > 0 && stride * S < (1ull << 32) && tc < (1LL << 30)) {
            // hot sectors (walk_tables.hpp): measured on the device (total width of a block's six widest intervals, per shell),
            // chosen here (mean over the shells), then built once more with the destinations' flags in place
            std::vector<unsigned char> hot(n_levels, 0);
            if (ctx->wt.walk_hot != 0 && n_levels < (size_t)mc::WALK_HOT) {
                const long long nb = (long long)n_levels * (long long)S;
                HIP_TRY(ctx, ctx->wt.hot_sec.ensure((size_t)nb * 64));
                HIP_TRY(ctx, ctx->wt.hot_mass.ensure((size_t)nb * sizeof(unsigned)));
                HIP_TRY(ctx, ctx->wt.hot_flag.ensure(n_levels));
                auto launch_hot = [&](const unsigned char *flags, unsigned *mass) {
                    hipLaunchKernelGGL(mc::walk_hot_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ot.cum_t.as<double>(),
                                       ctx->ot.block_edge.as<int>(), ctx->ot.ttype.as<int>(), ctx->ot.dest.as<int>(), ctx->ot.tline.as<int>(), flags,
                                       (int)n_levels, (long long)T, (int)S, ctx->wt.hot_sec.as<unsigned>(), mass);
                    return hipGetLastError();
                };
                HIP_TRY(ctx, launch_hot(nullptr, ctx->wt.hot_mass.as<unsigned>()));
                std::vector<unsigned> mass((size_t)nb);
                HIP_TRY(ctx, hipMemcpyAsync(mass.data(), ctx->wt.hot_mass.p, (size_t)nb * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                for (size_t b = 0; b < n_levels; ++b) {
                    const long long rows = edge[b + 1] - edge[b];
                    if (rows <= 0) continue;
                    double m = 0.0;
                    for (size_t sh = 0; sh < S; ++sh) m += (double)mass[sh * n_levels + b];
                    m /= 65536.0 * (double)S;
                    const double need = 1e-3 * (double)(rows > 8 * mc::WALK_WINDOW_QUADS ? ctx->wt.walk_hot_min_mass_long : ctx->wt.walk_hot_min_mass);
                    if (ctx->wt.walk_hot == 1 || m >= need) { hot[b] = 1; ctx->wt.n_hot_blocks += 1; }
                }
                if (ctx->wt.n_hot_blocks > 0) {
                    HIP_TRY(ctx, hipMemcpyAsync(ctx->wt.hot_flag.p, hot.data(), n_levels, hipMemcpyHostToDevice, ctx->stream));
                    hipLaunchKernelGGL(mc::walk_hot_flag_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, ctx->stream, ctx->wt.hot_flag.as<unsigned char>(), nb,
                                       ctx->wt.hot_sec.as<unsigned>());  // (the destinations of the first pass's records, marked; no second walk over the blocks)
                    HIP_TRY(ctx, hipGetLastError());
                    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                    ctx->wt.have_hot = true;
                } else {  // no block qualifies (uniform short blocks): S x levels x 64 B -- 0.5 GB at the configs[4] shape -- are not kept for nothing
                    ctx->wt.hot_sec.release();
                    ctx->wt.hot_flag.release();
                }
                ctx->wt.hot_mass.release();  // (only the choice above read it)
            }
            {
                std::vector<int> bt(2 * n_levels);
                for (size_t b = 0; b < n_levels; ++b) {
                    bt[2 * b] = (int)c0[b];
                    bt[2 * b + 1] = (int)(edge[b + 1] - edge[b]);
                }
                if ((rc = upload(ctx, ctx->wt.blk_tab, bt.data(), bt.size()))) return rc;
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            }
            std::vector<int> qi(2 * (size_t)n_quads, 0), lbc(2 * L, 0);  // (quads of the sector padding: {0, 0} -> eight 0xffff entries)
            std::vector<mc::WalkRec> r16((size_t)tc + 1, mc::WalkRec{0u, 0u, 0.0});
            for (size_t b = 0; b < n_levels; ++b) {
                const long long b0 = edge[b], b1 = edge[b + 1];
                for (long long q = c0[b] / 8, k = b0; k < b1; ++q, k += 8) { qi[2 * q] = (int)k; qi[2 * q + 1] = (int)(b1 - k); }
                for (long long k = b0; k < b1; ++k) {
                    const long long c = c0[b] + (k - b0);
                    const int64_t tt = ttype[k];
                    if (tt >= 0) {
                        const int64_t lvl = dest[k];
                        if (hot[lvl]) { r16[c].a = (unsigned)lvl; r16[c].b = mc::WALK_HOT; }
                        else {
                            r16[c].a = (unsigned)c0[lvl];
                            r16[c].b = (unsigned)(edge[lvl + 1] - edge[lvl]);
                        }
                    } else if (tt == -1) {
                        r16[c].a = (unsigned)tline[k];
                        r16[c].b = mc::WALK_EMIT;
                        r16[c].nu = nu[tline[k]];
                    } else
                        r16[c].b = mc::WALK_EMIT | mc::WALK_UNSUPPORTED;
                }
            }
            for (size_t i = 0; i < L; ++i) {
                const int64_t lvl = l2l[i];
                if (hot[lvl]) { lbc[2 * i] = (int)lvl; lbc[2 * i + 1] = -1; }
                else {
                    lbc[2 * i] = (int)c0[lvl];
                    lbc[2 * i + 1] = (int)(edge[lvl + 1] - edge[lvl]);
                }
            }
            if ((rc = upload(ctx, ctx->wt.quad_info, qi.data(), qi.size()))) return rc;
            if ((rc = upload(ctx, ctx->wt.rec16, r16.data(), r16.size()))) return rc;
            if ((rc = upload(ctx, ctx->wt.line_block_c, lbc.data(), lbc.size()))) return rc;
            HIP_TRY(ctx, ctx->wt.cum16.ensure((size_t)stride * S * sizeof(unsigned short)));
            HIP_TRY(ctx, hipMemsetAsync(ctx->wt.cum16.p, 0xff, (size_t)stride * S * sizeof(unsigned short), ctx->stream));
            const long long n = n_quads * (long long)S;
            hipLaunchKernelGGL(mc::walk_cum16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ot.cum_t.as<double>(),
                               ctx->wt.quad_info.as<int2>(), n_quads, (long long)T, (int)S, (unsigned)stride, ctx->wt.cum16.as<unsigned short>());
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the host vectors above are the sources of asynchronous copies)
            ctx->wt.cum16_stride = (unsigned)stride;
            ctx->wt.have_walk_tables = true;
        }
    }
    return TARDIS_MC_OK;
}

int tardis_mc_set_opacity(TardisMcContext *ctx, const TardisMcOpacity *o)
{
    if (!ctx || !o || o->n_lines <= 0 || o->n_shells <= 0 || o->n_transitions <= 0 || !o->electron_density ||
        !o->line_list_nu || !o->tau_sobolev || !o->transition_probabilities)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid opacity state");
    if (o->n_lines > 0x7ffffff0LL || o->n_transitions > 0x7ffffff0LL)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "line / transition count exceeds 32-bit device indices");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drop_products(ctx, OPACITY_TOPOLOGY_REPLACED);
    const bool tmark_on = getenv("TARDIS_MC_TIME_OPACITY") != nullptr;  // (diagnostic: wall time of the stages of this call on stderr)
    auto tmark_t0 = std::chrono::steady_clock::now();
    const std::function<void(const char *)> tmark = [&](const char *what) {
        if (!tmark_on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "set_opacity: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tmark_t0).count());
        tmark_t0 = now;
    };
    const size_t L = (size_t)o->n_lines, S = (size_t)o->n_shells, T = (size_t)o->n_transitions;
    const size_t E = (size_t)o->n_macro_block_edges;
    // validate the macro-atom index tables on the host: the device walks them without bounds checks
    const bool macro = T > 1 || E > 1;
    if (macro) {
        if (!o->line2macro_level_upper || !o->macro_block_edge_index || !o->transition_type || !o->destination_level_id ||
            !o->transition_line_id || E < 2)
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "macro-atom tables missing");
        const long long n_levels = (long long)E - 1;
        for (size_t i = 0; i + 1 < E; ++i)
            if (o->macro_block_edge_index[i] < 0 || o->macro_block_edge_index[i] > o->macro_block_edge_index[i + 1] ||
                o->macro_block_edge_index[i + 1] > (long long)T)
                return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "macro_block_edge_index not monotone within [0,T]");
        for (size_t i = 0; i < L; ++i)
            if (o->line2macro_level_upper[i] < 0 || o->line2macro_level_upper[i] >= n_levels)
                return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "line2macro_level_upper[%zu] out of range", i);
        for (size_t i = 0; i < T; ++i) {
            if (o->transition_type[i] >= 0 && (o->destination_level_id[i] < 0 || o->destination_level_id[i] >= n_levels))
                return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "destination_level_id[%zu] out of range", i);
            if (o->transition_type[i] == -1 && (o->transition_line_id[i] < 0 || o->transition_line_id[i] >= (long long)L))
                return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "transition_line_id[%zu] out of range", i);
        }
    }
    tmark("validate");
    int rc;
    // (slack at the end of the line list and of the tau table: the lane sweep loads whole chunks, propagate_wave.hpp)
    HIP_TRY(ctx, ctx->ot.nu_line.ensure((L + 2 * mc::LS_CHUNK) * sizeof(double)));
    if ((rc = upload(ctx, ctx->ot.nu_line, o->line_list_nu, L))) return rc;
    if ((rc = upload(ctx, ctx->ot.n_e, o->electron_density, S))) return rc;
    // tau [L,S] -> [S][L]
    HIP_TRY(ctx, ctx->staging.ensure(std::max(L, T) * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ot.tau_t.ensure((L * S + 2 * mc::LS_CHUNK) * sizeof(double)));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, host_copy(ctx, {{(void *)o->tau_sobolev, ctx->staging.p, L * S * sizeof(double)}}, true));
    HIP_TRY(ctx, launch_transpose(ctx->stream, ctx->staging.as<double>(), ctx->ot.tau_t.as<double>(), (long long)L, (long long)S));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    tmark("nu, n_e, tau up + transpose");
    // probabilities [T,S] -> [S][T]
    HIP_TRY(ctx, ctx->ot.prob_t.ensure(T * S * sizeof(double)));
    HIP_TRY(ctx, host_copy(ctx, {{(void *)o->transition_probabilities, ctx->staging.p, T * S * sizeof(double)}}, true));
    HIP_TRY(ctx, launch_transpose(ctx->stream, ctx->staging.as<double>(), ctx->ot.prob_t.as<double>(), (long long)T, (long long)S));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    tmark("probabilities up + transpose");
    static const int64_t zero64 = 0;
    std::vector<int> (&idx32)[5] = ctx->ot.h_idx;  // (one staging vector per table: the copies are asynchronous, ONE synchronisation below covers them all; kept for derive_opacity_tables)
    auto up32 = [&](int k, DevBuf &buf, const int64_t *host, size_t n) -> int {
        idx32[k].resize(n);
        for (size_t i = 0; i < n; ++i) idx32[k][i] = (int)host[i];
        return upload(ctx, buf, idx32[k].data(), n);
    };
    if ((rc = up32(0, ctx->ot.line2level, macro ? o->line2macro_level_upper : &zero64, macro ? L : 1))) return rc;
    if ((rc = up32(1, ctx->ot.block_edge, macro ? o->macro_block_edge_index : &zero64, macro ? E : 1))) return rc;
    if ((rc = up32(2, ctx->ot.ttype, macro ? o->transition_type : &zero64, macro ? T : 1))) return rc;
    if ((rc = up32(3, ctx->ot.dest, macro ? o->destination_level_id : &zero64, macro ? T : 1))) return rc;
    if ((rc = up32(4, ctx->ot.tline, macro ? o->transition_line_id : &zero64, macro ? T : 1))) return rc;
    ctx->ot.h_nu.assign(o->line_list_nu, o->line_list_nu + L);
    ctx->ot.h_macro = macro;
    drop_from(ctx, RUNG_LINE_DATA);  // (the line data belong to one topology: tardis_mc_set_line_data again)
    tmark("index tables int32 up");
    {   // packed macro-atom tables of the cooperative kernel
        std::vector<int> lb(2 * (macro ? L : 1), 0), rec(4 * (macro ? T : 1), 0);
        if (macro) {
            for (size_t i = 0; i < L; ++i) {
                const int64_t lvl = o->line2macro_level_upper[i];
                lb[2 * i] = (int)o->macro_block_edge_index[lvl];
                lb[2 * i + 1] = (int)o->macro_block_edge_index[lvl + 1];
            }
            for (size_t t = 0; t < T; ++t) {
                rec[4 * t] = (int)o->transition_line_id[t];
                rec[4 * t + 1] = (int)o->transition_type[t];
                if (o->transition_type[t] >= 0) {
                    const int64_t lvl = o->destination_level_id[t];
                    rec[4 * t + 2] = (int)o->macro_block_edge_index[lvl];
                    rec[4 * t + 3] = (int)o->macro_block_edge_index[lvl + 1];
                }
            }
        }
        if ((rc = upload(ctx, ctx->ot.line_block, lb.data(), lb.size()))) return rc;
        if ((rc = upload(ctx, ctx->ot.trans_rec, rec.data(), rec.size()))) return rc;
        // frequency of the line every emission transition ends in, next to its record (one round trip instead of two)
        std::vector<double> tnu(macro ? T : 1, 0.0);
        if (macro)
            for (size_t t = 0; t < T; ++t)
                if (o->transition_type[t] == -1) tnu[t] = o->line_list_nu[o->transition_line_id[t]];
        if ((rc = upload(ctx, ctx->ot.trans_nu, tnu.data(), tnu.size()))) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    tmark("packed tables lb / rec / tnu");
    if ((rc = derive_opacity_tables(ctx, L, S, T, tmark))) return rc;
    tmark("compact walk tables + hot sectors");
    ctx->ot.lines_sorted = true;
    for (size_t i = 0; i < L; ++i)
        if (!(o->line_list_nu[i] > 0.0) || (i > 0 && !(o->line_list_nu[i] <= o->line_list_nu[i - 1]))) { ctx->ot.lines_sorted = false; break; }
    if (ctx->ot.lines_sorted)
    {   // frequency-bucket index over the (descending) line list.  Resolution: bucket_lines_permille / 1000 lines per bucket on average
        // (default 0.75; rounds 1-4: 3).  A v-packet's shell crossing pins its stopping line with a window of four lines from the
        // bucket's first line: with three lines per bucket 22 % of the crossings missed the window and walked on line by line -- in a wave
        // of ~36 tracing lanes every step of the volley worker loop then waited for such a walk (profiles/r05_bucket_index.txt); at 0.75
        // lines per bucket 1.2 % miss, and the walk takes four lines per round trip (vp_walk_to_stop).  The table is 4 bytes per bucket.
        auto bits = [](double x) { uint64_t u; memcpy(&u, &x, 8); return u; };
        const double nu_hi = o->line_list_nu[0], nu_lo = o->line_list_nu[L - 1];
        int mbits = 4;
        if (nu_lo > 0 && nu_hi >= nu_lo) {
            const double binades = std::max(1.0, std::log2(nu_hi / nu_lo));
            const double per_binade = (double)L / binades;
            while (mbits < 22 && per_binade / (double)(1 << mbits) > 1e-3 * (double)ctx->ot.bucket_lines_permille) ++mbits;
        }
        const int shift = 52 - mbits;
        const long long kmin = (long long)(bits(nu_lo > 0 ? nu_lo : 1.0) >> shift), kmax = (long long)(bits(nu_hi > 0 ? nu_hi : 1.0) >> shift);
        const long long K = std::max<long long>(1, kmax - kmin + 1);
        if (K > (1LL << 26)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "line list frequency range too wide for the bucket index");
        std::vector<int> first((size_t)K, 0);
        // first[k] = smallest i with key(nu_line[i]) <= kmin + k; keys are non-increasing along the list
        size_t i = 0;
        for (long long k = K - 1; k >= 0; --k) {
            while (i < L && (long long)(bits(o->line_list_nu[i]) >> shift) - kmin > k) ++i;
            first[(size_t)k] = (int)i;
        }
        if ((rc = upload(ctx, ctx->ot.bucket_first, first.data(), first.size()))) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->ot.bucket_shift = shift; ctx->ot.bucket_n = (int)K; ctx->ot.bucket_kmin = kmin;
    }
    tmark("sorted check + bucket index");
    if (ctx->have_geometry && (int)S != ctx->n_shells)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "opacity has %zu shells, geometry has %d", S, ctx->n_shells);
    ctx->n_lines = (int)L; ctx->n_trans = (int)T; ctx->n_levels = macro ? (int)E - 1 : 0;
    if (!ctx->have_geometry) ctx->n_shells = (int)S;
    ctx->have_opacity = true;
    return ensure_estimators(ctx);
}

int tardis_mc_set_config(TardisMcContext *ctx, const TardisMcConfig *c)
{
    if (!ctx || !c) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid config");
    if (c->n_spectrum_grid < 0 || (c->n_spectrum_grid > 0 && !c->spectrum_frequency_grid))
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "spectrum_frequency_grid missing");
    if (c->number_of_vpackets > 0 && c->n_spectrum_grid < 2)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "v-packets need a spectrum grid with >= 2 edges");
    if (c->line_interaction_type < 0 || c->line_interaction_type > 2)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "line_interaction_type must be 0, 1 or 2");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drop_products(ctx, CONFIG_REPLACED);
    ctx->cfg = *c;
    ctx->grid_host.assign(c->spectrum_frequency_grid, c->spectrum_frequency_grid + c->n_spectrum_grid);
    ctx->cfg.spectrum_frequency_grid = ctx->grid_host.data();
    int rc;
    if ((rc = upload(ctx, ctx->grid, ctx->grid_host.data(), ctx->grid_host.size()))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->have_config = true;
    return ensure_estimators(ctx);
}

int tardis_mc_set_packets(TardisMcContext *ctx, const TardisMcPackets *p)
{
    if (!ctx || !p || p->n_packets < 0 ||
        (p->n_packets > 0 && (!p->initial_radii || !p->initial_nus || !p->initial_mus || !p->initial_energies || !p->packet_seeds)))
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid packets");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drop_products(ctx, PACKETS_REPLACED);
    const size_t P = (size_t)p->n_packets;
    int rc;
    HIP_TRY(ctx, ctx->pk.r0.ensure(P * 8)); HIP_TRY(ctx, ctx->pk.mu0.ensure(P * 8)); HIP_TRY(ctx, ctx->pk.nu0.ensure(P * 8)); HIP_TRY(ctx, ctx->pk.e0.ensure(P * 8));
    HIP_TRY(ctx, ctx->pk.seeds.ensure(P * 4));
    // The seeds arrive as int64 and the kernels read uint32 (np.random.seed(int) -> init_genrand(uint32)): sent as they are and narrowed on the device.  (A host
    // vector of P words -- zero-filled, then filled -- cost 100 ms of the 200 ms this call took at 1e8 packets; the extra 4 bytes per packet over the link cost 8.)
    HIP_TRY(ctx, ctx->staging.ensure(P * 8));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (nothing of an earlier call still reads the packet buffers)
    HIP_TRY(ctx, host_copy(ctx, {{(void *)p->initial_radii, ctx->pk.r0.p, P * 8}, {(void *)p->initial_mus, ctx->pk.mu0.p, P * 8},
                                      {(void *)p->initial_nus, ctx->pk.nu0.p, P * 8}, {(void *)p->initial_energies, ctx->pk.e0.p, P * 8},
                                      {(void *)p->packet_seeds, ctx->staging.p, P * 8}}, true));
    if (P > 0) {
        hipLaunchKernelGGL(narrow_seeds_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, ctx->stream, ctx->staging.as<long long>(), (long long)P, ctx->pk.seeds.as<uint32_t>());
        HIP_TRY(ctx, hipGetLastError());
    }
    (void)rc;
    HIP_TRY(ctx, ctx->pk.out_nu.ensure(P * sizeof(double)));
    HIP_TRY(ctx, ctx->pk.out_e.ensure(P * sizeof(double)));
    if (ctx->pk.track) {
        for (auto &b : ctx->pk.li_f64) HIP_TRY(ctx, b.ensure(P * sizeof(double)));
        for (auto &b : ctx->pk.li_i64) HIP_TRY(ctx, b.ensure(P * sizeof(long long)));
        HIP_TRY(ctx, ctx->pk.li_rec.ensure(P * 64));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pk.n_packets = (long long)P;
    ctx->have_packets = true;
    return TARDIS_MC_OK;
}

/* ---- black-body packet source on the device ------------------------------------------------------- */
namespace {
typedef unsigned __int128 hu128;
inline hu128 h128(uint64_t hi, uint64_t lo) { return ((hu128)hi << 64) | lo; }
const hu128 PCG_MULT = h128(2549297995355413924ULL, 4865540595714422341ULL);  // PCG_DEFAULT_MULTIPLIER_128

mc::PcgAffine affine(hu128 mult, hu128 plus)
{
    return mc::PcgAffine{(uint64_t)mult, (uint64_t)(mult >> 64), (uint64_t)plus, (uint64_t)(plus >> 64)};
}
}  // namespace

int tardis_mc_pcg64_seed(uint64_t seed, uint64_t out_state[4])
{
    if (!out_state) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    // numpy.random.SeedSequence(seed) with an empty spawn key, pool of 4 words (numpy/random/bit_generator.pyx)
    const uint32_t INIT_A = 0x43b0d7e5u, MULT_A = 0x931e8875u, INIT_B = 0x8b51f9ddu, MULT_B = 0x58f38dedu,
                   MIX_L = 0xca01f9ddu, MIX_R = 0x4973f715u;
    uint32_t entropy[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    const int n_entropy = entropy[1] ? 2 : 1;
    uint32_t hash_const = INIT_A;
    auto hashmix = [&](uint32_t v) {
        v ^= hash_const; hash_const *= MULT_A; v *= hash_const; v ^= v >> 16; return v;
    };
    auto mix = [&](uint32_t x, uint32_t y) { uint32_t r = MIX_L * x - MIX_R * y; r ^= r >> 16; return r; };
    uint32_t pool[4];
    for (int i = 0; i < 4; ++i) pool[i] = hashmix(i < n_entropy ? entropy[i] : 0u);
    for (int i_src = 0; i_src < 4; ++i_src)
        for (int i_dst = 0; i_dst < 4; ++i_dst)
            if (i_src != i_dst) pool[i_dst] = mix(pool[i_dst], hashmix(pool[i_src]));
    // generate_state(4, uint64): 8 words, little-endian pairs
    uint32_t words[8];
    uint32_t hc = INIT_B;
    for (int i = 0; i < 8; ++i) {
        uint32_t v = pool[i & 3];
        v ^= hc; hc *= MULT_B; v *= hc; v ^= v >> 16;
        words[i] = v;
    }
    uint64_t st[4];
    for (int i = 0; i < 4; ++i) st[i] = (uint64_t)words[2 * i] | ((uint64_t)words[2 * i + 1] << 32);
    // pcg64_set_seed: initstate = (st[0] high, st[1] low), initseq = (st[2] high, st[3] low); pcg_setseq_128_srandom_r
    const hu128 initstate = h128(st[0], st[1]), initseq = h128(st[2], st[3]);
    const hu128 inc = (initseq << 1) | 1;
    hu128 state = 0;
    state = state * PCG_MULT + inc;
    state += initstate;
    state = state * PCG_MULT + inc;
    out_state[0] = (uint64_t)(state >> 64); out_state[1] = (uint64_t)state;
    out_state[2] = (uint64_t)(inc >> 64); out_state[3] = (uint64_t)inc;
    return TARDIS_MC_OK;
}

static int ensure_packet_buffers(TardisMcContext *ctx, size_t P)
{
    HIP_TRY(ctx, ctx->pk.r0.ensure(P * sizeof(double)));
    HIP_TRY(ctx, ctx->pk.mu0.ensure(P * sizeof(double)));
    HIP_TRY(ctx, ctx->pk.nu0.ensure(P * sizeof(double)));
    HIP_TRY(ctx, ctx->pk.e0.ensure(P * sizeof(double)));
    HIP_TRY(ctx, ctx->pk.seeds.ensure(P * sizeof(uint32_t)));
    HIP_TRY(ctx, ctx->pk.out_nu.ensure(P * sizeof(double)));
    HIP_TRY(ctx, ctx->pk.out_e.ensure(P * sizeof(double)));
    if (ctx->pk.track) {
        for (auto &b : ctx->pk.li_f64) HIP_TRY(ctx, b.ensure(P * sizeof(double)));
        for (auto &b : ctx->pk.li_i64) HIP_TRY(ctx, b.ensure(P * sizeof(long long)));
        HIP_TRY(ctx, ctx->pk.li_rec.ensure(P * 64));
    }
    return TARDIS_MC_OK;
}

// beta and the per-packet energy of BlackBodySimpleSourceRelativistic, in the reference's operation order (the build has
// -ffp-contract=off: 1 - beta*beta stays a product and a difference).  An empty string, or what is wrong with the arguments.
static std::string relativistic_source_factors(double radius, double time_explosion, int64_t n_total, double *out_beta, double *out_energy)
{
    char buf[160];
    if (!std::isfinite(radius) || radius < 0.0) {
        snprintf(buf, sizeof buf, "relativistic packet source: radius %g is not finite and non-negative", radius);
        return buf;
    }
    if (!std::isfinite(time_explosion) || !(time_explosion > 0.0)) {
        snprintf(buf, sizeof buf, "relativistic packet source: time_explosion %g is not finite and positive", time_explosion);
        return buf;
    }
    if (n_total < 1) {
        snprintf(buf, sizeof buf, "relativistic packet source: n_total %lld is less than 1", (long long)n_total);
        return buf;
    }
    const double beta = (radius / time_explosion) / mc::C_LIGHT;
    if (!(beta >= 0.0 && beta < 1.0)) {
        snprintf(buf, sizeof buf, "relativistic packet source: beta = radius / time_explosion / c = %g is not in [0, 1)", beta);
        return buf;
    }
    const double gamma = 1.0 / std::sqrt(1.0 - beta * beta);
    const double factor = (2.0 * beta + 1.0) / (1.0 - beta * beta);
    *out_beta = beta;
    *out_energy = ((1.0 / (double)n_total) * factor) / gamma;
    return std::string();
}

int tardis_mc_relativistic_source_factors(double radius, double time_explosion, int64_t n_total, double *out_beta, double *out_energy)
{
    if (!out_beta || !out_energy) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "relativistic packet source: an output pointer is missing");
    const std::string err = relativistic_source_factors(radius, time_explosion, n_total, out_beta, out_energy);
    if (!err.empty()) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    return TARDIS_MC_OK;
}

// both forms of the source: `time_explosion` is read only by the relativistic one
static int create_blackbody_packets(TardisMcContext *ctx, const bool relativistic, int64_t n_total, int64_t first, int64_t count, double radius,
                                    double temperature, double time_explosion, const uint64_t pcg_state[4], uint32_t max_seed_val,
                                    const double *l_array, int64_t n_l)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (n_total < 0 || first < 0 || count < 0 || first + count > n_total || !pcg_state || !l_array || n_l < 1 || n_l > (1 << 24) ||
        max_seed_val < 2 || (uint64_t)n_total >= (1ULL << 44))
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid packet source arguments");
    double beta = 0.0, energy = n_total > 0 ? 1.0 / (double)n_total : 0.0;
    if (relativistic) {
        const std::string err = relativistic_source_factors(radius, time_explosion, n_total, &beta, &energy);
        if (!err.empty()) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drop_products(ctx, PACKETS_REPLACED);
    const size_t P = (size_t)count;
    int rc = ensure_packet_buffers(ctx, P);
    if (rc) return rc;
    // jump tables of the LCG  s -> M s + inc
    const hu128 inc = h128(pcg_state[2], pcg_state[3]);
    std::vector<mc::PcgAffine> jump(mc::PCG_JUMP_BITS);
    hu128 jm[mc::PCG_JUMP_BITS], jp[mc::PCG_JUMP_BITS];
    jm[0] = PCG_MULT; jp[0] = inc;
    for (int j = 1; j < mc::PCG_JUMP_BITS; ++j) { jm[j] = jm[j - 1] * jm[j - 1]; jp[j] = (jm[j - 1] + 1) * jp[j - 1]; }
    for (int j = 0; j < mc::PCG_JUMP_BITS; ++j) jump[j] = affine(jm[j], jp[j]);
    hu128 nm = 1, np_ = 0;  // n_total-step map, composed from the set bits
    for (int j = 0; j < mc::PCG_JUMP_BITS; ++j)
        if (((uint64_t)n_total >> j) & 1) { nm = jm[j] * nm; np_ = jm[j] * np_ + jp[j]; }
    ScopedDevBuf d_jump, d_l, d_rej, d_cnt;
    HIP_TRY(ctx, d_jump.ensure(jump.size() * sizeof(mc::PcgAffine)));
    HIP_TRY(ctx, hipMemcpyAsync(d_jump.p, jump.data(), jump.size() * sizeof(mc::PcgAffine), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, d_l.ensure((size_t)n_l * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(d_l.p, l_array, (size_t)n_l * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const int capacity = 1 << 16;
    HIP_TRY(ctx, d_rej.ensure((size_t)capacity * sizeof(long long)));
    HIP_TRY(ctx, d_cnt.ensure(sizeof(unsigned int)));
    HIP_TRY(ctx, hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned int), ctx->stream));

    mc::PacketSourceArgs a{};
    a.n_total = n_total; a.first = first; a.count = count;
    a.state_hi = pcg_state[0]; a.state_lo = pcg_state[1];
    a.jump = d_jump.as<mc::PcgAffine>();
    a.step_n = affine(nm, np_);
    a.seed_range_excl = max_seed_val;
    a.seed_threshold = (uint32_t)((0x100000000ULL - max_seed_val) % max_seed_val);  // (UINT32_MAX - rng) % rng_excl
    a.l_array = d_l.as<double>(); a.n_l = (int)n_l;
    a.l_coef = 1.082323233711138;  // np.pi**4 / 90.0 (black_body.py:175)
    a.radius = radius;
    a.kT = 1.3806488e-16 * temperature;   // tardis/constants.py:1 (CODATA 2010, cgs)
    a.h = 6.62606957e-27;
    a.energy = energy;
    a.beta = beta;
    a.r0 = ctx->pk.r0.as<double>(); a.mu0 = ctx->pk.mu0.as<double>(); a.nu0 = ctx->pk.nu0.as<double>(); a.e0 = ctx->pk.e0.as<double>();
    a.seeds = ctx->pk.seeds.as<uint32_t>();

    // pass 1: rejected u32 positions of the bounded-integer draw (threshold / 2^32 of all draws; none for almost every
    // run with the reference's MAX_SEED_VAL = 2^32 - 1)
    std::vector<long long> rejected;
    long long consumed_u32 = 0;
    if (n_total > 0) {
        unsigned int n_rej = 0;
        if (a.seed_threshold > 0) {
            const long long n_positions = n_total + capacity;
            const int blocks = (int)std::min<long long>((n_positions / 2 + 255) / 256 + 1, 8192);
            hipLaunchKernelGGL(mc::packet_source_scan_kernel, dim3(blocks), dim3(256), 0, ctx->stream, a, n_positions,
                               d_rej.as<long long>(), capacity, d_cnt.as<unsigned int>());
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(&n_rej, d_cnt.p, sizeof(n_rej), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if ((long long)n_rej >= capacity)
                return fail(ctx, TARDIS_MC_ERR_UNSUPPORTED, "packet source: too many rejected seed draws for this seed range");
            rejected.resize(n_rej);
            if (n_rej) {
                HIP_TRY(ctx, hipMemcpy(rejected.data(), d_rej.p, n_rej * sizeof(long long), hipMemcpyDeviceToHost));
                std::sort(rejected.begin(), rejected.end());
                HIP_TRY(ctx, hipMemcpy(d_rej.p, rejected.data(), n_rej * sizeof(long long), hipMemcpyHostToDevice));
            }
        }
        long long pos = n_total - 1;
        for (size_t k = 0; k < rejected.size() && rejected[k] <= pos; ++k) ++pos;
        consumed_u32 = pos + 1;
    }
    a.rejected = d_rej.as<long long>();
    a.n_rejected = (int)rejected.size();
    a.xi_first_u64 = (consumed_u32 + 1) / 2;
    if (count > 0) {
        const int blocks = (int)std::min<long long>((count + 255) / 256, 16384);
        if (relativistic)
            hipLaunchKernelGGL(mc::packet_source_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL(mc::packet_source_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pk.n_packets = count;
    ctx->have_packets = true;
    return TARDIS_MC_OK;
}

int tardis_mc_create_blackbody_packets(TardisMcContext *ctx, int64_t n_total, int64_t first, int64_t count, double radius,
                                       double temperature, const uint64_t pcg_state[4], uint32_t max_seed_val,
                                       const double *l_array, int64_t n_l)
{
    return create_blackbody_packets(ctx, false, n_total, first, count, radius, temperature, 0.0, pcg_state, max_seed_val, l_array, n_l);
}

int tardis_mc_create_blackbody_packets_relativistic(TardisMcContext *ctx, int64_t n_total, int64_t first, int64_t count, double radius,
                                                    double temperature, double time_explosion, const uint64_t pcg_state[4],
                                                    uint32_t max_seed_val, const double *l_array, int64_t n_l)
{
    return create_blackbody_packets(ctx, true, n_total, first, count, radius, temperature, time_explosion, pcg_state, max_seed_val, l_array, n_l);
}

int tardis_mc_get_packets(TardisMcContext *ctx, double *initial_radii, double *initial_nus, double *initial_mus,
                          double *initial_energies, int64_t *packet_seeds)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->have_packets) return fail(ctx, TARDIS_MC_ERR_STATE, "no packets resident");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->pk.n_packets;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (initial_radii && P) HIP_TRY(ctx, hipMemcpy(initial_radii, ctx->pk.r0.p, P * 8, hipMemcpyDeviceToHost));
    if (initial_nus && P) HIP_TRY(ctx, hipMemcpy(initial_nus, ctx->pk.nu0.p, P * 8, hipMemcpyDeviceToHost));
    if (initial_mus && P) HIP_TRY(ctx, hipMemcpy(initial_mus, ctx->pk.mu0.p, P * 8, hipMemcpyDeviceToHost));
    if (initial_energies && P) HIP_TRY(ctx, hipMemcpy(initial_energies, ctx->pk.e0.p, P * 8, hipMemcpyDeviceToHost));
    if (packet_seeds && P) {
        std::vector<uint32_t> tmp(P);
        HIP_TRY(ctx, hipMemcpy(tmp.data(), ctx->pk.seeds.p, P * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < P; ++i) packet_seeds[i] = (int64_t)tmp[i];
    }
    return TARDIS_MC_OK;
}

int tardis_mc_reset_estimators(TardisMcContext *ctx)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drop_products(ctx, ESTIMATORS_CHANGED);
    int rc = ensure_estimators(ctx);
    if (rc) return rc;
    if (!ctx->es.est_valid) return fail(ctx, TARDIS_MC_ERR_STATE, "set_opacity and set_config must precede reset_estimators");
    EstLayout e = est_layout(ctx->es.est_S, ctx->es.est_L, ctx->es.est_G, ctx->es.est_copies);
    HIP_TRY(ctx, hipMemsetAsync(ctx->es.est.p, 0, e.total * sizeof(double), ctx->stream));
    if (ctx->bf.have && ctx->ct.have) {  // (the rates of tardis_mc_bf_estimator_rates stay)
        HIP_TRY(ctx, hipMemsetAsync(ctx->bf.tables.p, 0, (size_t)mc::BF_TABLES * (size_t)ctx->ct.continua * (size_t)ctx->n_shells * sizeof(double), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->bf.totals.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
    }
    ctx->es.est_propagated = false;
    HIP_TRY(ctx, ctx->counters.ensure(TARDIS_MC_N_COUNTERS * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->counters.p, 0, TARDIS_MC_N_COUNTERS * sizeof(unsigned long long), ctx->stream));
    return TARDIS_MC_OK;
}

int tardis_mc_propagate(TardisMcContext *ctx)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->have_geometry || !ctx->have_opacity || !ctx->have_config || !ctx->have_packets)
        return fail(ctx, TARDIS_MC_ERR_STATE, "set_geometry/set_opacity/set_config/set_packets must precede propagate");
    if (ctx->bf.on && !(ctx->bf.have && ctx->ct.have))
        return fail(ctx, TARDIS_MC_ERR_STATE, "the option bf_estimators needs tardis_mc_set_bf_estimators (after set_continuum_data) before propagate");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->wv.compactions = 0;
    drop_products(ctx, PROPAGATE_BEGINS);
    const TardisMcConfig &c = ctx->cfg;
    if (ctx->vl.vlog_li && c.enable_vpacket_tracking && c.number_of_vpackets > 0 && !ctx->pk.track && !ctx->el.track_full)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "the option vpacket_last_interaction needs a tracker: track_last_interaction 1 or track_full 1");
    PropagateCall call{};
    call.vpk = c.number_of_vpackets > 0;
    call.full = c.enable_full_relativity != 0;
    call.cus = ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256;
    call.rs_armed = ctx->rs.armed;
    ctx->rs.armed = false; ctx->rs.upto = 0; ctx->rs.n_late = 0;
    call.tune_pending = ctx->lt.ls_tune.pending;
    ctx->lt.ls_tune.pending = -1;
    call.tune_slot = -1;
    int rc = ensure_estimators(ctx);
    if (rc) return rc;
    if (!ctx->counters.p) {
        HIP_TRY(ctx, ctx->counters.ensure(TARDIS_MC_N_COUNTERS * sizeof(unsigned long long)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->counters.p, 0, TARDIS_MC_N_COUNTERS * sizeof(unsigned long long), ctx->stream));
    }
    if (ctx->pk.track) {  // (tracking may have been switched on after the packets were set)
        const size_t P = (size_t)std::max<long long>(ctx->pk.n_packets, 1);
        for (auto &b : ctx->pk.li_f64) HIP_TRY(ctx, b.ensure(P * sizeof(double)));
        for (auto &b : ctx->pk.li_i64) HIP_TRY(ctx, b.ensure(P * sizeof(long long)));
        HIP_TRY(ctx, ctx->pk.li_rec.ensure(P * 64));
    }
    if (ctx->el.track_full || ctx->bf.on) HIP_TRY(ctx, ctx->pk.li_rec.ensure((size_t)std::max<long long>(ctx->pk.n_packets, 1) * 64));
    // v-packet log buffers
    if (c.enable_vpacket_tracking && call.vpk) {
        // (sized for the current call: the engine is cached per process, a later, larger run must not inherit a smaller log)
        if (!ctx->vl.vlog_capacity_user) ctx->vl.vlog_capacity = std::max<long long>(1024, ctx->pk.n_packets * c.number_of_vpackets * 64);
        size_t cap = (size_t)ctx->vl.vlog_capacity;
        HIP_TRY(ctx, ctx->vl.vlog_count.ensure(sizeof(unsigned long long)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->vl.vlog_count.p, 0, sizeof(unsigned long long), ctx->stream));
        HIP_TRY(ctx, ctx->vl.vlog_packet.ensure(cap * sizeof(long long)));
        HIP_TRY(ctx, ctx->vl.vlog_seq.ensure(cap * sizeof(int)));
        HIP_TRY(ctx, ctx->vl.vlog_nu.ensure(cap * sizeof(double)));
        HIP_TRY(ctx, ctx->vl.vlog_energy.ensure(cap * sizeof(double)));
        HIP_TRY(ctx, ctx->vl.vlog_mu.ensure(cap * sizeof(double)));
        // (option vpacket_last_interaction: vlog_r [cap] | before_nu [cap] | ids [cap] x 16 B in one allocation, mc_device.hpp -- what the VLI instantiations write)
        HIP_TRY(ctx, ctx->vl.vlog_r.ensure(cap * sizeof(double) * (vlog_li_call(ctx) ? 4 : 1)));
    }
    HIP_TRY(ctx, ctx->first_error.ensure(2 * sizeof(long long)));
    // (argument blocks reach the device through store_value(): consecutive propagate calls -- iterations, chunks submitted by
    // the host -- are not serialised by a stream synchronisation here)
    HIP_TRY(ctx, store_value(ctx->stream, ctx->first_error.as<FirstErrorInit>(), FirstErrorInit{{0x7fffffffffffffffLL, 0}}));
    ctx->pg.progress_done = false; ctx->pg.progress_wave = false; ctx->pg.progress_total = ctx->pk.n_packets;
    {
        std::lock_guard<std::mutex> lock(ctx->pg.progress_mutex);  // (tardis_mc_progress may be reading next_packet)
        HIP_TRY(ctx, ctx->next_packet.ensure(sizeof(unsigned long long)));
        if (!ctx->pg.ev_progress_reset) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pg.ev_progress_reset, hipEventDisableTiming));
    }
    HIP_TRY(ctx, hipMemsetAsync(ctx->next_packet.p, 0, sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->pg.ev_progress_reset, ctx->stream));
    // which kernel (propagate_plan.hpp).  The screening tables are built by the first call whose plan screens; a negative optical depth in them
    // means no screening, and the plan is made again knowing that
    call.plan = plan::plan_propagate(plan_input(ctx));
    if (!call.plan.error && call.plan.screen_on && !ctx->sc.pfx_valid) {
        rc = build_screening_tables(ctx);
        if (rc) return rc;
        if (ctx->sc.pfx_negative) call.plan = plan::plan_propagate(plan_input(ctx));
    }
    if (call.plan.error) return fail(ctx, call.plan.error, "%s", call.plan.message);
    ctx->last_table_offsets = call.plan.last_table_offsets;
    ctx->last_variant = call.plan.last_variant;
    ctx->sw.last_sweep_skip = 0;  // (set by choose_wave_kernel where the call's lane sweeps skip)
    ctx->wv.last_tracker_defer = -1;  // (the wave kernel's runner says otherwise)
    ctx->last_kernel_table = -1;      // (the lookup of the call's kernel says otherwise)
    std::fill(std::begin(ctx->last_kernel_key), std::end(ctx->last_kernel_key), 0);
    rc = call.plan.cooperative ? run_cooperative(ctx, call) : run_lane_kernel(ctx, call);
    if (rc) return rc;
    {   // events per packet of this call, for the log sizing of the next one (asynchronous, pinned host memory)
        if (!ctx->wv.events_host) {
            HIP_TRY(ctx, hipHostMalloc((void **)&ctx->wv.events_host, 2 * sizeof(unsigned long long), hipHostMallocDefault));
            ctx->wv.events_host[0] = ctx->wv.events_host[1] = 0;
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->wv.ev_events, hipEventDisableTiming));
        }
        ctx->wv.events_host[1] = (unsigned long long)ctx->pk.n_packets;
        HIP_TRY(ctx, hipMemcpyAsync(&ctx->wv.events_host[0], ctx->counters.as<unsigned long long>() + TARDIS_MC_CNT_EVENTS,
                                    sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->wv.ev_events, ctx->stream));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->timed = true;
    ctx->es.est_propagated = true;
    if (call.tune_slot >= 0) {
        HIP_TRY(ctx, hipEventRecord(ctx->lt.ev_tune[1], ctx->stream));
        ctx->lt.ls_tune.pending = call.tune_slot;
    }
    ctx->el.ev_valid = ctx->el.track_full;  // (a call that failed half-way leaves no event log to read)
    if (ctx->bf.on && ctx->pk.n_packets > 0) {  // the accumulate pass, behind the last launch and behind every existing timer's last event; it consumes the log
        const mc::SegmentLog &L = ctx->problem_host.seglog;
        rc = bf_accumulate_pass(ctx, L.recs, L.keys, L.chunk_fill, (int)L.n_chunks, L.chunk_rows, L.dropped);
        if (rc) return rc;
        ctx->bf.seg_valid = ctx->bf.seg_keep;
    }
    ctx->pk.li_valid = ctx->pk.track;
    ctx->vl.vl_valid = c.enable_vpacket_tracking && call.vpk && ctx->vl.vlog_capacity > 0;
    ctx->vl.vl_li = vlog_li_call(ctx);
    ctx->vl.vl_packets = ctx->pk.n_packets;
    ctx->vl.vl_capacity = ctx->vl.vlog_capacity;
    return TARDIS_MC_OK;
}

int tardis_mc_synchronize(TardisMcContext *ctx)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pg.progress_done = true;
    return TARDIS_MC_OK;
}

int tardis_mc_progress(TardisMcContext *ctx, int64_t *out_packets_started, int64_t *out_packets_total)
{
    if (!ctx || !out_packets_started || !out_packets_total) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    const long long total = ctx->pg.progress_total.load();
    *out_packets_total = total;
    *out_packets_started = 0;
    if (ctx->pg.progress_done.load()) { *out_packets_started = total; return TARDIS_MC_OK; }
    if (!ctx->pg.progress_wave.load()) return TARDIS_MC_OK;
    std::lock_guard<std::mutex> lock(ctx->pg.progress_mutex);
    if (hipSetDevice(ctx->device) != hipSuccess) return TARDIS_MC_ERR_HIP;  // (the polling thread's current device is 0 until it says otherwise)
    if (!ctx->next_packet.p || !ctx->pg.ev_progress_reset || hipEventQuery(ctx->pg.ev_progress_reset) != hipSuccess) return TARDIS_MC_OK;  // (not reset yet)
    if (!ctx->pg.stream_progress && hipStreamCreateWithFlags(&ctx->pg.stream_progress, hipStreamNonBlocking) != hipSuccess) return TARDIS_MC_ERR_HIP;
    if (!ctx->pg.progress_host && hipHostMalloc((void **)&ctx->pg.progress_host, sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) return TARDIS_MC_ERR_HIP;
    if (hipMemcpyAsync(ctx->pg.progress_host, ctx->next_packet.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->pg.stream_progress) != hipSuccess ||
        hipStreamSynchronize(ctx->pg.stream_progress) != hipSuccess)
        return TARDIS_MC_ERR_HIP;
    *out_packets_started = (int64_t)std::min<unsigned long long>(*ctx->pg.progress_host, (unsigned long long)std::max<long long>(total, 0));  // (a wave reserves 32 at a time)
    return TARDIS_MC_OK;
}

int tardis_mc_last_propagate_ms(TardisMcContext *ctx, double *out_ms)
{
    if (!ctx || !out_ms) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no propagate has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    *out_ms = (double)ms;
    return TARDIS_MC_OK;
}

int tardis_mc_last_kernel_times(TardisMcContext *ctx, double *out_seed_ms, double *out_propagate_ms, int *out_launches)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no propagate has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop));
    double seed = 0.0, prop = 0.0;
    if (ctx->wv.wave_epoch_mode) {  // wave kernel: launch preparation once, then one propagation launch + estimator passes per epoch
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_chunk[0], ctx->ev_chunk[1]));
        ctx->sum_seed_ms = ms;
        if (ctx->wv.prop_pending) {
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_chunk[2], ctx->ev_chunk[3]));
            ctx->sum_prop_ms += ms;
            ctx->wv.prop_pending = false;
        }
        for (int b = 0; b < 2; ++b)
            if (ctx->wv.post_pending[b]) {
                HIP_TRY(ctx, hipEventSynchronize(ctx->wv.ev_post[2 * b + 1]));
                HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->wv.ev_post[2 * b], ctx->wv.ev_post[2 * b + 1]));
                ctx->sum_post_ms += ms;
                ctx->wv.post_pending[b] = false;
            }
        ctx->last_post_ms = ctx->sum_post_ms;
        if (out_seed_ms) *out_seed_ms = ctx->sum_seed_ms;
        if (out_propagate_ms) *out_propagate_ms = ctx->sum_prop_ms;
        if (out_launches) *out_launches = std::max(ctx->launches, 1);
        return TARDIS_MC_OK;
    }
    if (ctx->chunks_timed == 0) {  // lane-per-packet variant: one launch, no seeding kernel
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
        prop = ms;
    }
    double post = 0.0;
    for (int ci = 0; ci < ctx->chunks_timed; ++ci) {
        float a = 0.f, b = 0.f, c = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&a, ctx->ev_chunk[4 * ci], ctx->ev_chunk[4 * ci + 1]));
        HIP_TRY(ctx, hipEventElapsedTime(&b, ctx->ev_chunk[4 * ci + 1], ctx->ev_chunk[4 * ci + 2]));
        HIP_TRY(ctx, hipEventElapsedTime(&c, ctx->ev_chunk[4 * ci + 2], ctx->ev_chunk[4 * ci + 3]));
        seed += a;
        prop += b;
        post += c;
    }
    ctx->last_post_ms = post;
    if (out_seed_ms) *out_seed_ms = seed;
    if (out_propagate_ms) *out_propagate_ms = prop;
    if (out_launches) *out_launches = ctx->chunks_timed ? ctx->chunks_timed : 1;
    return TARDIS_MC_OK;
}

int tardis_mc_last_counters(TardisMcContext *ctx, int64_t out_counters[TARDIS_MC_N_COUNTERS])
{
    if (!ctx || !out_counters) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->counters.p) return fail(ctx, TARDIS_MC_ERR_STATE, "no work counters yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long cnt[TARDIS_MC_N_COUNTERS];
    HIP_TRY(ctx, hipMemcpyAsync(cnt, ctx->counters.p, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < TARDIS_MC_N_COUNTERS; ++k) out_counters[k] = (int64_t)cnt[k];
    out_counters[TARDIS_MC_CNT_PACKETS] = ctx->pk.n_packets;
    return TARDIS_MC_OK;
}

int tardis_mc_last_variant(TardisMcContext *ctx) { return ctx ? ctx->last_variant : -1; }
int tardis_mc_last_sweep_skip(TardisMcContext *ctx) { return ctx ? ctx->sw.last_sweep_skip : -1; }
int tardis_mc_last_table_offsets(TardisMcContext *ctx) { return ctx ? ctx->last_table_offsets : -1; }
int tardis_mc_last_compactions(TardisMcContext *ctx) { return ctx ? ctx->wv.compactions : -1; }
int tardis_mc_last_tracker_defer(TardisMcContext *ctx) { return ctx ? ctx->wv.last_tracker_defer : -1; }

int tardis_mc_kernel_table_row(int table, int row, int key[12])
{
    if (table == 0) return kernel_table_row(LANE_KERNELS, row, key);
    if (table == 1) return kernel_table_row(GROUP_KERNELS, row, key);
    if (table == 2) return kernel_table_row(WAVE_KERNELS, row, key);
    return TARDIS_MC_ERR_INVALID_ARGUMENT;
}

int tardis_mc_last_kernel_key(TardisMcContext *ctx, int *table, int key[12])
{
    if (!ctx || !table || !key) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    *table = ctx->last_kernel_table;
    std::copy(std::begin(ctx->last_kernel_key), std::end(ctx->last_kernel_key), key);
    return TARDIS_MC_OK;
}

int tardis_mc_last_estimator_ms(TardisMcContext *ctx, double *out_ms)
{
    if (!ctx || !out_ms) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    double seed, prop;
    int launches;
    int rc = tardis_mc_last_kernel_times(ctx, &seed, &prop, &launches);
    if (rc) return rc;
    *out_ms = ctx->last_post_ms;
    return TARDIS_MC_OK;
}

static int reduce_estimator_copies(TardisMcContext *ctx)
{
    if (ctx->es.est_copies <= 1) return TARDIS_MC_OK;
    EstLayout e = est_layout(ctx->es.est_S, ctx->es.est_L, ctx->es.est_G, ctx->es.est_copies);
    long long n = (long long)(2 * ctx->es.est_S * ctx->es.est_L);
    hipLaunchKernelGGL(reduce_copies_kernel, dim3(2048), dim3(256), 0, ctx->stream, ctx->es.est.as<double>() + e.jblue, n,
                       (long long)e.copy_stride, ctx->es.est_copies);
    HIP_TRY(ctx, hipGetLastError());
    return TARDIS_MC_OK;
}

int tardis_mc_get_results(TardisMcContext *ctx, TardisMcResult *res)
{
    if (!ctx || !res) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->es.est_valid) return fail(ctx, TARDIS_MC_ERR_STATE, "nothing to fetch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = reduce_estimator_copies(ctx);
    if (rc) return rc;
    const size_t P = (size_t)ctx->pk.n_packets, S = ctx->es.est_S, L = ctx->es.est_L, G = ctx->es.est_G;
    EstLayout e = est_layout(S, L, G, ctx->es.est_copies);
    double *base = ctx->es.est.as<double>();
    auto d2h = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        if (!dst || !bytes) return hipSuccess;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    };
    if (ctx->have_packets) {
        // (arrays a streaming propagate has been filling, tardis_mc_stream_results: only what has not been sent yet)
        void *dev[16], *host[16];
        per_packet_device_arrays(ctx, dev);
        per_packet_host_arrays(res, host);
        std::vector<CopyJob> jobs;
        bool patch[16];
        for (int a = 0; a < 16; ++a) {
            patch[a] = false;
            if (!host[a] || !dev[a]) continue;
            if (ctx->rs.valid && host[a] == ctx->rs.dst[a]) {
                patch[a] = ctx->rs.n_late > 0;
                const size_t off = (size_t)ctx->rs.upto * 8;
                if (P * 8 > off) jobs.push_back({(char *)host[a] + off, (char *)dev[a] + off, P * 8 - off});
            } else {
                jobs.push_back({host[a], dev[a], P * 8});
            }
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the propagation and the tracker unpacking are over)
        if (ctx->rs.valid && ctx->rs.n_late > 0) {  // the packets that were in flight when their range was sent
            const size_t m = (size_t)ctx->rs.n_late;
            std::vector<unsigned> idx(m);
            std::vector<unsigned long long> vals(m);
            HIP_TRY(ctx, hipMemcpy(idx.data(), ctx->rs.late.p, m * sizeof(unsigned), hipMemcpyDeviceToHost));
            for (int a = 0; a < 16; ++a) {
                if (!patch[a]) continue;
                HIP_TRY(ctx, hipMemcpy(vals.data(), ctx->rs.vals.as<unsigned long long>() + (size_t)a * m, m * 8, hipMemcpyDeviceToHost));
                unsigned long long *out = (unsigned long long *)host[a];
                for (size_t j = 0; j < m; ++j) out[idx[j]] = vals[j];
            }
        }
        HIP_TRY(ctx, host_copy(ctx, jobs, false));
    }
    HIP_TRY(ctx, d2h(res->j_estimator, base + e.J, S * 8));
    HIP_TRY(ctx, d2h(res->nu_bar_estimator, base + e.nubar, S * 8));
    HIP_TRY(ctx, d2h(res->v_packets_energy_hist, base + e.vhist, G * 8));
    if (res->j_blue_estimator || res->edotlu_estimator) {
        HIP_TRY(ctx, ctx->staging.ensure(L * S * sizeof(double)));
        if (res->j_blue_estimator) {
            HIP_TRY(ctx, launch_transpose(ctx->stream, base + e.jblue, ctx->staging.as<double>(), (long long)S, (long long)L));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, host_copy(ctx, {{res->j_blue_estimator, ctx->staging.p, L * S * 8}}, false));
        }
        if (res->edotlu_estimator) {
            HIP_TRY(ctx, launch_transpose(ctx->stream, base + e.edot, ctx->staging.as<double>(), (long long)S, (long long)L));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, host_copy(ctx, {{res->edotlu_estimator, ctx->staging.p, L * S * 8}}, false));
        }
    }
    unsigned long long cnt[TARDIS_MC_N_COUNTERS] = {0};
    if (ctx->counters.p) HIP_TRY(ctx, d2h(cnt, ctx->counters.p, sizeof cnt));
    long long ferr[2] = {0x7fffffffffffffffLL, 0};
    if (ctx->first_error.p) HIP_TRY(ctx, d2h(ferr, ctx->first_error.p, sizeof ferr));
    unsigned long long vcount = 0;
    const bool vlog = ctx->cfg.enable_vpacket_tracking && ctx->cfg.number_of_vpackets > 0 && ctx->vl.vlog_count.p;
    if (vlog) HIP_TRY(ctx, d2h(&vcount, ctx->vl.vlog_count.p, sizeof vcount));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < TARDIS_MC_N_COUNTERS; ++k) res->counters[k] = (int64_t)cnt[k];
    res->counters[TARDIS_MC_CNT_PACKETS] = ctx->pk.n_packets;
    if (ctx->pk.n_packets > 0) ctx->wv.traces_per_packet = (double)cnt[TARDIS_MC_CNT_EVENTS] / (double)ctx->pk.n_packets;
    res->first_error_packet = -1;
    res->error_code = 0;
    if (ferr[0] != 0x7fffffffffffffffLL) {
        res->first_error_packet = ferr[0];
        double marker = 0.0;  // the failing lane stored its error code in out_nu[packet]
        HIP_TRY(ctx, hipMemcpy(&marker, ctx->pk.out_nu.as<double>() + ferr[0], 8, hipMemcpyDeviceToHost));
        res->error_code = (int)marker;
    }
    res->vpacket_log_count = 0;
    if (vlog) {
        res->vpacket_log_count = (int64_t)vcount;
        size_t n = (size_t)std::min<unsigned long long>(vcount, (unsigned long long)ctx->vl.vlog_capacity);
        std::vector<long long> pk(n);
        std::vector<int> seq(n);
        std::vector<double> nu(n), en(n), mu(n), rr(n);
        if (n) {
            HIP_TRY(ctx, hipMemcpy(pk.data(), ctx->vl.vlog_packet.p, n * 8, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(seq.data(), ctx->vl.vlog_seq.p, n * 4, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(nu.data(), ctx->vl.vlog_nu.p, n * 8, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(en.data(), ctx->vl.vlog_energy.p, n * 8, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(mu.data(), ctx->vl.vlog_mu.p, n * 8, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(rr.data(), ctx->vl.vlog_r.p, n * 8, hipMemcpyDeviceToHost));
        }
        // the reference consolidates per-packet lists in packet order (packet_collections.py:310-396)
        std::vector<size_t> order(n);
        std::iota(order.begin(), order.end(), (size_t)0);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return pk[a] != pk[b] ? pk[a] < pk[b] : seq[a] < seq[b]; });
        size_t m = std::min<size_t>(n, (size_t)std::max<int64_t>(0, res->vpacket_log_capacity));
        for (size_t k = 0; k < m; ++k) {
            size_t s = order[k];
            if (res->vpacket_nus) res->vpacket_nus[k] = nu[s];
            if (res->vpacket_energies) res->vpacket_energies[k] = en[s];
            if (res->vpacket_initial_mus) res->vpacket_initial_mus[k] = mu[s];
            if (res->vpacket_initial_rs) res->vpacket_initial_rs[k] = rr[s];
        }
    }
    return res->error_code;
}

int tardis_mc_get_event_log(TardisMcContext *ctx, TardisMcEventLog *log)
{
    if (!ctx || !log) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    log->count = 0;
    log->dropped = 0;
    if (!ctx->el.ev_valid) return fail(ctx, TARDIS_MC_ERR_STATE, "no event log: the last tardis_mc_propagate ran without the option track_full");
    if (ctx->pk.n_packets != ctx->el.ev_packets)
        return fail(ctx, TARDIS_MC_ERR_STATE, "no event log: the resident packets were replaced after the tracked tardis_mc_propagate");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {   // a call in which a packet failed has no complete log (that packet's rows end at the error)
        long long fe = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&fe, ctx->first_error.p, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (fe != 0x7fffffffffffffffLL)
            return fail(ctx, TARDIS_MC_ERR_STATE, "no event log: packet %lld of the tracked tardis_mc_propagate failed", fe);
    }
    const long long n = ctx->el.ev_packets;
    const long long tiles = std::max<long long>(1, (n + mc::EV_SCAN_TILE - 1) / mc::EV_SCAN_TILE);
    HIP_TRY(ctx, ctx->el.ev_offsets.ensure((size_t)(n + 1) * sizeof(long long)));
    HIP_TRY(ctx, ctx->el.ev_tiles.ensure((size_t)tiles * sizeof(long long)));
    long long *offsets = ctx->el.ev_offsets.as<long long>();
    hipLaunchKernelGGL(mc::event_scan_tiles_kernel, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, ctx->el.ev_counts.as<int>(), n,
                       ctx->el.ev_tiles.as<long long>());
    hipLaunchKernelGGL(mc::event_scan_sums_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->el.ev_tiles.as<long long>(), tiles, offsets, n);
    hipLaunchKernelGGL(mc::event_scan_apply_kernel, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, ctx->el.ev_counts.as<int>(), n,
                       ctx->el.ev_tiles.as<long long>(), offsets);
    HIP_TRY(ctx, hipGetLastError());
    long long total = 0;
    unsigned long long state[2] = {0, 0};  // {pool_next (low 32 bits), dropped}
    HIP_TRY(ctx, hipMemcpyAsync(&total, offsets + n, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(state, ctx->el.ev_state.p, sizeof state, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    log->count = total;
    log->dropped = (int64_t)state[1];
    if (log->offsets) HIP_TRY(ctx, hipMemcpyAsync(log->offsets, offsets, (size_t)(n + 1) * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    // the columns only when every row is there and fits the caller's arrays (otherwise: re-run with event_log_capacity = count)
    if (state[1] == 0 && total > 0 && total <= log->capacity) {
        HIP_TRY(ctx, ctx->el.ev_cols.ensure((size_t)total * 14 * 8));
        long long *ci = ctx->el.ev_cols.as<long long>();
        double *cf = reinterpret_cast<double *>(ci + 7 * total);
        mc::EventColumns col{ci, ci + total, ci + 2 * total, ci + 3 * total, ci + 4 * total, ci + 5 * total, ci + 6 * total,
                             cf, cf + total, cf + 2 * total, cf + 3 * total, cf + 4 * total, cf + 5 * total, cf + 6 * total};
        const unsigned used_chunks = std::min<unsigned>((unsigned)(state[0] & 0xffffffffull), ctx->el.ev_n_chunks);
        const long long n_slots = (long long)used_chunks * ctx->el.ev_chunk_rows;
        const int blocks = (int)std::max<long long>(1, std::min<long long>((n_slots + 255) / 256, 65536));
        hipLaunchKernelGGL(mc::event_scatter_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->el.ev_rows.as<mc::EventRow>(),
                           ctx->el.ev_fill.as<unsigned>(), ctx->el.ev_chunk_rows, n_slots, offsets, col);
        HIP_TRY(ctx, hipGetLastError());
        int64_t *dst_i[7] = {log->event_id, log->interaction_type, log->status, log->shell_id, log->after_shell_id, log->line_absorb_id,
                             log->line_emit_id};
        double *dst_f[7] = {log->radius, log->before_nu, log->before_mu, log->before_energy, log->after_nu, log->after_mu, log->after_energy};
        for (int k = 0; k < 7; ++k) {
            if (dst_i[k]) HIP_TRY(ctx, hipMemcpyAsync(dst_i[k], ci + k * total, (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
            if (dst_f[k]) HIP_TRY(ctx, hipMemcpyAsync(dst_f[k], cf + k * total, (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TARDIS_MC_OK;
}

int tardis_mc_stream_results(TardisMcContext *ctx, const TardisMcResult *dst)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    ctx->rs.armed = false;
    if (!dst) return TARDIS_MC_OK;
    per_packet_host_arrays(dst, ctx->rs.dst);
    ctx->rs.armed = true;
    return TARDIS_MC_OK;
}

int tardis_mc_streamed_packets(TardisMcContext *ctx, int64_t *out_streamed, int64_t *out_resent)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (out_streamed) *out_streamed = ctx->rs.valid ? ctx->rs.upto : 0;
    if (out_resent) *out_resent = ctx->rs.valid ? ctx->rs.n_late : 0;
    return TARDIS_MC_OK;
}

int tardis_mc_run(TardisMcContext *ctx, const TardisMcPackets *packets, const TardisMcGeometry *geometry,
                  const TardisMcOpacity *opacity, const TardisMcConfig *config, TardisMcResult *result)
{
    int rc;
    if ((rc = tardis_mc_set_geometry(ctx, geometry))) return rc;
    if ((rc = tardis_mc_set_opacity(ctx, opacity))) return rc;
    if ((rc = tardis_mc_set_config(ctx, config))) return rc;
    // the caller's log capacity is for this call only, whichever way the call ends (the context is cached per process)
    struct VlogScope {
        TardisMcContext *c; bool was_user; long long was;
        ~VlogScope() { c->vl.vlog_capacity_user = was_user; if (was_user) c->vl.vlog_capacity = was; }
    } scope{ctx, ctx->vl.vlog_capacity_user, ctx->vl.vlog_capacity};
    if (result && result->vpacket_log_capacity > 0) { ctx->vl.vlog_capacity = result->vpacket_log_capacity; ctx->vl.vlog_capacity_user = true; }
    if ((rc = tardis_mc_set_packets(ctx, packets))) return rc;
    if ((rc = tardis_mc_reset_estimators(ctx))) return rc;
    if (result && (rc = tardis_mc_stream_results(ctx, result))) return rc;  // (the result arrays are known from the start: filled launch by launch)
    if ((rc = tardis_mc_propagate(ctx))) return rc;
    if ((rc = tardis_mc_synchronize(ctx))) return rc;
    return tardis_mc_get_results(ctx, result);
}

int tardis_mc_packet_spectrum(TardisMcContext *ctx, double time_of_simulation, double luminosity_nu_start,
                              double luminosity_nu_end, double *emitted_luminosity_hist, double *reabsorbed_luminosity_hist,
                              double *out_emitted_luminosity, double *out_reabsorbed_luminosity)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->have_packets || !ctx->have_config || ctx->cfg.n_spectrum_grid < 2)
        return fail(ctx, TARDIS_MC_ERR_STATE, "packet spectrum needs propagated packets and a spectrum grid");
    if (!(time_of_simulation > 0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "time_of_simulation must be positive");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t B = (size_t)ctx->cfg.n_spectrum_grid - 1;
    ScopedDevBuf work;
    HIP_TRY(ctx, work.ensure((2 * B + 2) * sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(work.p, 0, (2 * B + 2) * sizeof(double), ctx->stream));
    double *w = work.as<double>();
    if (ctx->pk.n_packets > 0) {
        const int blocks = (int)std::min<long long>((ctx->pk.n_packets + 255) / 256, 4096);
        hipLaunchKernelGGL(spectrum_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->pk.out_nu.as<double>(), ctx->pk.out_e.as<double>(),
                           ctx->pk.n_packets, ctx->grid.as<double>(), (int)ctx->cfg.n_spectrum_grid, time_of_simulation,
                           luminosity_nu_start, luminosity_nu_end, w, w + B, w + 2 * B);
        HIP_TRY(ctx, hipGetLastError());
    }
    double lum[2] = {0, 0};
    if (emitted_luminosity_hist) HIP_TRY(ctx, hipMemcpyAsync(emitted_luminosity_hist, w, B * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (reabsorbed_luminosity_hist) HIP_TRY(ctx, hipMemcpyAsync(reabsorbed_luminosity_hist, w + B, B * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(lum, w + 2 * B, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (out_emitted_luminosity) *out_emitted_luminosity = lum[0];
    if (out_reabsorbed_luminosity) *out_reabsorbed_luminosity = lum[1];
    return TARDIS_MC_OK;
}

/* ---- consumer next to the path: the emitted spectrum decomposed by last interaction (packet_decomposition.hpp) ------------------ */
int tardis_mc_decomposition_path(int64_t n_classes, int64_t n_bins, int64_t n_shells)
{
    return decomp::choose_path(n_classes, n_bins, n_shells);
}

// The two decompositions share everything but the seven input columns: the resident per-packet results (tardis_mc_packet_decomposition) or
// the consolidated v-packet log (tardis_mc_vpacket_decomposition, virtual = true; consolidated first where it is not yet).
static int consolidate_vpacket_log(TardisMcContext *ctx, const char *who);

static int decomposition_impl(TardisMcContext *ctx, TardisMcDecomposition *d, const bool virt)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!d) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "packet decomposition: no argument block");
    d->n_selected = d->n_line = d->n_electron_scatter = d->n_no_interaction = 0;
    if (!d->line_class) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "packet decomposition: line_class is NULL");
    if (d->n_classes < 1 || d->n_classes > 0x7fffffffLL)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "packet decomposition: n_classes must be in [1, 2^31)");
    if (!(d->time_of_simulation > 0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "time_of_simulation must be positive");
    if (virt && (!ctx->have_packets || !ctx->have_opacity || !ctx->have_geometry || !ctx->vl.vl_valid || !ctx->vl.vl_li))
        return fail(ctx, TARDIS_MC_ERR_STATE, "v-packet decomposition: no v-packet log with last-interaction columns -- it follows a completed "
                    "tardis_mc_propagate with v-packet tracking and the option vpacket_last_interaction on, before the packets or the configuration are replaced");
    if (!virt && (!ctx->have_packets || !ctx->have_opacity || !ctx->have_geometry || !ctx->pk.li_valid))
        return fail(ctx, TARDIS_MC_ERR_STATE, "packet decomposition: no last-interaction results of the resident packets -- it follows a completed "
                    "tardis_mc_propagate with track_last_interaction on, before the packets are replaced");
    if (!ctx->have_config || ctx->cfg.n_spectrum_grid < 2) return fail(ctx, TARDIS_MC_ERR_STATE, "packet decomposition needs a spectrum grid");
    const long long C = d->n_classes, B = ctx->cfg.n_spectrum_grid - 1, S = ctx->n_shells, L = ctx->n_lines;
    long long P = ctx->pk.n_packets;
    // the class table, narrowed to 32 bits; no class is used as an index before it has passed this check
    std::vector<int> cls((size_t)L);
    for (long long i = 0; i < L; ++i) {
        const int64_t c = d->line_class[i];
        if (c < 0 || c >= C)
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "packet decomposition: line_class[%lld] = %lld is outside [0, %lld)", i, (long long)c, C);
        cls[(size_t)i] = (int)c;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    {   // a call in which a packet failed has no complete results (the failing lane's output_nu holds its error code)
        long long fe = 0x7fffffffffffffffLL;
        if (ctx->first_error.p) HIP_TRY(ctx, hipMemcpyAsync(&fe, ctx->first_error.p, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (fe != 0x7fffffffffffffffLL) return fail(ctx, TARDIS_MC_ERR_STATE, "packet decomposition: packet %lld of the last tardis_mc_propagate failed", fe);
    }
    bool timing_open = false;  // (a consolidation inside this call is part of its device time)
    if (virt) {
        if (!ctx->vl.vl_consolidated) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
            timing_open = true;
            const int rc = consolidate_vpacket_log(ctx, "v-packet decomposition");
            if (rc) return rc;
        }
        if (!ctx->vl.vl_consolidated)
            return fail(ctx, TARDIS_MC_ERR_STATE, "v-packet decomposition: the v-packet log overflowed (%lld entries, capacity %lld): run the call again with "
                        "vpacket_log_capacity >= %lld", ctx->vl.vl_count, ctx->vl.vl_capacity, ctx->vl.vl_count);
        P = ctx->vl.vl_count;
    }
    // one allocation: cells [(2C+2)B] doubles | shell_packets [(C+1)S] | line_emit [L] | line_absorb [L] | counts [4] | line_class [L] int32
    const size_t n_cells = (size_t)(2 * C + 2) * (size_t)B, n_shell = (size_t)(C + 1) * (size_t)S;
    const size_t n_words = n_cells + n_shell + 2 * (size_t)L + 4;
    HIP_TRY(ctx, ctx->pk.dc_work.ensure(n_words * 8 + (size_t)L * sizeof(int)));
    double *cells = ctx->pk.dc_work.as<double>();
    unsigned long long *shell = reinterpret_cast<unsigned long long *>(cells + n_cells), *line_emit = shell + n_shell, *line_absorb = line_emit + L,
                       *counts = line_absorb + L;
    int *d_cls = reinterpret_cast<int *>(counts + 4);
    HIP_TRY(ctx, hipMemcpyAsync(d_cls, cls.data(), (size_t)L * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (!timing_open) HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(cells, 0, n_words * 8, ctx->stream));
    if (P > 0) {
        mc::DecompositionArgs a{};
        if (virt) {  // the columns of the consolidated log, vl_cols: source_packet | nu | energy | mu | r | in_nu | in_r | type | in_id | out_id | shell_id
            double *f = ctx->vl.vl_cols.as<double>();
            long long *g = ctx->vl.vl_cols.as<long long>();
            a.out_nu = f + 1 * P; a.out_e = f + 2 * P; a.before_nu = f + 5 * P;
            a.type = g + 7 * P; a.absorb_id = g + 8 * P; a.emit_id = g + 9 * P; a.shell_id = g + 10 * P;
        } else {
            a.out_nu = ctx->pk.out_nu.as<double>(); a.out_e = ctx->pk.out_e.as<double>(); a.before_nu = ctx->pk.li_f64[3].as<double>();
            a.shell_id = ctx->pk.li_i64[0].as<long long>(); a.type = ctx->pk.li_i64[1].as<long long>();
            a.absorb_id = ctx->pk.li_i64[2].as<long long>(); a.emit_id = ctx->pk.li_i64[3].as<long long>();
        }
        a.n_packets = P;
        a.line_class = d_cls; a.n_lines = L; a.n_classes = C;
        a.edges = ctx->grid.as<double>(); a.n_edges = (int)ctx->cfg.n_spectrum_grid; a.n_shells = (int)S;
        a.t_sim = d->time_of_simulation; a.nu_start = d->nu_start; a.nu_end = d->nu_end;
        a.cells = cells; a.shell_packets = shell; a.line_emit = line_emit; a.line_absorb = line_absorb; a.counts = counts;
        const int cus = ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256;
        const long long want = (P + mc::DC_BLOCK - 1) / mc::DC_BLOCK;
        if (decomp::choose_path(C, B, S) == decomp::PATH_PRIVATISED) {
            // two workgroups per CU (the LDS budget allows it): each flushes its private copy once, so few of them
            const size_t lds = (size_t)decomp::private_bytes(C, B, S);
            hipLaunchKernelGGL(mc::packet_decomposition_kernel<true>, dim3((unsigned)std::min<long long>(want, 2LL * cus)), dim3(mc::DC_BLOCK), lds, ctx->stream, a);
        } else {
            hipLaunchKernelGGL(mc::packet_decomposition_kernel<false>, dim3((unsigned)std::min<long long>(want, 16LL * cus)), dim3(mc::DC_BLOCK), (size_t)decomp::FIXED_BYTES, ctx->stream, a);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->timed = true;
    ctx->chunks_timed = 0;
    auto d2h = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        if (!dst || !bytes) return hipSuccess;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    };
    const size_t CB = (size_t)C * (size_t)B;
    HIP_TRY(ctx, d2h(d->emission, cells, CB * 8));
    HIP_TRY(ctx, d2h(d->absorption, cells + CB, CB * 8));
    HIP_TRY(ctx, d2h(d->no_interaction, cells + 2 * CB, (size_t)B * 8));
    HIP_TRY(ctx, d2h(d->electron_scatter, cells + 2 * CB + B, (size_t)B * 8));
    HIP_TRY(ctx, d2h(d->shell_packets, shell, n_shell * 8));
    HIP_TRY(ctx, d2h(d->line_emit_packets, line_emit, (size_t)L * 8));
    HIP_TRY(ctx, d2h(d->line_absorb_packets, line_absorb, (size_t)L * 8));
    unsigned long long cnt[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, d2h(cnt, counts, sizeof cnt));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    d->n_selected = (int64_t)cnt[0]; d->n_line = (int64_t)cnt[1]; d->n_electron_scatter = (int64_t)cnt[2]; d->n_no_interaction = (int64_t)cnt[3];
    return TARDIS_MC_OK;
}

int tardis_mc_packet_decomposition(TardisMcContext *ctx, TardisMcDecomposition *d) { return decomposition_impl(ctx, d, false); }
int tardis_mc_vpacket_decomposition(TardisMcContext *ctx, TardisMcDecomposition *d) { return decomposition_impl(ctx, d, true); }

/* ---- the v-packet log, consolidated on the device (vpacket_log.hpp) ------------------------------------------------------------- */
// Checks the state, counts, scans and scatters.  On success vl_count holds the entries of the call; vl_consolidated says whether the
// columns are there (not when the device log overflowed: the caller then reports the count).
static int consolidate_vpacket_log(TardisMcContext *ctx, const char *who)
{
    if (!ctx->vl.vl_valid || !ctx->have_packets || ctx->pk.n_packets != ctx->vl.vl_packets)
        return fail(ctx, TARDIS_MC_ERR_STATE, "%s: no v-packet log -- it follows a completed tardis_mc_propagate with v-packet tracking, before the "
                    "packets or the configuration are replaced", who);
    if (ctx->vl.vl_consolidated) return TARDIS_MC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    long long fe = 0x7fffffffffffffffLL;
    unsigned long long vcount = 0;
    if (ctx->first_error.p) HIP_TRY(ctx, hipMemcpyAsync(&fe, ctx->first_error.p, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&vcount, ctx->vl.vlog_count.p, sizeof vcount, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (fe != 0x7fffffffffffffffLL) return fail(ctx, TARDIS_MC_ERR_STATE, "%s: packet %lld of the last tardis_mc_propagate failed", who, fe);
    ctx->vl.vl_count = (long long)vcount;
    if (ctx->vl.vl_count > ctx->vl.vl_capacity) return TARDIS_MC_OK;  // overflowed: only the count is known
    const long long n = ctx->vl.vl_packets, m = ctx->vl.vl_count;
    const long long tiles = std::max<long long>(1, (n + mc::EV_SCAN_TILE - 1) / mc::EV_SCAN_TILE);
    const int n_cols = ctx->vl.vl_li ? 11 : 5;
    HIP_TRY(ctx, ctx->vl.vl_counts.ensure((size_t)std::max<long long>(n, 1) * sizeof(int)));
    HIP_TRY(ctx, ctx->vl.vl_offsets.ensure((size_t)(n + 1) * sizeof(long long)));
    HIP_TRY(ctx, ctx->vl.vl_tiles.ensure((size_t)tiles * sizeof(long long)));
    HIP_TRY(ctx, ctx->vl.vl_errors.ensure(sizeof(unsigned long long)));
    HIP_TRY(ctx, ctx->vl.vl_cols.ensure((size_t)std::max<long long>(m, 1) * n_cols * 8));
    HIP_TRY(ctx, hipMemsetAsync(ctx->vl.vl_counts.p, 0, (size_t)std::max<long long>(n, 1) * sizeof(int), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->vl.vl_errors.p, 0, sizeof(unsigned long long), ctx->stream));
    const int blocks = (int)std::max<long long>(1, std::min<long long>((m + 255) / 256, 65536));
    long long *offsets = ctx->vl.vl_offsets.as<long long>();
    unsigned long long *errors = ctx->vl.vl_errors.as<unsigned long long>();
    if (m > 0) hipLaunchKernelGGL(mc::vpacket_log_count_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->vl.vlog_packet.as<long long>(), m, n, ctx->vl.vl_counts.as<int>(), errors);
    hipLaunchKernelGGL(mc::event_scan_tiles_kernel, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, ctx->vl.vl_counts.as<int>(), n, ctx->vl.vl_tiles.as<long long>());
    hipLaunchKernelGGL(mc::event_scan_sums_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->vl.vl_tiles.as<long long>(), tiles, offsets, n);
    hipLaunchKernelGGL(mc::event_scan_apply_kernel, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, ctx->vl.vl_counts.as<int>(), n, ctx->vl.vl_tiles.as<long long>(), offsets);
    if (m > 0) {
        mc::VpacketLogRaw raw{ctx->vl.vlog_packet.as<long long>(), ctx->vl.vlog_seq.as<int>(), ctx->vl.vlog_nu.as<double>(), ctx->vl.vlog_energy.as<double>(),
                              ctx->vl.vlog_mu.as<double>(), ctx->vl.vlog_r.as<double>(), ctx->vl.vl_li ? mc::vlog_last_ids(ctx->vl.vlog_r.as<double>(), ctx->vl.vl_capacity) : nullptr,
                              ctx->vl.vl_li ? mc::vlog_last_nu(ctx->vl.vlog_r.as<double>(), ctx->vl.vl_capacity) : nullptr};
        double *f = ctx->vl.vl_cols.as<double>();
        long long *g = ctx->vl.vl_cols.as<long long>();
        mc::VpacketLogColumns col{g, f + m, f + 2 * m, f + 3 * m, f + 4 * m, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (ctx->vl.vl_li) { col.li_in_nu = f + 5 * m; col.li_in_r = f + 6 * m; col.li_type = g + 7 * m; col.li_in_id = g + 8 * m; col.li_out_id = g + 9 * m; col.li_shell_id = g + 10 * m; }
        hipLaunchKernelGGL(mc::vpacket_log_scatter_kernel, dim3(blocks), dim3(256), 0, ctx->stream, raw, m, n, m, ctx->vl.vl_counts.as<int>(), offsets, col, errors);
    }
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long bad = 0;
    long long total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, errors, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&total, offsets + n, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != 0 || total != m)
        return fail(ctx, TARDIS_MC_ERR_STATE, "%s: the v-packet log is inconsistent (%llu entries with a packet, an ordinal or a position out of range; %lld of %lld "
                    "entries counted)", who, bad, total, m);
    ctx->vl.vl_consolidated = true;
    return TARDIS_MC_OK;
}

int tardis_mc_get_vpacket_log(TardisMcContext *ctx, TardisMcVpacketLog *log)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!log) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "v-packet log: no argument block");
    log->count = 0;
    void *li_dst[6] = {log->last_interaction_in_nu, log->last_interaction_in_r, log->last_interaction_type, log->last_interaction_in_id,
                       log->last_interaction_out_id, log->last_interaction_shell_id};
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = consolidate_vpacket_log(ctx, "v-packet log");  // (the timers of the propagate call stay as they are)
    if (rc) return rc;
    if (!ctx->vl.vl_li)
        for (void *q : li_dst)
            if (q) return fail(ctx, TARDIS_MC_ERR_STATE, "v-packet log: the last tardis_mc_propagate ran without the option vpacket_last_interaction, the six "
                               "last_interaction_* columns must be NULL");
    const long long m = ctx->vl.vl_count, n = ctx->vl.vl_packets;
    log->count = m;
    if (!ctx->vl.vl_consolidated || m > log->capacity) return TARDIS_MC_OK;  // overflow: only the count (run again with vpacket_log_capacity >= count)
    auto d2h = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        if (!dst || !bytes) return hipSuccess;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    };
    HIP_TRY(ctx, d2h(log->offsets, ctx->vl.vl_offsets.p, (size_t)(n + 1) * 8));
    const char *cols = static_cast<const char *>(ctx->vl.vl_cols.p);
    void *dst[5] = {log->source_packet, log->nus, log->energies, log->initial_mus, log->initial_rs};
    for (int k = 0; k < 5; ++k) HIP_TRY(ctx, d2h(dst[k], cols + (size_t)k * m * 8, (size_t)m * 8));
    if (ctx->vl.vl_li)
        for (int k = 0; k < 6; ++k) HIP_TRY(ctx, d2h(li_dst[k], cols + (size_t)(5 + k) * m * 8, (size_t)m * 8));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TARDIS_MC_OK;
}

// The kernels of tardis_mc_radiation_field, enqueued on the context's stream: t_rad, W and the j_blue normalisation into work ([4 S]: volume, t_rad, W, norm),
// and, where out_t is given, the j_blues [S][L] into it.  Shared with the detailed mode of tardis_mc_update_opacity, whose j are these bits.
static int radiation_field_enqueue(TardisMcContext *ctx, double time_of_simulation, const double *volume, double w_epsilon, int detailed_optical_window,
                                   DevBuf &work, double *out_t)
{
    int rc = reduce_estimator_copies(ctx);
    if (rc) return rc;
    const size_t S = ctx->es.est_S, L = ctx->es.est_L;
    EstLayout e = est_layout(S, L, ctx->es.est_G, ctx->es.est_copies);
    double *base = ctx->es.est.as<double>();
    // constants, tardis/constants.py:1 (CODATA 2010, cgs)
    const double h = H_PLANCK, k_b = K_BOLTZMANN, sigma_sb = 5.670373e-5, c = mc::C_LIGHT, zeta5 = 1.0369277551433699;
    const double pi = 3.141592653589793;
    RadFieldConsts k;
    k.t_rad_const = (pi * pi * pi * pi / (15 * 24 * zeta5)) * (h / k_b);
    k.four_sigma = 4 * sigma_sb;
    k.jblue_norm_num = c * ctx->t_exp;
    k.four_pi_tsim = 4 * pi * time_of_simulation;
    k.tsim = time_of_simulation;
    k.planck_coef = 2 * h / (c * c);
    k.h = h; k.k_b = k_b; k.w_epsilon = w_epsilon; k.c_ang = c * 1e8;
    HIP_TRY(ctx, work.ensure(4 * S * sizeof(double)));
    double *d_vol = work.as<double>(), *d_t = d_vol + S, *d_w = d_t + S, *d_norm = d_w + S;
    HIP_TRY(ctx, hipMemcpyAsync(d_vol, volume, S * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(radfield_shell_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, ctx->stream, base + e.J, base + e.nubar,
                       d_vol, (int)S, k, d_t, d_w, d_norm);
    HIP_TRY(ctx, hipGetLastError());
    if (out_t && L > 0) {
        const unsigned bx = (unsigned)std::min<size_t>((L + 255) / 256, 1024);
        hipLaunchKernelGGL(radfield_jblue_kernel, dim3(bx, (unsigned)S), dim3(256), 0, ctx->stream, base + e.jblue,
                           ctx->ot.nu_line.as<double>(), d_t, d_w, d_norm, (int)S, (long long)L, k, detailed_optical_window, out_t);
        HIP_TRY(ctx, hipGetLastError());
    }
    return TARDIS_MC_OK;
}

int tardis_mc_radiation_field(TardisMcContext *ctx, double time_of_simulation, const double *volume, double w_epsilon,
                              int detailed_optical_window, double *t_radiative, double *dilution_factor, double *j_blues)
{
    if (!ctx || !volume) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->es.est_valid || !ctx->have_opacity || !ctx->have_geometry)
        return fail(ctx, TARDIS_MC_ERR_STATE, "radiation field update needs propagated estimators");
    if (!(time_of_simulation > 0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "time_of_simulation must be positive");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t S = ctx->es.est_S, L = ctx->es.est_L;
    const bool want_j = j_blues && L > 0;
    ScopedDevBuf work, out_t;
    if (want_j) {
        HIP_TRY(ctx, out_t.ensure(L * S * sizeof(double)));
        HIP_TRY(ctx, ctx->staging.ensure(L * S * sizeof(double)));
    }
    int rc = radiation_field_enqueue(ctx, time_of_simulation, volume, w_epsilon, detailed_optical_window, work, want_j ? out_t.as<double>() : nullptr);
    if (rc) return rc;
    const double *d_t = work.as<double>() + S, *d_w = d_t + S;
    if (t_radiative) HIP_TRY(ctx, hipMemcpyAsync(t_radiative, d_t, S * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (dilution_factor) HIP_TRY(ctx, hipMemcpyAsync(dilution_factor, d_w, S * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (want_j) {
        HIP_TRY(ctx, launch_transpose(ctx->stream, out_t.as<double>(), ctx->staging.as<double>(), (long long)S, (long long)L));
        HIP_TRY(ctx, hipMemcpyAsync(j_blues, ctx->staging.p, L * S * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TARDIS_MC_OK;
}

// exp(-tau) in the layout of tau_t, kept until the next set_opacity: the source function and the resident formal integral after it read one table
static int ensure_exp_tau(TardisMcContext *ctx)
{
    if (ctx->sf.exp_valid) return TARDIS_MC_OK;
    const size_t n = (size_t)ctx->n_shells * (size_t)ctx->n_lines;
    HIP_TRY(ctx, ctx->sf.exp_tau.ensure(n * sizeof(double)));
    hipLaunchKernelGGL(mc::fi_exp_tau_kernel, dim3(2048), dim3(256), 0, ctx->stream, ctx->ot.tau_t.as<double>(), (long long)n, ctx->sf.exp_tau.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    ctx->sf.exp_valid = true;
    return TARDIS_MC_OK;
}

// What a formal integral runs on -- the geometry, the electron densities and the four [n_shells][n_lines] tables, all on the device: the context's own
// (host-fed and resident entry points) or the interpolated ones of a call (formal_interpolate.hpp).  The host-fed entry point has no tables yet
// (exp_tau == nullptr): its three host arrays are uploaded into the call's scratch and exp(-tau) of the resident optical depths is tabulated beside them.
struct FormalIntegralInput {
    size_t n_shells = 0;
    const double *r_inner = nullptr, *r_outer = nullptr, *n_e = nullptr;                        // [n_shells]
    const double *exp_tau = nullptr, *att = nullptr, *jred = nullptr, *jblue = nullptr;         // [n_shells][n_lines]
    const double *host_att = nullptr, *host_jred = nullptr, *host_jblue = nullptr;              // (exp_tau == nullptr)
    bool timer_started = false;  // ev_start is recorded already, in front of kernels of the caller that belong to the call's device time
};

// state and arguments of the three formal integral entry points (`resident`: the call reads the resident source function)
static int formal_integral_check(TardisMcContext *ctx, bool resident, const double *frequencies, bool have_tables, const double *luminosity_densities,
                                 int64_t n_frequencies, int64_t n_impact_parameters)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->have_geometry || !ctx->have_opacity)
        return fail(ctx, TARDIS_MC_ERR_STATE, "formal integral needs set_geometry and set_opacity");
    if (resident && !ctx->sf.valid)
        return fail(ctx, TARDIS_MC_ERR_STATE, "no resident source function: tardis_mc_source_function must follow the last propagate / all-reduce");
    if (!frequencies || !have_tables || !luminosity_densities || n_frequencies < 0 || n_impact_parameters < 2 ||
        n_frequencies > (1LL << 30) || n_impact_parameters > 65535)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid formal integral arguments");
    return TARDIS_MC_OK;
}

// the formal integral on `in` (checked by formal_integral_check)
static int formal_integral_impl(TardisMcContext *ctx, const FormalIntegralInput &in, double inner_temperature, const double *frequencies,
                                int64_t n_frequencies, int64_t n_impact_parameters, double *luminosity_densities, double *intensities_nu_p)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t S = in.n_shells, L = (size_t)ctx->n_lines, n_nu = (size_t)n_frequencies, N = (size_t)n_impact_parameters;
    if (n_nu == 0) return TARDIS_MC_OK;
    const bool host_fed = in.exp_tau == nullptr;
    ScopedDevBuf work;  // [exp_tau | att | jred | jblue | freqs | z | I | Lum] doubles, then sid / n_int ints (tables on the device already: none in front)
    const size_t n_tab = host_fed ? S * L : 0;
    const size_t n_d = 4 * n_tab + n_nu + N * 2 * S + n_nu * N + n_nu;
    HIP_TRY(ctx, work.ensure(n_d * sizeof(double) + (N * 2 * S + N) * sizeof(int)));
    double *d_exp = work.as<double>(), *d_att = d_exp + n_tab, *d_jred = d_att + n_tab, *d_jblue = d_jred + n_tab,
           *d_freq = d_jblue + n_tab, *d_z = d_freq + n_nu, *d_I = d_z + N * 2 * S, *d_lum = d_I + n_nu * N;
    int *d_sid = reinterpret_cast<int *>(d_lum + n_nu), *d_nint = d_sid + N * 2 * S;
    if (host_fed) {
        HIP_TRY(ctx, hipMemcpyAsync(d_att, in.host_att, S * L * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_jred, in.host_jred, S * L * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_jblue, in.host_jblue, S * L * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_freq, frequencies, n_nu * 8, hipMemcpyHostToDevice, ctx->stream));
    if (!in.timer_started) HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    const double *t_exp_tau = in.exp_tau, *t_att = in.att, *t_jred = in.jred, *t_jblue = in.jblue;
    if (host_fed) {
        if (S * L > 0)
            hipLaunchKernelGGL(mc::fi_exp_tau_kernel, dim3(2048), dim3(256), 0, ctx->stream, ctx->ot.tau_t.as<double>(), (long long)(S * L), d_exp);
        t_exp_tau = d_exp; t_att = d_att; t_jred = d_jred; t_jblue = d_jblue;
    }
    hipLaunchKernelGGL(mc::fi_intersections_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, ctx->stream, (int)S,
                       in.r_inner, in.r_outer, ctx->t_exp, (int)N, d_z, d_sid, d_nint);
    std::vector<double> r_last(1);
    HIP_TRY(ctx, hipMemcpyAsync(r_last.data(), in.r_outer + (S - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    mc::FormalIntegralArgs a{};
    a.n_shells = (int)S; a.n_lines = (int)L; a.n_nu = (int)n_nu; a.N = (int)N;
    a.t_exp = ctx->t_exp; a.inner_temperature = inner_temperature; a.radius_max = r_last[0];
    a.sigma_thomson = 6.652458734e-25;  // SIGMA_THOMSON, transport/montecarlo/configuration/constants.py:3 (astropy const13)
    a.r_inner = in.r_inner; a.nu_line = ctx->ot.nu_line.as<double>(); a.n_e = in.n_e;
    a.exp_tau = t_exp_tau; a.att_S_ul = t_att; a.Jred_lu = t_jred; a.Jblue_lu = t_jblue; a.frequencies = d_freq;
    a.z = d_z; a.sid = d_sid; a.n_int = d_nint; a.intensities_nu_p = d_I;
    HIP_TRY(ctx, ctx->counters.ensure(TARDIS_MC_N_COUNTERS * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->counters.p, 0, TARDIS_MC_N_COUNTERS * sizeof(unsigned long long), ctx->stream));
    a.line_steps = ctx->counters.as<unsigned long long>();  // counters[0] (line visits) = resonances crossed by the rays
    hipLaunchKernelGGL(mc::fi_rays_kernel, dim3((unsigned)((n_nu + 63) / 64), (unsigned)N), dim3(64), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(mc::fi_trapezoid_kernel, dim3((unsigned)((n_nu + 63) / 64)), dim3(64), 0, ctx->stream, d_I, (int)n_nu, (int)N,
                       a.radius_max, d_lum);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->timed = true;
    ctx->chunks_timed = 0;
    HIP_TRY(ctx, hipMemcpyAsync(luminosity_densities, d_lum, n_nu * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (intensities_nu_p) HIP_TRY(ctx, hipMemcpyAsync(intensities_nu_p, d_I, n_nu * N * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TARDIS_MC_OK;
}

// the context's own geometry and electron densities (tables: the caller's)
static FormalIntegralInput resident_formal_input(TardisMcContext *ctx)
{
    FormalIntegralInput in;
    in.n_shells = (size_t)ctx->n_shells;
    in.r_inner = ctx->r_inner.as<double>(); in.r_outer = ctx->r_outer.as<double>(); in.n_e = ctx->ot.n_e.as<double>();
    return in;
}

int tardis_mc_formal_integral(TardisMcContext *ctx, double inner_temperature, const double *frequencies, int64_t n_frequencies,
                              const double *att_S_ul, const double *Jred_lu, const double *Jblue_lu, int64_t n_impact_parameters,
                              double *luminosity_densities, double *intensities_nu_p)
{
    int rc = formal_integral_check(ctx, false, frequencies, att_S_ul && Jred_lu && Jblue_lu, luminosity_densities, n_frequencies, n_impact_parameters);
    if (rc) return rc;
    FormalIntegralInput in = resident_formal_input(ctx);
    in.host_att = att_S_ul; in.host_jred = Jred_lu; in.host_jblue = Jblue_lu;
    return formal_integral_impl(ctx, in, inner_temperature, frequencies, n_frequencies, n_impact_parameters, luminosity_densities, intensities_nu_p);
}

int tardis_mc_formal_integral_resident(TardisMcContext *ctx, double inner_temperature, const double *frequencies, int64_t n_frequencies,
                                       int64_t n_impact_parameters, double *luminosity_densities, double *intensities_nu_p)
{
    int rc = formal_integral_check(ctx, true, frequencies, true, luminosity_densities, n_frequencies, n_impact_parameters);
    if (rc) return rc;
    // (the source function has computed exp(-tau): set_opacity, which drops the table, drops sf.valid too)
    FormalIntegralInput in = resident_formal_input(ctx);
    in.exp_tau = ctx->sf.exp_tau.as<double>(); in.att = ctx->sf.att.as<double>(); in.jred = ctx->sf.jred.as<double>(); in.jblue = ctx->sf.jblue.as<double>();
    return formal_integral_impl(ctx, in, inner_temperature, frequencies, n_frequencies, n_impact_parameters, luminosity_densities, intensities_nu_p);
}

/* ---- interpolate_shells: the resident source function on the integrator's grid (formal_interpolate.hpp) ------------------- */
// The scratch of one call: the grid and the maps on the host (they back the uploads until the call has synchronised) and on the device, the four
// interpolated tables and, where asked for, the interpolated level rates.
struct InterpolatedSource {
    size_t n_shells = 0, table_stride = 0;  // (a table starts on a 16-byte boundary: the stride is even)
    mc::FiInterpolationGrid grid;
    std::vector<double> n_e;
    ScopedDevBuf shells, tables, levels;
    const double *d_dx = nullptr, *d_dxn = nullptr, *d_r_inner = nullptr, *d_r_outer = nullptr, *d_n_e = nullptr;
    const int *d_lo = nullptr, *d_hi = nullptr, *d_near = nullptr;
    double *table(int k) const { return tables.as<double>() + (size_t)k * table_stride; }  // 0 att, 1 jred, 2 jblue, 3 exp_tau
};

static int interpolate_check(TardisMcContext *ctx, int64_t interpolate_shells)
{
    if (interpolate_shells < 2 || interpolate_shells > 65536)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "interpolate_shells must be a number of grid points from 2 to 65536");
    if (ctx->n_shells < 2)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "interpolate_shells needs a model of two shells or more (linear interpolation has two nodes)");
    return TARDIS_MC_OK;
}

// Builds the interpolated tables of `interpolate_shells` grid points from the resident source function: records ev_start and launches the kernel(s) on
// the context's stream, does not wait for them.  `out` frees its scratch when it leaves the caller's scope, whatever is returned.
static int interpolate_source(TardisMcContext *ctx, int64_t interpolate_shells, bool want_levels, InterpolatedSource &out)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t S = (size_t)ctx->n_shells, L = (size_t)ctx->n_lines, Si = (size_t)interpolate_shells - 1, K = (size_t)ctx->n_levels;
    std::vector<double> r_in(S), r_out(S), n_e(S);
    HIP_TRY(ctx, hipMemcpyAsync(r_in.data(), ctx->r_inner.p, S * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(r_out.data(), ctx->r_outer.p, S * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(n_e.data(), ctx->ot.n_e.p, S * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    out.n_shells = Si;
    out.grid = mc::fi_interpolation_grid(r_in, r_out, (int)interpolate_shells);
    out.n_e.resize(Si);
    for (size_t j = 0; j < Si; ++j) out.n_e[j] = n_e[(size_t)out.grid.near[j]];
    out.table_stride = (Si * L + 1) & ~(size_t)1;
    HIP_TRY(ctx, out.shells.ensure(5 * Si * sizeof(double) + 3 * Si * sizeof(int)));
    HIP_TRY(ctx, out.tables.ensure(4 * out.table_stride * sizeof(double)));
    double *d = out.shells.as<double>();
    int *di = reinterpret_cast<int *>(d + 5 * Si);
    out.d_dx = d; out.d_dxn = d + Si; out.d_r_inner = d + 2 * Si; out.d_r_outer = d + 3 * Si; out.d_n_e = d + 4 * Si;
    out.d_lo = di; out.d_hi = di + Si; out.d_near = di + 2 * Si;
    const mc::FiInterpolationGrid &g = out.grid;
    const double *host_d[5] = {g.dx.data(), g.dxn.data(), g.r_inner.data(), g.r_outer.data(), out.n_e.data()};
    const int *host_i[3] = {g.lo.data(), g.hi.data(), g.near.data()};
    for (int k = 0; k < 5; ++k) HIP_TRY(ctx, hipMemcpyAsync(d + (size_t)k * Si, host_d[k], Si * 8, hipMemcpyHostToDevice, ctx->stream));
    for (int k = 0; k < 3; ++k) HIP_TRY(ctx, hipMemcpyAsync(di + (size_t)k * Si, host_i[k], Si * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    mc::FiInterpolateArgs a{};
    a.L = (long long)L;
    a.lo = out.d_lo; a.hi = out.d_hi; a.near = out.d_near; a.dx = out.d_dx; a.dxn = out.d_dxn;
    a.att = ctx->sf.att.as<double>(); a.jred = ctx->sf.jred.as<double>(); a.jblue = ctx->sf.jblue.as<double>(); a.exp_tau = ctx->sf.exp_tau.as<double>();
    a.att_i = out.table(0); a.jred_i = out.table(1); a.jblue_i = out.table(2); a.exp_tau_i = out.table(3);
    // about 2048 blocks in all, each striding over the pairs of lines of one output row
    const size_t row_blocks = std::max<size_t>(1, std::min<size_t>((L / 2 + 256) / 256, (2048 + Si - 1) / Si));
    hipLaunchKernelGGL(mc::fi_interpolate_kernel, dim3((unsigned)row_blocks, (unsigned)Si), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    if (want_levels && K > 0) {
        HIP_TRY(ctx, out.levels.ensure(Si * K * sizeof(double)));
        hipLaunchKernelGGL(mc::fi_interpolate_levels_kernel, dim3((unsigned)std::min<size_t>((K + 255) / 256, 64), (unsigned)Si), dim3(256), 0, ctx->stream,
                           out.d_lo, out.d_hi, out.d_dx, out.d_dxn, (long long)K, ctx->sf.c_level, out.levels.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    return TARDIS_MC_OK;
}

int tardis_mc_formal_integral_interpolated(TardisMcContext *ctx, int64_t interpolate_shells, double inner_temperature, const double *frequencies,
                                           int64_t n_frequencies, int64_t n_impact_parameters, double *luminosity_densities, double *intensities_nu_p)
{
    int rc = formal_integral_check(ctx, true, frequencies, true, luminosity_densities, n_frequencies, n_impact_parameters);
    if (rc || (rc = interpolate_check(ctx, interpolate_shells))) return rc;
    if (n_frequencies == 0) return TARDIS_MC_OK;
    InterpolatedSource src;
    rc = interpolate_source(ctx, interpolate_shells, false, src);
    if (!rc) {
        FormalIntegralInput in;
        in.n_shells = src.n_shells;
        in.r_inner = src.d_r_inner; in.r_outer = src.d_r_outer; in.n_e = src.d_n_e;
        in.att = src.table(0); in.jred = src.table(1); in.jblue = src.table(2); in.exp_tau = src.table(3);
        in.timer_started = true;
        rc = formal_integral_impl(ctx, in, inner_temperature, frequencies, n_frequencies, n_impact_parameters, luminosity_densities, intensities_nu_p);
    }
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (nothing of the call is in flight when its scratch goes)
    return rc;
}

static int download_interpolated_source(TardisMcContext *ctx, const InterpolatedSource &src, double *r_inner_i, double *r_outer_i,
                                        double *electron_density_i, double *tau_sobolev_i, double *att_S_ul_i, double *Jred_lu_i, double *Jblue_lu_i,
                                        double *e_dot_u_i)
{
    const size_t Si = src.n_shells, L = (size_t)ctx->n_lines, K = (size_t)ctx->n_levels;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->timed = true;
    ctx->chunks_timed = 0;
    if (r_inner_i) memcpy(r_inner_i, src.grid.r_inner.data(), Si * 8);
    if (r_outer_i) memcpy(r_outer_i, src.grid.r_outer.data(), Si * 8);
    if (electron_density_i) memcpy(electron_density_i, src.n_e.data(), Si * 8);
    double *const host[3] = {att_S_ul_i, Jred_lu_i, Jblue_lu_i};
    for (int k = 0; k < 3; ++k)
        if (host[k]) HIP_TRY(ctx, hipMemcpyAsync(host[k], src.table(k), Si * L * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (tau_sobolev_i)  // the rows of the resident optical depths, gathered by the copies themselves
        for (size_t j = 0; j < Si; ++j)
            HIP_TRY(ctx, hipMemcpyAsync(tau_sobolev_i + j * L, ctx->ot.tau_t.as<double>() + (size_t)src.grid.near[j] * L, L * 8, hipMemcpyDeviceToHost,
                                        ctx->stream));
    if (e_dot_u_i && K > 0) {  // [S'][levels] -> level-major, as tardis_mc_source_function returns e_dot_u
        HIP_TRY(ctx, ctx->staging.ensure(Si * K * sizeof(double)));
        HIP_TRY(ctx, launch_transpose(ctx->stream, src.levels.as<double>(), ctx->staging.as<double>(), (long long)Si, (long long)K));
        HIP_TRY(ctx, hipMemcpyAsync(e_dot_u_i, ctx->staging.p, Si * K * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TARDIS_MC_OK;
}

int tardis_mc_interpolated_source(TardisMcContext *ctx, int64_t interpolate_shells, double *r_inner_i, double *r_outer_i, double *electron_density_i,
                                  double *tau_sobolev_i, double *att_S_ul_i, double *Jred_lu_i, double *Jblue_lu_i, double *e_dot_u_i)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->have_geometry || !ctx->have_opacity || !ctx->sf.valid)
        return fail(ctx, TARDIS_MC_ERR_STATE, "no resident source function: tardis_mc_source_function must follow the last propagate / all-reduce");
    int rc = interpolate_check(ctx, interpolate_shells);
    if (rc) return rc;
    InterpolatedSource src;
    rc = interpolate_source(ctx, interpolate_shells, e_dot_u_i != nullptr, src);
    if (!rc) rc = download_interpolated_source(ctx, src, r_inner_i, r_outer_i, electron_density_i, tau_sobolev_i, att_S_ul_i, Jred_lu_i, Jblue_lu_i, e_dot_u_i);
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

/* ---- the source function of the formal integral from the resident estimators (source_function.hpp) ---------------- */
// The two CSR indices and the emission row of every line, by counting sort over the index tables (once per set_opacity).
static int build_source_topology(TardisMcContext *ctx)
{
    if (ctx->sf.topo_valid) return TARDIS_MC_OK;
    const size_t L = (size_t)ctx->n_lines, T = (size_t)ctx->n_trans, K = (size_t)ctx->n_levels;
    std::vector<int> l2l(L), edge(K + 1), ttype(T), dest(T), tline(T);
    HIP_TRY(ctx, hipMemcpyAsync(l2l.data(), ctx->ot.line2level.p, L * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(edge.data(), ctx->ot.block_edge.p, (K + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ttype.data(), ctx->ot.ttype.p, T * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dest.data(), ctx->ot.dest.p, T * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(tline.data(), ctx->ot.tline.p, T * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // lines by upper level (the tables were range-checked by set_opacity)
    std::vector<int> lvl_ptr(K + 1, 0), lvl_line(L);
    for (size_t l = 0; l < L; ++l) lvl_ptr[(size_t)l2l[l] + 1]++;
    for (size_t k = 0; k < K; ++k) lvl_ptr[k + 1] += lvl_ptr[k];
    {
        std::vector<int> at(lvl_ptr.begin(), lvl_ptr.end() - 1);
        for (size_t l = 0; l < L; ++l) lvl_line[(size_t)at[(size_t)l2l[l]]++] = (int)l;
    }
    // internal rows by destination level, each with the level (block) it leaves; emission rows by line
    std::vector<int> in_ptr(K + 1, 0), emit_row(L, 0), emit_level(L, 0), emit_n(L, 0);
    for (size_t k = 0; k < K; ++k)
        for (int t = edge[k]; t < edge[k + 1]; ++t) {
            if (ttype[(size_t)t] >= 0) in_ptr[(size_t)dest[(size_t)t] + 1]++;
            else if (ttype[(size_t)t] == -1) {
                const size_t l = (size_t)tline[(size_t)t];
                if (emit_n[l]++ == 0) { emit_row[l] = t; emit_level[l] = (int)k; }
            }
        }
    for (size_t k = 0; k < K; ++k) in_ptr[k + 1] += in_ptr[k];
    const size_t nnz = (size_t)in_ptr[K];
    std::vector<int> in_row(std::max<size_t>(nnz, 1)), in_src(std::max<size_t>(nnz, 1));
    {
        std::vector<int> at(in_ptr.begin(), in_ptr.end() - 1);
        for (size_t k = 0; k < K; ++k)
            for (int t = edge[k]; t < edge[k + 1]; ++t)
                if (ttype[(size_t)t] >= 0) {
                    const int j = at[(size_t)dest[(size_t)t]]++;
                    in_row[(size_t)j] = t; in_src[(size_t)j] = (int)k;
                }
    }
    ctx->sf.topo_error.clear();
    for (size_t l = 0; l < L; ++l)
        if (emit_n[l] != 1) {
            char buf[128];
            snprintf(buf, sizeof buf, "line %zu has %d emission rows (transition_type -1) in the macro-atom blocks, expected one", l, emit_n[l]);
            ctx->sf.topo_error = buf;
            break;
        }
    int rc;
    if ((rc = upload(ctx, ctx->sf.lvl_ptr, lvl_ptr.data(), K + 1))) return rc;
    if ((rc = upload(ctx, ctx->sf.lvl_line, lvl_line.data(), L))) return rc;
    if ((rc = upload(ctx, ctx->sf.in_ptr, in_ptr.data(), K + 1))) return rc;
    if ((rc = upload(ctx, ctx->sf.in_row, in_row.data(), in_row.size()))) return rc;
    if ((rc = upload(ctx, ctx->sf.in_src, in_src.data(), in_src.size()))) return rc;
    if ((rc = upload(ctx, ctx->sf.emit_row, emit_row.data(), L))) return rc;
    if ((rc = upload(ctx, ctx->sf.emit_level, emit_level.data(), L))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the staging vectors go out of scope)
    ctx->sf.nnz = (long long)nnz;
    ctx->sf.topo_valid = true;
    return TARDIS_MC_OK;
}

int tardis_mc_source_function(TardisMcContext *ctx, double time_of_simulation, const double *volume, const double *wavelength_cm,
                              double *att_S_ul, double *Jred_lu, double *Jblue_lu, double *e_dot_u)
{
    if (!ctx || !volume) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    drop_products(ctx, ESTIMATORS_CHANGED);
    if (!ctx->es.est_valid || !ctx->have_opacity || !ctx->have_geometry || !ctx->have_config)
        return fail(ctx, TARDIS_MC_ERR_STATE, "source function needs propagated estimators");
    if (!(time_of_simulation > 0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "time_of_simulation must be positive");
    const int mode = ctx->cfg.line_interaction_type;
    if (mode == TARDIS_MC_LINE_SCATTER || ctx->n_levels <= 0 || ctx->n_trans <= 1)
        return fail(ctx, TARDIS_MC_ERR_UNSUPPORTED, "the source function needs macro-atom tables (line_interaction_type downbranch or macroatom)");
    if (mode != TARDIS_MC_LINE_DOWNBRANCH && mode != TARDIS_MC_LINE_MACROATOM)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "unknown line_interaction_type %d", mode);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = build_source_topology(ctx);
    if (rc) return rc;
    if (!ctx->sf.topo_error.empty()) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", ctx->sf.topo_error.c_str());
    if ((rc = reduce_estimator_copies(ctx))) return rc;
    const size_t S = ctx->es.est_S, L = ctx->es.est_L, K = (size_t)ctx->n_levels, T = (size_t)ctx->n_trans;
    const long long nnz = ctx->sf.nnz;
    const bool solve = mode == TARDIS_MC_LINE_MACROATOM && nnz > 0;
    EstLayout lay = est_layout(S, L, ctx->es.est_G, ctx->es.est_copies);
    const double *est = ctx->es.est.as<double>();
    HIP_TRY(ctx, ctx->sf.shell.ensure(3 * S * sizeof(double)));
    HIP_TRY(ctx, ctx->sf.e.ensure(S * K * sizeof(double)));
    HIP_TRY(ctx, ctx->sf.att.ensure(S * L * sizeof(double)));
    HIP_TRY(ctx, ctx->sf.jred.ensure(S * L * sizeof(double)));
    HIP_TRY(ctx, ctx->sf.jblue.ensure(S * L * sizeof(double)));
    if (solve) {
        HIP_TRY(ctx, ctx->sf.x[0].ensure(S * K * sizeof(double)));
        HIP_TRY(ctx, ctx->sf.x[1].ensure(S * K * sizeof(double)));
        HIP_TRY(ctx, ctx->sf.q.ensure(S * (size_t)nnz * sizeof(double)));
        HIP_TRY(ctx, ctx->sf.conv.ensure(2 * S * sizeof(double)));
        if (!ctx->sf.conv_host) HIP_TRY(ctx, hipHostMalloc((void **)&ctx->sf.conv_host, 2 * 4096 * sizeof(double), hipHostMallocDefault));
        if (S > 4096) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "source function: more than 4096 shells");
    }
    if (wavelength_cm && (rc = upload(ctx, ctx->sf.wave, wavelength_cm, L))) return rc;
    double *d_vol = ctx->sf.shell.as<double>(), *d_ne = d_vol + S, *d_nj = d_ne + S;
    HIP_TRY(ctx, hipMemcpyAsync(d_vol, volume, S * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    const double pi = 3.141592653589793;
    hipLaunchKernelGGL(mc::sf_shell_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, ctx->stream, d_vol, (int)S, time_of_simulation,
                       mc::C_LIGHT * ctx->t_exp, 4 * pi * time_of_simulation, d_ne, d_nj);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = ensure_exp_tau(ctx))) return rc;
    // lanes per CSR row of the two indices (a function of the tables alone: the summation order does not change from call to call)
    const int g_lvl = mc::sf_group_width((long long)L, (long long)K), g_in = mc::sf_group_width(nnz, (long long)K);
    auto row_grid = [&](int g) { return dim3((unsigned)((K * (size_t)g + 255) / 256), (unsigned)S); };
    {
        auto kernel = g_lvl == 1 ? mc::sf_level_sums_kernel<1> : (g_lvl == 4 ? mc::sf_level_sums_kernel<4> : mc::sf_level_sums_kernel<16>);
        hipLaunchKernelGGL(kernel, row_grid(g_lvl), dim3(256), 0, ctx->stream, ctx->sf.lvl_ptr.as<int>(), ctx->sf.lvl_line.as<int>(), (int)K,
                           (long long)L, ctx->sf.exp_tau.as<double>(), est + lay.edot, d_ne, ctx->sf.e.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    const double *c_level = ctx->sf.e.as<double>();
    int iterations = 0;
    if (solve) {
        const unsigned gx = (unsigned)std::min<long long>((nnz + 255) / 256, 2048);
        hipLaunchKernelGGL(mc::sf_gather_q_kernel, dim3(gx, (unsigned)S), dim3(256), 0, ctx->stream, ctx->sf.in_row.as<int>(), nnz,
                           ctx->ot.prob_t.as<double>(), (long long)T, ctx->sf.q.as<double>());
        HIP_TRY(ctx, hipGetLastError());
        // x ping-pongs between sf.x[0] and sf.x[1]; the first iteration reads e itself.  Every 16 iterations (or at the cap) the per-shell
        // {max |dx|, max |x|} of the last one come to the host; the solve ends when the last iteration changed no level of any shell.
        auto iterate = g_in == 1 ? mc::sf_iterate_kernel<1> : (g_in == 4 ? mc::sf_iterate_kernel<4> : mc::sf_iterate_kernel<16>);
        const double *cur = ctx->sf.e.as<double>();
        const long long cap = ctx->sf.max_iterations;
        bool converged = false, diverged = false;
        int worst = 0;
        double worst_ratio = 0.0;
        while (!converged && !diverged && iterations < cap) {
            const int n = (int)std::min<long long>(16, cap - iterations);
            const double *prev = cur;
            for (int i = 0; i < n; ++i, ++iterations) {
                double *next = ctx->sf.x[iterations & 1].as<double>();
                hipLaunchKernelGGL(iterate, row_grid(g_in), dim3(256), 0, ctx->stream, ctx->sf.in_ptr.as<int>(), ctx->sf.in_src.as<int>(), (int)K,
                                   nnz, ctx->sf.q.as<double>(), ctx->sf.e.as<double>(), cur, next);
                prev = cur;
                cur = next;
            }
            HIP_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(mc::sf_convergence_kernel, dim3((unsigned)S), dim3(256), 0, ctx->stream, prev, cur, (int)K, ctx->sf.conv.as<double>());
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(ctx->sf.conv_host, ctx->sf.conv.p, 2 * S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            converged = true;
            worst_ratio = -1.0;
            for (size_t s = 0; s < S; ++s) {
                const double dx = ctx->sf.conv_host[2 * s], xm = ctx->sf.conv_host[2 * s + 1];
                if (!(dx == 0)) converged = false;  // (the stop rule: no level of the shell has changed, see source_function.hpp)
                const bool finite = dx == dx && xm < __builtin_huge_val();  // (NaN or infinite rates: no later iteration repairs them)
                const double ratio = (finite && xm > 0) ? dx / xm : __builtin_huge_val();
                if (dx != 0 && ratio > worst_ratio) { worst_ratio = ratio; worst = (int)s; }
                diverged |= !finite;
            }
        }
        ctx->sf.last_iterations = iterations;
        if (!converged) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
            ctx->timed = true; ctx->chunks_timed = 0;
            if (diverged)
                return fail(ctx, TARDIS_MC_ERR_STATE, "source function: the level solve produced NaN or infinite rates in shell %d after %d iterations "
                            "(estimators or transition probabilities not finite, or internal jumps that sum to more than one)", worst, iterations);
            return fail(ctx, TARDIS_MC_ERR_STATE, "source function: the level solve has not converged after %d iterations (option source_max_iterations); "
                        "worst shell %d with max|dx| / max|x| = %.3g", iterations, worst, worst_ratio);
        }
        c_level = cur;
    } else
        ctx->sf.last_iterations = 0;
    const unsigned lx = (unsigned)std::min<size_t>((L + 255) / 256, 1024);
    hipLaunchKernelGGL(mc::sf_close_kernel, dim3(lx, (unsigned)S), dim3(256), 0, ctx->stream, ctx->sf.emit_row.as<int>(), ctx->sf.emit_level.as<int>(),
                       (long long)L, (long long)T, (int)K, ctx->ot.prob_t.as<double>(), c_level, wavelength_cm ? ctx->sf.wave.as<double>() : nullptr,
                       ctx->ot.nu_line.as<double>(), ctx->sf.exp_tau.as<double>(), est + lay.jblue, d_nj, time_of_simulation, 4 * pi,
                       ctx->sf.att.as<double>(), ctx->sf.jred.as<double>(), ctx->sf.jblue.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->timed = true;
    ctx->chunks_timed = 0;
    if (att_S_ul) HIP_TRY(ctx, hipMemcpyAsync(att_S_ul, ctx->sf.att.p, S * L * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (Jred_lu) HIP_TRY(ctx, hipMemcpyAsync(Jred_lu, ctx->sf.jred.p, S * L * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (Jblue_lu) HIP_TRY(ctx, hipMemcpyAsync(Jblue_lu, ctx->sf.jblue.p, S * L * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (e_dot_u) {  // [S][levels] -> level-major, as the reference returns it
        HIP_TRY(ctx, ctx->staging.ensure(S * K * sizeof(double)));
        HIP_TRY(ctx, launch_transpose(ctx->stream, c_level, ctx->staging.as<double>(), (long long)S, (long long)K));
        HIP_TRY(ctx, hipMemcpyAsync(e_dot_u, ctx->staging.p, S * K * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->sf.c_level = c_level;
    ctx->sf.valid = true;
    return TARDIS_MC_OK;
}

int tardis_mc_last_source_iterations(TardisMcContext *ctx) { return ctx ? ctx->sf.last_iterations : -1; }

/* ---- opacity update from level populations (opacity_update.hpp) --------------------------------------- */
int tardis_mc_opacity_update_path(int64_t rows) { return opup::choose_path((long long)rows); }

int tardis_mc_set_line_data(TardisMcContext *ctx, const TardisMcLineData *d)
{
    if (!ctx || !d) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->have_opacity) return fail(ctx, TARDIS_MC_ERR_STATE, "set_opacity must precede set_line_data");
    drop_from(ctx, RUNG_LINE_DATA);
    const size_t L = (size_t)ctx->n_lines, T = (size_t)ctx->n_trans;
    if (d->n_lines != (int64_t)L || d->n_transitions != (int64_t)T)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "line data of %lld lines / %lld transitions, the resident opacity state has %zu / %zu",
                    (long long)d->n_lines, (long long)d->n_transitions, L, T);
    if (d->n_levels <= 0 || d->n_levels > 0x7ffffff0LL || !d->f_lu || !d->wavelength_cm || !d->g_lower || !d->g_upper || !d->level_lower || !d->level_upper)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid line data");
    const bool coef = d->transition_probability_coef != nullptr;
    if (coef && !ctx->ot.h_macro)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "transition_probability_coef given, but the resident opacity state has no macro-atom tables");
    // everything the kernels index with is checked here, on the host
    std::vector<int> lo(L), up(L);
    for (size_t i = 0; i < L; ++i) {
        if (d->level_lower[i] < 0 || d->level_lower[i] >= d->n_levels) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "level_lower[%zu] out of range", i);
        if (d->level_upper[i] < 0 || d->level_upper[i] >= d->n_levels) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "level_upper[%zu] out of range", i);
        lo[i] = (int)d->level_lower[i];
        up[i] = (int)d->level_upper[i];
    }
    if (coef) {
        const std::vector<int> &ttype = ctx->ot.h_idx[2], &tline = ctx->ot.h_idx[4];
        if (ttype.size() != T || tline.size() != T) return fail(ctx, TARDIS_MC_ERR_STATE, "the resident index tables do not match the transition count");
        for (size_t t = 0; t < T; ++t)
            if (tline[t] < 0 || tline[t] >= (int)L) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "transition_line_id[%zu] out of range", t);
        for (size_t t = 0; t < T; ++t)
            if (ttype[t] < -1 || ttype[t] > 1)
                return fail(ctx, TARDIS_MC_ERR_UNSUPPORTED, "transition_type[%zu] = %d: the opacity update knows -1, 0 and 1", t, ttype[t]);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = upload(ctx, ctx->ou.f_lu, d->f_lu, L))) return rc;
    if ((rc = upload(ctx, ctx->ou.wave, d->wavelength_cm, L))) return rc;
    if ((rc = upload(ctx, ctx->ou.g_lower, d->g_lower, L))) return rc;
    if ((rc = upload(ctx, ctx->ou.g_upper, d->g_upper, L))) return rc;
    if ((rc = upload(ctx, ctx->ou.level_lower, lo.data(), L))) return rc;
    if ((rc = upload(ctx, ctx->ou.level_upper, up.data(), L))) return rc;
    if (coef && (rc = upload(ctx, ctx->ou.coef, d->transition_probability_coef, T))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (lo / up are the sources of asynchronous copies)
    ctx->ou.h_lower.swap(lo);
    ctx->ou.h_upper.swap(up);
    ctx->ou.levels = d->n_levels;
    ctx->ou.have_coef = coef;
    ctx->ou.sobolev_coefficient = d->sobolev_coefficient;
    ctx->ou.long_rows_built = -2;  // (the list of the long blocks is made by the first update)
    ctx->ou.have = true;
    return TARDIS_MC_OK;
}

// What both producers of an opacity state check before they touch anything: the call order and the j_blues_mode block of the update.
static int opacity_update_check(TardisMcContext *ctx, const TardisMcOpacityUpdate *u)
{
    if (!ctx->have_opacity || !ctx->ou.have) return fail(ctx, TARDIS_MC_ERR_STATE, "set_opacity and set_line_data must precede update_opacity");
    if (!ctx->have_geometry) return fail(ctx, TARDIS_MC_ERR_STATE, "update_opacity needs the geometry (time_explosion)");
    const int mode = u->j_blues_mode;
    if (mode != 0 && mode != 1) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "unknown j_blues_mode %d", mode);
    if (mode == 0 && (!u->t_radiative || !u->dilution_factor))
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "j_blues_mode 0 needs t_radiative and dilution_factor");
    const size_t S = (size_t)ctx->n_shells, L = (size_t)ctx->n_lines;
    if (mode == 1) {
        if (!ctx->es.est_valid || !ctx->es.est_propagated || ctx->es.est_S != S || ctx->es.est_L != L)
            return fail(ctx, TARDIS_MC_ERR_STATE, "j_blues_mode 1 needs propagated estimators");
        if (!u->volume || !(u->time_of_simulation > 0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "j_blues_mode 1 needs volume and a positive time_of_simulation");
    }
    return TARDIS_MC_OK;
}

// Which segments of an edge table take the 16-lane row form of their kernel -- macro-atom blocks here, ions in the partition function, one rule with the
// `threshold` as choose_path takes it -- uploaded into `list`, their number into `count`.
static_assert(plup::PATH_ROW == opup::PATH_ROW && plup::LONG_ION_LEVELS == opup::LONG_BLOCK_ROWS, "the partition kernel's rule is the block kernel's");
static int upload_row_form_list(TardisMcContext *ctx, const std::vector<int> &edge, long long threshold, DevBuf &list, long long *count)
{
    std::vector<int> rows;
    for (size_t b = 0; b + 1 < edge.size(); ++b)
        if (opup::choose_path((long long)edge[b + 1] - edge[b], threshold) == opup::PATH_ROW) rows.push_back((int)b);
    int rc;
    if ((rc = upload(ctx, list, rows.data(), rows.size()))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *count = (long long)rows.size();
    return TARDIS_MC_OK;
}

// The list of the blocks that take the row form, and the buffers of an update: n_t[S][K], the [S] inputs, beta_t / sef_t / j_t [S][L].
static int opacity_update_buffers(TardisMcContext *ctx)
{
    const size_t S = (size_t)ctx->n_shells, L = (size_t)ctx->n_lines, K = (size_t)ctx->ou.levels;
    int rc;
    const bool blocks = ctx->ou.have_coef && ctx->ot.h_macro && ctx->n_levels > 0;
    if (blocks && ctx->ou.long_rows_built != ctx->ou.long_rows) {
        if ((rc = upload_row_form_list(ctx, ctx->ot.h_idx[1], ctx->ou.long_rows, ctx->ou.long_blocks, &ctx->ou.n_long))) return rc;
        ctx->ou.long_rows_built = ctx->ou.long_rows;
    }
    HIP_TRY(ctx, ctx->ou.n_t.ensure(K * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ou.shell.ensure(4 * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ou.beta_t.ensure(L * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ou.sef_t.ensure(L * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ou.j_t.ensure(L * S * sizeof(double)));
    return TARDIS_MC_OK;
}

static int opacity_update_stages(TardisMcContext *ctx, const TardisMcOpacityUpdate *u);

int tardis_mc_update_opacity(TardisMcContext *ctx, const TardisMcOpacityUpdate *u)
{
    if (!ctx || !u || !u->level_number_density) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid opacity update");
    int rc;
    if ((rc = opacity_update_check(ctx, u))) return rc;
    const int mode = u->j_blues_mode;
    const size_t S = (size_t)ctx->n_shells, K = (size_t)ctx->ou.levels;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drop_products(ctx, OPACITY_UPDATE_BEGINS);
    ctx->ou.valid = false;
    ctx->pl.valid = false;  // (the populations are the caller's from here on)
    if ((rc = opacity_update_buffers(ctx))) return rc;
    HIP_TRY(ctx, ctx->staging.ensure(K * S * sizeof(double)));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // populations [K,S] -> [S][K]
    HIP_TRY(ctx, host_copy(ctx, {{(void *)u->level_number_density, ctx->staging.p, K * S * sizeof(double)}}, true));
    if (u->electron_density && (rc = upload(ctx, ctx->ot.n_e, u->electron_density, S))) return rc;
    double *d_t = ctx->ou.shell.as<double>() + S, *d_w = d_t + S;  // (the layout of radiation_field_enqueue's work: volume, t_rad, W, norm)
    if (mode == 0) {
        HIP_TRY(ctx, hipMemcpyAsync(d_t, u->t_radiative, S * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_w, u->dilution_factor, S * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    ctx->ou.timed = false;
    if ((rc = ensure_events(ctx, ctx->ou.ev))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ou.ev[0], ctx->stream));
    HIP_TRY(ctx, launch_transpose(ctx->stream, ctx->staging.as<double>(), ctx->ou.n_t.as<double>(), (long long)K, (long long)S));
    return opacity_update_stages(ctx, u);
}

// Everything of an opacity update behind the populations: with n_t[S][K], the electron densities and (mode 0) t_rad / W resident and ev_start / ou.ev[0]
// recorded, the detailed j_blues of mode 1, the line kernel, the block kernels and the derived tables.  Shared by tardis_mc_update_opacity (populations
// uploaded) and tardis_mc_update_plasma (populations solved on the device).
static int opacity_update_stages(TardisMcContext *ctx, const TardisMcOpacityUpdate *u)
{
    const int mode = u->j_blues_mode;
    const size_t S = (size_t)ctx->n_shells, L = (size_t)ctx->n_lines, T = (size_t)ctx->n_trans, K = (size_t)ctx->ou.levels;
    const bool blocks = ctx->ou.have_coef && ctx->ot.h_macro && ctx->n_levels > 0;
    double *d_t = ctx->ou.shell.as<double>() + S, *d_w = d_t + S;  // (the layout of radiation_field_enqueue's work: volume, t_rad, W, norm)
    int rc;
    if (mode == 1 && (rc = radiation_field_enqueue(ctx, u->time_of_simulation, u->volume, u->w_epsilon, u->detailed_optical_window, ctx->ou.shell,
                                                   ctx->ou.j_t.as<double>())))
        return rc;
    const double h = H_PLANCK, c = mc::C_LIGHT;
    mc::OpacityUpdateConsts k;
    k.coef_sobolev = ctx->ou.sobolev_coefficient; k.t_exp = ctx->t_exp; k.planck_coef = 2 * h / (c * c); k.h = h; k.k_b = K_BOLTZMANN;
    {
        const unsigned bx = (unsigned)std::min<size_t>((L + 255) / 256, 1024);
        auto kernel = mode == 0 ? mc::opacity_line_kernel<true> : mc::opacity_line_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(bx, (unsigned)S), dim3(256), 0, ctx->stream, ctx->ou.n_t.as<double>(), ctx->ou.level_lower.as<int>(),
                           ctx->ou.level_upper.as<int>(), ctx->ou.f_lu.as<double>(), ctx->ou.wave.as<double>(), ctx->ou.g_lower.as<double>(),
                           ctx->ou.g_upper.as<double>(), ctx->ot.nu_line.as<double>(), d_t, d_w, (long long)K, (long long)L, k, ctx->ot.tau_t.as<double>(),
                           ctx->ou.beta_t.as<double>(), ctx->ou.sef_t.as<double>(), ctx->ou.j_t.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ou.ev[1], ctx->stream));
    if (blocks) {
        const long long n_blocks = ctx->n_levels, n_long = ctx->ou.n_long;
        const long long long_rows = ctx->ou.long_rows < 0 ? opup::LONG_BLOCK_ROWS : ctx->ou.long_rows;
        if (n_long < n_blocks) {
            const long long n = n_blocks * (long long)S;
            hipLaunchKernelGGL(mc::opacity_block_lane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ot.block_edge.as<int>(), (int)n_blocks,
                               (long long)T, (long long)L, (int)S, long_rows, ctx->ou.coef.as<double>(), ctx->ot.tline.as<int>(), ctx->ot.ttype.as<int>(),
                               ctx->ou.beta_t.as<double>(), ctx->ou.sef_t.as<double>(), ctx->ou.j_t.as<double>(), ctx->ot.prob_t.as<double>());
            HIP_TRY(ctx, hipGetLastError());
        }
        if (n_long > 0) {
            const long long n = n_long * (long long)S * 16;
            hipLaunchKernelGGL(mc::opacity_block_row_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ou.long_blocks.as<int>(), (int)n_long,
                               ctx->ot.block_edge.as<int>(), (long long)T, (long long)L, (int)S, ctx->ou.coef.as<double>(), ctx->ot.tline.as<int>(), ctx->ot.ttype.as<int>(),
                               ctx->ou.beta_t.as<double>(), ctx->ou.sef_t.as<double>(), ctx->ou.j_t.as<double>(), ctx->ot.prob_t.as<double>());
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ou.ev[2], ctx->stream));
    rc = derive_opacity_tables(ctx, L, S, T, [](const char *) {});
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ou.ev[3], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timed = true;
    ctx->chunks_timed = 0;
    ctx->ou.timed = true;
    ctx->ou.valid = true;
    return TARDIS_MC_OK;
}

int tardis_mc_last_opacity_update_ms(TardisMcContext *ctx, double *out_line_ms, double *out_block_ms, double *out_derive_ms)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->ou.timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no update_opacity has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *const out[3] = {out_line_ms, out_block_ms, out_derive_ms};
    return event_intervals_ms(ctx, ctx->ou.ev, 3, out);
}

int tardis_mc_get_opacity(TardisMcContext *ctx, double *tau_sobolev, double *transition_probabilities, double *beta_sobolev,
                          double *stimulated_emission_factor, double *j_blues)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->have_opacity) return fail(ctx, TARDIS_MC_ERR_STATE, "set_opacity must precede get_opacity");
    if ((beta_sobolev || stimulated_emission_factor || j_blues) && !ctx->ou.valid)
        return fail(ctx, TARDIS_MC_ERR_STATE, "beta_sobolev, stimulated_emission_factor and j_blues exist only after update_opacity");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t S = (size_t)ctx->n_shells, L = (size_t)ctx->n_lines, T = (size_t)ctx->n_trans;
    HIP_TRY(ctx, ctx->staging.ensure(std::max(L, T) * S * sizeof(double)));  // (the largest of them first: the staging grows once)
    int rc;
    if ((rc = download_transposed(ctx, tau_sobolev, ctx->ot.tau_t.as<double>(), L))) return rc;
    if ((rc = download_transposed(ctx, transition_probabilities, ctx->ot.prob_t.as<double>(), T))) return rc;
    if ((rc = download_transposed(ctx, beta_sobolev, ctx->ou.beta_t.as<double>(), L))) return rc;
    if ((rc = download_transposed(ctx, stimulated_emission_factor, ctx->ou.sef_t.as<double>(), L))) return rc;
    return download_transposed(ctx, j_blues, ctx->ou.j_t.as<double>(), L);
}

/* ---- mean opacities and optical depths from the resident optical depths (mean_opacity.hpp) ------------------ */
static_assert(mopl::ERR_INVALID_ARGUMENT == TARDIS_MC_ERR_INVALID_ARGUMENT, "mean_opacity_plan.hpp repeats the error code");

int tardis_mc_mean_opacity_path(int64_t n_bins) { return mopl::choose_path((long long)n_bins); }

int64_t tardis_mc_mean_opacity_bins(int64_t n_lines, const double *line_list_nu, int64_t bin_size, int64_t *first_degenerate_bin)
{
    mopl::Layout lay;
    std::string msg;
    long long first = -1;
    const long long n = mopl::plan_bins((long long)n_lines, line_list_nu, (long long)bin_size, lay, &first, msg);
    if (first_degenerate_bin) *first_degenerate_bin = first;
    if (n < 0) return fail(nullptr, (int)n, "%s", msg.c_str());
    return n;
}

int tardis_mc_mean_opacity(TardisMcContext *ctx, const TardisMcMeanOpacity *q)
{
    if (!ctx || !q) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid mean opacity request");
    if (!ctx->have_geometry || !ctx->have_opacity) return fail(ctx, TARDIS_MC_ERR_STATE, "set_geometry and set_opacity must precede mean_opacity");
    const size_t S = (size_t)ctx->n_shells, L = (size_t)ctx->n_lines;
    if (ctx->ot.h_nu.size() != L) return fail(ctx, TARDIS_MC_ERR_STATE, "the resident line list does not match the line count");
    // everything is refused here, on the host, before anything is allocated or launched
    mopl::Layout lay;
    std::string msg;
    const long long n_bins = mopl::plan_bins((long long)L, ctx->ot.h_nu.data(), (long long)q->bin_size, lay, nullptr, msg);
    if (n_bins < 0) return fail(ctx, (int)n_bins, "%s", msg.c_str());
    if (!q->t_radiative) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "mean opacity: t_radiative is missing");
    for (size_t s = 0; s < S; ++s)
        if (!(std::isfinite(q->t_radiative[s]) && q->t_radiative[s] > 0.0))
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "mean opacity: t_radiative[%zu] = %g is not finite and positive", s, q->t_radiative[s]);
    if (S > 65535) return fail(ctx, TARDIS_MC_ERR_UNSUPPORTED, "mean opacity: %zu shells, the bin kernel's grid takes 65535", S);
    const size_t B = (size_t)n_bins;
    std::vector<double> low(B), dnu(B);
    for (size_t b = 0; b < B; ++b) {
        low[b] = mopl::bin_low(lay, ctx->ot.h_nu.data(), (long long)b);
        dnu[b] = mopl::bin_high(lay, ctx->ot.h_nu.data(), (long long)b) - low[b];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ScopedDevBuf d_low, d_dnu, d_t, kexp_t, sums, out, kexp_lines;
    const int rc = [&]() -> int {
        int rc1;
        if ((rc1 = upload(ctx, d_low, low.data(), B))) return rc1;
        if ((rc1 = upload(ctx, d_dnu, dnu.data(), B))) return rc1;
        if ((rc1 = upload(ctx, d_t, q->t_radiative, S))) return rc1;
        HIP_TRY(ctx, kexp_t.ensure(S * B * sizeof(double)));
        HIP_TRY(ctx, sums.ensure(4 * S * sizeof(double)));
        HIP_TRY(ctx, out.ensure(4 * S * sizeof(double)));
        if (q->kappa_expansion) HIP_TRY(ctx, kexp_lines.ensure(S * B * sizeof(double)));
        int rc2;
        ctx->mo.timed = false;
        if ((rc2 = ensure_events(ctx, ctx->mo.ev))) return rc2;
        const double h = H_PLANCK, c = mc::C_LIGHT;
        mc::MeanOpacityConsts k;
        k.ct = ctx->t_exp * c; k.planck_coef = 2 * h / (c * c); k.h = h; k.k_b = K_BOLTZMANN; k.c = c;
        k.sigma_thomson = ctx->have_config ? ctx->cfg.sigma_thomson : 6.652458734e-25;  // (without a configuration: SIGMA_THOMSON, as the formal integral has it)
        HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->mo.ev[0], ctx->stream));
        hipLaunchKernelGGL(mc::mean_opacity_bin_kernel, dim3((unsigned)((B + 255) / 256), (unsigned)S), dim3(256), 0, ctx->stream, ctx->ot.tau_t.as<double>(),
                           (long long)L, lay.m, lay.e, n_bins, d_low.as<double>(), d_dnu.as<double>(), k.ct, kexp_t.as<double>());
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ctx->mo.ev[1], ctx->stream));
        if (mopl::choose_path(n_bins, ctx->mo.long_bins) == mopl::PATH_ROW)
            hipLaunchKernelGGL(mc::mean_opacity_reduce_row_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, ctx->stream, kexp_t.as<double>(), n_bins, (int)S,
                               d_low.as<double>(), d_dnu.as<double>(), d_t.as<double>(), ctx->ot.n_e.as<double>(), k, sums.as<double>());
        else
            hipLaunchKernelGGL(mc::mean_opacity_reduce_lane_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, ctx->stream, kexp_t.as<double>(), n_bins, (int)S,
                               d_low.as<double>(), d_dnu.as<double>(), d_t.as<double>(), ctx->ot.n_e.as<double>(), k, sums.as<double>());
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(mc::mean_opacity_final_kernel, dim3(1), dim3(64), 0, ctx->stream, sums.as<double>(), (int)S, ctx->ot.n_e.as<double>(),
                           ctx->r_inner.as<double>(), ctx->r_outer.as<double>(), k.sigma_thomson, out.as<double>());
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ctx->mo.ev[2], ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
        ctx->timed = true;
        ctx->chunks_timed = 0;
        double *const host[4] = {q->kappa_planck, q->kappa_rosseland, q->tau_planck, q->tau_rosseland};
        for (int v = 0; v < 4; ++v)
            if (host[v]) HIP_TRY(ctx, hipMemcpyAsync(host[v], out.as<double>() + (size_t)v * S, S * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (q->kappa_expansion) {  // [S][n_bins] -> [n_bins, S]
            HIP_TRY(ctx, launch_transpose(ctx->stream, kexp_t.as<double>(), kexp_lines.as<double>(), (long long)S, n_bins));
            HIP_TRY(ctx, hipMemcpyAsync(q->kappa_expansion, kexp_lines.p, S * B * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->mo.timed = true;
        return TARDIS_MC_OK;
    }();
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (nothing of the call is in flight when its scratch goes)
    if (rc) return rc;
    if (q->bins_low) memcpy(q->bins_low, low.data(), B * 8);
    if (q->delta_nu) memcpy(q->delta_nu, dnu.data(), B * 8);
    return TARDIS_MC_OK;
}

int tardis_mc_last_mean_opacity_ms(TardisMcContext *ctx, double *out_bin_ms, double *out_reduce_ms)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->mo.timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no mean_opacity has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *const out[2] = {out_bin_ms, out_reduce_ms};
    return event_intervals_ms(ctx, ctx->mo.ev, 2, out);
}


/* ---- plasma update: ion and level populations from (t_rad, W) (plasma_update.hpp) ----------------------- */
int tardis_mc_plasma_update_path(int64_t levels) { return plup::choose_path((long long)levels); }

int tardis_mc_set_plasma_data(TardisMcContext *ctx, const TardisMcPlasmaData *d)
{
    if (!ctx || !d) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->have_opacity || !ctx->ou.have) return fail(ctx, TARDIS_MC_ERR_STATE, "set_opacity and set_line_data must precede set_plasma_data");
    drop_from(ctx, RUNG_PLASMA_DATA);
    if (d->n_levels != ctx->ou.levels)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "plasma data of %lld levels, the line data have %lld", (long long)d->n_levels, ctx->ou.levels);
    if (d->n_shells != ctx->n_shells)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "plasma data of %lld shells, the resident opacity state has %d", (long long)d->n_shells, ctx->n_shells);
    if (d->n_ions <= 0 || d->n_elements <= 0 || d->n_ions > d->n_levels || d->n_elements > d->n_ions || d->n_zeta_temperatures < 2 ||
        d->n_zeta_temperatures > 0x7ffffff0LL || !d->level_energy || !d->level_g || !d->level_metastable || !d->ion_level_edge || !d->element_ion_edge ||
        !d->ion_charge || !d->ionization_energy || !d->zeta_temperatures || !d->zeta || !d->number_density)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid plasma data");
    if (!(d->link_t_rad_t_electron > 0) || !(d->chi_0 == d->chi_0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid link_t_rad_t_electron / chi_0");
    const size_t K = (size_t)d->n_levels, I = (size_t)d->n_ions, E = (size_t)d->n_elements, NT = (size_t)d->n_zeta_temperatures, S = (size_t)d->n_shells;
    // everything the kernels index with is checked here, on the host
    if (d->ion_level_edge[0] != 0 || d->ion_level_edge[I] != (int64_t)K) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "ion_level_edge must run from 0 to n_levels");
    for (size_t i = 0; i < I; ++i)
        if (d->ion_level_edge[i + 1] <= d->ion_level_edge[i]) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "ion %zu has no level (ion_level_edge not increasing)", i);
    if (d->element_ion_edge[0] != 0 || d->element_ion_edge[E] != (int64_t)I)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "element_ion_edge must run from 0 to n_ions");
    for (size_t e = 0; e < E; ++e)
        if (d->element_ion_edge[e + 1] <= d->element_ion_edge[e]) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "element %zu has no ion (element_ion_edge not increasing)", e);
    for (size_t k = 0; k < K; ++k)
        if (!(d->level_g[k] > 0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "level_g[%zu] is not positive", k);
    for (size_t i = 0; i < I; ++i)
        if (!(d->level_energy[d->ion_level_edge[i]] >= 0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "the first level of ion %zu has a negative energy", i);
    for (size_t t = 0; t + 1 < NT; ++t)
        if (!(d->zeta_temperatures[t] < d->zeta_temperatures[t + 1])) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "zeta_temperatures must ascend");
    std::vector<int> ion_edge(I + 1), elem_edge(E + 1), meta(K), level_ion(K);
    for (size_t i = 0; i <= I; ++i) ion_edge[i] = (int)d->ion_level_edge[i];
    for (size_t e = 0; e <= E; ++e) elem_edge[e] = (int)d->element_ion_edge[e];
    for (size_t i = 0; i < I; ++i)
        for (int k = ion_edge[i]; k < ion_edge[i + 1]; ++k) level_ion[k] = (int)i;
    for (size_t k = 0; k < K; ++k) meta[k] = d->level_metastable[k] != 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = upload(ctx, ctx->pl.energy, d->level_energy, K))) return rc;
    if ((rc = upload(ctx, ctx->pl.g, d->level_g, K))) return rc;
    if ((rc = upload(ctx, ctx->pl.meta, meta.data(), K))) return rc;
    if ((rc = upload(ctx, ctx->pl.level_ion, level_ion.data(), K))) return rc;
    if ((rc = upload(ctx, ctx->pl.ion_edge, ion_edge.data(), I + 1))) return rc;
    if ((rc = upload(ctx, ctx->pl.elem_edge, elem_edge.data(), E + 1))) return rc;
    if ((rc = upload(ctx, ctx->pl.charge, d->ion_charge, I))) return rc;
    if ((rc = upload(ctx, ctx->pl.chi, d->ionization_energy, I))) return rc;
    if ((rc = upload(ctx, ctx->pl.zeta_t, d->zeta_temperatures, NT))) return rc;
    if ((rc = upload(ctx, ctx->pl.zeta, d->zeta, I * NT))) return rc;
    if ((rc = upload(ctx, ctx->pl.density, d->number_density, E * S))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the staging vectors are the sources of asynchronous copies)
    ctx->pl.h_ion_edge.swap(ion_edge);
    ctx->pl.h_elem_edge.swap(elem_edge);
    ctx->pl.h_charge.assign(d->ion_charge, d->ion_charge + I);
    ctx->pl.ions = (int)I; ctx->pl.elements = (int)E; ctx->pl.nt = (int)NT;
    ctx->pl.t_min = d->zeta_temperatures[0]; ctx->pl.t_max = d->zeta_temperatures[NT - 1];
    ctx->pl.chi_0 = d->chi_0; ctx->pl.link = d->link_t_rad_t_electron;
    ctx->pl.long_rows_built = -2;  // (the list of the long ions is made by the first update)
    ctx->pl.have = true;
    return TARDIS_MC_OK;
}

/* ---- the options of the ionisation stage: helium_treatment recomb-nlte, delta_treatment (plasma_update.hpp) ---- */
int tardis_mc_check_ionization_options(const TardisMcIonizationOptions *o, int64_t n_elements, const int64_t *element_ion_edge, const int64_t *ion_level_edge,
                                       const double *ion_charge)
{
    if (!o) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid ionization options");
    const std::string err = plup::check_ionization_options(o->helium_treatment, o->use_delta_treatment, (long long)o->helium_element, o->delta_treatment,
                                                           (long long)n_elements, element_ion_edge, ion_level_edge, ion_charge);
    return err.empty() ? TARDIS_MC_OK : fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
}

int tardis_mc_set_ionization_options(TardisMcContext *ctx, const TardisMcIonizationOptions *o)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->pl.have) return fail(ctx, TARDIS_MC_ERR_STATE, "set_plasma_data must precede set_ionization_options");
    ctx->he.have = ctx->he.valid = false;
    if (!o) return TARDIS_MC_OK;
    // everything the kernels index with is checked here, on the host
    const std::string err = plup::check_ionization_options(o->helium_treatment, o->use_delta_treatment, (long long)o->helium_element, o->delta_treatment,
                                                           (long long)ctx->pl.elements, ctx->pl.h_elem_edge.data(), ctx->pl.h_ion_edge.data(), ctx->pl.h_charge.data());
    if (!err.empty()) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    ctx->he.helium = o->helium_treatment;
    ctx->he.fixed_delta = o->use_delta_treatment != 0;
    ctx->he.delta = ctx->he.fixed_delta ? o->delta_treatment : 0.0;
    ctx->he.element = ctx->he.ion = ctx->he.k0 = ctx->he.n1 = ctx->he.n2 = 0;
    if (ctx->he.helium) {
        const int a = ctx->pl.h_elem_edge[(size_t)o->helium_element];
        ctx->he.element = (int)o->helium_element;
        ctx->he.ion = a;
        ctx->he.k0 = ctx->pl.h_ion_edge[(size_t)a];
        ctx->he.n1 = ctx->pl.h_ion_edge[(size_t)a + 1] - ctx->he.k0;
        ctx->he.n2 = ctx->pl.h_ion_edge[(size_t)a + 2] - ctx->he.k0;
    }
    ctx->he.have = true;
    return TARDIS_MC_OK;
}

/* ---- NLTE excitation of selected species inside update_plasma (nlte_excitation.hpp) ------------------------ */
int tardis_mc_nlte_solve_path(int64_t levels) { return nlte::choose_path((long long)levels); }
int tardis_mc_nlte_solve_form(int64_t levels) { return nlte::choose_form((long long)levels); }

int tardis_mc_check_nlte_data(const TardisMcNlteData *d, int64_t n_ions, const int64_t *ion_level_edge, int64_t n_lines, const int64_t *level_lower,
                              const int64_t *level_upper)
{
    if (!d || n_ions <= 0 || !ion_level_edge || n_lines < 0 || !level_lower || !level_upper) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid NLTE data");
    if (d->n_nlte_lines > 0 && (!d->A_ul || !d->B_ul || !d->B_lu)) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid NLTE data: a pointer is missing");
    const std::string err = nlte::check_data((long long)d->n_species, d->species_ion, (long long)d->n_nlte_lines, d->species_line_edge, d->line_id, (long long)n_ions,
                                             ion_level_edge, (long long)n_lines, level_lower, level_upper);
    return err.empty() ? TARDIS_MC_OK : fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
}

// The launches of the solve kernel for the current values of options nlte_lds_levels and nlte_blocked_levels (nlte::plan_launches,
// nlte::plan_blocked), their lists uploaded.
// TARDIS_MC_ERR_UNSUPPORTED when the slabs of all shells together exceed nlte::MAX_SCRATCH_BYTES.
static int nlte_build_lists(TardisMcContext *ctx)
{
    const long long S = ctx->n_shells;
    nlte::LaunchPlan plan = nlte::plan_launches(ctx->nl.h_n, S, ctx->nl.lds_levels);
    if (plan.refused >= 0)
        return fail(ctx, TARDIS_MC_ERR_UNSUPPORTED, "NLTE species %lld (ion %d, %lld levels) needs %lld bytes of scratch over %lld shells in the global-memory form of the "
                    "solve: with the %lld bytes of the species before it that exceeds the %lld the plan allows", plan.refused, ctx->nl.h_ion[(size_t)plan.refused],
                    (long long)ctx->nl.h_n[(size_t)plan.refused], plan.refused_bytes, S, plan.refused_before_bytes, nlte::MAX_SCRATCH_BYTES);
    if (plan.max_lds_bytes > 65536)  // (a launch with more dynamic LDS than the default bound has to announce it: once per list, not per update)
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&mc::nlte_solve_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)plan.max_lds_bytes));
    int rc;
    if ((rc = upload(ctx, ctx->nl.list, plan.list.data(), plan.list.size()))) return rc;
    if ((rc = upload(ctx, ctx->nl.slab, plan.slab.data(), plan.slab.size()))) return rc;
    nlte::BlockedPlan blocked = nlte::plan_blocked(plan, ctx->nl.h_n, S, ctx->nl.blocked_levels);
    std::vector<int> form_list(blocked.single);
    std::vector<long long> form_slab(blocked.single_slab);
    form_list.insert(form_list.end(), blocked.blocked.begin(), blocked.blocked.end());
    form_slab.insert(form_slab.end(), blocked.blocked_slab.begin(), blocked.blocked_slab.end());
    if ((rc = upload(ctx, ctx->nl.form_list, form_list.data(), form_list.size()))) return rc;
    if ((rc = upload(ctx, ctx->nl.form_slab, form_slab.data(), form_slab.size()))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->nl.launches.swap(plan.launches);
    ctx->nl.steps.swap(blocked.steps);
    ctx->nl.n_single = (int)blocked.single.size(); ctx->nl.n_blocked = (int)blocked.blocked.size();
    ctx->nl.scratch_doubles = plan.scratch_doubles;
    ctx->nl.lists_built = ctx->nl.lds_levels;
    ctx->nl.blocked_built = ctx->nl.blocked_levels;
    return TARDIS_MC_OK;
}

int tardis_mc_set_nlte_data(TardisMcContext *ctx, const TardisMcNlteData *d)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->pl.have) return fail(ctx, TARDIS_MC_ERR_STATE, "set_plasma_data must precede set_nlte_data");
    drop_from(ctx, RUNG_NLTE_DATA);
    if (!d) return TARDIS_MC_OK;
    if (d->n_nlte_lines > 0 && (!d->A_ul || !d->B_ul || !d->B_lu)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid NLTE data: a pointer is missing");
    // everything the kernels index with is checked here, on the host
    std::vector<int> lower, upper;
    const std::string err = nlte::check_data((long long)d->n_species, d->species_ion, (long long)d->n_nlte_lines, d->species_line_edge, d->line_id, (long long)ctx->pl.ions,
                                             ctx->pl.h_ion_edge.data(), (long long)ctx->n_lines, ctx->ou.h_lower.data(), ctx->ou.h_upper.data(), &lower, &upper);
    if (!err.empty()) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    const size_t NS = (size_t)d->n_species, NL = (size_t)d->n_nlte_lines;
    std::vector<int> k0(NS), n(NS), x0(NS), ion(NS), edge(NS + 1), line_id(NL);
    long long nx = 0;
    for (size_t sp = 0; sp < NS; ++sp) {
        ion[sp] = (int)d->species_ion[sp];
        k0[sp] = ctx->pl.h_ion_edge[(size_t)ion[sp]];
        n[sp] = ctx->pl.h_ion_edge[(size_t)ion[sp] + 1] - k0[sp];
        x0[sp] = (int)nx;
        nx += n[sp];
    }
    for (size_t sp = 0; sp <= NS; ++sp) edge[sp] = (int)d->species_line_edge[sp];
    for (size_t q = 0; q < NL; ++q) line_id[q] = (int)d->line_id[q];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->nl.species = (long long)NS; ctx->nl.lines = (long long)NL; ctx->nl.nx = nx;
    ctx->nl.h_n = n; ctx->nl.h_ion = ion;
    int rc;
    if ((rc = nlte_build_lists(ctx))) return rc;
    if ((rc = upload(ctx, ctx->nl.line_id, line_id.data(), NL))) return rc;
    if ((rc = upload(ctx, ctx->nl.a_ul, d->A_ul, NL))) return rc;
    if ((rc = upload(ctx, ctx->nl.b_ul, d->B_ul, NL))) return rc;
    if ((rc = upload(ctx, ctx->nl.b_lu, d->B_lu, NL))) return rc;
    if ((rc = upload(ctx, ctx->nl.lower, lower.data(), NL))) return rc;
    if ((rc = upload(ctx, ctx->nl.upper, upper.data(), NL))) return rc;
    if ((rc = upload(ctx, ctx->nl.sp_k0, k0.data(), NS))) return rc;
    if ((rc = upload(ctx, ctx->nl.sp_n, n.data(), NS))) return rc;
    if ((rc = upload(ctx, ctx->nl.sp_x0, x0.data(), NS))) return rc;
    if ((rc = upload(ctx, ctx->nl.sp_line_edge, edge.data(), NS + 1))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the staging vectors are the sources of asynchronous copies)
    ctx->nl.coronal = d->coronal_approximation != 0;
    ctx->nl.classical = d->classical_nebular != 0;
    ctx->nl.have = true;
    return TARDIS_MC_OK;
}

/* ---- collisional rates of the NLTE species (atomic data with collision_data) ------------------------------ */
// scipy's interp1d bounds error of the reference's get_collision_matrix: t_e = link * t_rad of every shell against the temperature grid
static int collision_temperature_check(TardisMcContext *ctx, double link, long long n_shells, const double *t_radiative, double t_first, double t_last)
{
    const long long s = nlte::first_t_e_outside(link, n_shells, t_radiative, t_first, t_last);
    if (s < 0) return TARDIS_MC_OK;
    return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "t_electron of shell %lld = %g lies outside the collision temperatures [%g, %g]", s, link * t_radiative[s], t_first,
                t_last);
}

static std::string nlte_collision_check(const TardisMcNlteCollisionData *d, long long n_nlte_species, const int64_t *species_levels)
{
    return nlte::check_collision_data((long long)d->n_species, n_nlte_species, species_levels, (long long)d->n_temperatures, d->collision_temperatures,
                                      (long long)d->n_pairs, d->species_pair_edge, d->level_lower, d->level_upper, d->delta_e, d->g_ratio, d->C_ul);
}

int tardis_mc_check_nlte_collision_data(const TardisMcNlteCollisionData *d, int64_t n_species, const int64_t *species_levels, double link_t_rad_t_electron,
                                        int64_t n_shells, const double *t_radiative)
{
    if (!d || !species_levels) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid collision data: a pointer is missing");
    const std::string err = nlte_collision_check(d, (long long)n_species, species_levels);
    if (!err.empty()) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    if (!t_radiative) return TARDIS_MC_OK;
    return collision_temperature_check(nullptr, link_t_rad_t_electron, (long long)n_shells, t_radiative, d->collision_temperatures[0],
                                       d->collision_temperatures[d->n_temperatures - 1]);
}

int tardis_mc_set_nlte_collision_data(TardisMcContext *ctx, const TardisMcNlteCollisionData *d)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->nl.have) return fail(ctx, TARDIS_MC_ERR_STATE, "set_nlte_data must precede set_nlte_collision_data");
    drop_from(ctx, RUNG_COLLISION_DATA);
    if (!d) return TARDIS_MC_OK;
    // everything the kernels index with is checked here, on the host
    std::vector<int64_t> levels(ctx->nl.h_n.begin(), ctx->nl.h_n.end());
    const std::string err = nlte_collision_check(d, ctx->nl.species, levels.data());
    if (!err.empty()) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    const size_t NS = (size_t)d->n_species, NP = (size_t)d->n_pairs, NT = (size_t)d->n_temperatures;
    std::vector<int> edge(NS + 1), lower(NP), upper(NP);
    std::vector<double> inv_g(NP), c_t(NT * NP);
    for (size_t sp = 0; sp <= NS; ++sp) edge[sp] = (int)d->species_pair_edge[sp];
    for (size_t q = 0; q < NP; ++q) {
        lower[q] = (int)d->level_lower[q];
        upper[q] = (int)d->level_upper[q];
        inv_g[q] = 1 / d->g_ratio[q];  // (the reference flips g_ratio when it builds its matrices)
        for (size_t t = 0; t < NT; ++t) c_t[t * NP + q] = d->C_ul[q * NT + t];  // [NP][NT] -> [NT][NP]: a shell reads two rows
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = upload(ctx, ctx->nc.temperatures, d->collision_temperatures, NT))) return rc;
    if ((rc = upload(ctx, ctx->nc.c_t, c_t.data(), NT * NP))) return rc;
    if ((rc = upload(ctx, ctx->nc.delta_e, d->delta_e, NP))) return rc;
    if ((rc = upload(ctx, ctx->nc.inv_g, inv_g.data(), NP))) return rc;
    if ((rc = upload(ctx, ctx->nc.lower, lower.data(), NP))) return rc;
    if ((rc = upload(ctx, ctx->nc.upper, upper.data(), NP))) return rc;
    if ((rc = upload(ctx, ctx->nc.sp_pair_edge, edge.data(), NS + 1))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the staging vectors are the sources of asynchronous copies)
    ctx->nc.pairs = (long long)NP; ctx->nc.nt = (long long)NT;
    ctx->nc.t_first = d->collision_temperatures[0]; ctx->nc.t_last = d->collision_temperatures[NT - 1];
    ctx->nc.have = true;
    return TARDIS_MC_OK;
}

int tardis_mc_get_nlte_collision_rates(TardisMcContext *ctx, double *c_ul, double *c_lu)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->nc.valid || !ctx->nl.valid || !ctx->pl.valid)
        return fail(ctx, TARDIS_MC_ERR_STATE, "get_nlte_collision_rates needs a successful update_plasma that ran the NLTE stage with collision data");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t NP = (size_t)ctx->nc.pairs;
    if (NP == 0) return TARDIS_MC_OK;
    int rc;
    if ((rc = download_transposed(ctx, c_ul, ctx->nc.c_ul.as<double>(), NP))) return rc;
    return download_transposed(ctx, c_lu, ctx->nc.c_lu.as<double>(), NP);
}

// What the NLTE stage needs before the update's first kernel: the launches for the current option, the buffers of a call.
static int nlte_prepare(TardisMcContext *ctx)
{
    int rc;
    if ((ctx->nl.lists_built != ctx->nl.lds_levels || ctx->nl.blocked_built != ctx->nl.blocked_levels) && (rc = nlte_build_lists(ctx))) return rc;
    const size_t S = (size_t)ctx->n_shells, NL = (size_t)ctx->nl.lines;
    HIP_TRY(ctx, ctx->nl.r_ul.ensure(std::max<size_t>(1, NL * S) * sizeof(double)));
    HIP_TRY(ctx, ctx->nl.r_lu.ensure(std::max<size_t>(1, NL * S) * sizeof(double)));
    HIP_TRY(ctx, ctx->nl.x_t.ensure((size_t)ctx->nl.nx * S * sizeof(double)));
    HIP_TRY(ctx, ctx->nl.status.ensure((size_t)ctx->nl.species * S * sizeof(int)));
    HIP_TRY(ctx, ctx->nl.scratch.ensure(std::max<size_t>(1, (size_t)ctx->nl.scratch_doubles) * sizeof(double)));
    if (ctx->nl.n_blocked > 0) HIP_TRY(ctx, ctx->nl.pivrow.ensure((size_t)ctx->nl.nx * S * sizeof(int)));
    if (ctx->nc.have) {
        HIP_TRY(ctx, ctx->nc.c_ul.ensure(std::max<size_t>(1, (size_t)ctx->nc.pairs * S) * sizeof(double)));
        HIP_TRY(ctx, ctx->nc.c_lu.ensure(std::max<size_t>(1, (size_t)ctx->nc.pairs * S) * sizeof(double)));
    }
    return TARDIS_MC_OK;
}

// The elimination and the back substitution of the blocked form on assembled slabs: per panel step one panel and one trailing launch over all
// systems of the launch, then the back substitution; stream order is the only ordering.
static int nlte_blocked_enqueue(TardisMcContext *ctx, const mc::NlteSolveArgs &a, const std::vector<nlte::BlockedStep> &steps, int n_species, int *pivrow)
{
    static_assert(nlte::PANEL_COLUMNS == mc::NLTE_NB && nlte::TILE_COLUMNS == mc::NLTE_TN && nlte::TILE_ROWS == mc::NLTE_TM, "the plan and the kernels share the tile shape");
    for (size_t t = 0; t < steps.size(); ++t) {
        const nlte::BlockedStep &b = steps[t];
        const int c0 = (int)t * nlte::PANEL_COLUMNS;
        hipLaunchKernelGGL(mc::nlte_panel_kernel, dim3(b.panel_x, b.panel_y), dim3(256), 0, ctx->stream, a, pivrow, c0);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(mc::nlte_trailing_kernel, dim3(b.trailing_x, b.trailing_y, b.trailing_z), dim3(256), 0, ctx->stream, a, (const int *)pivrow, c0);
        HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(mc::nlte_backsolve_kernel, dim3((unsigned)n_species, (unsigned)a.S), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return TARDIS_MC_OK;
}

// The NLTE stage of an update, enqueued behind the Boltzmann kernel: the rates of the species' lines from the j of this update and the beta of the
// previous one, then a workgroup per (species, shell) that overwrites the species' rows of lbf_t.  d_t / d_w: the call's (t_rad, W) on the device.
static int nlte_stage(TardisMcContext *ctx, const TardisMcPlasmaUpdate *p, const double *beta_t, const double *d_t, const double *d_w)
{
    const size_t S = (size_t)ctx->n_shells, L = (size_t)ctx->n_lines, NL = (size_t)ctx->nl.lines;
    const double h = H_PLANCK, k_b = K_BOLTZMANN, c = mc::C_LIGHT;
    int rc;
    HIP_TRY(ctx, hipEventRecord(ctx->nl.ev[0], ctx->stream));
    mc::NlteRateArgs r{};
    r.S = (int)S; r.L = (long long)L; r.NL = (long long)NL;
    r.line_id = ctx->nl.line_id.as<int>(); r.a_ul = ctx->nl.a_ul.as<double>(); r.b_ul = ctx->nl.b_ul.as<double>(); r.b_lu = ctx->nl.b_lu.as<double>();
    r.nu_line = ctx->ot.nu_line.as<double>(); r.beta_t = beta_t; r.t_rad = d_t; r.w = d_w;
    r.planck_coef = 2 * h / (c * c); r.h = h; r.k_b = k_b; r.w_epsilon = p->w_epsilon; r.c_ang = c * 1e8; r.optical_window = p->detailed_optical_window;
    r.r_ul_t = ctx->nl.r_ul.as<double>(); r.r_lu_t = ctx->nl.r_lu.as<double>();
    const int jmode = ctx->nl.coronal ? mc::NLTE_J_CORONAL : p->j_blues_mode == 1 ? mc::NLTE_J_DETAILED : mc::NLTE_J_DILUTE;
    if (jmode == mc::NLTE_J_DETAILED) {  // the estimators' own t_rad / W / norm, as the j_blues kernel of the stages behind will compute them again
        if ((rc = radiation_field_enqueue(ctx, p->time_of_simulation, p->volume, p->w_epsilon, p->detailed_optical_window, ctx->nl.work, nullptr))) return rc;
        EstLayout e = est_layout(ctx->es.est_S, ctx->es.est_L, ctx->es.est_G, ctx->es.est_copies);
        const double *work = ctx->nl.work.as<double>();
        r.t_rad = work + S; r.w = work + 2 * S; r.norm = work + 3 * S; r.jblue_t = ctx->es.est.as<double>() + e.jblue;
    }
    if (NL > 0) {
        const unsigned bx = (unsigned)std::min<size_t>((NL + 255) / 256, 1024);
        auto kernel = jmode == mc::NLTE_J_CORONAL ? mc::nlte_rates_kernel<mc::NLTE_J_CORONAL>
                      : jmode == mc::NLTE_J_DETAILED ? mc::nlte_rates_kernel<mc::NLTE_J_DETAILED> : mc::nlte_rates_kernel<mc::NLTE_J_DILUTE>;
        hipLaunchKernelGGL(kernel, dim3(bx, (unsigned)S), dim3(256), 0, ctx->stream, r);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (ctx->nc.have && ctx->nc.pairs > 0) {  // c_ul / c_lu of every pair from the call's t_rad (counted with the rates kernel: assemble_ms)
        mc::NlteCollisionArgs c{};
        c.S = (int)S; c.NT = (int)ctx->nc.nt; c.NP = ctx->nc.pairs;
        c.temperatures = ctx->nc.temperatures.as<double>(); c.c_t = ctx->nc.c_t.as<double>(); c.delta_e = ctx->nc.delta_e.as<double>();
        c.inv_g_ratio = ctx->nc.inv_g.as<double>(); c.t_rad = d_t; c.link = ctx->pl.link;
        c.c_ul_t = ctx->nc.c_ul.as<double>(); c.c_lu_t = ctx->nc.c_lu.as<double>();
        const unsigned bx = (unsigned)std::min<size_t>(((size_t)ctx->nc.pairs + 255) / 256, 1024);
        hipLaunchKernelGGL(mc::nlte_collision_kernel, dim3(bx, (unsigned)S), dim3(256), 0, ctx->stream, c);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->nl.ev[1], ctx->stream));
    mc::NlteSolveArgs a{};
    a.S = (int)S; a.K = ctx->ou.levels; a.NL = (long long)NL; a.NX = ctx->nl.nx;
    a.sp_k0 = ctx->nl.sp_k0.as<int>(); a.sp_n = ctx->nl.sp_n.as<int>(); a.sp_x0 = ctx->nl.sp_x0.as<int>(); a.sp_line_edge = ctx->nl.sp_line_edge.as<int>();
    a.lower = ctx->nl.lower.as<int>(); a.upper = ctx->nl.upper.as<int>(); a.r_ul_t = r.r_ul_t; a.r_lu_t = r.r_lu_t; a.g = ctx->pl.g.as<double>();
    a.lbf_t = ctx->pl.lbf_t.as<double>(); a.x_t = ctx->nl.x_t.as<double>(); a.status = ctx->nl.status.as<int>(); a.scratch = ctx->nl.scratch.as<double>();
    if (ctx->nc.have && ctx->nc.pairs > 0) {  // (the resident electron density is still the previous update's: this call installs its own behind the solve)
        a.NP = ctx->nc.pairs; a.sp_pair_edge = ctx->nc.sp_pair_edge.as<int>(); a.pair_lower = ctx->nc.lower.as<int>(); a.pair_upper = ctx->nc.upper.as<int>();
        a.c_ul_t = ctx->nc.c_ul.as<double>(); a.c_lu_t = ctx->nc.c_lu.as<double>(); a.n_e = ctx->ot.n_e.as<double>();
    }
    for (const nlte::Launch &l : ctx->nl.launches) {
        a.list = ctx->nl.list.as<int>() + l.first;
        a.slab = ctx->nl.slab.as<long long>() + l.first;
        if (l.global) {  // split by form: the one-workgroup kernel for the first n_single of form_list, the blocked form for the rest
            a.list = ctx->nl.form_list.as<int>();
            a.slab = ctx->nl.form_slab.as<long long>();
            if (ctx->nl.n_single > 0) hipLaunchKernelGGL(mc::nlte_solve_kernel<false>, dim3((unsigned)ctx->nl.n_single, (unsigned)S), dim3(256), 0, ctx->stream, a);
            HIP_TRY(ctx, hipGetLastError());
            a.list += ctx->nl.n_single;
            a.slab += ctx->nl.n_single;
            if (ctx->nl.n_blocked > 0) {
                hipLaunchKernelGGL(mc::nlte_assemble_kernel, dim3((unsigned)ctx->nl.n_blocked, (unsigned)S), dim3(256), 0, ctx->stream, a);
                HIP_TRY(ctx, hipGetLastError());
                if ((rc = nlte_blocked_enqueue(ctx, a, ctx->nl.steps, ctx->nl.n_blocked, ctx->nl.pivrow.as<int>()))) return rc;
            }
            continue;
        }
        hipLaunchKernelGGL(mc::nlte_solve_kernel<true>, dim3((unsigned)l.count, (unsigned)S), dim3(256), l.lds_bytes, ctx->stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->nl.ev[2], ctx->stream));
    return TARDIS_MC_OK;
}

int tardis_mc_get_nlte(TardisMcContext *ctx, double *level_boltzmann_factor, double *relative_populations)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->nl.valid || !ctx->pl.valid) return fail(ctx, TARDIS_MC_ERR_STATE, "get_nlte needs a successful update_plasma that ran the NLTE stage");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = download_transposed(ctx, level_boltzmann_factor, ctx->pl.lbf_t.as<double>(), (size_t)ctx->ou.levels))) return rc;
    return download_transposed(ctx, relative_populations, ctx->nl.x_t.as<double>(), (size_t)ctx->nl.nx);
}

int tardis_mc_last_nlte_ms(TardisMcContext *ctx, double *out_assemble_ms, double *out_solve_ms)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->nl.timed || !ctx->pl.timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no update_plasma with an NLTE stage has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *const out[2] = {out_assemble_ms, out_solve_ms};
    return event_intervals_ms(ctx, ctx->nl.ev, 2, out);
}

/* ---- continuum stage of update_plasma: photo-ionisation data, rate coefficients, chi_bf, the free-free factor (continuum_rates.hpp) ---- */
// element_ion_edge runs from 0 to n_ions: the number of its elements, or -1 when it does not get there in ascending steps
static long long continuum_count_elements(const int64_t *element_ion_edge, int64_t n_ions)
{
    if (!element_ion_edge || n_ions < 1 || element_ion_edge[0] != 0) return -1;
    long long e = 0;
    while (element_ion_edge[e] < n_ions) {
        if (e >= n_ions || element_ion_edge[e + 1] <= element_ion_edge[e]) return -1;
        ++e;
    }
    return element_ion_edge[e] == n_ions ? e : -1;
}

int tardis_mc_check_continuum_data(const TardisMcContinuumData *d, int64_t n_levels, int64_t n_ions, const int64_t *ion_level_edge, const int64_t *element_ion_edge)
{
    if (!d) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "continuum data: a pointer is missing");
    if (!ion_level_edge || !element_ion_edge) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "continuum data: a pointer is missing (the plasma data's edge tables)");
    const long long n_elements = continuum_count_elements(element_ion_edge, n_ions);
    if (n_elements < 1) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "continuum data: element_ion_edge must run from 0 to n_ions in ascending steps");
    const std::string err = cont::check_data((long long)d->n_continua, d->level, d->block_edge, (long long)d->n_points, d->nu, d->x_sect, (long long)n_levels,
                                             (long long)n_ions, ion_level_edge, n_elements, element_ion_edge);
    return err.empty() ? TARDIS_MC_OK : fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
}

int tardis_mc_set_continuum_data(TardisMcContext *ctx, const TardisMcContinuumData *d)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->pl.have) return fail(ctx, TARDIS_MC_ERR_STATE, "set_plasma_data must precede set_continuum_data");
    ctx->ct.have = ctx->ct.valid = false;
    ctx->bf.have = ctx->bf.rates_valid = false;  // (whatever drops the continuum data drops the estimators on it)
    if (!d) return TARDIS_MC_OK;
    // everything the kernels index with is checked here, on the host
    std::vector<int> level_ion((size_t)std::max<int64_t>(d->n_continua, 1));
    const std::string err = cont::check_data((long long)d->n_continua, d->level, d->block_edge, (long long)d->n_points, d->nu, d->x_sect, ctx->ou.levels,
                                             (long long)ctx->pl.ions, ctx->pl.h_ion_edge.data(), (long long)ctx->pl.elements, ctx->pl.h_elem_edge.data(),
                                             d->n_continua >= 1 && d->n_continua <= 0x7ffffff0LL ? level_ion.data() : nullptr);
    if (!err.empty()) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    const size_t NC = (size_t)d->n_continua, NP = (size_t)d->n_points;
    std::vector<int> level(NC), edge(NC + 1), point_cont(NP);
    std::vector<double> nu_min(NC), nu_max(NC);
    for (size_t c = 0; c <= NC; ++c) edge[c] = (int)d->block_edge[c];
    for (size_t c = 0; c < NC; ++c) {
        level[c] = (int)d->level[c];
        nu_min[c] = d->nu[edge[c]];
        nu_max[c] = d->nu[edge[c + 1] - 1];
        for (int p = edge[c]; p < edge[c + 1]; ++p) point_cont[(size_t)p] = (int)c;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = upload(ctx, ctx->ct.level, level.data(), NC))) return rc;
    if ((rc = upload(ctx, ctx->ct.level_ion, level_ion.data(), NC))) return rc;
    if ((rc = upload(ctx, ctx->ct.block_edge, edge.data(), NC + 1))) return rc;
    if ((rc = upload(ctx, ctx->ct.point_cont, point_cont.data(), NP))) return rc;
    if ((rc = upload(ctx, ctx->ct.nu, d->nu, NP))) return rc;
    if ((rc = upload(ctx, ctx->ct.x_sect, d->x_sect, NP))) return rc;
    if ((rc = upload(ctx, ctx->ct.nu_min, nu_min.data(), NC))) return rc;
    if ((rc = upload(ctx, ctx->ct.nu_max, nu_max.data(), NC))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the staging vectors are the sources of asynchronous copies)
    ctx->ct.continua = (long long)NC; ctx->ct.points = (long long)NP;
    ctx->ct.have = true;
    return TARDIS_MC_OK;
}

// The buffers and the events of the continuum stage.  Nothing of a previous update is written to.
static int continuum_prepare(TardisMcContext *ctx)
{
    const size_t S = (size_t)ctx->n_shells, K = (size_t)ctx->ou.levels, I = (size_t)ctx->pl.ions, NC = (size_t)ctx->ct.continua, NP = (size_t)ctx->ct.points;
    HIP_TRY(ctx, ctx->ct.t_e.ensure(S * sizeof(double)));
    HIP_TRY(ctx, ctx->ct.ff.ensure(S * sizeof(double)));
    HIP_TRY(ctx, ctx->ct.lbf_e.ensure(K * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ct.z_e.ensure(I * S * sizeof(double)));
    for (DevBuf *b : {&ctx->ct.bfp, &ctx->ct.y_sp, &ctx->ct.y_g, &ctx->ct.y_st, &ctx->ct.chi_bf}) HIP_TRY(ctx, b->ensure(NP * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ct.rates.ensure(7 * NC * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ct.counts.ensure(2 * mc::CONTINUUM_COUNT_BLOCKS * sizeof(int)));
    // the cooling sub-stage behind it (cooling_rates.hpp)
    for (DevBuf *b : {&ctx->ck.y_cool, &ctx->ck.y_em, &ctx->ck.fb_cdf}) HIP_TRY(ctx, b->ensure(NP * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ck.rates.ensure(3 * NC * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ck.shell.ensure(3 * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ck.k_cdf.ensure((2 + 2 * NC) * S * sizeof(double)));
    HIP_TRY(ctx, ctx->ck.counts.ensure(mc::CONTINUUM_COUNT_BLOCKS * sizeof(int)));
    int rc;
    if ((rc = ensure_events(ctx, ctx->ck.ev))) return rc;
    return ensure_events(ctx, ctx->ct.ev);
}

static unsigned continuum_count_blocks(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, mc::CONTINUUM_COUNT_BLOCKS); }

// The cooling sub-stage, enqueued behind the continuum stage's last kernel and event: it reads that stage's bfp, y_sp, phi_ik, coll_ion and t_e, the update's
// n_t, N and n_e and the geometry's time_explosion, and writes only its own buffers.
static int cooling_stage(TardisMcContext *ctx, const mc::ContinuumArgs &c)
{
    const long long ncs = (long long)c.NC * c.S;
    mc::CoolingArgs a{};
    a.S = c.S; a.NC = c.NC; a.I = c.I; a.K = c.K; a.NP = c.NP;
    a.h = c.h; a.k_b = c.k_b; a.time_explosion = ctx->t_exp;
    a.level = c.level; a.level_ion = c.level_ion; a.block_edge = c.block_edge; a.point_cont = c.point_cont; a.nu = c.nu; a.x_sect = c.x_sect;
    a.charge = c.charge; a.bfp = c.bfp; a.y_sp = c.y_sp; a.phi_ik = c.rates; a.coll_ion = c.rates + 5 * ncs; a.t_e = c.t_e;
    a.n_t = c.n_t; a.n_ion = c.n_ion; a.n_e = c.n_e;
    a.y_cool = ctx->ck.y_cool.as<double>(); a.y_em = ctx->ck.y_em.as<double>(); a.rates = ctx->ck.rates.as<double>(); a.fb_cdf = ctx->ck.fb_cdf.as<double>();
    a.shell = ctx->ck.shell.as<double>(); a.k_cdf = ctx->ck.k_cdf.as<double>(); a.counts = ctx->ck.counts.as<int>();
    HIP_TRY(ctx, hipEventRecord(ctx->ck.ev[0], ctx->stream));
    hipLaunchKernelGGL(mc::cooling_point_kernel, dim3((unsigned)std::min<long long>((a.NP * (long long)a.S + 255) / 256, 65536)), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ck.ev[1], ctx->stream));
    hipLaunchKernelGGL(mc::cooling_block_kernel, dim3(continuum_count_blocks(ncs)), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ck.ev[2], ctx->stream));
    hipLaunchKernelGGL(mc::cooling_table_kernel, dim3((unsigned)((a.S + 63) / 64)), dim3(64), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ck.ev[3], ctx->stream));
    return TARDIS_MC_OK;
}

// The continuum stage, enqueued behind the population kernels of a solve that succeeded: it reads the call's (t_rad, W), the update's n_t, N and n_e and
// writes only its own buffers.
static int continuum_stage(TardisMcContext *ctx)
{
    const size_t S = (size_t)ctx->n_shells, K = (size_t)ctx->ou.levels, I = (size_t)ctx->pl.ions;
    const long long NC = ctx->ct.continua, NP = ctx->ct.points;
    double *d_t = ctx->ou.shell.as<double>() + S, *d_w = d_t + S;  // (where plasma_update_enqueue put the call's t_rad and W)
    const double h = H_PLANCK, c = mc::C_LIGHT;
    mc::ContinuumArgs a{};
    a.S = (int)S; a.NC = (int)NC; a.I = (int)I; a.K = (long long)K; a.NP = NP;
    a.link = ctx->pl.link; a.k_b = K_BOLTZMANN; a.h = h; a.two_pi_me = 2 * M_PI * M_ELECTRON; a.hh = h * h;
    a.planck_coef = 2 * h / (c * c); a.cc = c * c; a.eight_pi = 8 * M_PI; a.four_pi = 4 * M_PI; a.h_over_k = h / K_BOLTZMANN;
    a.level = ctx->ct.level.as<int>(); a.level_ion = ctx->ct.level_ion.as<int>(); a.block_edge = ctx->ct.block_edge.as<int>();
    a.point_cont = ctx->ct.point_cont.as<int>(); a.nu = ctx->ct.nu.as<double>(); a.x_sect = ctx->ct.x_sect.as<double>();
    a.charge = ctx->pl.charge.as<double>(); a.chi = ctx->pl.chi.as<double>(); a.t_rad = d_t; a.w = d_w;
    a.lbf_e = ctx->ct.lbf_e.as<double>(); a.z_e = ctx->ct.z_e.as<double>(); a.n_t = ctx->ou.n_t.as<double>(); a.n_ion = ctx->pl.n_ion.as<double>();
    a.n_e = ctx->pl.n_e.as<double>(); a.t_e = ctx->ct.t_e.as<double>(); a.ff = ctx->ct.ff.as<double>();
    a.bfp = ctx->ct.bfp.as<double>(); a.y_sp = ctx->ct.y_sp.as<double>(); a.y_g = ctx->ct.y_g.as<double>(); a.y_st = ctx->ct.y_st.as<double>();
    a.rates = ctx->ct.rates.as<double>(); a.chi_bf = ctx->ct.chi_bf.as<double>(); a.counts = ctx->ct.counts.as<int>();
    if (ctx->bf.continuum_field == 1) {  // (tardis_mc_update_plasma has checked that the rates are resident)
        a.gamma_est = ctx->bf.rates.as<double>();
        a.stim_est = a.gamma_est + NC * (long long)S;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ct.ev[0], ctx->stream));
    // thermal: t_e and the free-free factor, lbf_e = g exp(E (-beta_e)) (the LTE Boltzmann kernel on t_e), Z_e (the partition kernels of the plasma stage)
    hipLaunchKernelGGL(mc::continuum_shell_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    const unsigned bx = (unsigned)std::min<size_t>((K + 255) / 256, 1024);
    hipLaunchKernelGGL(mc::plasma_boltzmann_kernel<false>, dim3(bx, (unsigned)S), dim3(256), 0, ctx->stream, ctx->pl.energy.as<double>(), ctx->pl.g.as<double>(),
                       ctx->pl.meta.as<int>(), (const double *)a.t_e, (const double *)d_w, (long long)K, K_BOLTZMANN, ctx->ct.lbf_e.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    const long long n_long = ctx->pl.n_long;
    if (n_long < (long long)I) {
        const long long n = (long long)I * (long long)S;
        hipLaunchKernelGGL(mc::plasma_partition_lane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->pl.ion_edge.as<int>(), (int)I,
                           (long long)K, (int)S, ctx->pl.long_rows < 0 ? plup::LONG_ION_LEVELS : ctx->pl.long_rows, (const double *)a.lbf_e, ctx->ct.z_e.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    if (n_long > 0) {
        const long long n = n_long * (long long)S * 16;
        hipLaunchKernelGGL(mc::plasma_partition_row_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->pl.long_ions.as<int>(), (int)n_long,
                           ctx->pl.ion_edge.as<int>(), (long long)K, (int)S, (const double *)a.lbf_e, ctx->ct.z_e.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ct.ev[1], ctx->stream));
    hipLaunchKernelGGL(mc::continuum_point_kernel, dim3((unsigned)std::min<long long>((NP * (long long)S + 255) / 256, 65536)), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ct.ev[2], ctx->stream));
    hipLaunchKernelGGL(mc::continuum_rate_kernel, dim3(continuum_count_blocks(NC * (long long)S)), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ct.ev[3], ctx->stream));
    hipLaunchKernelGGL(mc::continuum_chi_kernel, dim3(continuum_count_blocks(NP * (long long)S)), dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ct.ev[4], ctx->stream));
    int rc;
    if ((rc = cooling_stage(ctx, a))) return rc;  // behind the stage's last event: tardis_mc_last_continuum_ms does not count it
    ctx->ct.ran = true;
    return TARDIS_MC_OK;
}

static bool continuum_resident(const TardisMcContext *ctx) { return ctx->ct.valid && ctx->pl.valid; }

int tardis_mc_get_continuum_rates(TardisMcContext *ctx, double *phi_ik, double *alpha_sp, double *gamma, double *alpha_stim, double *gamma_corr, double *coll_ion,
                                  double *coll_recomb)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!continuum_resident(ctx)) return fail(ctx, TARDIS_MC_ERR_STATE, "get_continuum_rates needs a successful update_plasma that ran the continuum stage");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t n = (size_t)ctx->ct.continua * (size_t)ctx->n_shells;
    double *const host[7] = {phi_ik, alpha_sp, gamma, alpha_stim, gamma_corr, coll_ion, coll_recomb};
    std::vector<CopyJob> jobs;
    for (int v = 0; v < 7; ++v) jobs.push_back({(void *)host[v], ctx->ct.rates.as<double>() + (size_t)v * n, n * sizeof(double)});
    HIP_TRY(ctx, host_copy(ctx, jobs, false));
    return TARDIS_MC_OK;
}

int tardis_mc_get_continuum_opacity(TardisMcContext *ctx, double *chi_bf, double *ff_opacity_factor, double *t_electrons, int64_t *n_negative_chi_bf,
                                    int64_t *n_negative_gamma_corr)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!continuum_resident(ctx)) return fail(ctx, TARDIS_MC_ERR_STATE, "get_continuum_opacity needs a successful update_plasma that ran the continuum stage");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t S = (size_t)ctx->n_shells, NP = (size_t)ctx->ct.points, NC = (size_t)ctx->ct.continua;
    HIP_TRY(ctx, host_copy(ctx, {{(void *)chi_bf, ctx->ct.chi_bf.p, NP * S * sizeof(double)},
                                 {(void *)ff_opacity_factor, ctx->ct.ff.p, S * sizeof(double)},
                                 {(void *)t_electrons, ctx->ct.t_e.p, S * sizeof(double)}}, false));
    if (n_negative_chi_bf || n_negative_gamma_corr) {  // the workgroups' counts, added here
        std::vector<int> counts(2 * (size_t)mc::CONTINUUM_COUNT_BLOCKS);
        HIP_TRY(ctx, hipMemcpy(counts.data(), ctx->ct.counts.p, counts.size() * sizeof(int), hipMemcpyDeviceToHost));
        const unsigned blocks[2] = {continuum_count_blocks((long long)(NC * S)), continuum_count_blocks((long long)(NP * S))};
        int64_t sum[2] = {0, 0};
        for (int v = 0; v < 2; ++v)
            for (unsigned b = 0; b < blocks[v]; ++b) sum[v] += counts[(size_t)v * mc::CONTINUUM_COUNT_BLOCKS + b];
        if (n_negative_gamma_corr) *n_negative_gamma_corr = sum[0];
        if (n_negative_chi_bf) *n_negative_chi_bf = sum[1];
    }
    return TARDIS_MC_OK;
}

int tardis_mc_last_continuum_ms(TardisMcContext *ctx, double *out_thermal_ms, double *out_points_ms, double *out_rates_ms, double *out_opacity_ms)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->ct.timed || !ctx->pl.timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no update_plasma with a continuum stage has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *const out[4] = {out_thermal_ms, out_points_ms, out_rates_ms, out_opacity_ms};
    return event_intervals_ms(ctx, ctx->ct.ev, 4, out);
}

int tardis_mc_continuum_opacity(TardisMcContext *ctx, const TardisMcContinuumQuery *q)
{
    if (!ctx || !q) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid continuum query");
    if (!continuum_resident(ctx)) return fail(ctx, TARDIS_MC_ERR_STATE, "continuum_opacity needs a successful update_plasma that ran the continuum stage");
    if (q->n < 0 || q->n > 0x7ffffff0LL || (q->n > 0 && (!q->nu || !q->shell))) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid continuum query");
    const size_t n = (size_t)q->n, S = (size_t)ctx->n_shells, NC = (size_t)ctx->ct.continua;
    // everything the kernel indexes with is checked here, on the host
    std::vector<int> shell(n);
    for (size_t e = 0; e < n; ++e) {
        if (!(std::isfinite(q->nu[e]) && q->nu[e] > 0.0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "continuum query: nu[%zu] = %g is not finite and positive", e, q->nu[e]);
        if (q->shell[e] < 0 || q->shell[e] >= (int64_t)S)
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "continuum query: shell[%zu] = %lld lies outside [0, %zu)", e, (long long)q->shell[e], S);
        shell[e] = (int)q->shell[e];
    }
    if (n == 0) return TARDIS_MC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ScopedDevBuf d_nu, d_shell, d_tot, d_ff, d_cur, d_chi_each, d_x_each;
    std::vector<int> current(q->n_current ? n : 0);
    const int rc = [&]() -> int {
        int rc1;
        if ((rc1 = upload(ctx, d_nu, q->nu, n))) return rc1;
        if ((rc1 = upload(ctx, d_shell, shell.data(), n))) return rc1;
        if (q->chi_bf_tot) HIP_TRY(ctx, d_tot.ensure(n * sizeof(double)));
        if (q->chi_ff) HIP_TRY(ctx, d_ff.ensure(n * sizeof(double)));
        if (q->n_current) HIP_TRY(ctx, d_cur.ensure(n * sizeof(int)));
        if (q->chi_bf_each) HIP_TRY(ctx, d_chi_each.ensure(n * NC * sizeof(double)));
        if (q->x_sect_each) HIP_TRY(ctx, d_x_each.ensure(n * NC * sizeof(double)));
        mc::ContinuumTables t{};
        t.S = (int)S; t.NC = (int)NC; t.h = H_PLANCK; t.k_b = K_BOLTZMANN;
        t.block_edge = ctx->ct.block_edge.as<int>(); t.nu = ctx->ct.nu.as<double>(); t.x_sect = ctx->ct.x_sect.as<double>();
        t.nu_min = ctx->ct.nu_min.as<double>(); t.nu_max = ctx->ct.nu_max.as<double>();
        t.chi_bf = ctx->ct.chi_bf.as<double>(); t.ff = ctx->ct.ff.as<double>(); t.t_e = ctx->ct.t_e.as<double>();
        mc::ContinuumQueryArgs k{};
        k.n = (long long)n; k.nu = d_nu.as<double>(); k.shell = d_shell.as<int>();
        k.chi_bf_tot = q->chi_bf_tot ? d_tot.as<double>() : nullptr; k.chi_ff = q->chi_ff ? d_ff.as<double>() : nullptr;
        k.n_current = q->n_current ? d_cur.as<int>() : nullptr;
        k.chi_each = q->chi_bf_each ? d_chi_each.as<double>() : nullptr; k.x_each = q->x_sect_each ? d_x_each.as<double>() : nullptr;
        hipLaunchKernelGGL(mc::continuum_query_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, t, k);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, host_copy(ctx, {{(void *)q->chi_bf_tot, d_tot.p, n * sizeof(double)},
                                     {(void *)q->chi_ff, d_ff.p, n * sizeof(double)},
                                     {(void *)(q->n_current ? current.data() : nullptr), d_cur.p, n * sizeof(int)},
                                     {(void *)q->chi_bf_each, d_chi_each.p, n * NC * sizeof(double)},
                                     {(void *)q->x_sect_each, d_x_each.p, n * NC * sizeof(double)}}, false));
        return TARDIS_MC_OK;
    }();
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (nothing of the call is in flight when its scratch goes)
    if (rc) return rc;
    if (q->n_current)
        for (size_t e = 0; e < n; ++e) q->n_current[e] = current[e];
    return TARDIS_MC_OK;
}

/* ---- cooling sub-stage behind the continuum stage: cooling rates, emission CDFs, the k-packet table and its samplers (cooling_rates.hpp, kpacket_sample.hpp) ---- */
int tardis_mc_get_cooling_rates(TardisMcContext *ctx, double *c_fb_sp, double *cool_rate_fb, double *cool_rate_coll_ion, double *cool_rate_ff,
                                double *cool_rate_adiabatic, double *cool_rate_total)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!continuum_resident(ctx)) return fail(ctx, TARDIS_MC_ERR_STATE, "get_cooling_rates needs a successful update_plasma that ran the continuum stage");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t S = (size_t)ctx->n_shells, n = (size_t)ctx->ct.continua * S;
    double *const per_continuum[3] = {c_fb_sp, cool_rate_fb, cool_rate_coll_ion};
    double *const per_shell[3] = {cool_rate_ff, cool_rate_adiabatic, cool_rate_total};
    std::vector<CopyJob> jobs;
    for (int v = 0; v < 3; ++v) jobs.push_back({(void *)per_continuum[v], ctx->ck.rates.as<double>() + (size_t)v * n, n * sizeof(double)});
    for (int v = 0; v < 3; ++v) jobs.push_back({(void *)per_shell[v], ctx->ck.shell.as<double>() + (size_t)v * S, S * sizeof(double)});
    HIP_TRY(ctx, host_copy(ctx, jobs, false));
    return TARDIS_MC_OK;
}

int tardis_mc_get_kpacket_tables(TardisMcContext *ctx, double *fb_emission_cdf, double *k_cdf, int64_t *n_degenerate_fb_cdf)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!continuum_resident(ctx)) return fail(ctx, TARDIS_MC_ERR_STATE, "get_kpacket_tables needs a successful update_plasma that ran the continuum stage");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t S = (size_t)ctx->n_shells, NP = (size_t)ctx->ct.points, NC = (size_t)ctx->ct.continua;
    HIP_TRY(ctx, host_copy(ctx, {{(void *)fb_emission_cdf, ctx->ck.fb_cdf.p, NP * S * sizeof(double)},
                                 {(void *)k_cdf, ctx->ck.k_cdf.p, (2 + 2 * NC) * S * sizeof(double)}}, false));
    if (n_degenerate_fb_cdf) {  // the workgroups' counts, added here
        std::vector<int> counts((size_t)mc::CONTINUUM_COUNT_BLOCKS);
        HIP_TRY(ctx, hipMemcpy(counts.data(), ctx->ck.counts.p, counts.size() * sizeof(int), hipMemcpyDeviceToHost));
        int64_t sum = 0;
        for (unsigned b = 0; b < continuum_count_blocks((long long)(NC * S)); ++b) sum += counts[b];
        *n_degenerate_fb_cdf = sum;
    }
    return TARDIS_MC_OK;
}

int tardis_mc_last_cooling_ms(TardisMcContext *ctx, double *out_points_ms, double *out_blocks_ms, double *out_table_ms)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->ct.timed || !ctx->pl.timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no update_plasma with a continuum stage has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *const out[3] = {out_points_ms, out_blocks_ms, out_table_ms};
    return event_intervals_ms(ctx, ctx->ck.ev, 3, out);
}

int tardis_mc_kpacket_sample(TardisMcContext *ctx, const TardisMcKpacketQuery *q)
{
    if (!ctx || !q) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid k-packet query");
    if (!continuum_resident(ctx)) return fail(ctx, TARDIS_MC_ERR_STATE, "kpacket_sample needs a successful update_plasma that ran the continuum stage");
    if (q->n < 0 || q->n > 0x7ffffff0LL || (q->n > 0 && (!q->shell || !q->z_process || !q->z_nu))) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid k-packet query");
    const size_t n = (size_t)q->n, S = (size_t)ctx->n_shells;
    const int64_t NC = (int64_t)ctx->ct.continua;
    // everything the kernel indexes with is checked here, on the host
    std::vector<int> shell(n), force_kind(q->force_kind ? n : 0), force_continuum(q->force_kind ? n : 0);
    for (size_t e = 0; e < n; ++e) {
        if (q->shell[e] < 0 || q->shell[e] >= (int64_t)S)
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "k-packet query: shell[%zu] = %lld lies outside [0, %zu)", e, (long long)q->shell[e], S);
        shell[e] = (int)q->shell[e];
        if (!(q->z_process[e] >= 0.0 && q->z_process[e] < 1.0))
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "k-packet query: z_process[%zu] = %g lies outside [0, 1)", e, q->z_process[e]);
        if (!(q->z_nu[e] >= 0.0 && q->z_nu[e] < 1.0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "k-packet query: z_nu[%zu] = %g lies outside [0, 1)", e, q->z_nu[e]);
        const int64_t kind = q->force_kind ? q->force_kind[e] : -1, forced = q->force_continuum ? q->force_continuum[e] : -1;
        if (kind < -1 || kind > 3) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "k-packet query: force_kind[%zu] = %lld lies outside [-1, 3]", e, (long long)kind);
        if (kind >= 2 && (forced < 0 || forced >= NC))
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "k-packet query: force_continuum[%zu] = %lld lies outside [0, %lld)", e, (long long)forced, (long long)NC);
        if (kind < 2 && forced != -1)
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "k-packet query: force_continuum[%zu] = %lld, but force_kind[%zu] = %lld has no continuum to force (-1)", e,
                        (long long)forced, e, (long long)kind);
        if (q->force_kind) { force_kind[e] = (int)kind; force_continuum[e] = (int)forced; }
    }
    if (n == 0) return TARDIS_MC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ScopedDevBuf d_shell, d_zp, d_zn, d_fk, d_fc, d_kind, d_cont, d_nu;
    std::vector<int> kind(q->kind ? n : 0), cont(q->continuum ? n : 0);
    const int rc = [&]() -> int {
        int rc1;
        if ((rc1 = upload(ctx, d_shell, shell.data(), n))) return rc1;
        if ((rc1 = upload(ctx, d_zp, q->z_process, n))) return rc1;
        if ((rc1 = upload(ctx, d_zn, q->z_nu, n))) return rc1;
        if (q->force_kind && (rc1 = upload(ctx, d_fk, force_kind.data(), n))) return rc1;
        if (q->force_kind && (rc1 = upload(ctx, d_fc, force_continuum.data(), n))) return rc1;
        if (q->kind) HIP_TRY(ctx, d_kind.ensure(n * sizeof(int)));
        if (q->continuum) HIP_TRY(ctx, d_cont.ensure(n * sizeof(int)));
        if (q->nu) HIP_TRY(ctx, d_nu.ensure(n * sizeof(double)));
        mc::KpacketTables t{};
        t.S = (int)S; t.NC = (int)NC; t.h = H_PLANCK; t.k_b = K_BOLTZMANN;
        t.block_edge = ctx->ct.block_edge.as<int>(); t.nu = ctx->ct.nu.as<double>(); t.fb_cdf = ctx->ck.fb_cdf.as<double>();
        t.k_cdf = ctx->ck.k_cdf.as<double>(); t.t_e = ctx->ct.t_e.as<double>();
        mc::KpacketQueryArgs k{};
        k.n = (long long)n; k.shell = d_shell.as<int>(); k.z_process = d_zp.as<double>(); k.z_nu = d_zn.as<double>();
        k.force_kind = q->force_kind ? d_fk.as<int>() : nullptr; k.force_continuum = q->force_kind ? d_fc.as<int>() : nullptr;
        k.kind = q->kind ? d_kind.as<int>() : nullptr; k.continuum = q->continuum ? d_cont.as<int>() : nullptr; k.nu = q->nu ? d_nu.as<double>() : nullptr;
        hipLaunchKernelGGL(mc::kpacket_query_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, t, k);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, host_copy(ctx, {{(void *)(q->kind ? kind.data() : nullptr), d_kind.p, n * sizeof(int)},
                                     {(void *)(q->continuum ? cont.data() : nullptr), d_cont.p, n * sizeof(int)},
                                     {(void *)q->nu, d_nu.p, n * sizeof(double)}}, false));
        return TARDIS_MC_OK;
    }();
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (nothing of the call is in flight when its scratch goes)
    if (rc) return rc;
    for (size_t e = 0; e < n && q->kind; ++e) q->kind[e] = kind[e];
    for (size_t e = 0; e < n && q->continuum; ++e) q->continuum[e] = cont[e];
    return TARDIS_MC_OK;
}

// Everything that can refuse the call before the device is touched: the call order, the modes, the shell bound, the bounds of the two temperature tables.
static int plasma_update_check(TardisMcContext *ctx, const TardisMcPlasmaUpdate *p, const TardisMcOpacityUpdate *u)
{
    if (!ctx->have_opacity || !ctx->ou.have || !ctx->pl.have)
        return fail(ctx, TARDIS_MC_ERR_STATE, "set_opacity, set_line_data and set_plasma_data must precede update_plasma");
    if ((p->ionization_mode != 0 && p->ionization_mode != 1) || (p->excitation_mode != 0 && p->excitation_mode != 1))
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "unknown ionization_mode %d / excitation_mode %d", p->ionization_mode, p->excitation_mode);
    if (ctx->he.have && ctx->he.helium) {
        if (p->ionization_mode != 0)
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "helium_treatment recomb-nlte belongs to the nebular ionisation: ionization_mode %d is refused", p->ionization_mode);
        if (ctx->nl.have)
            for (size_t sp = 0; sp < ctx->nl.h_ion.size(); ++sp)
                if (ctx->nl.h_ion[sp] >= ctx->he.ion && ctx->nl.h_ion[sp] < ctx->he.ion + 3)
                    return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "helium_treatment recomb-nlte while NLTE species %zu is the helium ion %d: both treat helium's levels, no order is defined",
                                sp, ctx->nl.h_ion[sp]);
    }
    int rc;
    if ((rc = opacity_update_check(ctx, u))) return rc;
    const size_t S = (size_t)ctx->n_shells;
    if ((long long)S > plup::MAX_SHELLS)
        return fail(ctx, TARDIS_MC_ERR_UNSUPPORTED, "update_plasma iterates the electron density inside one workgroup: at most %lld shells", plup::MAX_SHELLS);
    if (p->ionization_mode == 0)
        for (size_t s = 0; s < S; ++s)
            if (!(p->t_radiative[s] >= ctx->pl.t_min && p->t_radiative[s] <= ctx->pl.t_max))
                return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "t_radiative[%zu] = %g lies outside the zeta table [%g, %g]", s, p->t_radiative[s], ctx->pl.t_min,
                            ctx->pl.t_max);
    if (ctx->nl.have && ctx->nc.have) return collision_temperature_check(ctx, ctx->pl.link, (long long)S, p->t_radiative, ctx->nc.t_first, ctx->nc.t_last);
    return TARDIS_MC_OK;
}

// The list of the ions that take the row form, the buffers and the events of every stage.  Nothing of a previous update is written to.
static int plasma_update_prepare(TardisMcContext *ctx)
{
    const size_t S = (size_t)ctx->n_shells, K = (size_t)ctx->ou.levels, I = (size_t)ctx->pl.ions;
    int rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->pl.long_rows_built != ctx->pl.long_rows) {
        if ((rc = upload_row_form_list(ctx, ctx->pl.h_ion_edge, ctx->pl.long_rows, ctx->pl.long_ions, &ctx->pl.n_long))) return rc;
        ctx->pl.long_rows_built = ctx->pl.long_rows;
    }
    if ((rc = opacity_update_buffers(ctx))) return rc;
    if (ctx->nl.have && (rc = nlte_prepare(ctx))) return rc;
    HIP_TRY(ctx, ctx->pl.lbf_t.ensure(K * S * sizeof(double)));
    HIP_TRY(ctx, ctx->pl.z.ensure(I * S * sizeof(double)));
    HIP_TRY(ctx, ctx->pl.phi.ensure(I * S * sizeof(double)));
    HIP_TRY(ctx, ctx->pl.n_ion.ensure(I * S * sizeof(double)));
    HIP_TRY(ctx, ctx->pl.n_e.ensure(S * sizeof(double)));
    HIP_TRY(ctx, ctx->pl.status.ensure(2 * sizeof(int)));
    if ((rc = ensure_events(ctx, ctx->ou.ev))) return rc;
    if ((rc = ensure_events(ctx, ctx->pl.ev))) return rc;
    if (ctx->he.have && ctx->he.helium) {
        const size_t KH = (size_t)ctx->he.n2 + 1;
        HIP_TRY(ctx, ctx->he.hp.ensure(KH * S * sizeof(double)));
        HIP_TRY(ctx, ctx->he.v.ensure(KH * S * sizeof(double)));
        if ((rc = ensure_events(ctx, ctx->he.ev))) return rc;
    }
    if (ctx->ct.have && (rc = continuum_prepare(ctx))) return rc;
    return ensure_events(ctx, ctx->nl.ev);
}

// The solve, enqueued: Boltzmann factors, the NLTE stage, partition functions, ionisation.  It writes the stages' own buffers -- lbf_t, x, Z, phi, N, pl.n_e,
// the status words -- and the call's (t_rad, W); the resident n_t, the electron densities and the opacity tables wait for plasma_update_install.
static int plasma_update_enqueue(TardisMcContext *ctx, const TardisMcPlasmaUpdate *p)
{
    const size_t S = (size_t)ctx->n_shells, K = (size_t)ctx->ou.levels, I = (size_t)ctx->pl.ions;
    double *d_t = ctx->ou.shell.as<double>() + S, *d_w = d_t + S;  // (the layout of radiation_field_enqueue's work: volume, t_rad, W, norm)
    // beta_sobolev of the previous update, read before this update's line kernel writes over it; none since the last set_opacity: 1.0
    const double *nlte_beta = ctx->ou.valid && !ctx->nl.classical ? ctx->ou.beta_t.as<double>() : nullptr;
    int rc;
    ctx->pl.valid = ctx->nl.valid = ctx->nc.valid = ctx->he.valid = false;
    ctx->he.ran = ctx->he.timed = false;
    ctx->ct.valid = ctx->ct.ran = ctx->ct.timed = false;
    HIP_TRY(ctx, hipMemcpyAsync(d_t, p->t_radiative, S * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_w, p->dilution_factor, S * 8, hipMemcpyHostToDevice, ctx->stream));
    ctx->nl.ran = ctx->nl.timed = ctx->pl.timed = false;  // (ou.timed and the ou.ev events stay the previous update's until this solve has succeeded)
    HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->pl.ev[0], ctx->stream));
    const unsigned bx = (unsigned)std::min<size_t>((K + 255) / 256, 1024);
    auto kernel = p->excitation_mode == 0 ? mc::plasma_boltzmann_kernel<true> : mc::plasma_boltzmann_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(bx, (unsigned)S), dim3(256), 0, ctx->stream, ctx->pl.energy.as<double>(), ctx->pl.g.as<double>(), ctx->pl.meta.as<int>(), d_t,
                       d_w, (long long)K, K_BOLTZMANN, ctx->pl.lbf_t.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->pl.ev[1], ctx->stream));
    if (ctx->nl.have && (rc = nlte_stage(ctx, p, nlte_beta, d_t, d_w))) return rc;  // the NLTE species' Boltzmann factors, before anything reads them
    const bool helium = ctx->he.have && ctx->he.helium;
    const bool fixed_delta = ctx->he.have && ctx->he.fixed_delta;
    if (helium) {  // hp of helium's levels from the Boltzmann factors as they now stand
        mc::HeliumArgs h;
        h.S = (int)S; h.NT = ctx->pl.nt; h.K = (long long)K;
        h.k0 = ctx->he.k0; h.n1 = ctx->he.n1; h.n2 = ctx->he.n2; h.ion = ctx->he.ion;
        h.fixed_delta = fixed_delta; h.delta_treatment = ctx->he.delta;
        h.link = ctx->pl.link; h.chi_0 = ctx->pl.chi_0; h.k_b = K_BOLTZMANN; h.two_pi_me = 2 * M_PI * M_ELECTRON; h.hh = H_PLANCK * H_PLANCK;
        h.g = ctx->pl.g.as<double>(); h.chi = ctx->pl.chi.as<double>(); h.zeta_t = ctx->pl.zeta_t.as<double>(); h.zeta = ctx->pl.zeta.as<double>();
        h.t_rad = d_t; h.w = d_w; h.lbf_t = ctx->pl.lbf_t.as<double>(); h.hp = ctx->he.hp.as<double>();
        const long long n = (long long)(h.n2 + 1) * (long long)S;
        HIP_TRY(ctx, hipEventRecord(ctx->he.ev[0], ctx->stream));
        hipLaunchKernelGGL(mc::helium_relative_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, h);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ctx->he.ev[1], ctx->stream));
        ctx->he.ran = true;
    }
    const long long n_long = ctx->pl.n_long;
    if (n_long < (long long)I) {
        const long long n = (long long)I * (long long)S;
        hipLaunchKernelGGL(mc::plasma_partition_lane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->pl.ion_edge.as<int>(), (int)I,
                           (long long)K, (int)S, ctx->pl.long_rows < 0 ? plup::LONG_ION_LEVELS : ctx->pl.long_rows, ctx->pl.lbf_t.as<double>(), ctx->pl.z.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    if (n_long > 0) {
        const long long n = n_long * (long long)S * 16;
        hipLaunchKernelGGL(mc::plasma_partition_row_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->pl.long_ions.as<int>(), (int)n_long,
                           ctx->pl.ion_edge.as<int>(), (long long)K, (int)S, ctx->pl.lbf_t.as<double>(), ctx->pl.z.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->pl.ev[2], ctx->stream));
    mc::PlasmaIonArgs a;
    a.S = (int)S; a.I = (int)I; a.E = ctx->pl.elements; a.NT = ctx->pl.nt;
    a.nebular = p->ionization_mode == 0;
    a.max_iter = ctx->pl.max_iterations;
    a.link = ctx->pl.link; a.chi_0 = ctx->pl.chi_0; a.k_b = K_BOLTZMANN; a.two_pi_me = 2 * M_PI * M_ELECTRON; a.hh = H_PLANCK * H_PLANCK;
    a.element_edge = ctx->pl.elem_edge.as<int>(); a.charge = ctx->pl.charge.as<double>(); a.chi = ctx->pl.chi.as<double>();
    a.zeta_t = ctx->pl.zeta_t.as<double>(); a.zeta = ctx->pl.zeta.as<double>(); a.density = ctx->pl.density.as<double>();
    a.t_rad = d_t; a.w = d_w; a.z = ctx->pl.z.as<double>();
    a.phi = ctx->pl.phi.as<double>(); a.n_ion = ctx->pl.n_ion.as<double>(); a.n_e = ctx->pl.n_e.as<double>(); a.status = ctx->pl.status.as<int>();
    a.delta_treatment = fixed_delta ? ctx->he.delta : 0.0;
    a.he_element = a.he_ion = a.he_n1 = a.he_n2 = 0; a.hp = nullptr; a.he_v = nullptr;
    if (helium) {
        a.he_element = ctx->he.element; a.he_ion = ctx->he.ion; a.he_n1 = ctx->he.n1; a.he_n2 = ctx->he.n2;
        a.hp = ctx->he.hp.as<double>(); a.he_v = ctx->he.v.as<double>();
    }
    auto ionization_kernel = helium ? (fixed_delta ? mc::plasma_ionization_kernel<true, true> : mc::plasma_ionization_kernel<true, false>)
                                    : (fixed_delta ? mc::plasma_ionization_kernel<false, true> : mc::plasma_ionization_kernel<false, false>);
    hipLaunchKernelGGL(ionization_kernel, dim3(1), dim3((unsigned)((S + 63) / 64 * 64)), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->pl.ev[3], ctx->stream));
    return TARDIS_MC_OK;
}

// Waits for the solve and reads {status, passes} and the status words of the NLTE solves.  A failed solve is worded here and nowhere else; its kernels are what
// tardis_mc_last_propagate_ms then reports, between a matching pair of events.
static int plasma_update_status(TardisMcContext *ctx)
{
    const long long S = ctx->n_shells;
    int status[2] = {mc::PLASMA_NAN, 0};
    HIP_TRY(ctx, hipMemcpyAsync(status, ctx->pl.status.p, sizeof status, hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->nl.have) {
        ctx->nl.h_status.assign((size_t)(ctx->nl.species * S), -1);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->nl.h_status.data(), ctx->nl.status.p, ctx->nl.h_status.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->pl.iterations = status[1];
    long long nlte_failed = -1;
    if (ctx->nl.have)
        for (size_t q = 0; q < ctx->nl.h_status.size() && nlte_failed < 0; ++q)
            if (ctx->nl.h_status[q] != 0) nlte_failed = (long long)q;
    if (status[0] == mc::PLASMA_OK && nlte_failed < 0) return TARDIS_MC_OK;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->timed = true;
    ctx->chunks_timed = 0;
    if (nlte_failed >= 0) {  // (whatever the stages behind it made of the unfinished Boltzmann factors)
        const long long sp = nlte_failed / S, shell = nlte_failed % S;
        const int code = ctx->nl.h_status[(size_t)nlte_failed], n = ctx->nl.h_n[(size_t)sp];
        if (code >= 1 && code <= n)
            return fail(ctx, TARDIS_MC_ERR_STATE, "update_plasma: the NLTE solve of species %lld (ion %d, %d levels) in shell %lld met a zero or non-finite pivot in elimination "
                        "step %d (singular rate matrix); the opacity state is unchanged", sp, ctx->nl.h_ion[(size_t)sp], n, shell, code - 1);
        return fail(ctx, TARDIS_MC_ERR_STATE, "update_plasma: the NLTE solve of species %lld (ion %d, %d levels) in shell %lld gave %s after all %d elimination steps; the "
                    "opacity state is unchanged", sp, ctx->nl.h_ion[(size_t)sp], n, shell, code == n + 1 ? "x[0] == 0" : "a population that is not finite", n);
    }
    if (status[0] == mc::PLASMA_NAN)
        return fail(ctx, TARDIS_MC_ERR_STATE, "update_plasma: the electron density became NaN in pass %d (PlasmaIonizationError); the opacity state is unchanged", status[1] + 1);
    return fail(ctx, TARDIS_MC_ERR_STATE, "update_plasma: the electron density has not converged after %d passes (option plasma_max_iterations); the opacity state is unchanged",
                status[1]);
}

// The solve is good: the level populations into the resident n_t, the solved electron densities into the resident ones, and on them the opacity update.
static int plasma_update_install(TardisMcContext *ctx, const TardisMcOpacityUpdate *u)
{
    const size_t S = (size_t)ctx->n_shells, K = (size_t)ctx->ou.levels;
    drop_products(ctx, OPACITY_UPDATE_BEGINS);
    ctx->ou.valid = ctx->ou.timed = false;
    const unsigned bx = (unsigned)std::min<size_t>((K + 255) / 256, 1024);
    hipLaunchKernelGGL(mc::plasma_population_kernel, dim3(bx, (unsigned)S), dim3(256), 0, ctx->stream, ctx->pl.lbf_t.as<double>(), ctx->pl.level_ion.as<int>(),
                       ctx->pl.z.as<double>(), ctx->pl.n_ion.as<double>(), (long long)K, (int)S, ctx->ou.n_t.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->he.ran) {  // helium's levels are the v of the last pass
        const int levels = ctx->he.n2 + 1;
        const long long n = (long long)levels * (long long)S;
        hipLaunchKernelGGL(mc::helium_population_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->he.v.as<double>(), ctx->he.k0, levels,
                           (long long)K, (int)S, ctx->ou.n_t.as<double>());
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, ctx->ot.n_e.ensure(S * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ot.n_e.p, ctx->pl.n_e.p, S * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->pl.ev[4], ctx->stream));
    int rc;
    if (ctx->ct.have && (rc = continuum_stage(ctx))) return rc;  // between the two stages' events: neither timer counts it
    HIP_TRY(ctx, hipEventRecord(ctx->ou.ev[0], ctx->stream));
    if ((rc = opacity_update_stages(ctx, u))) return rc;
    ctx->pl.timed = ctx->pl.valid = true;
    ctx->nl.ran = ctx->nl.valid = ctx->nl.timed = ctx->nl.have;
    ctx->nc.valid = ctx->nl.have && ctx->nc.have;
    ctx->he.valid = ctx->he.timed = ctx->he.ran;
    ctx->ct.valid = ctx->ct.timed = ctx->ct.ran;
    return TARDIS_MC_OK;
}

int tardis_mc_update_plasma(TardisMcContext *ctx, const TardisMcPlasmaUpdate *p)
{
    if (!ctx || !p || !p->t_radiative || !p->dilution_factor) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid plasma update");
    TardisMcOpacityUpdate u{};  // the opacity stages' view of this call: no host populations, the solved electron densities installed by plasma_update_install
    u.j_blues_mode = p->j_blues_mode;
    u.t_radiative = p->t_radiative; u.dilution_factor = p->dilution_factor;
    u.time_of_simulation = p->time_of_simulation; u.volume = p->volume; u.w_epsilon = p->w_epsilon;
    u.detailed_optical_window = p->detailed_optical_window;
    int rc;
    if ((rc = plasma_update_check(ctx, p, &u))) return rc;
    if (ctx->ct.have && ctx->bf.continuum_field == 1 && !(ctx->bf.have && ctx->bf.rates_valid))
        return fail(ctx, TARDIS_MC_ERR_STATE, "update_plasma: the option continuum_field is 1 and no estimator rates are resident (tardis_mc_bf_estimator_rates)");
    if ((rc = plasma_update_prepare(ctx))) return rc;
    if ((rc = plasma_update_enqueue(ctx, p))) return rc;  // into the solve's own buffers
    if ((rc = plasma_update_status(ctx))) return rc;      // a failed solve ends here: the opacity state has not been written
    return plasma_update_install(ctx, &u);                // n_t, n_e and the opacity tables, only now
}

int tardis_mc_last_plasma_update_ms(TardisMcContext *ctx, double *out_boltzmann_ms, double *out_partition_ms, double *out_ionization_ms, double *out_population_ms)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->pl.timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no update_plasma has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *const out[4] = {out_boltzmann_ms, out_partition_ms, out_ionization_ms, out_population_ms};
    hipEvent_t ev[5];
    std::copy(ctx->pl.ev, ctx->pl.ev + 5, ev);
    int rc = event_intervals_ms(ctx, ev, 1, out);
    if (rc) return rc;
    // (the NLTE stage sits between the Boltzmann and the partition stage and has events of its own: tardis_mc_last_nlte_ms)
    if (ctx->nl.ran) ev[1] = ctx->nl.ev[2];
    if (ctx->he.ran) ev[1] = ctx->he.ev[1];  // (helium_relative_kernel, behind the NLTE stage: tardis_mc_last_helium_ms)
    return event_intervals_ms(ctx, ev + 1, 3, out + 1);
}

int tardis_mc_get_plasma(TardisMcContext *ctx, double *level_number_density, double *ion_number_density, double *partition_function, double *electron_density,
                         int32_t *iterations)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->pl.valid) return fail(ctx, TARDIS_MC_ERR_STATE, "get_plasma needs an update_plasma since the last set_opacity / update_opacity");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t S = (size_t)ctx->n_shells, I = (size_t)ctx->pl.ions;
    int rc;
    if ((rc = download_transposed(ctx, level_number_density, ctx->ou.n_t.as<double>(), (size_t)ctx->ou.levels))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, host_copy(ctx, {{(void *)ion_number_density, ctx->pl.n_ion.p, I * S * sizeof(double)},
                                 {(void *)partition_function, ctx->pl.z.p, I * S * sizeof(double)},
                                 {(void *)electron_density, ctx->pl.n_e.p, S * sizeof(double)}}, false));
    if (iterations) *iterations = ctx->pl.iterations;
    return TARDIS_MC_OK;
}

int tardis_mc_get_helium(TardisMcContext *ctx, double *relative_population, double *level_number_density)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->he.valid || !ctx->pl.valid) return fail(ctx, TARDIS_MC_ERR_STATE, "get_helium needs a successful update_plasma that ran with helium_treatment");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = ((size_t)ctx->he.n2 + 1) * (size_t)ctx->n_shells * sizeof(double);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, host_copy(ctx, {{(void *)relative_population, ctx->he.hp.p, bytes}, {(void *)level_number_density, ctx->he.v.p, bytes}}, false));
    return TARDIS_MC_OK;
}

int tardis_mc_last_helium_ms(TardisMcContext *ctx, double *out_relative_ms)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->he.timed || !ctx->pl.timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no update_plasma with helium_treatment has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *const out[1] = {out_relative_ms};
    return event_intervals_ms(ctx, ctx->he.ev, 1, out);
}

/* ---- photo-ionisation and heating estimators from the transport's segment log (bf_estimators.hpp) ---- */
int tardis_mc_check_bf_estimator_setup(const TardisMcBfEstimatorSetup *setup, int64_t n_shells)
{
    if (!setup || !setup->t_electrons) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "bf estimator setup: a pointer is missing");
    if (n_shells < 1) return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "bf estimator setup: n_shells = %lld is not positive", (long long)n_shells);
    for (int64_t s = 0; s < n_shells; ++s)
        if (!(std::isfinite(setup->t_electrons[s]) && setup->t_electrons[s] > 0.0))
            return fail(nullptr, TARDIS_MC_ERR_INVALID_ARGUMENT, "bf estimator setup: t_electrons[%lld] = %g is not finite and positive", (long long)s, setup->t_electrons[s]);
    return TARDIS_MC_OK;
}

int tardis_mc_set_bf_estimators(TardisMcContext *ctx, const TardisMcBfEstimatorSetup *setup)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!setup) {  // off: the tables go
        ctx->bf.have = ctx->bf.rates_valid = ctx->bf.seg_valid = false;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        release_buffers(ctx->bf.t_e, ctx->bf.tables, ctx->bf.totals, ctx->bf.rates);
        return TARDIS_MC_OK;
    }
    if (!ctx->have_geometry || !ctx->ct.have) return fail(ctx, TARDIS_MC_ERR_STATE, "set_geometry and set_continuum_data must precede set_bf_estimators");
    const size_t S = (size_t)ctx->n_shells, NC = (size_t)ctx->ct.continua;
    if (tardis_mc_check_bf_estimator_setup(setup, (int64_t)S)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "%s", g_create_error.c_str());
    // (a refused call has changed nothing up to here; from here on the previous setup, its tables and its rates are gone)
    ctx->bf.have = ctx->bf.rates_valid = ctx->bf.seg_valid = false;
    int rc;
    if ((rc = upload(ctx, ctx->bf.t_e, setup->t_electrons, S))) return rc;
    HIP_TRY(ctx, ctx->bf.tables.ensure(mc::BF_TABLES * NC * S * sizeof(double)));
    HIP_TRY(ctx, ctx->bf.totals.ensure(2 * sizeof(unsigned long long)));
    HIP_TRY(ctx, ctx->bf.rates.ensure(2 * NC * S * sizeof(double)));
    HIP_TRY(ctx, hipMemsetAsync(ctx->bf.tables.p, 0, mc::BF_TABLES * NC * S * sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->bf.totals.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's array is the source of an asynchronous copy)
    ctx->bf.have = true;
    return TARDIS_MC_OK;
}

static bool bf_resident(const TardisMcContext *ctx) { return ctx->bf.have && ctx->ct.have; }

int tardis_mc_get_bf_estimators(TardisMcContext *ctx, double *photo_ion, double *stim_recomb, double *bf_heating, double *stim_recomb_cooling, int64_t *statistics,
                                int64_t *n_records, int64_t *n_dropped)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!bf_resident(ctx)) return fail(ctx, TARDIS_MC_ERR_STATE, "get_bf_estimators needs tardis_mc_set_bf_estimators");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long totals[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpy(totals, ctx->bf.totals.p, sizeof totals, hipMemcpyDeviceToHost));
    if (n_records) *n_records = (int64_t)totals[0];
    if (n_dropped) *n_dropped = (int64_t)totals[1];
    if (totals[1] > 0)
        return fail(ctx, TARDIS_MC_ERR_STATE,
                    "photo-ionisation estimators: %llu segment records were dropped (%llu logged) since the last reset: the tables are incomplete; raise the option "
                    "segment_log_capacity or propagate fewer packets per call (the run is deterministic)", totals[1], totals[0]);
    const size_t n = (size_t)ctx->ct.continua * (size_t)ctx->n_shells;
    void *const host[mc::BF_TABLES] = {photo_ion, stim_recomb, bf_heating, stim_recomb_cooling, statistics};
    std::vector<CopyJob> jobs;
    for (int v = 0; v < mc::BF_TABLES; ++v) jobs.push_back({host[v], ctx->bf.tables.as<double>() + (size_t)v * n, n * sizeof(double)});
    HIP_TRY(ctx, host_copy(ctx, jobs, false));
    return TARDIS_MC_OK;
}

int tardis_mc_get_segment_log(TardisMcContext *ctx, double *nu, double *ed, int64_t *shell, int64_t capacity, int64_t *count)
{
    if (!ctx || !count || capacity < 0) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid segment log request");
    if (!ctx->bf.seg_valid) return fail(ctx, TARDIS_MC_ERR_STATE, "no segment log: the last tardis_mc_propagate ran without the options bf_estimators and segment_log_keep");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const mc::SegmentLog &L = ctx->problem_host.seglog;
    std::vector<unsigned> fill(L.n_chunks);
    HIP_TRY(ctx, hipMemcpy(fill.data(), L.chunk_fill, fill.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    int64_t total = 0;
    for (unsigned f : fill) total += std::min(f, L.chunk_rows);
    *count = total;
    if (total > capacity || total == 0) return TARDIS_MC_OK;  // (the columns only when they fit the caller's arrays)
    std::vector<mc::SegmentRecord> chunk(L.chunk_rows);
    int64_t j = 0;
    for (unsigned c = 0; c < L.n_chunks; ++c) {
        const unsigned f = std::min(fill[c], L.chunk_rows);
        if (!f) continue;
        HIP_TRY(ctx, hipMemcpy(chunk.data(), L.recs + (size_t)c * L.chunk_rows, f * sizeof(mc::SegmentRecord), hipMemcpyDeviceToHost));
        for (unsigned k = 0; k < f; ++k, ++j) {
            if (nu) nu[j] = chunk[k].comov_nu;
            if (ed) ed[j] = chunk[k].ed;
            if (shell) shell[j] = chunk[k].shell;
        }
    }
    return TARDIS_MC_OK;
}

int tardis_mc_debug_bf_accumulate(TardisMcContext *ctx, int64_t n, const double *nu, const double *ed, const int64_t *shell)
{
    if (!ctx || n < 0 || n > 0x7ffffff0LL || (n > 0 && (!nu || !ed || !shell))) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid segment records");
    if (!bf_resident(ctx)) return fail(ctx, TARDIS_MC_ERR_STATE, "debug_bf_accumulate needs tardis_mc_set_bf_estimators");
    if (ctx->n_shells > mc::EST_MAX_BINS)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "photo-ionisation estimators: more than %d shells (the pass groups the records by shell in LDS)", mc::EST_MAX_BINS);
    // everything the kernels index with is checked here, on the host
    std::vector<mc::SegmentRecord> recs((size_t)n);
    std::vector<unsigned> keys((size_t)n);
    for (int64_t e = 0; e < n; ++e) {
        if (!(std::isfinite(nu[e]) && nu[e] > 0.0)) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "segment records: nu[%lld] = %g is not finite and positive", (long long)e, nu[e]);
        if (!std::isfinite(ed[e])) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "segment records: ed[%lld] = %g is not finite", (long long)e, ed[e]);
        if (shell[e] < 0 || shell[e] >= (int64_t)ctx->n_shells)
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "segment records: shell[%lld] = %lld lies outside [0, %d)", (long long)e, (long long)shell[e], ctx->n_shells);
        recs[(size_t)e].comov_nu = nu[e]; recs[(size_t)e].ed = ed[e]; recs[(size_t)e].shell = (int)shell[e]; recs[(size_t)e].pad = 0;
        keys[(size_t)e] = (unsigned)shell[e];
    }
    if (n == 0) return TARDIS_MC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->bf.seg_valid = false;  // (the pass takes the sorted-slot buffer of the last call's log)
    ScopedDevBuf d_recs, d_keys, d_fill;
    const unsigned fill = (unsigned)n;
    const int rc = [&]() -> int {
        int rc1;
        if ((rc1 = upload(ctx, d_recs, recs.data(), (size_t)n))) return rc1;
        if ((rc1 = upload(ctx, d_keys, keys.data(), (size_t)n))) return rc1;
        if ((rc1 = upload(ctx, d_fill, &fill, 1))) return rc1;
        return bf_accumulate_pass(ctx, d_recs.as<mc::SegmentRecord>(), d_keys.as<unsigned>(), d_fill.as<unsigned>(), 1, fill, nullptr);  // one chunk holds them all
    }();
    (void)hipStreamSynchronize(ctx->stream);  // (nothing of the call is in flight when its scratch and the staging vectors go)
    return rc;
}

int tardis_mc_last_bf_estimator_ms(TardisMcContext *ctx, double *out_group_ms, double *out_accumulate_ms)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->bf.timed) return fail(ctx, TARDIS_MC_ERR_STATE, "no accumulate pass of the photo-ionisation estimators has been timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *const out[2] = {out_group_ms, out_accumulate_ms};
    return event_intervals_ms(ctx, ctx->bf.ev, 2, out);
}

int tardis_mc_bf_estimator_rates(TardisMcContext *ctx, double time_of_simulation, const double *volume)
{
    if (!ctx || !volume) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid estimator rates request");
    if (!bf_resident(ctx)) return fail(ctx, TARDIS_MC_ERR_STATE, "bf_estimator_rates needs tardis_mc_set_bf_estimators");
    if (!(std::isfinite(time_of_simulation) && time_of_simulation > 0.0))
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "bf_estimator_rates: time_of_simulation = %g is not finite and positive", time_of_simulation);
    const size_t S = (size_t)ctx->n_shells;
    for (size_t s = 0; s < S; ++s)
        if (!(std::isfinite(volume[s]) && volume[s] > 0.0))
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "bf_estimator_rates: volume[%zu] = %g is not finite and positive", s, volume[s]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->bf.rates_valid = false;
    ScopedDevBuf d_volume;
    const long long cells = ctx->ct.continua * (long long)S;
    int rc = upload(ctx, d_volume, volume, S);
    if (!rc) {
        hipLaunchKernelGGL(mc::bf_rates_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, (int)S, cells, time_of_simulation, H_PLANCK,
                           d_volume.as<double>(), ctx->bf.tables.as<double>(), ctx->bf.rates.as<double>());
        if (hipGetLastError() != hipSuccess) rc = fail(ctx, TARDIS_MC_ERR_HIP, "bf_rates_kernel failed to launch");
    }
    (void)hipStreamSynchronize(ctx->stream);  // (the scratch and the caller's array outlive the call's work)
    if (rc) return rc;
    ctx->bf.rates_valid = true;
    return TARDIS_MC_OK;
}

int tardis_mc_get_bf_estimator_rates(TardisMcContext *ctx, double *gamma_est, double *stim_est)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!bf_resident(ctx) || !ctx->bf.rates_valid) return fail(ctx, TARDIS_MC_ERR_STATE, "get_bf_estimator_rates needs tardis_mc_bf_estimator_rates");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t n = (size_t)ctx->ct.continua * (size_t)ctx->n_shells;
    HIP_TRY(ctx, host_copy(ctx, {{(void *)gamma_est, ctx->bf.rates.p, n * sizeof(double)}, {(void *)stim_est, ctx->bf.rates.as<double>() + n, n * sizeof(double)}}, false));
    return TARDIS_MC_OK;
}


/* ---- multi-GPU -------------------------------------------------------------------------------------- */
int tardis_mc_comm_get_unique_id(uint8_t out_id[TARDIS_MC_UNIQUE_ID_BYTES])
{
    std::string err;
    if (!out_id) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!load_rccl(err)) return fail(nullptr, TARDIS_MC_ERR_COMM, "%s", err.c_str());
    Id128 id;
    memset(&id, 0, sizeof id);
    int r = g_rccl.GetUniqueId(&id);
    if (r != 0) return fail(nullptr, TARDIS_MC_ERR_COMM, "ncclGetUniqueId failed (%d)", r);
    memcpy(out_id, id.bytes, TARDIS_MC_UNIQUE_ID_BYTES);
    return TARDIS_MC_OK;
}

int tardis_mc_comm_init(TardisMcContext *ctx, int rank, int world_size, const uint8_t id[TARDIS_MC_UNIQUE_ID_BYTES])
{
    if (!ctx || !id || world_size < 1 || rank < 0 || rank >= world_size)
        return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid communicator arguments");
    std::string err;
    if (!load_rccl(err)) return fail(ctx, TARDIS_MC_ERR_COMM, "%s", err.c_str());
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Id128 uid;
    memcpy(uid.bytes, id, TARDIS_MC_UNIQUE_ID_BYTES);
    int r = g_rccl.CommInitRank(&ctx->comm, world_size, uid, rank);
    if (r != 0) return fail(ctx, TARDIS_MC_ERR_COMM, "ncclCommInitRank failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    ctx->rank = rank;
    ctx->world = world_size;
    return TARDIS_MC_OK;
}

int tardis_mc_allreduce_estimators(TardisMcContext *ctx)
{
    if (!ctx) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    if (!ctx->es.est_valid) return fail(ctx, TARDIS_MC_ERR_STATE, "no estimators allocated");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drop_products(ctx, ESTIMATORS_CHANGED);
    int rc = reduce_estimator_copies(ctx);
    if (rc) return rc;
    if (!ctx->comm) {
        if (ctx->world <= 1) return TARDIS_MC_OK;  // single process, no communicator: nothing to reduce
        return fail(ctx, TARDIS_MC_ERR_STATE, "tardis_mc_comm_init has not been called");
    }
    EstLayout e = est_layout(ctx->es.est_S, ctx->es.est_L, ctx->es.est_G, ctx->es.est_copies);
    // ncclDouble = 8, ncclSum = 0; one in-place all-reduce over [J | nu_bar | v-hist | j_blue | Edotlu]
    int r = g_rccl.AllReduce(ctx->es.est.p, ctx->es.est.p, e.reduce_elems, 8, 0, ctx->comm, ctx->stream);
    if (r != 0) return fail(ctx, TARDIS_MC_ERR_COMM, "ncclAllReduce failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    return TARDIS_MC_OK;
}

// One-element all-reduce of (rank + 1): every rank must read N (N + 1) / 2 back -- the communicator really spans N ranks and sums.
__global__ void comm_check_fill_kernel(double *p, double v) { if (threadIdx.x == 0 && blockIdx.x == 0) *p = v; }

int tardis_mc_comm_check(TardisMcContext *ctx, int *out_ranks)
{
    if (!ctx || !out_ranks) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    *out_ranks = 0;
    if (!ctx->comm) return fail(ctx, TARDIS_MC_ERR_STATE, "tardis_mc_comm_init has not been called");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ScopedDevBuf cell;
    HIP_TRY(ctx, cell.ensure(sizeof(double)));
    hipLaunchKernelGGL(comm_check_fill_kernel, dim3(1), dim3(64), 0, ctx->stream, cell.as<double>(), (double)(ctx->rank + 1));
    hipError_t e = hipGetLastError();
    int r = e == hipSuccess ? g_rccl.AllReduce(cell.p, cell.p, 1, 8, 0, ctx->comm, ctx->stream) : 0;
    double got = 0.0;
    if (e == hipSuccess && r == 0) e = hipMemcpyAsync(&got, cell.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && r == 0) e = hipStreamSynchronize(ctx->stream);
    HIP_TRY(ctx, e);
    if (r != 0) return fail(ctx, TARDIS_MC_ERR_COMM, "ncclAllReduce failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    const double want = 0.5 * (double)ctx->world * (double)(ctx->world + 1);
    if (got != want)
        return fail(ctx, TARDIS_MC_ERR_COMM, "communicator self-check: the sum of (rank + 1) over %d ranks came back as %.17g, not %.17g", ctx->world, got, want);
    *out_ranks = ctx->world;
    return TARDIS_MC_OK;
}

/* ---- diagnostics (numerics parity tests) ------------------------------------------------------------- */
int tardis_mc_debug_eval(TardisMcContext *ctx, int op, const double *x, const double *y, double *out, int64_t n)
{
    if (!ctx || !x || !out || n <= 0) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (op == 100) {  // tests: the wave kernel's raw tracker records of the last call (mc::TrackerRecord, 8 doubles each), n / 8 of them from packet x[0] on
        const long long first = (long long)x[0], count = n / 8;
        if (n % 8 || first < 0 || first + count > ctx->pk.n_packets || !ctx->pk.li_rec.p || ctx->wv.last_tracker_defer < 0)
            return fail(ctx, TARDIS_MC_ERR_STATE, "debug_eval: no tracker records of a wave-kernel call for packets [%lld, %lld)", first, first + count);
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(out, (const char *)ctx->pk.li_rec.p + (size_t)first * 64, (size_t)count * 64, hipMemcpyDeviceToHost));
        return TARDIS_MC_OK;
    }
    if (op == 101) {  // tests: the resident prefix-sum tables as the kernels read them (tau_prefix.hpp, sweep_skip.hpp): n doubles of table x[0] from its double x[1] on
        const long long which = (long long)x[0], first = (long long)x[1];
        const long long S = ctx->n_shells, L = ctx->n_lines;
        const bool screening = ctx->sc.pfx_valid && ctx->sc.tau_pfx.p && ctx->sc.tau_rowsum.p;
        const bool skip = ctx->sw.nt_valid && ctx->sw.sk_valid && ctx->sw.nt_t.p && ctx->sw.sk_rowsum.p;
        const double host[3] = {ctx->sw.sk_margin, ctx->sw.sk_negative ? 1.0 : 0.0, (double)ctx->sw.nt_stride};
        const char *src = nullptr;  // (device; table 5 comes from the context)
        long long size = 0;         // doubles
        bool valid = false;
        switch (which) {
        case 0: valid = screening; src = (const char *)ctx->sc.tau_pfx.p; size = S * (L + 1); break;
        case 1: valid = screening; src = (const char *)ctx->sc.tau_rowsum.p; size = S; break;
        case 2: valid = skip; src = (const char *)ctx->sw.nt_t.p + (size_t)ctx->sw.sk_pn_off * 16; size = 2 * S * (L + 1); break;
        case 3: valid = skip; src = (const char *)ctx->sw.nt_t.p + (size_t)ctx->sw.sk_ct_off * 16; size = 2 * ((long long)(ctx->sw.nt_stride / 8) * S + 16); break;
        case 4: valid = skip; src = (const char *)ctx->sw.sk_rowsum.p; size = S; break;
        case 5: valid = skip; size = 3; break;
        default: return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "debug_eval: op 101 has no table %lld", which);
        }
        if (!valid) return fail(ctx, TARDIS_MC_ERR_STATE, "debug_eval: table %lld of op 101 is not built for the resident opacity state", which);
        if (first < 0 || first > size || n > size - first)
            return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "debug_eval: doubles [%lld, %lld) of table %lld, which holds %lld", first, first + (long long)n, which, size);
        if (which == 5) {
            for (int64_t i = 0; i < n; ++i) out[i] = host[first + i];
            return TARDIS_MC_OK;
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(out, src + (size_t)first * 8, (size_t)n * 8, hipMemcpyDeviceToHost));
        return TARDIS_MC_OK;
    }
    ScopedDevBuf dx, dy, dout, scratch;
    size_t nx = (op == 7) ? 1 : (size_t)n;
    HIP_TRY(ctx, dx.ensure(nx * 8));
    HIP_TRY(ctx, dout.ensure((size_t)n * 8));
    HIP_TRY(ctx, scratch.ensure(mc::MT_N * 4));
    HIP_TRY(ctx, hipMemcpy(dx.p, x, nx * 8, hipMemcpyHostToDevice));
    if (y) { HIP_TRY(ctx, dy.ensure((size_t)n * 8)); HIP_TRY(ctx, hipMemcpy(dy.p, y, (size_t)n * 8, hipMemcpyHostToDevice)); }
    int blocks = op == 7 ? 1 : (int)((n + 255) / 256);
    hipLaunchKernelGGL(debug_eval_kernel, dim3(blocks), dim3(op == 7 ? 64 : 256), 0, ctx->stream, op, dx.as<double>(),
                       y ? dy.as<double>() : nullptr, dout.as<double>(), (long long)n, scratch.as<uint32_t>());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return TARDIS_MC_OK;
}

int tardis_mc_debug_set_line_estimators(TardisMcContext *ctx, const double *j_blue, const double *edotlu)
{
    if (!ctx || !j_blue || !edotlu) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid debug_set_line_estimators arguments");
    if (!ctx->have_opacity || !ctx->have_config)
        return fail(ctx, TARDIS_MC_ERR_STATE, "debug_set_line_estimators: set_opacity and set_config must precede it");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    drop_products(ctx, ESTIMATORS_CHANGED);
    int rc = ensure_estimators(ctx);  // (allocated and zeroed if no call has done so yet: as tardis_mc_propagate finds them)
    if (rc) return rc;
    const size_t S = ctx->es.est_S, L = ctx->es.est_L;
    EstLayout e = est_layout(S, L, ctx->es.est_G, ctx->es.est_copies);
    // [n_lines, n_shells] -> copy 0 of the two shell-major tables, which lie one behind the other; the other copies are zeroed
    std::vector<double> tables(2 * S * L);
    for (size_t l = 0; l < L; ++l)
        for (size_t s = 0; s < S; ++s) {
            tables[s * L + l] = j_blue[l * S + s];
            tables[S * L + s * L + l] = edotlu[l * S + s];
        }
    double *base = ctx->es.est.as<double>();
    HIP_TRY(ctx, hipMemcpyAsync(base + e.jblue, tables.data(), 2 * S * L * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (ctx->es.est_copies > 1)
        HIP_TRY(ctx, hipMemsetAsync(base + e.jblue + e.copy_stride, 0, (size_t)(ctx->es.est_copies - 1) * e.copy_stride * sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the staging vector goes out of scope)
    return TARDIS_MC_OK;
}

int tardis_mc_debug_nlte_solve(TardisMcContext *ctx, int64_t n, int64_t n_systems, const double *m, const double *b, double *x, int32_t *status)
{
    if (!ctx || n <= 0 || n_systems <= 0 || n > 0x7ffffff0LL || n_systems > 65535 || !m || !b || !x || !status) return fail(ctx, TARDIS_MC_ERR_INVALID_ARGUMENT, "invalid debug_nlte_solve arguments");
    const long long N = n, S = n_systems, ld = nlte::leading_dimension(N), work = nlte::work_bytes(N) / 8;
    if (nlte::work_bytes(N) > nlte::MAX_SCRATCH_BYTES / S)
        return fail(ctx, TARDIS_MC_ERR_UNSUPPORTED, "debug_nlte_solve: %lld systems of %lld levels exceed the %lld bytes of scratch the plan allows", S, N, nlte::MAX_SCRATCH_BYTES);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one species of n levels, a system per "shell": the slabs as nlte_assemble_kernel leaves them (column-major, ld = n | 1, b behind the matrix)
    std::vector<double> slabs((size_t)(work * S), 0.0);
    for (long long s = 0; s < S; ++s) {
        double *M = slabs.data() + s * work;
        for (long long i = 0; i < N; ++i)
            for (long long j = 0; j < N; ++j) M[i + j * ld] = m[(s * N + i) * N + j];
        for (long long i = 0; i < N; ++i) M[ld * N + i] = b[s * N + i];
    }
    const int zero = 0, levels = (int)N;
    const long long slab0 = 0;
    const double one = 1.0;
    ScopedDevBuf scratch, ints, offset, g, lbf, x_t, st, pivrow;
    HIP_TRY(ctx, scratch.ensure(slabs.size() * sizeof(double)));
    HIP_TRY(ctx, ints.ensure(2 * sizeof(int)));
    HIP_TRY(ctx, offset.ensure(sizeof(long long)));
    HIP_TRY(ctx, g.ensure(sizeof(double)));
    HIP_TRY(ctx, lbf.ensure((size_t)(N * S) * sizeof(double)));
    HIP_TRY(ctx, x_t.ensure((size_t)(N * S) * sizeof(double)));
    HIP_TRY(ctx, st.ensure((size_t)S * sizeof(int)));
    HIP_TRY(ctx, pivrow.ensure((size_t)(N * S) * sizeof(int)));
    HIP_TRY(ctx, hipMemcpyAsync(scratch.p, slabs.data(), slabs.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ints.p, &zero, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ints.as<int>() + 1, &levels, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(offset.p, &slab0, sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(g.p, &one, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(st.p, 0, (size_t)S * sizeof(int), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(x_t.p, 0, (size_t)(N * S) * sizeof(double), ctx->stream));
    mc::NlteSolveArgs a{};
    a.S = (int)S; a.K = N; a.NX = N;
    a.list = ints.as<int>(); a.sp_k0 = ints.as<int>(); a.sp_x0 = ints.as<int>(); a.sp_n = ints.as<int>() + 1;  // species 0: first level 0, first row of x 0
    a.g = g.as<double>(); a.lbf_t = lbf.as<double>(); a.x_t = x_t.as<double>(); a.status = st.as<int>();
    a.scratch = scratch.as<double>(); a.slab = offset.as<long long>();
    std::vector<nlte::BlockedStep> steps;
    for (long long t = 0; t < nlte::panel_steps(N); ++t)
        steps.push_back({1u, (unsigned)S, (unsigned)nlte::trailing_strips(N, t * nlte::PANEL_COLUMNS), 1u, (unsigned)S});
    int rc;
    if ((rc = nlte_blocked_enqueue(ctx, a, steps, 1, pivrow.as<int>()))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(x, x_t.p, (size_t)(N * S) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(status, st.p, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TARDIS_MC_OK;
}

int tardis_mc_debug_microbench(TardisMcContext *ctx, int which, int64_t n_doubles, int iters, int blocks, double *out_ms)
{
    if (!ctx || !out_ms || n_doubles < 1024 || iters < 1 || blocks < 1) return TARDIS_MC_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ScopedDevBuf table, sink;
    HIP_TRY(ctx, table.ensure((size_t)n_doubles * 8));
    HIP_TRY(ctx, sink.ensure(8));
    HIP_TRY(ctx, hipMemsetAsync(table.p, 0, (size_t)n_doubles * 8, ctx->stream));
    for (int rep = 0; rep < 2; ++rep) {  // first launch warms up
            HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
        if (which == 15) hipLaunchKernelGGL(stream_copy_kernel, dim3(blocks), dim3(256), 0, ctx->stream, table.as<double>(), (long long)n_doubles, iters);
        else hipLaunchKernelGGL(microbench_kernel, dim3(blocks), dim3(256), 0, ctx->stream, which, table.as<double>(),
                                (long long)n_doubles, iters, sink.as<double>());
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop));
    }
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    *out_ms = ms;
    return TARDIS_MC_OK;
}

}  // extern "C"
