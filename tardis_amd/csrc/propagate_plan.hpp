// propagate_plan.hpp -- which kernel a propagate call runs on: the host's decision as a pure function.
//
// Standard C++ only (no HIP header, no context, no allocation, no device call): tests/test_propagate_plan.py compiles it
// with a host compiler and pins the rules.  tardis_mc_propagate fills a PlanInput from the context, calls plan_propagate,
// and -- the one step that needs the device -- builds the v-packet screening tables when the plan screens and they are
// not built yet; if they turn out to hold a negative optical depth it plans again with that fact.
#pragma once

#include "../../include/tardis_mc.h"

namespace plan {

// ---- debug_flags bits the HOST decides on (the others only reach the kernels)
constexpr int DBG_WALK_LANE_FP64 = 128;          // macro-atom jumps of the wave kernel: per-lane search in the fp64 running sums (cross-check)
constexpr int DBG_WALK_GROUP_FP64 = 8192;        // ... the cooperative group scan of the fp64 running sums / the fp64 search (cross-check)
constexpr int DBG_LONG_INSTANTIATIONS = 1048576; // the long (cross-check) instantiations of the wave kernel, for A/B
constexpr int DBG_NO_SCREENING = 33554432;       // no v-packet screening whatever the option says
constexpr int DBG_SKIP_FALLBACK = 536870912;     // block skip of the lane sweeps: every interval-mode decision counts as ambiguous, i.e. every skipped trace falls back (tests)
// the bits that read the wave kernel's profiling / test counters or ablation switches (mc::WV_DBG_FLAGS, propagate_wave.hpp: the host file asserts that the two are equal)
constexpr int DBG_WAVE_COUNTERS = 1 | 2 | 4 | 16 | 32 | 16384 | 32768 | 65536 | 131072 | 524288 | 2097152 | 4194304 | 8388608 | 16777216 | 134217728 | 268435456;
constexpr int DBG_FP64_WALKS = DBG_WALK_LANE_FP64 | DBG_WALK_GROUP_FP64;  // the compact walk tables are not used
// everything that needs a cross-check instantiation of the wave kernel: those have neither full tracking nor 64-bit table offsets
constexpr int DBG_WAVE_CROSS_CHECK = DBG_FP64_WALKS | DBG_LONG_INSTANTIATIONS | DBG_WAVE_COUNTERS;

struct PlanInput {
    // the shape
    int n_shells, n_lines, n_trans;
    long long n_packets;
    // the config fields that matter
    long long number_of_vpackets;
    double survival_probability;
    int enable_full_relativity, line_interaction_type;
    // the tables
    bool lines_sorted, prob_negative, have_walk_tables;
    // the options
    int variant, table_offsets, vpacket_screening;  // (-1: automatic, each)
    long long vpk_wave_min_packets;
    bool track_full;
    int debug_flags;
    // the screening tables: whether they are built, and whether they then hold a negative optical depth
    bool pfx_valid, pfx_negative;
    // option bf_estimators (the segment log of the photo-ionisation estimators): lives in the instantiations full tracking runs on, and routes as track_full does
    bool bf_estimators;
};

struct Plan {
    int variant;       // 0: lane-per-packet kernel; 1: group-per-packet kernel; 2: wave-owner kernel, group sweeps; 3: wave-owner kernel, lane sweeps (partial relativity;
                       // group sweeps under full relativity); 4: wave-owner kernel with the volley queue
    bool cooperative;  // variants 1 - 4 (else the lane kernel, whatever `variant` says)
    bool w64;          // the cooperative kernel's instantiation with 64-bit table offsets
    bool screen_on;    // v-packet screening on the prefix sums of tau (the caller builds the tables)
    int last_variant, last_table_offsets;  // what tardis_mc_last_variant / tardis_mc_last_table_offsets report
    int error;            // TARDIS_MC_OK, or the code the call fails with
    const char *message;  // ... and its text
};

inline Plan plan_error(Plan p, const char *message)
{
    p.error = TARDIS_MC_ERR_INVALID_ARGUMENT;
    p.message = message;
    return p;
}

inline Plan plan_propagate(const PlanInput &in)
{
    Plan p{};
    p.error = TARDIS_MC_OK;
    p.message = "";
    const bool vpk = in.number_of_vpackets > 0;
    const bool small_shape = in.n_shells <= 30 && in.n_lines <= 100000;  // (the tardis_example shape)
    // the cooperative kernel relies on a sorted line list (bucket index, monotone stopping predicate); anything else --
    // which the reference would also mis-handle -- goes through the sequential lane-per-packet kernel
    // automatic choice: the wave-owner kernel (its pooled v-packet volleys take up to 32 v-packets per volley: one bit of
    // the roulette predictor each; beyond that the lane-per-packet kernel); lane sweeps where their bounds hold (partial
    // relativity) and no volleys run.  On the macroatom shape (5e5 lines, ~36 lines per trace) the lane sweeps overtook the
    // group sweeps once the walk ran per lane on the compact tables and a call became epochs over one packet supply
    // (19.3 vs 13.4 Mpkt/s at 2e7 packets): the group sweeps' 280 instructions per 16-line step had become the bound.
    // v-packet screening (tau_prefix.hpp): with the default survival probability 0 a v-packet whose optical depth passes
    // tau_russian is dropped whatever the depth was -- decided from prefix sums, two reads per shell crossing.
    // It pays where a shell crossing passes many lines (two prefix reads against ~40 optical depths on the 100-shell x 5e5-line
    // shape: 1.7x - 2.1x); on the tardis_example shape (~12 lines per crossing, most v-packets leave the grid alive) the
    // screening is a second trace on top of the first: -36 % (profiles/r03_vpacket_screening.txt).  "vpacket_screening" 0 / 1
    // overrides the automatic choice.
    // (decided from cheap predicates first: whether the tables are BUILT depends on the kernel the call ends up on -- calls that
    // take the lane kernel (more than 32 v-packets per volley, unsorted line list, variant 0) never read them: S x (L + 1)
    // doubles, 400 MB at the configs[4] shape, and a blocking read-back of the negative-depth flag)
    const bool screen_auto = (long long)in.n_lines >= 2500LL * (long long)in.n_shells;
    const bool screen = in.vpacket_screening < 0 ? screen_auto : in.vpacket_screening != 0;
    // (a negative optical depth: no screening -- the prefix sums would not bound the serial sum)
    p.screen_on = vpk && in.survival_probability == 0.0 && screen && !(in.debug_flags & DBG_NO_SCREENING) && !(in.pfx_valid && in.pfx_negative);
    const bool prefer_lane_sweeps = !in.enable_full_relativity && !vpk;
    // With v-packets the wave kernel's pooled volleys win where a v-packet crosses few shells and few lines (the tardis_example
    // shape: 8.0 vs 5.2 Mpkt/s); on finer grids and longer line lists the group kernel -- every lane of a packet's group traces one
    // v-packet of the volley, no speculation on the draw positions -- was measured 1.2x to 2.2x ahead
    // (profiles/r02_vpacket_kernel_choice.txt).
    // With the screening the v-packets of such a shape are half of the wave kernel's pass instead of nearly all of it, and its
    // lane-per-packet event code wins once the call is long enough to amortise its drain: 1.39-1.46 vs 1.33 Mpkt/s at 3e6 packets of
    // the configs[4] shape, 0.63 vs 1.10 at 1e6 (profiles/r03_vpacket_screening.txt).
    // (round 5: with the finer bucket index, the carried walks and the cut-off of the volley phases the wave kernel is ahead from 1e6 packets per call on:
    // 1.20 vs 1.81 s there, 4.5 vs 12.7 s at 1e7 -- and still at 1e5, 0.63 vs 0.74 s: profiles/r05_vpacket_kernel_choice.txt; the threshold was 2.5e6 in round 3)
    // (the automatic choice counts on the screening for long calls of the wave kernel: where the tables turn out negative, the second plan takes what it picks without)
    const bool vpk_wave = vpk && (small_shape || (p.screen_on && in.n_packets >= in.vpk_wave_min_packets));
    const int wave_auto = prefer_lane_sweeps ? 3 : 2;
    int variant = in.variant >= 0 ? in.variant : ((vpk && in.number_of_vpackets > 32) ? 0 : (vpk ? (vpk_wave ? 2 : 1) : wave_auto));
    auto is_wave = [](int v) { return v == 2 || v == 3 || v == 4; };
    // (the rules below apply in this order)
    if (in.prob_negative && (variant == 2 || variant == 3)) variant = 1;  // (the wave kernel searches the monotone running sums)
    // Russian roulette with survivors (virtual_packet.py:221-232; the reference's SURVIVAL_PROBABILITY is 0 in every run, nothing
    // sets it): a surviving v-packet may play again in a later shell, so its draw count is unbounded, while the wave kernel's
    // pooled volleys budget one roulette draw per v-packet -- such problems run on the group kernel
    if (vpk && in.survival_probability > 0.0 && is_wave(variant)) variant = 1;
    // variant 4: the wave kernel with the volley queue (v-packets traced by vpacket_trace_kernel between its launches); without
    // v-packets there is nothing to queue
    if (variant == 4 && !vpk) variant = wave_auto;
    if (in.prob_negative && variant == 4) variant = 1;
    // full r-packet tracking: the wave-owner kernel with group sweeps (variant 2, its default launch shape) where it can run the call --
    // sorted lines, monotone probabilities, no surviving v-packets, at most 32 v-packets, the compact walk tables, no cross-check flags --
    // else the lane kernel (variants 1, 3 and 4 are not instrumented).  The segment log of the photo-ionisation estimators sits in the same instantiations.
    const bool instrumented = in.track_full || in.bf_estimators;
    if (instrumented) {
        const bool wave_ok = in.lines_sorted && !in.prob_negative && !(vpk && (in.number_of_vpackets > 32 || in.survival_probability > 0.0)) &&
                             (in.line_interaction_type == 0 || in.have_walk_tables) && !(in.debug_flags & DBG_WAVE_CROSS_CHECK) && in.n_packets < (1LL << 31);
        variant = (wave_ok && variant != 0) ? 2 : 0;
    }
    bool cooperative = in.lines_sorted && (variant == 1 || is_wave(variant)) && (!vpk || in.number_of_vpackets <= 32);
    // 64-bit row offsets (option table_offsets): the lane kernel always has them; the cooperative kernels have WIDE instantiations, used where
    // a shell-major table reaches 2^28 entries (or always, option 1) -- the 32-bit ones save registers on the hot path
    const bool big_tables = (long long)in.n_shells * in.n_lines >= (1LL << 28) || (long long)in.n_shells * in.n_trans >= (1LL << 28);
    bool w64 = false;
    if (cooperative && (in.table_offsets == 1 || (in.table_offsets < 0 && big_tables))) {
        if (variant == 4)
            return plan_error(p, "variant 4 (the volley queue) has no 64-bit table offsets: n_shells * n_lines or n_shells * n_trans "
                                 "reaches 2^28, or option table_offsets is 1; use the automatic variant");
        if (is_wave(variant) && (in.debug_flags & DBG_WAVE_CROSS_CHECK))
            return plan_error(p, "the cross-check instantiations of the wave kernel (debug flags 128, 8192, 1048576 and the counter "
                                 "flags) have no 64-bit table offsets");
        if (is_wave(variant) && (long long)in.n_shells * in.n_lines >= (1LL << 32)) {
            // (the line-visit log of the wave kernels indexes (shell, line) in 32 bits; the group kernel adds its terms directly)
            if (in.variant >= 0)
                return plan_error(p, "n_shells * n_lines reaches 2^32: the line-visit log of the wave kernels (variants 2-4) "
                                     "indexes (shell, line) in 32 bits; use variant 1 or the automatic variant");
            if (instrumented) { cooperative = false; variant = 0; }  // (the group kernel has no full tracking)
            else { variant = 1; w64 = true; }
        } else if (is_wave(variant) && in.line_interaction_type != 0 && !in.have_walk_tables) {
            // (the compact walk tables were not built for these tables: the fp64 walks are only in the 32-bit cross-check instantiations)
            cooperative = false;
            variant = 0;
        } else
            w64 = true;
    }
    if (cooperative && big_tables && !w64)
        return plan_error(p, "n_shells * n_lines or n_shells * n_trans reaches 2^28, the limit of the cooperative kernels' 32-bit "
                             "table offsets, and option table_offsets is 0");
    p.variant = variant;
    p.cooperative = cooperative;
    p.w64 = w64;
    p.last_table_offsets = (w64 || !cooperative) ? 64 : 32;
    p.last_variant = cooperative ? ((variant == 3 && in.enable_full_relativity) ? 2 : variant) : 0;
    if (!cooperative) p.screen_on = false;  // (the lane kernel traces line by line)
    return p;
}

// ---- the block skip of the lane sweeps (sweep_skip.hpp): whether a call's sweeps clear whole 8-line blocks on the coarse table.  Decided once the wave
// kernel's instantiation is known: the code is compiled into the two production lane-sweep forms on the interleaved table (sixteen waves at eight loads per step,
// twelve waves at ten), and its proof needs what the interleaved table's lean proof needs, plus line
// scattering (a trace without it never stops on a line: nothing to gain, and lane_exact_line's code 3 is what the interval check is about).
struct SkipInput {
    int sweep_skip;            // the option: -1 automatic, 0 off, 1 on where allowed
    bool lane_sweep, vpk, full_relativity, wide, cross_check, shell_log, full_tracking;
    int waves_per_simd, nt;    // the instantiation: waves per SIMD it is compiled for; 0 separate tables, 1 interleaved, 2 aligned runs
    bool line_scattering;
    bool nt_negative, pfx_negative;  // a negative or non-finite optical depth, seen by the interleaved table's / the prefix sums' builder
    bool twelve_wave_skip;     // the build's twelve-wave instantiation on the interleaved table carries the skip as well (TMC_SWEEP_SKIP_12, propagate_wave.hpp)
};
inline bool plan_sweep_skip(const SkipInput &in)
{
    if (in.sweep_skip == 0) return false;
    // (the twelve-wave form under the same conditions as the sixteen-wave one)
    const bool instantiation = in.waves_per_simd == 4 || (in.waves_per_simd == 3 && in.twelve_wave_skip);
    return in.lane_sweep && !in.vpk && !in.full_relativity && !in.wide && !in.cross_check && !in.shell_log && !in.full_tracking && instantiation &&
           in.nt == 1 && in.line_scattering && !in.nt_negative && !in.pfx_negative;
}

}  // namespace plan
