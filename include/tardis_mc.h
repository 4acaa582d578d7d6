/* tardis_mc.h -- C ABI of the MI355X-native Monte Carlo packet-propagation engine (libtardis_mc_hip.so).
 *
 * This is the drop-in boundary for ONE path of tardis-sn/tardis: the Monte Carlo main loop
 *     montecarlo_transport_with_vpackets(packet_collection, geometry_state_numba, time_explosion,
 *         opacity_state_numba, montecarlo_configuration, spectrum_frequency_grid, trackers,
 *         number_of_vpackets, show_progress_bars, packet_propagation_function)
 *       -> (v_packets_energy_hist, vpacket_tracker, estimators_bulk, estimators_line)
 *     tardis/transport/montecarlo/modes/montecarlo_transport.py:238-373
 * as called from MCTransportSolverClassic.run_classic
 *     tardis/transport/montecarlo/modes/classic/solver.py:223-234.
 * The reference has no FFI for this path (it is a Numba @njit function), so these entry points are what a
 * ctypes binding inside run_classic would bind; see INTEGRATION.md for the stub.
 *
 * Conventions
 *   - plain pointers and sizes only; all reals are float64, all integers int64 (the reference's dtypes);
 *   - every array is caller-owned, C-contiguous, and is neither retained nor freed by the library after
 *     the call that takes it returns (inputs are copied to HBM; outputs are written in place);
 *   - 2-D arrays use the REFERENCE's layout: tau_sobolev[L,S], transition_probabilities[T,S],
 *     j_blue[L,S], Edotlu[L,S], row-major (line index slow, shell index fast).  The engine keeps its own
 *     shell-major copies in HBM;
 *   - functions return 0 on success or a negative TARDIS_MC_ERR_* code; tardis_mc_last_error() gives text;
 *   - a context is bound to one HIP device and one stream; entry points are not re-entrant per context.
 */
#ifndef TARDIS_MC_H
#define TARDIS_MC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TARDIS_MC_ABI_VERSION 2  /* 2 (round 6): + tardis_mc_comm_check, tardis_mc_stream_results, tardis_mc_streamed_packets, tardis_mc_last_compactions, microbench 15;
                                    * additive since: tardis_mc_formal_integral_interpolated, tardis_mc_interpolated_source,
                                    * tardis_mc_packet_decomposition, tardis_mc_decomposition_path, option "vpacket_last_interaction",
                                    * TardisMcVpacketLog, tardis_mc_get_vpacket_log, tardis_mc_vpacket_decomposition;
                                    * the plasma, NLTE, continuum and cooling entry points; TardisMcBfEstimatorSetup and the eight
                                    * tardis_mc_*bf_estimator* / tardis_mc_get_segment_log / tardis_mc_debug_bf_accumulate entry points, the
                                    * options "bf_estimators", "segment_log_*", "continuum_field".  The number stays 2 for these additions, as for
                                    * the earlier ones: the suite pins it, and nothing that existed changed.  A build older than a binding
                                    * therefore fails when the binding looks a new symbol up, not at the version check. */

enum {
    TARDIS_MC_OK = 0,
    TARDIS_MC_ERR_INVALID_ARGUMENT = -1,
    TARDIS_MC_ERR_HIP = -2,          /* HIP runtime failure (no device, OOM, launch failure) */
    TARDIS_MC_ERR_MONTECARLO = -3,   /* reference: MonteCarloException("nu difference is less than 0.0"),
                                        transport/geometry/calculate_distances.py:105-106 */
    TARDIS_MC_ERR_MACRO_ATOM = -4,   /* reference: MacroAtomError, transport/montecarlo/macro_atom.py:94-99 */
    TARDIS_MC_ERR_UNSUPPORTED = -5,  /* transition type outside classic mode (continuum processes) */
    TARDIS_MC_ERR_COMM = -6,         /* RCCL failure */
    TARDIS_MC_ERR_STATE = -7         /* call order violated (e.g. propagate before set_opacity) */
};

/* LineInteractionType, transport/montecarlo/interaction_events.py:220-223 */
enum { TARDIS_MC_LINE_SCATTER = 0, TARDIS_MC_LINE_DOWNBRANCH = 1, TARDIS_MC_LINE_MACROATOM = 2 };

/* MonteCarloConfiguration fields the classic path reads, transport/montecarlo/configuration/base.py:11-49,
 * plus SIGMA_THOMSON (configuration/constants.py:3; 1e-200 when electron scattering is disabled,
 * modes/classic/solver.py:291-300). */
typedef struct TardisMcConfig {
    int32_t enable_full_relativity;        /* ENABLE_FULL_RELATIVITY */
    int32_t line_interaction_type;         /* LINE_INTERACTION_TYPE */
    int32_t disable_line_scattering;       /* DISABLE_LINE_SCATTERING */
    int32_t enable_vpacket_tracking;       /* ENABLE_VPACKET_TRACKING */
    int64_t number_of_vpackets;            /* NUMBER_OF_VPACKETS */
    double survival_probability;           /* SURVIVAL_PROBABILITY (default 0.0) */
    double vpacket_tau_russian;            /* VPACKET_TAU_RUSSIAN (default 10.0) */
    double vpacket_spawn_start_frequency;  /* VPACKET_SPAWN_START_FREQUENCY */
    double vpacket_spawn_end_frequency;    /* VPACKET_SPAWN_END_FREQUENCY */
    double sigma_thomson;                  /* SIGMA_THOMSON [cm^2] */
    int64_t n_spectrum_grid;               /* len(spectrum_frequency_grid) = bins + 1 */
    const double *spectrum_frequency_grid; /* uniform ascending edges [Hz] */
} TardisMcConfig;

/* PacketCollection inputs, transport/montecarlo/packets/packet_collections.py:14-76 */
typedef struct TardisMcPackets {
    int64_t n_packets;
    const double *initial_radii;
    const double *initial_nus;
    const double *initial_mus;
    const double *initial_energies;
    const int64_t *packet_seeds;           /* MT19937 init_genrand seed per packet, in [0, 2^32-2] */
} TardisMcPackets;

/* NumbaHomologousRadial1DGeometry, model/geometry/radial1d_homologous.py:199-226 */
typedef struct TardisMcGeometry {
    int64_t n_shells;
    const double *r_inner;
    const double *r_outer;
    double time_explosion;
} TardisMcGeometry;

/* OpacityStateNumba fields used by classic mode, opacities/opacity_state_numba.py:14-196 */
typedef struct TardisMcOpacity {
    int64_t n_lines;                       /* L */
    int64_t n_shells;                      /* S */
    int64_t n_transitions;                 /* T (1 for "scatter" dummies) */
    int64_t n_macro_block_edges;           /* len(macro_block_edge_index) = levels + 1 */
    const double *electron_density;        /* [S] */
    const double *line_list_nu;            /* [L] descending */
    const double *tau_sobolev;             /* [L,S] */
    const double *transition_probabilities;/* [T,S] */
    const int64_t *line2macro_level_upper; /* [L] */
    const int64_t *macro_block_edge_index; /* [levels+1] */
    const int64_t *transition_type;        /* [T] */
    const int64_t *destination_level_id;   /* [T] */
    const int64_t *transition_line_id;     /* [T] */
} TardisMcOpacity;

/* Work counters accumulated by the kernels (bytes = 48 V + 56 E + 8 M + 16 Vv + 56 P) */
enum {
    TARDIS_MC_CNT_LINE_VISITS = 0,         /* V: iterations of the trace_packet line loop */
    TARDIS_MC_CNT_EVENTS = 1,              /* E: trace_packet calls */
    TARDIS_MC_CNT_MACRO_TRANSITIONS = 2,   /* M: transition probabilities examined */
    TARDIS_MC_CNT_VPACKET_LINE_VISITS = 3, /* Vv */
    TARDIS_MC_CNT_VPACKETS = 4,            /* v-packets traced */
    TARDIS_MC_CNT_RNG_DRAWS = 5,           /* MT19937 doubles consumed */
    TARDIS_MC_CNT_PACKETS = 6,             /* P */
    TARDIS_MC_CNT_RESERVED = 7,
    TARDIS_MC_N_COUNTERS = 8
};

/* Outputs.  Any pointer may be NULL to skip that output (sizes in comments). */
typedef struct TardisMcResult {
    double *output_nus;                    /* [P]  packet_collection.output_nus */
    double *output_energies;               /* [P]  +e EMITTED / -e REABSORBED (montecarlo_transport.py:70-90) */
    double *j_estimator;                   /* [S]  EstimatorsBulk.mean_intensity_total */
    double *nu_bar_estimator;              /* [S]  EstimatorsBulk.mean_frequency */
    double *j_blue_estimator;              /* [L,S] EstimatorsLine.mean_intensity_blueward */
    double *edotlu_estimator;              /* [L,S] EstimatorsLine.energy_deposition_line_rate */
    double *v_packets_energy_hist;         /* [n_spectrum_grid] */
    /* TrackerLastInteraction as SoA, packets/trackers/tracker_last_interaction.py:8-254 */
    double *li_radius, *li_nu, *li_energy;                 /* [P] each */
    double *li_before_nu, *li_before_mu, *li_before_energy;
    double *li_after_nu, *li_after_mu, *li_after_energy;
    int64_t *li_shell_id, *li_interaction_type;
    int64_t *li_line_absorb_id, *li_line_emit_id, *li_interactions_count;
    /* consolidated v-packet log (only when enable_vpacket_tracking), packet order */
    int64_t vpacket_log_capacity;          /* in: entries available in the four arrays below */
    int64_t vpacket_log_count;             /* out: entries produced (may exceed capacity -> truncated) */
    double *vpacket_nus, *vpacket_energies, *vpacket_initial_mus, *vpacket_initial_rs;
    int64_t counters[TARDIS_MC_N_COUNTERS];
    int64_t first_error_packet;            /* out: lowest packet index that failed, or -1 */
    int32_t error_code;                    /* out: 0 or TARDIS_MC_ERR_MONTECARLO / _MACRO_ATOM / _UNSUPPORTED */
    int32_t reserved;
} TardisMcResult;

/* Full r-packet tracking (option "track_full" = 1; TrackerFull, packets/trackers/tracker_full.py): one row per trace_packet
 * outcome of every packet, in order, in a CSR layout -- packet p's rows are [offsets[p], offsets[p + 1]).  Row fields:
 * event_id (ordinal within the packet), interaction_type (1 BOUNDARY, 2 LINE, 4 ESCATTERING), status after the event
 * (0 IN_PROCESS, 1 EMITTED, 2 REABSORBED), shell_id (shell of the event), after_shell_id (shell after it: n_shells or -1 for a
 * crossing out of the grid), radius, before_* (lab frame on arrival, after move_r_packet), after_* (after the event; equal to
 * before_* for BOUNDARY rows), line_absorb_id / line_emit_id (LINE rows, -1 otherwise).  V-packets produce no rows. */
typedef struct TardisMcEventLog {
    int64_t capacity;                      /* in: rows available in each column array below */
    int64_t count;                         /* out: rows of the last propagate call (offsets[n_packets]) */
    int64_t dropped;                       /* out: rows the device pool could not hold (option event_log_capacity too small) */
    int64_t *offsets;                      /* [n_packets + 1], or NULL */
    /* [count] each, or NULL; written only when dropped == 0 and count <= capacity */
    int64_t *event_id, *interaction_type, *status, *shell_id, *after_shell_id, *line_absorb_id, *line_emit_id;
    double *radius, *before_nu, *before_mu, *before_energy, *after_nu, *after_mu, *after_energy;
} TardisMcEventLog;

/* The emitted spectrum decomposed by last interaction (tardis_mc_packet_decomposition below). */
typedef struct TardisMcDecomposition {
    /* in */
    int64_t n_classes;            /* C, 1 <= C < 2^31 */
    const int64_t *line_class;    /* [n_lines], every value in [0, C): the caller's grouping of lines (species, ion, ...) */
    double time_of_simulation;    /* > 0 */
    double nu_start, nu_end;      /* packet filter on output_nu: nu_start < nu < nu_end (0, inf = all) */
    /* out, host, any may be NULL.  B = n_spectrum_grid - 1, S = n_shells, L = n_lines */
    double *emission;             /* [C*B] class-major */
    double *absorption;           /* [C*B] class-major */
    double *no_interaction;       /* [B] */
    double *electron_scatter;     /* [B] */
    int64_t *shell_packets;       /* [(C+1)*S]: rows 0..C-1 by emit class, row C electron scattering; column li_shell_id */
    int64_t *line_emit_packets;   /* [L] */
    int64_t *line_absorb_packets; /* [L] */
    /* out */
    int64_t n_selected, n_line, n_electron_scatter, n_no_interaction;
} TardisMcDecomposition;

/* The v-packet log of the last tardis_mc_propagate (ENABLE_VPACKET_TRACKING), consolidated on the device: packet order, then spawn order
 * -- the order of the vpacket_* arrays of TardisMcResult -- in a CSR layout, packet p's entries are [offsets[p], offsets[p + 1]).  The six
 * last_interaction_* columns (option "vpacket_last_interaction") hold the spawning r-packet's last-interaction tracker at the time of the
 * volley, i.e. its last non-boundary interaction before it: in_nu (the tracker's before_nu), in_r (the radius of that interaction; bit for
 * bit the entry's initial_r, the volley is traced from there), type (2 LINE, 4 ESCATTERING), in_id (absorb line), out_id (emit line),
 * shell_id.  The entries of the launch volley have type = in_id = out_id = shell_id = -1 and in_nu = in_r = NaN, the conventions of
 * LastInteractionTrackers. */
typedef struct TardisMcVpacketLog {
    int64_t capacity;        /* in: entries available in each column */
    int64_t count;           /* out: entries the last propagate call produced */
    int64_t *offsets;        /* [n_packets + 1] or NULL: packet p's entries are [offsets[p], offsets[p+1]) */
    int64_t *source_packet;  /* [count] each below, any may be NULL */
    double *nus, *energies, *initial_mus, *initial_rs;
    double *last_interaction_in_nu, *last_interaction_in_r;
    int64_t *last_interaction_type, *last_interaction_in_id, *last_interaction_out_id, *last_interaction_shell_id;
} TardisMcVpacketLog;

typedef struct TardisMcContext TardisMcContext;

/* ---- library / device ---------------------------------------------------------------------------- */
int tardis_mc_abi_version(void);
int tardis_mc_device_count(void);
/* Create a context on HIP device `device_id` (one process per GPU: pass LOCAL_RANK). */
int tardis_mc_create(int device_id, TardisMcContext **out_ctx);
void tardis_mc_destroy(TardisMcContext *ctx);
const char *tardis_mc_last_error(const TardisMcContext *ctx);   /* ctx may be NULL: last create() error */

/* Tunables.  name: "track_last_interaction" (0/1, default 1), "vpacket_log_capacity" (entries),
 * "vpacket_last_interaction" (0/1, default 0: every v-packet log entry also carries the last-interaction tracker of its r-packet at the
 * time of the volley, 24 B more per entry on the device, TardisMcVpacketLog; needs ENABLE_VPACKET_TRACKING, v-packets and a tracker --
 * a propagate call with it, v-packet tracking and neither "track_last_interaction" nor "track_full" fails with TARDIS_MC_ERR_INVALID_ARGUMENT
 * before anything is launched; without v-packet tracking it does nothing; per-packet results do not depend on it),
 * "track_full" (0/1, default 0: full r-packet tracking, TardisMcEventLog; whatever "variant" says, a call runs on the wave-owner
 * kernel with group sweeps, variant 2, where that can run it -- sorted lines, monotone probabilities, <= 32 v-packets and no surviving
 * ones, no cross-check debug flags -- else on the lane-per-packet kernel, variant 0), "event_log_capacity" (rows the device log holds, 0 = automatic: 32 per packet; a call whose log
 * overflows drops rows, keeps the counts exact and reports them through tardis_mc_get_event_log), "event_log_max_bytes" (bound on
 * the log's device memory, default 16 GiB: 96 B per pool row + 112 B per row for the columns + 12 B per packet; a call over it fails
 * with TARDIS_MC_ERR_INVALID_ARGUMENT),
 * "table_offsets" (row offsets of the cooperative kernels, variants 1-3: -1, the default, 64-bit only where n_shells * n_lines or
 * n_shells * n_trans reaches 2^28; 0 always 32-bit -- such tables then fail with TARDIS_MC_ERR_INVALID_ARGUMENT; 1 always 64-bit.  Per-packet
 * results do not depend on it.  The 64-bit wave kernels need n_shells * n_lines < 2^32 (beyond, the automatic choice runs variant 1, or variant 0
 * with "track_full"; a forced variant 2-4 fails) and the compact walk tables (macroatom / downbranch; where those are not built the call runs on
 * variant 0); a forced variant 4 and the wave kernel's cross-check debug flags on 64-bit offsets fail),
 * "variant" (kernel variant: -1 automatic, 0 lane-per-packet, 1 group-per-packet, 2 wave-owner with group sweeps, 3 wave-owner
 * with lane sweeps, 4 wave-owner with the volley queue: v-packets traced by a kernel of their own between its launches --
 * never the automatic choice; falls back to 2/3 without v-packets and to 1 with a survival probability > 0),
 * "vq_min_items" (variant 4: switch the queue off for the rest of a call once a launch requests fewer v-packets; -1 automatic,
 * 0 never), "vq_min_active", "vq_oversubscribe", "vq_tracer_waves_per_simd" (variant 4 launch shape),
 * "lane_sweep_min_active" / "lane_sweep_max_steps" (when variant 3 leaves its sweep phase; lane_sweep_min_active < 0: automatic --
 * 8, or 12 where most macro-atom blocks are entered through hot sectors),
 * "walk_min_active" (macroatom walks are carried over to the next pass once this few lanes still walk; -1 never, < -1 automatic:
 * 8 / 12 likewise),
 * "tracker_defer" (last-interaction tracker of variant 3 without v-packets: 1, the default: a packet's record of its last interaction stays on
 * the chip and is written once, when the packet ends; 0: the record is written at every interaction, as the other variants do.  A problem of more
 * than 2^15 shells or 2^24 - 1 lines runs as with 0.  Results do not depend on it; tardis_mc_last_tracker_defer tells what a call ran with),
 * "tracker_pack_max_lines" (tests: problems of more lines than this run as with "tracker_defer" 0; 0, the default: only the real bound),
 * "rng_complete" (variant 3 without v-packets: 1: once a packet is past the first 624 words of its MT19937 stream, the wave that holds it produces the
 * rest of the generation the packet is in at the top of a pass, 64 words per round, and the packet's refills out of that generation read 32 bytes and
 * store nothing, csrc/mt_generation.hpp; 0: every refill regenerates its 8 words itself.  1 is the default.  Results do not depend on it;
 * the other kernels ignore it),
 * "sweep_skip" (variant 3 without v-packets, the lane sweeps on the interleaved table, sixteen-wave and twelve-wave form alike ("ls_waves_per_simd"): a trace
 * proves whole aligned blocks of 8 lines harmless on a coarse table of prefix sums of the optical depths, seven blocks per step at sixteen waves and nine at
 * twelve, and sweeps line by line -- eight and ten lines per step -- only from the block that may stop it,
 * csrc/sweep_skip.hpp; -1, the default: automatic; 0 off; 1 on where the call allows it -- partial relativity, 32-bit table offsets, line scattering
 * enabled, no negative or non-finite optical depth, not the shell-sorted log or the cross-check instantiations.  Results do not depend on it;
 * tardis_mc_last_sweep_skip tells what a call ran with; debug flag 536870912 (tests) makes every skipped trace fall back to the line-by-line sweep),
 * "sweep_start_held" (calls whose lane sweeps run with "sweep_skip" only, ignored elsewhere: 1: an emission that a hot sector of the macro-atom walk decided
 * reads its line's frequency from the skip's {frequency, prefix sum} table together with the neighbouring entry, the start entry of the trace that
 * follows, and that trace's coarse steps do not load the entry again; 0: the frequency is read from the interleaved table and every trace loads its
 * start entry; -1, the default: automatic, on where the call's sweeps skip.  Results and work counters do not depend on it),
 * "log_tail_split" (1, the default: a call whose line-visit log fits one epoch is split where the drain of its longest-lived packets
 * begins -- "log_tail_packets" (8) packets' worth of traces per lane before the estimated end -- so that the estimator passes over
 * the bulk run beside the drain; 0 off), "log_chunk_records" (records per chunk of the log's pool, <= 4096 by default),
 * "est_pipeline" (how an epoch's line-visit log becomes j_blue / Edotlu: 1, the default: the records are partitioned by shell and then
 * by (shell, 2048-line tile) in two LDS-staged passes and added up in order, csrc/estimator_partition.hpp; 0: an index of the records is
 * counting-sorted and the records are fetched through it, csrc/estimator_log.hpp -- also what runs for line lists of more than 2e6 lines
 * or more than 1024 shells), "est_accumulate" (est_pipeline 0 only: 1 block sums, 0 one LDS add per line visit),
 * "log_capacity" (line-visit records per epoch and buffer set of the wave-owner kernel; a call that logs more runs as several
 * launches over one packet supply), "log_sets" (1: the estimator passes of an epoch run before the next
 * epoch instead of beside it), "chunk_packets" (packets per launch of the group kernel), "waves_per_simd", "group_size",
 * "blocks_per_cu", "estimator_copies" (1..8 private j_blue/Edotlu copies),
 * "vpacket_screening" (v-packets whose Russian roulette is decided from prefix sums of tau instead of a line-by-line trace,
 * csrc/tau_prefix.hpp: -1 automatic -- on where a shell crossing passes many lines --, 0 off, 1 on),
 * "walk_sector_packing" (1, the default: blocks of the compact walk tables do not straddle 64-byte sectors; takes effect at the
 * next tardis_mc_set_opacity),
 * "walk_hot" (hot sectors of the macro-atom walk, csrc/walk_tables.hpp: one 64-byte record per (shell, block) with the block's
 * six widest probability intervals decides most jumps out of skewed blocks in one request; -1, the default: for the blocks
 * whose six intervals cover at least "walk_hot_min_mass" (per mille, default 800; blocks of more than 32 transitions:
 * "walk_hot_min_mass_long", default 400) of the block on average over the shells; 0 none; 1 every block; all three take effect
 * at the next tardis_mc_set_opacity), "drain_split" (1: the drain of a call runs as a launch of its own beside the estimator passes of
 * what was logged before it; measured, off by default),
 * "vp_carry_min_active" (pooled v-packet volleys of the wave-owner kernel: a volley phase ends once every v-packet of the round has been handed
 * to a lane and at most this many lanes still trace; those keep their v-packets for the next pass; default 16, 0: a phase runs to its end),
 * "bucket_lines_permille" (resolution of the frequency-bucket index of the line list, lines per bucket x 1000; default 750; takes effect at the
 * next tardis_mc_set_opacity), "vpk_wide_registers" (1, the default: v-packet calls on grids whose per-shell LDS arrays allow at most eight
 * waves per CU run the instantiation compiled for two waves per SIMD -- 239 VGPRs, no spills; 0 never; 2 always),
 * "vpk_wave_min_packets" (v-packet calls on fine grids take the wave-owner kernel from this many packets on, the group kernel below; default
 * 100000), "ls_waves_per_simd" (which instantiation of the lane-sweep kernel: 4 = 128 VGPRs, sixteen waves per CU, eight lines per step; 3 = 166 VGPRs,
 * twelve waves per CU, twelve lines per step -- faster where a call is mostly the drain of its longest packets; 0, the default: the engine times both on
 * the first calls of a (packet count, tables) key and keeps the faster; per-packet results are bit-identical either way), "pass_cus" (CUs per XCD set aside for the line-estimator passes through CU-masked streams; default 0 = off: measured, never pays),
 * "source_max_iterations" (tardis_mc_source_function: bound on the fixed-point iterations of the macro-atom level solve, default 20000; a solve
 * that reaches it fails with TARDIS_MC_ERR_STATE),
 * "debug_flags" (profiling experiments / cross-checks only: 1 skips the j_blue/Edotlu updates, 2 the J/nu_bar updates, 128
 * walks the macro atom by a per-lane search in the fp64 running sums, 8192 by the cooperative group scan; tests: 16384 counts
 * the jumps out of blocks longer than one window of the compact walk tables into counters[7], 32768 the jumps decided by the
 * fp64 running sums because 16-bit entries tie, 65536 / 131072 the jumps a hot sector decided / handed on to the block's own
 * tables, 67108864 the v-packets decided by the screening into counters[7] >> 40;
 * diagnostics of a call's drain: 2097152 / 4194304 / 8388608 sum, per wave and from the pass in which its packet supply ran out,
 * the 10-ns ticks to its end / its passes / its live lanes over those passes into counters[7]; 16777216 restores the fixed
 * cut-offs of the sweep and walk phases of rounds 1-2; 33554432 switches the v-packet screening off; 134217728 / 268435456 sum the lanes that
 * traced / the steps of the pooled volleys' worker loop into counters[7]; 2048 starts a new packet's roulette predictor at zero as in rounds
 * 1-4.  The flags that read a profiling counter or switch an ablation -- 1, 2, 4, 16, 32, 16384 ... 131072, 524288, 2097152 ... 16777216,
 * 134217728, 268435456 -- make the engine launch the cross-check instantiation of the kernel, which alone carries them). */
int tardis_mc_set_option(TardisMcContext *ctx, const char *name, long long value);

/* ---- staged API: inputs resident in HBM, kernels timed separately -------------------------------- */
int tardis_mc_set_geometry(TardisMcContext *ctx, const TardisMcGeometry *geometry);
/* Uploads and re-lays the opacity tables shell-major; once per MC iteration (the plasma changes them). */
int tardis_mc_set_opacity(TardisMcContext *ctx, const TardisMcOpacity *opacity);
int tardis_mc_set_config(TardisMcContext *ctx, const TardisMcConfig *config);
int tardis_mc_set_packets(TardisMcContext *ctx, const TardisMcPackets *packets);
/* Zero J, nu_bar, j_blue, Edotlu, v-hist and the counters (start of an iteration). */
int tardis_mc_reset_estimators(TardisMcContext *ctx);
/* Launch the propagation kernels for the resident packets on the context stream.
 * Estimators ACCUMULATE across calls until tardis_mc_reset_estimators (packet chunks of one iteration).
 * Blocking behaviour: the lane and group kernels (variants 0, 1) are queued and the call returns at once.  The wave-owner
 * kernel (variants 2-4, the automatic choice for sorted line lists) runs a call as a sequence of launches ("epochs") over one
 * packet supply; after every launch the HOST waits for one word (did any wave suspend on a full line-visit log region?) to
 * decide whether another launch follows, so the call returns when the LAST propagation launch has been queued and all earlier
 * ones have finished -- for a one-epoch call that is after its only launch.  The estimator passes of the last epoch, the
 * tracker unpacking and the result copies are still asynchronous: call tardis_mc_synchronize before reading results.  One host
 * thread driving several contexts therefore serialises their propagations; use one thread (or process) per context.
 * Returns TARDIS_MC_ERR_STATE if the launch bound of a call is exhausted with waves still suspended (results incomplete). */
int tardis_mc_propagate(TardisMcContext *ctx);
int tardis_mc_synchronize(TardisMcContext *ctx);
/* Device time of the kernels launched by the last tardis_mc_propagate (HIP events on the ctx stream). */
int tardis_mc_last_propagate_ms(TardisMcContext *ctx, double *out_ms);
/* The same, split per kernel: total time of the MT19937 seeding launches and of the propagation launches of the last
 * tardis_mc_propagate, and how many propagation launches there were (packet chunks). */
int tardis_mc_last_kernel_times(TardisMcContext *ctx, double *out_seed_ms, double *out_propagate_ms, int *out_launches);
/* summed duration of the line-estimator passes (record binning + accumulation) of the last propagate call; 0 when the
 * kernel variant in use updates the estimators with atomics */
int tardis_mc_last_estimator_ms(TardisMcContext *ctx, double *out_ms);
/* raw work counters of the last kernel launches (TARDIS_MC_CNT_*; after tardis_mc_formal_integral counters[0] is the number
 * of resonances crossed by all rays) */
int tardis_mc_last_counters(TardisMcContext *ctx, int64_t out_counters[TARDIS_MC_N_COUNTERS]);
/* Which propagation kernel the last tardis_mc_propagate ran (the "variant" option, or the automatic choice): 0 lane-per-packet,
 * 1 group-per-packet, 2 wave-owner with group sweeps, 3 wave-owner with lane sweeps, 4 wave-owner with the volley queue;
 * -1 before the first call. */
int tardis_mc_last_variant(TardisMcContext *ctx);
/* Whether the lane sweeps of the last tardis_mc_propagate cleared whole blocks on the coarse table (option "sweep_skip"): 1 / 0; -1 without a context. */
int tardis_mc_last_sweep_skip(TardisMcContext *ctx);
/* Width of the table row offsets of the kernel the last tardis_mc_propagate ran (option "table_offsets"): 32 or 64; the lane-per-packet
 * kernel (variant 0) always reports 64; -1 before the first call. */
int tardis_mc_last_table_offsets(TardisMcContext *ctx);
/* How often the last tardis_mc_propagate packed the live lanes of its drain into fewer waves (option "drain_compact" = T: once the packet supply has run out a wave
 * suspends when T or fewer of its lanes still hold a packet; the live lanes of all waves are packed into full waves and the rest of the call runs as a launch of
 * fewer waves, beside the line-estimator passes of the launch before; 0 = off.  Per-packet results do not depend on it). */
int tardis_mc_last_compactions(TardisMcContext *ctx);
/* How the last tardis_mc_propagate kept the last-interaction tracker (option "tracker_defer"): 1 one record per packet, written when it ends;
 * 0 a record per interaction (the option, or a problem beyond the packed widths); -1 the call ran another kernel than variant 3 without
 * v-packets, or without a tracker, or nothing has run yet.  A packet that ended with an error leaves an empty record after a call that reports 1. */
int tardis_mc_last_tracker_defer(TardisMcContext *ctx);
/* The tables of compiled propagation kernels, row by row (needs no context and no device).  `table`: 0 the lane-per-packet kernel, 1 the
 * group-per-packet kernel, 2 the wave-owner kernel.  Returns the number of rows of that table and, for 0 <= row < that number, fills `key`
 * (may be NULL) with the row's template arguments in their order, the unused tail zero:
 *   lane:  FULL, VPK, TRACK, FT, VLI
 *   group: FULL, TRACK, G, BLOCK, OCC, VPK, WIDE, VLI
 *   wave:  FULL, TRACK, G, VPK, LS, XWALK, WPE, NT, SL, FT, WIDE, VLI
 * A `table` outside 0..2 returns TARDIS_MC_ERR_INVALID_ARGUMENT (negative). */
int tardis_mc_kernel_table_row(int table, int row, int key[12]);
/* Which row of which table the last tardis_mc_propagate launched: `*table` as above and `key` as tardis_mc_kernel_table_row fills it;
 * `*table` = -1 (and a zero key) when the call was refused before it looked its kernel up, or nothing has run yet. */
int tardis_mc_last_kernel_key(TardisMcContext *ctx, int *table, int key[12]);
/* Progress of the propagate call that is running (or of the last one): packets handed to the propagation kernel so far and the call's
 * packet count -- what the reference's packet progress bar shows (update_packets_pbar, modes/montecarlo_transport.py:94-120,
 * progress_bars.py).  Safe to call from ANOTHER host thread while tardis_mc_propagate blocks (it reads one device word on a stream of
 * its own); exact for the wave-owner kernel (one packet supply per call), 0 until the call is complete for the chunked / lane kernels. */
int tardis_mc_progress(TardisMcContext *ctx, int64_t *out_packets_started, int64_t *out_packets_total);
/* Per-packet results of the resident packets + estimators (re-laid to [L,S]) to caller memory. */
int tardis_mc_get_results(TardisMcContext *ctx, TardisMcResult *result);

/* ---- producer next to the path: black-body packet source on the device --------------------------------
 * BlackBodySimpleSource.create_packets (transport/montecarlo/packet_source/base.py:195-253, black_body.py:140-222) with
 * NumPy's Generator(PCG64) streams reproduced by jump-ahead: fills the resident packet inputs (radii, nus, mus,
 * energies, seeds) of packets [first, first+count) of a global n_total-packet draw, as if set_packets had been called
 * with that slice of the host-sampled collection.  pcg_state = {state_hi, state_lo, inc_hi, inc_lo} of the PCG64
 * bit generator (numpy: default_rng(seed).bit_generator.state, or tardis_mc_pcg64_seed below); max_seed_val is
 * BasePacketSource.MAX_SEED_VAL (base.py:25, 2^32-1); l_array is cumsum(arange(1, l_samples)**-4) (black_body.py:174).
 * packet_seeds are bit-exact; mus bit-exact; nus within 1 ulp of a host run (the reference's log is numexpr's). */
int tardis_mc_pcg64_seed(uint64_t seed, uint64_t out_state[4]);  /* SeedSequence(seed) -> PCG64 state; host only */
int tardis_mc_create_blackbody_packets(TardisMcContext *ctx, int64_t n_total, int64_t first, int64_t count, double radius,
                                       double temperature, const uint64_t pcg_state[4], uint32_t max_seed_val,
                                       const double *l_array, int64_t n_l);
/* The source of a full-relativity run: BlackBodySimpleSourceRelativistic (packet_source/black_body.py), which the reference builds when
 * montecarlo.enable_full_relativity is set because the inner boundary is not comoving with the ejecta.  Seeds, radii, nus and every
 * RNG stream position are those of the simple source above; only the directions and the energies differ.  With c = 2.99792458e10 and
 * n = n_total (the GLOBAL packet count, also for a shard), in this operation order, the squares written as products, nothing fused:
 *   beta   = (radius / time_explosion) / c
 *   gamma  = 1.0 / sqrt(1.0 - beta*beta)
 *   factor = (2.0*beta + 1.0) / (1.0 - beta*beta)
 *   energy = ((1.0 / n) * factor) / gamma                         every packet
 *   z      = rng.random(n)                                        the stream position of the simple source's direction draw
 *   mu     = (-beta) + sqrt(((beta*beta) + ((2.0*beta) * z)) + z) p(mu) = 2 (mu + beta) / (2 beta + 1) on [0, 1]; not clamped
 * beta = 0 gives the simple source bit for bit.  packet_seeds, mus, energies and radii are bit-exact against NumPy; the nus are
 * bit-identical to the simple source's of the same seed.
 * tardis_mc_relativistic_source_factors computes beta and energy on the host (no context, no device) and is where the device entry
 * point takes them from; it returns TARDIS_MC_ERR_INVALID_ARGUMENT when radius is not finite and non-negative, time_explosion is not
 * finite and positive, n_total < 1, or the resulting beta is not in [0, 1).
 * tardis_mc_create_blackbody_packets_relativistic has the contract of tardis_mc_create_blackbody_packets (shards, rejected seed draws,
 * what it invalidates) plus those argument errors, each with a message that names the offending value, raised before anything
 * resident is touched.  time_explosion is an argument, not what tardis_mc_set_geometry left: the call has no ordering dependency. */
int tardis_mc_relativistic_source_factors(double radius, double time_explosion, int64_t n_total, double *out_beta, double *out_energy);
int tardis_mc_create_blackbody_packets_relativistic(TardisMcContext *ctx, int64_t n_total, int64_t first, int64_t count, double radius,
                                                    double temperature, double time_explosion, const uint64_t pcg_state[4],
                                                    uint32_t max_seed_val, const double *l_array, int64_t n_l);
/* download the resident packet inputs (any pointer may be NULL) */
int tardis_mc_get_packets(TardisMcContext *ctx, double *initial_radii, double *initial_nus, double *initial_mus,
                          double *initial_energies, int64_t *packet_seeds);

/* ---- consumer next to the path: real-packet spectrum + filtered luminosities on the device -------------
 * From the per-packet outputs resident after tardis_mc_propagate: histograms of emitted / reabsorbed packet luminosity
 * (+/- output_energy / time_of_simulation) over the spectrum_frequency_grid passed to tardis_mc_set_config, with
 * numpy.histogram's edge rules (tardis/spectrum/base.py:140-159), and the luminosity sums over
 * luminosity_nu_start < nu < luminosity_nu_end (tardis/spectrum/luminosity.py:5-30).  Histograms have n_grid-1 bins. */
int tardis_mc_packet_spectrum(TardisMcContext *ctx, double time_of_simulation, double luminosity_nu_start,
                              double luminosity_nu_end, double *emitted_luminosity_hist, double *reabsorbed_luminosity_hist,
                              double *out_emitted_luminosity, double *out_reabsorbed_luminosity);

/* ---- consumer next to the path: the emitted spectrum decomposed by last interaction ------------------------------------------
 * What SDEC (emission and absorption by species), the last-interaction-velocity histogram (LIV) and LastLineInteraction compute on the
 * host from the last-interaction tracker, reduced on the device from the seven per-packet arrays resident after a tardis_mc_propagate
 * with "track_last_interaction" on: output_nu, output_energy, li_interaction_type, li_line_emit_id, li_line_absorb_id, li_before_nu,
 * li_shell_id.  A packet is SELECTED when output_energy >= 0 (emitted) and nu_start < output_nu < nu_end; its weight is
 * l = output_energy / time_of_simulation; its kind is li_interaction_type: 2 LINE, 4 ESCATTERING, -1 none (the tracker holds the last
 * non-boundary interaction: a packet that last scattered on an electron has line ids -1 and is no line packet).  With bin() the bin
 * of numpy.histogram on the spectrum_frequency_grid of tardis_mc_set_config (left-closed bins, the last one also right-closed, a
 * value outside [edges[0], edges[B]] in no bin):
 *   LINE         emission[line_class[li_line_emit_id]][bin(output_nu)] += l;  absorption[line_class[li_line_absorb_id]][bin(li_before_nu)] += l;
 *                shell_packets[emit class][li_shell_id] += 1;  line_emit_packets[emit id] += 1;  line_absorb_packets[absorb id] += 1
 *   ESCATTERING  electron_scatter[bin(output_nu)] += l;  shell_packets[C][li_shell_id] += 1
 *   none         no_interaction[bin(output_nu)] += l
 * n_selected, n_line, n_electron_scatter, n_no_interaction count the selected packets and the three kinds among them; a packet whose
 * frequency is outside the grid still counts in every integer output.
 * The double sums are accumulated with atomics (in LDS per workgroup where the matrices fit 64 KiB, csrc/decomposition_plan.hpp, else
 * straight in HBM): all addends are non-negative, so two calls agree within (n - 1) 2^-53 relatively in a cell of n addends, and a cell
 * without addends is exactly 0; the integer outputs agree exactly.  All outputs are additive over packet shards: ranks sum them on the host.
 * Errors: TARDIS_MC_ERR_STATE when no propagate call has completed, when the last one ran with "track_last_interaction" 0, when a packet of
 * it failed, when the resident packets were replaced since, or without a spectrum grid; TARDIS_MC_ERR_INVALID_ARGUMENT when d or
 * line_class is NULL, C < 1, a class is outside [0, C) (checked on the host before anything is indexed with it) or time_of_simulation is
 * not positive.  Nothing resident changes.  tardis_mc_last_propagate_ms then reports the device time of the call's kernels. */
int tardis_mc_packet_decomposition(TardisMcContext *ctx, TardisMcDecomposition *d);
/* The same decomposition of the VIRTUAL spectrum (SDEC / LIV with packets_mode="virtual"): packet_decomposition_kernel on the consolidated
 * v-packet log of the last tardis_mc_propagate (consolidated here where tardis_mc_get_vpacket_log has not done it yet), one entry per
 * v-packet with output_nu = nus, output_energy = energies, li_before_nu = last_interaction_in_nu, li_interaction_type = last_interaction_type,
 * li_line_emit_id = last_interaction_out_id, li_line_absorb_id = last_interaction_in_id, li_shell_id = last_interaction_shell_id.  Same struct,
 * outputs, accumulation paths, argument checks and additivity over packet shards.  A v-packet is selected when nu_start < nu < nu_end (its
 * energy is never negative); one the roulette dropped has energy 0.0: it adds 0.0 to its cell and still counts in the integer outputs.  The sum
 * of all double cells of emission, electron_scatter and no_interaction is sum(v_packets_energy_hist) / time_of_simulation to rounding.
 * TARDIS_MC_ERR_STATE without a valid v-packet log with last-interaction columns (option "vpacket_last_interaction"), when the log overflowed
 * (run again with vpacket_log_capacity >= the count tardis_mc_get_vpacket_log reports), when a packet failed, or without a spectrum grid.
 * Nothing resident changes.  tardis_mc_last_propagate_ms then reports the device time of the call's kernels. */
int tardis_mc_vpacket_decomposition(TardisMcContext *ctx, TardisMcDecomposition *d);
/* Which accumulation path a call with C classes, B bins and S shells takes: 0 privatised (LDS), 1 direct (HBM).  Host only. */
int tardis_mc_decomposition_path(int64_t n_classes, int64_t n_bins, int64_t n_shells);

/* ---- consumer next to the path: radiation-field update from the resident estimators -------------------
 * MCRadiationFieldPropertiesSolver.solve (transport/montecarlo/estimators/mc_rad_field_solver.py:37-144):
 *   t_radiative[s] = C_T nu_bar[s] / J[s];  dilution_factor[s] = J[s] / (4 sigma_sb t_rad^4 time_of_simulation volume[s]);
 *   j_blues[l][s] = j_blue_estimator[l][s] c t_exp / (4 pi time_of_simulation volume[s]), cells with a zero estimator get
 *   w_epsilon * W[s] B_nu(nu_l, t_rad[s]), and with detailed_optical_window lines outside 2500-10000 A get W B_nu.
 * Runs after tardis_mc_propagate (and, multi-GPU, after tardis_mc_allreduce_estimators).  volume: [n_shells] cm^3.
 * Outputs (host, any may be NULL): t_radiative[n_shells], dilution_factor[n_shells], j_blues[n_lines*n_shells] line-major. */
int tardis_mc_radiation_field(TardisMcContext *ctx, double time_of_simulation, const double *volume, double w_epsilon,
                              int detailed_optical_window, double *t_radiative, double *dilution_factor, double *j_blues);

/* ---- consumer next to the path: the formal integral of the spectrum ----------------------------------------
 * NumbaFormalIntegrator.formal_integral / numba_formal_integral (tardis/spectrum/formal_integral/formal_integral_numba.py:
 * 375-560, 563-642; CUDA twin formal_integral_cuda.py:272-489) on the resident geometry, line list, tau_sobolev and electron
 * densities (set_geometry / set_opacity).  (The three inputs can be computed on the device and stay there: tardis_mc_source_function /
 * tardis_mc_formal_integral_resident below.)  att_S_ul, Jred_lu, Jblue_lu: host, [n_shells * n_lines] in the shell-major flat
 * order the reference passes them (make_source_function, source_function.py:71-75).  Outputs (host): luminosity_densities
 * [n_frequencies]; intensities_nu_p [n_frequencies * n_impact_parameters] or NULL.  tardis_mc_last_propagate_ms then
 * reports the device time of the integration kernels. */
int tardis_mc_formal_integral(TardisMcContext *ctx, double inner_temperature, const double *frequencies, int64_t n_frequencies,
                              const double *att_S_ul, const double *Jred_lu, const double *Jblue_lu, int64_t n_impact_parameters,
                              double *luminosity_densities, double *intensities_nu_p);

/* ---- producer of the formal integral's inputs: the line source function from the resident estimators ---------------------
 * make_source_function (tardis/spectrum/formal_integral/source_function.py) on the resident probabilities, macro-atom index tables,
 * tau_sobolev and the j_blue / Edotlu estimators; runs after tardis_mc_propagate (multi-GPU: after tardis_mc_allreduce_estimators).
 * Per shell s:  Edotlu = (1 / (time_of_simulation volume[s])) (1 - exp(-tau)) Edotlu_estimator;  e_dot_u[k] = its sum over the lines
 * with upper level k;  C = e_dot_u (downbranch) or the solution of (I - Q_s)^T C = e_dot_u (macroatom; Q_s[i][j] = sum of the
 * probabilities of the rows of block i with transition_type >= 0 and destination level j), found by the fixed-point iteration
 * C <- e_dot_u + Q_s^T C from C = e_dot_u until an iteration has changed no level of any shell, tested every 16 iterations (option
 * "source_max_iterations").  With non-negative estimators, depths and probabilities the iterates never decrease, so the iteration ends, at the
 * fixed point of the rounded map: every C[k] is then within (r + n + 3) 2^-53 B[k] of the exact solution to first order, r the longest row of
 * Q_s^T, n the most lines on a level, B = (I - Q_s^T)^-1 C -- relative to the level itself, however weak beside the others of its shell;
 * att_S_ul[s][l] = wave[l] (prob[s][t] C[k]) time_of_simulation / (4 pi) for the emission row t (transition_type -1) of line l, in
 * block k;  Jblue_lu[s][l] = j_blue_estimator[s][l] c t_exp / (4 pi time_of_simulation volume[s]) (bit for bit the j_blues of
 * tardis_mc_radiation_field where the estimator is non-zero);  Jred_lu = Jblue_lu exp(-tau) + att_S_ul.
 * volume: [n_shells] cm^3.  wavelength_cm: [n_lines], or NULL for c / line_list_nu.  Outputs (host, any may be NULL): att_S_ul, Jred_lu,
 * Jblue_lu [n_shells * n_lines], flat shell-major as tardis_mc_formal_integral takes them; e_dot_u [levels * n_shells], level-major
 * (for macroatom: C, as the reference returns it).  The three arrays also stay in HBM, marked valid for
 * tardis_mc_formal_integral_resident until the next tardis_mc_set_opacity, _set_geometry, _reset_estimators, _propagate or
 * _allreduce_estimators.  Errors: TARDIS_MC_ERR_UNSUPPORTED for scatter mode (no macro-atom tables; the reference refuses it too),
 * TARDIS_MC_ERR_INVALID_ARGUMENT when some line has no emission row or several, TARDIS_MC_ERR_STATE without propagated estimators or when
 * the solve reaches its iteration bound or meets NaN / infinite rates (the message names the worst shell; nothing is left valid).  No atomics: two calls give
 * bit-identical results.  tardis_mc_last_propagate_ms then reports the device time of the call's kernels. */
int tardis_mc_source_function(TardisMcContext *ctx, double time_of_simulation, const double *volume, const double *wavelength_cm,
                              double *att_S_ul, double *Jred_lu, double *Jblue_lu, double *e_dot_u);
/* Fixed-point iterations of the last tardis_mc_source_function (a multiple of 16 unless the bound cut it short); 0 for downbranch,
 * -1 before the first call. */
int tardis_mc_last_source_iterations(TardisMcContext *ctx);
/* tardis_mc_formal_integral on the att_S_ul / Jred_lu / Jblue_lu that tardis_mc_source_function left in HBM: same kernels, same
 * outputs, no [n_shells * n_lines] array crosses the bus, and exp(-tau) is the table the source function computed.
 * TARDIS_MC_ERR_STATE when no valid resident source function exists. */
int tardis_mc_formal_integral_resident(TardisMcContext *ctx, double inner_temperature, const double *frequencies, int64_t n_frequencies,
                                       int64_t n_impact_parameters, double *luminosity_densities, double *intensities_nu_p);

/* ---- interpolate_shells: the formal integral on a refined (or coarsened) shell grid -----------------------------------------
 * What FormalIntegralSolver / interpolate_integrator_quantities (tardis/spectrum/formal_integral/) do before they integrate when the
 * configuration sets interpolate_shells = n > 0, here on the resident source function and without leaving the device.  With S the
 * resident shells and S' = n - 1:
 *   x[s]  = (r_inner[s] + r_outer[s]) / 2.0                                              the nodes
 *   r     = numpy.linspace(r_inner[0], r_outer[S-1], n):  step = (stop - start) / (n - 1), r[i] = i * step + start, r[n-1] = stop
 *   r_inner_i = r[:-1], r_outer_i = r[1:], xn[j] = (r_inner_i[j] + r_outer_i[j]) / 2.0    the new shells and their midpoints
 *   att_S_ul, Jred_lu, Jblue_lu, e_dot_u -- linear with extrapolation (scipy interp1d, fill_value="extrapolate"), clipped at zero:
 *       hi = clip(searchsorted(x, xn[j], side="left"), 1, S-1), lo = hi - 1
 *       slope = (y[hi] - y[lo]) / (x[hi] - x[lo]);  v = slope * (xn[j] - x[lo]) + y[lo];  result max(v, 0.0)
 *     in exactly this order -- one division, one product, one sum, no fused multiply-add -- so the tables are bit for bit scipy's
 *     (the clip matters inside the grid too: with y[hi] = 0 and xn = x[hi], v can round to a tiny negative value);
 *   tau_sobolev, electron_density -- the nearest node, ties to the lower shell ("constant within a shell, as in the MC simulation"):
 *       near = searchsorted((x[1:] + x[:-1]) / 2.0, xn[j], side="left");  result y[near]
 * and the formal integral runs unchanged on r_inner_i / r_outer_i, the nearest-shell tau and n_e and the three interpolated arrays,
 * with impact parameters up to r_outer_i[S'-1] = r_outer[S-1].  The maps are computed on the host in double, the tables by one
 * streaming kernel (csrc/formal_interpolate.hpp) into scratch memory that the call releases: nothing resident changes, the run's
 * geometry, opacity, estimators and source function stay valid.
 *
 * tardis_mc_formal_integral_interpolated: tardis_mc_formal_integral_resident on that grid; same outputs, same
 * TARDIS_MC_ERR_STATE without a valid resident source function, counters[0] and tardis_mc_last_propagate_ms as there (the device
 * time includes the interpolation kernel).  TARDIS_MC_ERR_INVALID_ARGUMENT for interpolate_shells < 2 or > 65536 (a number of grid
 * POINTS) and for a model of one shell (two nodes are needed; scipy refuses it too).
 * tardis_mc_interpolated_source: the same tables, downloaded -- r_inner_i, r_outer_i, electron_density_i [S'], tau_sobolev_i (the
 * gathered rows of the resident optical depths), att_S_ul_i, Jred_lu_i, Jblue_lu_i [S' * n_lines] flat shell-major, e_dot_u_i
 * [levels * S'] level-major; any pointer may be NULL.  Same errors. */
int tardis_mc_formal_integral_interpolated(TardisMcContext *ctx, int64_t interpolate_shells, double inner_temperature,
                                           const double *frequencies, int64_t n_frequencies, int64_t n_impact_parameters,
                                           double *luminosity_densities, double *intensities_nu_p);
int tardis_mc_interpolated_source(TardisMcContext *ctx, int64_t interpolate_shells, double *r_inner_i, double *r_outer_i,
                                  double *electron_density_i, double *tau_sobolev_i, double *att_S_ul_i, double *Jred_lu_i,
                                  double *Jblue_lu_i, double *e_dot_u_i);

/* ---- producer of the next iteration's opacity state: tau_sobolev and the transition probabilities from level populations ----
 * What the legacy plasma's StimulatedEmissionFactor, TauSobolev, BetaSobolev, JBluesDiluteBlackBody and
 * calculate_transition_probabilities compute between two iterations, on the device and in their operation order (fp64, no
 * contraction, exp as the transport evaluates it).  The atomic data are set once per topology (tardis_mc_set_line_data); every iteration
 * then uploads the populations [K,S] instead of tau_sobolev [L,S] and the probabilities [T,S].  Per line l and shell s, with
 * n_l = n[level_lower[l]][s], n_u = n[level_upper[l]][s]:
 *   sef  = 1.0 - (g_lower[l] n_u) / (g_upper[l] n_l);  0.0 where n_l == 0.0 and where the result is negative (the NLTE exception that
 *          keeps inversions is not part of this)
 *   tau  = ((((sobolev_coefficient f_lu[l]) wavelength_cm[l]) time_explosion) n_l) sef
 *   beta = 1.0 / tau where tau > 1e3;  1.0 - 0.5 tau where tau < 1e-4;  (1.0 - exp(-tau)) / tau otherwise
 *   j    = j_blues_mode 0, dilute black body: dilution_factor[s] (2h/c^2 nu^3 / (exp(h nu / (k_B t_radiative[s])) - 1)), the expression
 *          and constants of tardis_mc_radiation_field;  j_blues_mode 1, detailed: bit for bit the j_blues tardis_mc_radiation_field
 *          returns for the same (time_of_simulation, volume, w_epsilon, detailed_optical_window), from the resident estimators
 * and per transition row t of block b, with line = transition_line_id[t]:
 *   p = transition_probability_coef[t] beta[line][s];  for transition_type[t] == 1: p = p (sef[line][s] j[line][s]);
 *   the result is p / norm, norm the serial left-to-right sum of the block's p from 0.0;  0.0 where norm == 0.0.
 * No atomics anywhere: two calls give identical bits.
 *
 * TardisMcLineData: n_lines, n_transitions must equal the resident topology; n_levels = K, the rows of level_number_density.
 * level_lower / level_upper index those rows.  transition_probability_coef is NULL in scatter mode (no macro-atom tables): only tau,
 * beta, sef and j are then computed, the resident probabilities stay as they are. */
typedef struct TardisMcLineData {
    int64_t n_lines;                            /* L */
    int64_t n_transitions;                      /* T */
    int64_t n_levels;                           /* K */
    const double *f_lu;                         /* [L] */
    const double *wavelength_cm;                /* [L] */
    const double *g_lower;                      /* [L] statistical weight of the lower level */
    const double *g_upper;                      /* [L] ... of the upper level */
    const int64_t *level_lower;                 /* [L] in [0, K) */
    const int64_t *level_upper;                 /* [L] in [0, K) */
    const double *transition_probability_coef;  /* [T], or NULL (scatter mode) */
    double sobolev_coefficient;                 /* the plasma's constant: no constant is duplicated here */
} TardisMcLineData;

typedef struct TardisMcOpacityUpdate {
    const double *level_number_density;         /* [K,S] */
    const double *electron_density;             /* [S], or NULL to keep the resident values */
    int32_t j_blues_mode;                       /* 0 dilute black body, 1 detailed */
    const double *t_radiative;                  /* [S], mode 0 */
    const double *dilution_factor;              /* [S], mode 0 */
    double time_of_simulation;                  /* mode 1, as tardis_mc_radiation_field takes them */
    const double *volume;                       /* [S], mode 1 */
    double w_epsilon;                           /* mode 1 */
    int32_t detailed_optical_window;            /* mode 1 */
} TardisMcOpacityUpdate;

/* Static line data of the resident topology; after tardis_mc_set_opacity, which drops them (a later set_opacity: call this again).
 * Everything is checked on the host before anything is indexed: TARDIS_MC_ERR_INVALID_ARGUMENT when n_lines / n_transitions differ
 * from the resident tables, when a level index is outside [0, K), when ANY row's transition_line_id is outside [0, L) (set_opacity
 * checks only the emission rows), or when coefficients are given although no macro-atom tables are resident;
 * TARDIS_MC_ERR_UNSUPPORTED for a transition type outside {-1, 0, 1}; TARDIS_MC_ERR_STATE before set_opacity. */
int tardis_mc_set_line_data(TardisMcContext *ctx, const TardisMcLineData *line_data);
/* One iteration's update: uploads the populations (and electron densities), rewrites tau_sobolev in place, computes beta, sef, j
 * ([S][L] each, resident until the next update or set_opacity) and the probabilities, and derives from those every table that
 * tardis_mc_set_opacity derives -- afterwards the context is indistinguishable from a fresh one given the same tau_sobolev and
 * probabilities through tardis_mc_set_opacity.  The geometry's time_explosion is the one resident at the call.  Estimators and packets
 * stay valid; the resident source function is invalidated, exactly as set_opacity does.  TARDIS_MC_ERR_STATE without line data, without
 * geometry, and in mode 1 without propagated estimators (multi-GPU: call it after tardis_mc_allreduce_estimators);
 * TARDIS_MC_ERR_INVALID_ARGUMENT for an unknown mode or a missing array of the mode.  tardis_mc_last_propagate_ms then reports the
 * device time of the call's kernels. */
int tardis_mc_update_opacity(TardisMcContext *ctx, const TardisMcOpacityUpdate *update);
/* Device time of the stages of the last tardis_mc_update_opacity, in ms (any pointer may be NULL): the transpose of the populations, the
 * j_blues of mode 1 and the line kernel | the block kernels | the derived tables (with the host work between their kernels).  Their sum
 * is what tardis_mc_last_propagate_ms reports after the update.  TARDIS_MC_ERR_STATE before the first update. */
int tardis_mc_last_opacity_update_ms(TardisMcContext *ctx, double *out_line_ms, double *out_block_ms, double *out_derive_ms);
/* Downloads the resident opacity state, line-major as tardis_mc_set_opacity takes it: tau_sobolev, beta_sobolev,
 * stimulated_emission_factor, j_blues [L,S]; transition_probabilities [T,S].  Any pointer may be NULL.  The last three return
 * TARDIS_MC_ERR_STATE unless a tardis_mc_update_opacity produced them since the last set_opacity. */
int tardis_mc_get_opacity(TardisMcContext *ctx, double *tau_sobolev, double *transition_probabilities, double *beta_sobolev,
                          double *stimulated_emission_factor, double *j_blues);
/* Which form of the update's block kernel a macro-atom block of `rows` transition rows takes (csrc/opacity_update_plan.hpp): 0 a lane per
 * (block, shell), 1 a 16-lane row per (block, shell).  Host only; both forms add in the same order.  Option "opacity_update_long_rows"
 * (tardis_mc_set_option; -1, the default: this rule; n >= 0: blocks of n rows or more take the row form -- measurements only). */
int tardis_mc_opacity_update_path(int64_t rows);

/* ---- consumer of the resident optical depths: expansion opacity, Planck / Rosseland mean opacities and optical depths per shell ----
 * What the inner-velocity workflow's tau integration computes from tau_sobolev [L,S] between two iterations (expansion opacity in
 * frequency bins, its Planck and Rosseland means with electron scattering, the optical depths summed from the surface inward), here
 * on the resident table: four vectors of S doubles come back, no [L,S] array crosses the bus.  The definition below is the contract;
 * tests/mean_opacity_ref.py restates it serially and the device equals that bit for bit.
 *
 * All arithmetic is fp64 with no contraction: every product, quotient and sum is a rounding of its own.  exp is the transport's own.  The
 * constants are those of the radiation-field section above: h, k_B, c, and planck_coef = 2h/(c c) formed as there.
 *
 * Bins.  L resident lines, m = bin_size >= 1.  asc[i] = line_list_nu[L-1-i] is the list in ascending order.  e = m - L mod m, so
 * 1 <= e <= m, and n_bins = (L + e) / m.  The padded sequence is p[j] = j + 1 (Hz) for 0 <= j <= e and p[j] = asc[j-e-1] for e < j <= L + e;
 * the padded optical depth is q[j][s] = 0.0 for j <= e and the resident tau_sobolev of that line in shell s for j > e.  Bin b has
 * low_b = p[b m], high_b = p[(b+1) m], dnu_b = high_b - low_b, and the members j = b m + 1 .. (b+1) m: the line on the high edge belongs
 * to the bin, the one on the low edge does not.  (NumPy: nu_p = hstack([arange(1, e + 2), asc]); low = nu_p[:-m:m], high = nu_p[m::m].)
 *
 * Refused on the host, before anything is launched, with TARDIS_MC_ERR_INVALID_ARGUMENT: m < 1; asc[0] <= e + 1 (the pads must lie below
 * the list); any dnu_b == 0.0 (duplicate lines on two consecutive edges; the message names the first such bin); a t_radiative that is
 * not finite and positive; a missing t_radiative pointer.  TARDIS_MC_ERR_STATE without a resident geometry or opacity.
 *
 * Per (bin, shell):  x[b][s] = the serial sum, from 0.0, over the members in ascending j of (1.0 - exp(-q[j][s]));  ct = time_explosion c;
 *   kexp[b][s] = ((low_b / dnu_b) / ct) x[b][s].  No clamp: a negative resident tau gives the IEEE result.
 * Weights at nu = low_b, t = t_radiative[s]:  beta = 1 / (k_B t);  E = exp((h nu) beta);  B = (planck_coef (nu nu nu)) / (E - 1);
 *   cn = c / nu;  U = ((((B E) B) (cn cn)) / ((2 k_B) (t t)));  bd = B dnu_b;  ud = U dnu_b.  A bin where E is not finite or E - 1 == 0.0
 *   contributes exactly 0.0 to all four sums below (the plain NumPy spelling makes the whole shell NaN there).
 * Per shell:  kthom = electron_density[s] sigma_thomson, the resident values (sigma_thomson is the configuration's, 1e-200 with electron
 *   scattering disabled, as the transport sees it; 6.652458734e-25 cm^2 while no configuration is resident).  Four serial sums over
 *   the bins in ascending b from 0.0:  pn = sum bd kexp;  pd = sum bd;  rn = sum ud (1.0 / (kthom + kexp));  rd = sum ud.
 *   kappa_planck = kthom + pn / pd;  kappa_rosseland = 1.0 / (rn / rd);  dr = r_outer[s] - r_inner[s];  the depths are summed from the
 *   surface inward, tau[S-1] = kappa[S-1] dr[S-1], tau[s] = tau[s+1] + kappa[s] dr[s], for both means.
 * This is the order of NumPy's reductions over an outer axis, so agreement with a plain NumPy spelling (libm exp, **-1, **2, nu**3) is
 * to rounding, not bitwise: the largest relative deviation of the four vectors measured on the test models is 8.5e-15
 * (tests/test_mean_opacity_host.py asserts ten times that; a single bin of thin lines deviates by more, 1.0 - exp(-tau) cancels there).
 *
 * tardis_mc_mean_opacity reads the resident tau table, electron densities, geometry and sigma_thomson and changes nothing resident;
 * its scratch is released at return, as tardis_mc_formal_integral_interpolated does.  Outputs (host, any may be NULL): kappa_planck,
 * kappa_rosseland, tau_planck, tau_rosseland [S]; kappa_expansion [n_bins,S]; bins_low, delta_nu [n_bins] (n_bins from
 * tardis_mc_mean_opacity_bins).  No atomics: two calls give identical bits.  tardis_mc_last_propagate_ms then reports the call's kernels.
 * Kernels in csrc/mean_opacity.hpp, the bin layout and the choice below in csrc/mean_opacity_plan.hpp. */
typedef struct TardisMcMeanOpacity {
    int64_t bin_size;                           /* m */
    const double *t_radiative;                  /* [S] */
    double *kappa_planck;                       /* [S] cm^-1, or NULL */
    double *kappa_rosseland;                    /* [S] cm^-1, or NULL */
    double *tau_planck;                         /* [S], or NULL */
    double *tau_rosseland;                      /* [S], or NULL */
    double *kappa_expansion;                    /* [n_bins,S] cm^-1, or NULL */
    double *bins_low;                           /* [n_bins] Hz, or NULL */
    double *delta_nu;                           /* [n_bins] Hz, or NULL */
} TardisMcMeanOpacity;
int tardis_mc_mean_opacity(TardisMcContext *ctx, const TardisMcMeanOpacity *request);
/* The bin layout of a (descending) line list, host only, no context: returns n_bins, or a negative error code under the rules above
 * (tardis_mc_last_error(NULL) then carries the message).  first_degenerate_bin (may be NULL): the first bin of width 0, -1 where there is
 * none. */
int64_t tardis_mc_mean_opacity_bins(int64_t n_lines, const double *line_list_nu, int64_t bin_size, int64_t *first_degenerate_bin);
/* Device time of the stages of the last tardis_mc_mean_opacity, in ms (either pointer may be NULL): the bin kernel | the shell reduction
 * and the final kernel.  Their sum is what tardis_mc_last_propagate_ms reports after the call.  TARDIS_MC_ERR_STATE before the first call. */
int tardis_mc_last_mean_opacity_ms(TardisMcContext *ctx, double *out_bin_ms, double *out_reduce_ms);
/* Which form the shell reduction takes for n_bins bins (csrc/mean_opacity_plan.hpp): 0 a lane per shell, 1 a wave per shell whose four
 * 16-lane rows carry the four sums.  Host only; both forms add in the same order.  Option "mean_opacity_long_bins"
 * (tardis_mc_set_option; -1, the default: this rule; n >= 0: the row form from n bins upward -- tests and measurements only). */
int tardis_mc_mean_opacity_path(int64_t n_bins);

/* ---- producer of the next iteration's populations: ion and level number densities from (t_rad, W) ------------------------------
 * What the legacy plasma computes between two iterations in its default configuration -- ionization nebular (or lte), excitation
 * dilute-lte (or lte), NLTE excitation only through the section after this one, helium_treatment recomb-nlte and delta_treatment only through tardis_mc_set_ionization_options below, the continuum rate stage only through tardis_mc_set_continuum_data below: LevelBoltzmannFactor, PartitionFunction,
 * GElectron, PhiSahaLTE / PhiSahaNebular with RadiationFieldCorrection and the interpolated zeta, IonNumberDensity.calculate and
 * LevelNumberDensity -- on the device and in their operation order (fp64, no contraction, exp as the transport evaluates it, every
 * product and sum a rounding of its own).  The populations never leave the device: they are written where tardis_mc_update_opacity's
 * kernels read them, and the stages of that update run on them.  Constants: CODATA 2010 cgs, k_B = 1.3806488e-16,
 * h = 6.62606957e-27, m_e = 9.10938291e-28.  Per shell s, level k of ion i of element e:
 *   beta_rad = 1 / (k_B t_rad);  t_e = link_t_rad_t_electron t_rad;  beta_e = 1 / (k_B t_e)
 *   x = (((2 pi) m_e) / beta_rad) / (h h);  g_e = x sqrt(x)
 *       (the reference writes x ** 1.5.  No pow is bit-identical between a host libm and the device, while sqrt and the product are
 *       correctly rounded everywhere; x sqrt(x) rounds twice where a correctly rounded pow rounds once, so the two differ by at most an
 *       ulp of g_e, far below what the 5 % electron-density criterion resolves)
 *   lbf[k] = level_g[k] exp(level_energy[k] (-beta_rad)), times W for a level with level_metastable[k] == 0 when excitation_mode is 0
 *   Z[i]   = the serial sum of the ion's lbf in level order, from 0.0
 *       (pandas' groupby().sum(), which the reference uses, is a compensated sum: agreement with TARDIS is to rounding, not bitwise)
 *   per ion i that is not its element's last:  phi_lte = (Z[i+1] / Z[i]) ((2 g_e) exp(chi_i (-beta_rad))),  chi_i = ionization_energy[i]
 *   ionization_mode 1 (lte):      phi = phi_lte
 *   ionization_mode 0 (nebular):  phi = ((phi_lte W) ((zeta delta) + W (1 - zeta))) sqrt(t_e / t_rad)
 *     zeta  = zeta[i][.] interpolated linearly in t_rad over zeta_temperatures as interpolate_shells interpolates above:
 *             hi = clip(searchsorted(zeta_temperatures, t_rad, side="left"), 1, NT-1), lo = hi - 1,
 *             slope = (y[hi] - y[lo]) / (x[hi] - x[lo]);  zeta = slope (t_rad - x[lo]) + y[lo]   (one division, one product, one sum; not clipped)
 *     delta = RadiationFieldCorrection with departure_coefficient = 1 / W:  fa = t_e / (((1 / W) W) t_rad);
 *             chi_i >= chi_0:  delta = fa exp(chi_i (beta_rad - beta_e))
 *             otherwise:       delta = (1 - exp(chi_i beta_rad - beta_rad chi_0)) + fa exp(chi_i beta_rad - beta_e chi_0)
 *   IonNumberDensity.calculate:  n_e = the serial sum of number_density over the elements;  then per pass, per element with ions a .. b:
 *     pe_j = phi_j / n_e (NaN -> 0.0, +inf -> DBL_MAX: numpy.nan_to_num);  cp_j = pe_a ... pe_j, the running product;
 *     N_a = number_density[e] / (1 + sum cp), the sum serial;  N_(j+1) = N_a cp_j;  populations below 1e-20 become 0.0;
 *     new = sum_i N_i ion_charge[i], serial over all ion rows;  the pass count goes up by one;
 *     stop when |new - n_e| / n_e < 0.05 in EVERY shell, otherwise n_e = 0.5 (new + n_e).
 *     All shells run the same number of passes, as in the reference; the n_e handed out is the one the last pass used.
 *   n[k] = (lbf[k] / Z[i]) N[i]
 * Kernels (csrc/plasma_update.hpp): two streaming kernels over (level, shell); the partition functions by one lane per (ion, shell) or,
 * for long ions, by a 16-lane row that carries the sum in level order (csrc/plasma_update_plan.hpp; same bits); phi and the iteration
 * by ONE workgroup with a lane per shell, the all-shells vote a workgroup barrier -- which is why more than 1024 shells are refused
 * (TARDIS_MC_ERR_UNSUPPORTED): a form with one launch per pass is not built.  No atomics: two calls give identical bits.
 *
 * TardisMcPlasmaData: levels sorted by (element, ion, level) -- an ion's levels are contiguous, ion_level_edge[i] .. ion_level_edge[i+1]
 * -- and ions by (element, charge), element_ion_edge likewise.  The entries of an element's last ion in ionization_energy and zeta are
 * ignored; zeta rows are 1.0 where the reference has no data. */
typedef struct TardisMcPlasmaData {
    int64_t n_levels;                    /* K, the line data's n_levels */
    int64_t n_ions;                      /* I */
    int64_t n_elements;                  /* E */
    int64_t n_shells;                    /* S, the resident shells */
    int64_t n_zeta_temperatures;         /* NT >= 2 */
    const double *level_energy;          /* [K] erg */
    const double *level_g;               /* [K] > 0 */
    const int32_t *level_metastable;     /* [K] */
    const int64_t *ion_level_edge;       /* [I+1] */
    const int64_t *element_ion_edge;     /* [E+1] */
    const double *ion_charge;            /* [I] 0, 1, 2, ... */
    const double *ionization_energy;     /* [I] erg, from ion i to i + 1 */
    const double *zeta_temperatures;     /* [NT] ascending */
    const double *zeta;                  /* [I][NT] */
    const double *number_density;        /* [E][S] */
    double chi_0;                        /* erg (the reference takes the ionization energy of Ca II) */
    double link_t_rad_t_electron;        /* 0.9 in the reference */
} TardisMcPlasmaData;

typedef struct TardisMcPlasmaUpdate {
    const double *t_radiative;           /* [S] */
    const double *dilution_factor;       /* [S] */
    int32_t ionization_mode;             /* 0 nebular, 1 lte */
    int32_t excitation_mode;             /* 0 dilute-lte, 1 lte */
    int32_t j_blues_mode;                /* as in TardisMcOpacityUpdate (mode 0 uses t_radiative / dilution_factor above) */
    double time_of_simulation;           /* mode 1 */
    const double *volume;                /* [S], mode 1 */
    double w_epsilon;                    /* mode 1 */
    int32_t detailed_optical_window;     /* mode 1 */
} TardisMcPlasmaUpdate;

/* Static plasma data of the resident topology; after tardis_mc_set_line_data, and dropped like the line data by tardis_mc_set_opacity
 * (and by a later set_line_data).  Everything is checked on the host before anything is indexed: TARDIS_MC_ERR_INVALID_ARGUMENT when
 * n_levels differs from the line data's or n_shells from the resident tables', when an edge table does not run from 0 to its count or an
 * ion has no level / an element no ion, when a level_g is not positive, when the first level of an ion has a negative energy, when
 * NT < 2 or zeta_temperatures does not ascend, or a pointer is missing; TARDIS_MC_ERR_STATE without line data. */
int tardis_mc_set_plasma_data(TardisMcContext *ctx, const TardisMcPlasmaData *plasma_data);
/* One iteration's plasma: solves the populations, writes them over the resident n_t[S][K], installs the solved n_e as the resident
 * electron density and runs the stages of tardis_mc_update_opacity on them -- afterwards the context is indistinguishable from one
 * that received the same populations and n_e through tardis_mc_update_opacity.  TARDIS_MC_ERR_STATE without plasma data or geometry,
 * in mode 1 without propagated estimators, when the electron density becomes NaN (the reference's PlasmaIonizationError) and when the
 * iteration has not converged after option "plasma_max_iterations" passes (default 1000) -- in both cases the opacity state of before
 * the call stays as it was (tables, electron densities, tardis_mc_last_opacity_update_ms; tardis_mc_last_propagate_ms then reports the
 * failed solve's kernels, tardis_mc_get_plasma and tardis_mc_last_plasma_update_ms have nothing to report until the next successful
 * update); TARDIS_MC_ERR_INVALID_ARGUMENT for an unknown mode and, with ionization_mode 0, when some t_radiative lies
 * outside [zeta_temperatures[0], zeta_temperatures[NT-1]]; TARDIS_MC_ERR_UNSUPPORTED for more than 1024 shells. */
int tardis_mc_update_plasma(TardisMcContext *ctx, const TardisMcPlasmaUpdate *update);
/* The solved plasma: level_number_density [K,S], ion_number_density [I,S], partition_function [I,S], electron_density [S], the
 * passes of the iteration.  Any pointer may be NULL.  TARDIS_MC_ERR_STATE unless a tardis_mc_update_plasma produced the resident
 * populations (before the first one, after a failed one, after tardis_mc_update_opacity or set_opacity). */
int tardis_mc_get_plasma(TardisMcContext *ctx, double *level_number_density, double *ion_number_density, double *partition_function,
                         double *electron_density, int32_t *iterations);
/* Device time of the four plasma stages of the last tardis_mc_update_plasma, in ms (any pointer may be NULL): Boltzmann factors |
 * partition functions | phi and the iteration | populations.  tardis_mc_last_opacity_update_ms reports the three stages behind them
 * (no transpose in its first).  TARDIS_MC_ERR_STATE before the first update. */
int tardis_mc_last_plasma_update_ms(TardisMcContext *ctx, double *out_boltzmann_ms, double *out_partition_ms, double *out_ionization_ms,
                                    double *out_population_ms);
/* Which form of the partition kernel an ion of `levels` levels takes (csrc/plasma_update_plan.hpp): 0 a lane per (ion, shell), 1 a
 * 16-lane row per (ion, shell).  Host only; both forms add in the same order.  Option "plasma_update_long_rows" (-1, the default:
 * this rule; n >= 0: ions of n levels or more take the row form -- measurements and tests only). */
int tardis_mc_plasma_update_path(int64_t levels);

/* ---- NLTE excitation of selected species inside tardis_mc_update_plasma --------------------------------------------------------
 * What the legacy plasma computes for a configuration with plasma.nlte.species: LevelBoltzmannFactorNLTE._calculate_general /
 * _main_nlte_calculation for atomic data without collision_data.  With NLTE data installed, tardis_mc_update_plasma runs this stage
 * between the Boltzmann and the partition stage; it replaces the dilute-LTE / LTE Boltzmann factors of the species' levels BEFORE the
 * partition functions, and every later stage (Z, phi, the n_e iteration, the populations, the opacity stages) runs unchanged on them.
 * All arithmetic is fp64 with no contraction; every product, quotient and difference is rounded on its own.
 * For an NLTE species (an ion i of the plasma data with n levels, local index 0 .. n-1 in level order) and a shell s, per line of the
 * species with local lower level l and upper level u (level_lower / level_upper of the line data minus ion_level_edge[i]):
 *   j    = the mean intensity the same update stores for that (line, shell), bit for bit: j_blues_mode 0 the dilute black body of the
 *          call's t_radiative and dilution_factor, mode 1 the j_blues of tardis_mc_radiation_field; 0.0 with coronal_approximation
 *   beta = the resident beta_sobolev of the PREVIOUS update; 1.0 when no update has produced one since the last tardis_mc_set_opacity
 *          (the reference's previous_beta_sobolev is None), and 1.0 with classical_nebular
 *   r_ul = (A_ul + B_ul j) beta;   r_lu = (B_lu j) beta
 *   M[l][u] = r_ul, M[u][l] = r_lu (the row is the destination, the column the source); every other off-diagonal entry 0.0
 *   M[c][c] = -(the serial sum, from 0.0, of column c's off-diagonal entries in row order)
 *       (the reference sums the whole column while its diagonal is still 0.0; adding 0.0 changes nothing)
 *   then M[0][.] = 1.0 and b = (1, 0, ..., 0)
 * M x = b by unblocked LU with partial pivoting, in exactly this order.  For k = 0 .. n-1: p = the lowest row index >= k with the
 * largest |M[.][k]|; rows k and p of M and b are swapped; for i > k: l_i = M[i][k] / M[k][k]; for i, j > k: M[i][j] = M[i][j] - l_i M[k][j];
 * for i > k: b[i] = b[i] - l_i b[k].  Back substitution, column-oriented, for j = n-1 .. 0: x[j] = b[j] / M[j][j]; for i < j:
 * b[i] = b[i] - M[i][j] x[j].  Every entry sees its updates in the same order whatever the parallel decomposition: the device result
 * equals a serial restatement (tests/nlte_excitation_ref.py) bit for bit.
 *       (LAPACK's blocked dgetrf behind numpy.linalg.solve, which the reference uses, sums in another order and contracts: like the
 *       partition functions' compensated sum above, agreement with TARDIS is to rounding, not bitwise)
 * The solve fails (the reference's LinAlgError) when a pivot is 0.0 or not finite, when x[0] is 0.0 or when any x is not finite.
 *   lbf[k] = (x[k] g_0) / x[0], g_0 the level_g of the species' first level
 * The stimulated-emission factor needs no change: the existing clamp of negative values is what the reference does for the lines of
 * NLTE species.  NOT covered here: the collision matrix of atomic data with collision_data (the next section
 * adds it); helium_treatment recomb-nlte: tardis_mc_set_ionization_options; the continuum rate stage: tardis_mc_set_continuum_data; not covered at all: NLTE ionization, continuum transport.
 * Kernels (csrc/nlte_excitation.hpp): a streaming kernel writes r_ul / r_lu of the NLTE lines; then one workgroup per (species, shell)
 * builds and solves the system on a column-major matrix of odd leading dimension, either in its LDS (species of up to 141 levels) or in
 * a slab of HBM per (species, shell) -- same operations, same order, same bits (csrc/nlte_plan.hpp chooses per species).  No workgroup
 * waits on another, no atomics: two calls give identical bits.
 * A species in HBM has a third form, the blocked one: a right-looking LU in panels of 32 columns.  One workgroup per (species, shell)
 * eliminates inside a panel serially in k, multipliers kept in place below the diagonal; then workgroups all over the chip, each the
 * owner of 32 whole columns right of the panel (b is the last of them), apply the panel's row swaps to their columns, form their part
 * of the row block U by the recurrence u_k = ((a_k - l_k0 u_0) - l_k1 u_1) - ... and update the rows below as acc = a_ij, then
 * acc = acc - l_ik u_kj for the panel's k in ascending order: the products are never summed first, nothing is fused, so an entry sees
 * exactly the roundings the unblocked order gives it, in the same order, and the pivot search meets the same column.  The three forms
 * therefore give the same bits (tests/nlte_blocked_ref.py restates the blocked order in NumPy and compares).  Launches follow each other
 * in stream order and nothing else orders them: no workgroup waits on another, no flags, no atomics; a system that has failed is
 * skipped by the launches behind it. */
typedef struct TardisMcNlteData {
    int64_t n_species;                   /* NS */
    const int64_t *species_ion;          /* [NS] indices into the plasma data's ions, distinct */
    int64_t n_nlte_lines;                /* NL */
    const int64_t *species_line_edge;    /* [NS+1]: a species' lines are contiguous in the next four arrays */
    const int64_t *line_id;              /* [NL] indices into the resident line list */
    const double *A_ul;                  /* [NL] */
    const double *B_ul;                  /* [NL] */
    const double *B_lu;                  /* [NL] */
    int32_t coronal_approximation;       /* j = 0.0 */
    int32_t classical_nebular;           /* beta = 1.0 */
} TardisMcNlteData;

/* The NLTE species of the resident plasma data; after tardis_mc_set_plasma_data, dropped by whatever drops the plasma data
 * (tardis_mc_set_opacity, set_line_data, set_plasma_data); nlte_data == NULL removes it.  Everything is checked on the host before
 * anything is indexed: TARDIS_MC_ERR_INVALID_ARGUMENT for an ion index out of range or repeated, an edge table that does not run from 0
 * to NL, a line_id outside [0, L), a line whose levels are not both inside its species' ion, lower == upper, and a pair of levels
 * that two lines of a species share in either direction (the reference's fancy assignment would silently keep the last);
 * TARDIS_MC_ERR_STATE without plasma data; TARDIS_MC_ERR_UNSUPPORTED when the slabs of the global-memory form, over all shells, would
 * exceed 1 GiB (the message names the species and the bytes; the forms follow option "nlte_lds_levels", so a later
 * tardis_mc_update_plasma answers the same, before it touches anything, when the option has since moved a species that large into
 * the global form).  With NLTE data installed a failed NLTE solve makes
 * tardis_mc_update_plasma return TARDIS_MC_ERR_STATE -- the message names the species, the shell and the elimination step --; it has
 * written only the Boltzmann factors, so, as for a failed n_e iteration, the opacity state, the electron densities and
 * tardis_mc_get_opacity are those of before the call. */
int tardis_mc_set_nlte_data(TardisMcContext *ctx, const TardisMcNlteData *nlte_data);
/* The host-side check of tardis_mc_set_nlte_data on plain arrays, without a context or a device: ion_level_edge [n_ions + 1] of the
 * plasma data, level_lower / level_upper [n_lines] of the line data.  0 or TARDIS_MC_ERR_INVALID_ARGUMENT (the message:
 * tardis_mc_last_error(NULL)). */
int tardis_mc_check_nlte_data(const TardisMcNlteData *nlte_data, int64_t n_ions, const int64_t *ion_level_edge, int64_t n_lines,
                              const int64_t *level_lower, const int64_t *level_upper);
/* The NLTE stage's results of the last tardis_mc_update_plasma: level_boltzmann_factor [K,S] (all levels, the NLTE species' rows
 * overwritten) and relative_populations, the solutions x, [sum of n over the species][S] in species order.  Either pointer may be
 * NULL.  TARDIS_MC_ERR_STATE unless the last successful tardis_mc_update_plasma ran the stage and its populations are still resident. */
int tardis_mc_get_nlte(TardisMcContext *ctx, double *level_boltzmann_factor, double *relative_populations);
/* Device time of the NLTE stage of the last tardis_mc_update_plasma, in ms: the rates kernel (j, beta -> r_ul, r_lu of every NLTE line)
 * | the (species, shell) workgroups (matrix, elimination, substitution, write-out; a matrix that lives in LDS cannot be timed apart
 * from its solve).  tardis_mc_last_plasma_update_ms keeps its four outputs; its Boltzmann and partition figures exclude this stage.
 * TARDIS_MC_ERR_STATE unless the last update ran the stage. */
int tardis_mc_last_nlte_ms(TardisMcContext *ctx, double *out_assemble_ms, double *out_solve_ms);
/* Which form of the solve kernel a species of `levels` levels takes (csrc/nlte_plan.hpp): 0 the LDS form, 1 the global-memory form.
 * Host only; both forms run the same operations in the same order.  Option "nlte_lds_levels" (-1, the default: this rule; n >= 0:
 * species of n levels or more take the global form -- measurements and tests only).  Where the matrix lives: a species in the
 * blocked form answers 1. */
int tardis_mc_nlte_solve_path(int64_t levels);
/* Which form of the solve a species of `levels` levels takes under the rule (csrc/nlte_plan.hpp): 0 the LDS form, 1 the one-workgroup
 * global-memory form, 2 the blocked form (panels by one workgroup, the trailing update over the whole chip).  Host only.  Option
 * "nlte_blocked_levels" (-1, the default: this rule; n >= 0: of the species that are not in LDS those of n levels or more take the
 * blocked form, 0: all of them -- measurements and tests only); with "nlte_lds_levels" = 0 it reaches every species. */
int tardis_mc_nlte_solve_form(int64_t levels);

/* ---- collisional rates in the NLTE excitation stage (atomic data with collision_data) -------------------------------------------
 * What LevelBoltzmannFactorNLTE._calculate_general adds to every species' rate matrix when the atomic data carry collision_data:
 * get_collision_matrix(species, t_electrons) * previous_electron_densities.  With collision data installed beside the NLTE data, the
 * NLTE stage of tardis_mc_update_plasma forms, for an NLTE species with pairs, a shell s and a pair (l, u) of local level numbers of
 * the species' ion with l < u -- all arithmetic fp64 with no contraction, exp the transport's own (mcm::exp), every product, quotient
 * and sum a rounding of its own:
 *   t_e   = link_t_rad_t_electron t_rad[s]   (the product the plasma stage forms; t_rad the call's t_radiative)
 *   c_ul  = the pair's C_ul[.] interpolated linearly in t_e over collision_temperatures, by the rule stated for zeta above:
 *           hi = clip(searchsorted(collision_temperatures, t_e, side="left"), 1, NT-1), lo = hi - 1,
 *           slope = (y[hi] - y[lo]) / (x[hi] - x[lo]);  c_ul = slope (t_e - x[lo]) + y[lo]   (one division, one product, one sum);
 *           a NaN result becomes 0.0 (the reference zeroes NaN after interpolating: Chianti has none at the cool end of some pairs)
 *   c_lu  = (c_ul exp(-delta_e / t_e)) inv_g_ratio
 *           delta_e in kelvin, as collision_data.delta_e is; inv_g_ratio = 1 / g_ratio, formed once on the host when the data are set
 *           (the reference flips g_ratio when it builds its matrices)
 *   n_e   = the resident electron density of shell s AT ENTRY to the call: what tardis_mc_set_opacity, tardis_mc_update_opacity or
 *           the previous tardis_mc_update_plasma installed (the reference's previous_electron_densities)
 *   M[l][u] = r_ul + c_ul n_e;   M[u][l] = r_lu + c_lu n_e
 *           r as in the section above, 0.0 where the pair has no line; where a line has no collision pair the entry is r itself,
 *           bit for bit (nothing is added to it)
 * The diagonal (minus the serial sum of the column's off-diagonal entries), the row of ones, b, the LU factorisation, the failure
 * rules and lbf are those of the section above, unchanged.  coronal_approximation and classical_nebular act on j and beta only, as in
 * the reference.  A level no line reaches but a pair does no longer makes the matrix singular.
 * Against numpy.linalg.solve the restatement (tests/nlte_collision_ref.py) differs by at most 1.7e-14 relative in a population on the
 * test models' systems (8.6e-13 without collision data, above; bound 1e-11): to rounding, not bitwise, for the reason given there.
 * Kernels (csrc/nlte_excitation.hpp): nlte_collision_kernel streams the pairs of a shell, finds the bracket once per workgroup, reads
 * C_ul stored as [NT][NP] and writes c_ul / c_lu [S][NP]; nlte_solve_kernel adds c n_e of its species' pairs between the scatter of the
 * line rates and the column sums (one writer per entry: a repeated pair is refused), in its LDS form and in its global form alike:
 * same operations, same order, same bits.  The working set does not grow; the 141-level boundary stays.  No atomics.
 * Without collision data installed every path produces the bits it produced before. */
typedef struct TardisMcNlteCollisionData {
    int64_t n_species;                   /* NS, the installed NLTE data's */
    int64_t n_temperatures;              /* NT >= 2 */
    const double *collision_temperatures;/* [NT] kelvin, ascending */
    int64_t n_pairs;                     /* NP */
    const int64_t *species_pair_edge;    /* [NS+1]: a species' pairs are contiguous in the next five arrays (an empty range: no data) */
    const int64_t *level_lower;          /* [NP] local to the species' ion, 0 .. n-1 */
    const int64_t *level_upper;          /* [NP] local, > level_lower */
    const double *delta_e;               /* [NP] kelvin, finite */
    const double *g_ratio;               /* [NP] g_lower / g_upper as collision_data has it, finite and positive */
    const double *C_ul;                  /* [NP][NT]; NaN allowed */
} TardisMcNlteCollisionData;

/* The collision data of the installed NLTE species; after tardis_mc_set_nlte_data, dropped by whatever drops the NLTE data (a later
 * tardis_mc_set_nlte_data, NULL included, and tardis_mc_set_opacity, set_line_data, set_plasma_data); collision_data == NULL removes
 * it.  Everything is checked on the host before anything is indexed or uploaded: TARDIS_MC_ERR_INVALID_ARGUMENT for an n_species that
 * is not the NLTE data's, NT < 2 or temperatures that do not ascend, an edge table that does not run from 0 to NP, a level outside the
 * species' ion, lower >= upper, a pair repeated within a species, a g_ratio that is not finite and positive, a delta_e that is not
 * finite, a missing pointer; TARDIS_MC_ERR_STATE without NLTE data.  Pairs sorted by (lower, upper) within a species give the solve
 * kernel's added phase its best LDS access pattern; any order gives the same bits.
 * With collision data installed tardis_mc_update_plasma returns TARDIS_MC_ERR_INVALID_ARGUMENT when some t_e lies outside
 * [collision_temperatures[0], collision_temperatures[NT-1]] (scipy's interp1d bounds error; a t_e exactly on the first or last knot
 * is inside), checked on the host from the call's t_radiative before a kernel runs: the state stays as it was. */
int tardis_mc_set_nlte_collision_data(TardisMcContext *ctx, const TardisMcNlteCollisionData *collision_data);
/* The host-side check of tardis_mc_set_nlte_collision_data on plain arrays, without a context or a device: n_species and
 * species_levels [n_species] are the NLTE data's species and the level counts of their ions.  With t_radiative != NULL
 * ([n_shells]) also the bounds rule of tardis_mc_update_plasma for link_t_rad_t_electron.  0 or TARDIS_MC_ERR_INVALID_ARGUMENT (the
 * message: tardis_mc_last_error(NULL)). */
int tardis_mc_check_nlte_collision_data(const TardisMcNlteCollisionData *collision_data, int64_t n_species, const int64_t *species_levels,
                                        double link_t_rad_t_electron, int64_t n_shells, const double *t_radiative);
/* c_ul and c_lu [NP,S] as the last tardis_mc_update_plasma formed them, before the product with n_e.  Either pointer may be NULL.
 * TARDIS_MC_ERR_STATE unless the last successful tardis_mc_update_plasma ran the NLTE stage with collision data and its populations
 * are still resident.  tardis_mc_last_nlte_ms keeps its two outputs: the collision kernel counts under assemble_ms, the added phase
 * of the solve kernel under solve_ms. */
int tardis_mc_get_nlte_collision_rates(TardisMcContext *ctx, double *c_ul, double *c_lu);

/* ---- two switches of the nebular ionisation stage: helium_treatment recomb-nlte and delta_treatment ----------------------------
 * What the legacy plasma computes for a configuration with plasma.helium_treatment: recomb-nlte (HeliumNLTE, the He-rich models of
 * Type Ib / IIb) and / or plasma.delta_treatment: a number.  Both are properties of the installed options, like the NLTE data:
 * tardis_mc_update_plasma takes no argument for them.  fp64, no contraction, exp the transport's own (mcm::exp), every product and sum
 * a rounding of its own.  Notation of the plasma section above: lbf[k] the level Boltzmann factors as the Boltzmann stage (and the NLTE
 * stage, if any) left them -- with W on the non-metastable levels in dilute-lte --, g_e, beta_rad, t_e, zeta, delta, chi_i.
 * delta_treatment (use_delta_treatment 1): delta = delta_treatment for every ion and shell replaces both branches of the
 *   RadiationFieldCorrection expression; everything else of the nebular phi is unchanged; no exp is evaluated for delta.  In
 *   ionization_mode 1 (lte) there is no delta and the switch has no effect.
 * helium_treatment 1 (recomb-nlte): the ions a, a+1, a+2 of the element helium_element are He I, He II, He III; g1 = level_g of
 *   He II's first level, g2 = that of He III's only level.  Once per update and shell, the relative populations hp[k] of helium's levels:
 *     He I, first level:    0.0
 *     He I, other levels:   (((lbf[k] (1 / (2 g1))) (1 / g_e)) (1 / (W W))) exp(chi_a beta_rad)
 *     He II, first level:   1.0
 *     He II, other levels:  lbf[k] (1 / g1)
 *     He III:               (((((2 (g2 / g1)) g_e) exp(chi_(a+1) (-beta_rad))) W) ((delta_(a+1) zeta_(a+1)) + W (1 - zeta_(a+1)))) sqrt(t_e / t_rad)
 *                           (delta_(a+1) honours use_delta_treatment)
 *   Helium is no post-processing step: it sits INSIDE the electron-density iteration.  In every pass, after the ordinary ion
 *   populations of all elements -- helium included -- have been formed with this pass's n_e and cut at 1e-20:
 *     u[k] = hp[k] n_e for the levels of He I, u[k] = hp[k] for those of He II and He III
 *     total = the serial sum of u in level order (He I, He II, He III), from 0.0
 *     f = number_density[helium_element] / total;   v[k] = u[k] f
 *     N[a] = the serial sum of v over He I's levels from 0.0, N[a+1] likewise over He II's, N[a+2] = v[He III]
 *   These three rows replace the ordinary ones; the 1e-20 cut is NOT applied to them (the reference cuts before it overwrites).  The
 *   new n_e is the serial sum over all ion rows of N_i ion_charge[i] in the order stated above, the helium rows replaced.  The NaN
 *   vote, the 5 % rule in every shell and the averaging are unchanged.  After the iteration the populations of helium's levels are
 *   the v of the last pass -- the pass whose n_e is handed out --, not (lbf / Z) N; all other levels as above.
 *   tardis_mc_get_plasma then returns the replaced rows in ion_number_density, v in level_number_density and the unchanged
 *   partition_function; the opacity stages run on these populations.
 * Kernels (csrc/plasma_update.hpp): helium_relative_kernel, a thread per (helium level, shell), writes hp as [K_He][S] behind the NLTE
 * stage; the ionisation kernel has a compile-time helium form in which a lane (= shell) runs the three serial sums of a pass over
 * hp[.][s], the loads issued in batches ahead of the dependent adds, and writes v once, from the n_e it hands out; a small kernel
 * behind the population kernel copies v over helium's levels of n_t.  With no options installed the instantiation of before runs.  No
 * atomics: two calls give identical bits.  Not covered: helium_treatment numerical-nlte (it reads an external file), NLTE
 * ionisation, continuum transport (the photo-ionisation data and the continuum rate stage: tardis_mc_set_continuum_data below). */
typedef struct TardisMcIonizationOptions {
    int32_t helium_treatment;     /* 0 none, 1 recomb-nlte */
    int32_t use_delta_treatment;  /* 0: RadiationFieldCorrection as documented above; 1: delta = delta_treatment for every ion and shell */
    int64_t helium_element;       /* row of element_ion_edge; read only with helium_treatment 1 */
    double  delta_treatment;      /* read only with use_delta_treatment 1; must be finite */
} TardisMcIonizationOptions;

/* The options of the resident plasma data; after tardis_mc_set_plasma_data (TARDIS_MC_ERR_STATE before it), dropped by whatever drops
 * the plasma data (tardis_mc_set_opacity, set_line_data, set_plasma_data) and by nothing else -- tardis_mc_set_nlte_data and
 * tardis_mc_set_nlte_collision_data keep them; options == NULL clears them.  The call clears what was installed before it validates:
 * a refused call leaves none.  Checked on the host before anything is indexed (tardis_mc_check_ionization_options):
 * TARDIS_MC_ERR_INVALID_ARGUMENT for an unknown helium_treatment, a delta_treatment that is not finite, a helium_element outside
 * [0, E), a helium element without exactly three ions, ion charges other than 0, 1, 2, a He III without exactly one level; the
 * message names which.  With options installed tardis_mc_update_plasma returns TARDIS_MC_ERR_INVALID_ARGUMENT, before the device is
 * touched, for helium_treatment 1 with ionization_mode 1 and for helium_treatment 1 while an installed NLTE species is one of the
 * three helium ions (both would write the same Boltzmann factors' consumers; no order is defined). */
int tardis_mc_set_ionization_options(TardisMcContext *ctx, const TardisMcIonizationOptions *options);
/* The host-side check of tardis_mc_set_ionization_options on plain arrays, without a context or a device: element_ion_edge
 * [n_elements + 1], ion_level_edge and ion_charge of the plasma data (read only with helium_treatment 1).  0 or
 * TARDIS_MC_ERR_INVALID_ARGUMENT (the message: tardis_mc_last_error(NULL)). */
int tardis_mc_check_ionization_options(const TardisMcIonizationOptions *options, int64_t n_elements, const int64_t *element_ion_edge,
                                       const int64_t *ion_level_edge, const double *ion_charge);
/* Helium of the last successful tardis_mc_update_plasma: relative_population (hp) and level_number_density (the v of the pass whose
 * n_e was handed out), [K_He,S] each, K_He the level count of the helium element.  Either pointer may be NULL.
 * TARDIS_MC_ERR_STATE when that update ran without helium_treatment, after a failed update, and whenever tardis_mc_get_plasma
 * answers TARDIS_MC_ERR_STATE. */
int tardis_mc_get_helium(TardisMcContext *ctx, double *relative_population, double *level_number_density);
/* Device time of helium_relative_kernel in the last tardis_mc_update_plasma, in ms (the helium form of the iteration counts under
 * out_ionization_ms of tardis_mc_last_plasma_update_ms, whose partition figure excludes this kernel).  TARDIS_MC_ERR_STATE unless
 * the last update ran with helium_treatment. */
int tardis_mc_last_helium_ms(TardisMcContext *ctx, double *out_relative_ms);

/* ---- photo-ionisation data and the continuum stage of tardis_mc_update_plasma: rate coefficients, chi_bf, the free-free factor ----
 * What plasma.continuum_interaction.species adds to the legacy plasma, up to the opacity state's continuum fields: the Saha factors, the
 * photo-ionisation, recombination and collisional-ionisation rate coefficients in the dilute black body, the resident bound-free
 * opacity table, the free-free factor, and the function that evaluates the continuum opacity at a frequency in a shell.  It restates
 * SahaFactor, SpontRecombRateCoeff, PhotoIonRateCoeff (dilute Planckian field), StimRecombRateCoeff, CorrPhotoIonRateCoeff,
 * CollIonRateCoeffSeaton, CollRecombRateCoeff, BoundFreeOpacity, ff_opacity_factor, chi_continuum_calculator / chi_bf_interpolator /
 * chi_ff_calculator.  Like NLTE it is a property of the installed data: tardis_mc_update_plasma takes no argument for it.  With
 * continuum data installed the stage runs behind the population stage of a solve that SUCCEEDED, on that update's populations; it reads
 * nothing of the opacity stages and writes nothing they read; it feeds back into nothing.  A failed electron-density iteration or NLTE
 * solve returns before it.  Without continuum data no launch of the update changes.  Transport kernels do not read any of this yet.
 * The radiation field is the dilute black body of the call's t_radiative and dilution_factor, also with j_blues_mode 1, unless the
 * option "continuum_field" is 1: then gamma and alpha_stim come from the transport's photo-ionisation estimators (the section after the
 * cooling sub-stage).
 * fp64, no contraction, exp the transport's own (mcm::exp); every product, quotient, sum and difference a rounding of its own, in
 * exactly the order written; the constants of the plasma section (CODATA 2010 cgs) and c = 2.99792458e10.
 * Per shell:
 *   t_e = link_t_rad_t_electron t_rad;   beta_e = 1 / (k_B t_e);   beta_rad = 1 / (k_B t_rad)
 *   x = (((2 pi) m_e) / beta_e) / (h h);   g_ee = x sqrt(x)
 *   lbf_e[k] = level_g[k] exp(level_energy[k] (-beta_e))      every level: thermal LTE -- no W, no NLTE replacement, no helium treatment
 *   Z_e[i] = the serial sum of the ion's lbf_e in level order, from 0.0
 * Per continuum c, its level k in ion i, the upper ion i + 1:
 *   saha = (Z_e[i+1] / Z_e[i]) ((2 g_ee) exp(chi_i (-beta_e)));   saha == 0.0 becomes DBL_MIN
 *   phi_ik[c] = lbf_e[k] / (saha Z_e[i])
 * Per point p of its block, nu = nu[p]:
 *   bfp[p] = exp((h nu) (-beta_e))
 *   J[p] = W ((planck_coef ((nu nu) nu)) / (exp((h nu) beta_rad) - 1)),  planck_coef = (2 h) / (c c)   (the opacity stage's dilute black body)
 *   y_sp[p] = ((((8 pi) x_sect[p]) (nu nu)) / (c c)) bfp[p]
 *   y_g[p] = J[p] ((((4 pi) x_sect[p]) / nu) / h);   y_st[p] = y_g[p] bfp[p]
 * Over a block [a, b):  T(y) = the serial sum from 0.0, j = a .. b-2, of ((nu[j+1] - nu[j]) (y[j+1] + y[j])) / 2.0  (numpy.trapz forms the
 *   same terms and adds them pairwise: agreement with the reference is to rounding, not bitwise, as for the partition functions).
 * Rates, n_i = the update's population of level k, N_up = N[i+1], n_e the solved electron density:
 *   alpha_sp = T(y_sp) phi_ik;   gamma = T(y_g);   alpha_stim = T(y_st) phi_ik
 *   gamma_corr = gamma - ((alpha_stim N_up) n_e) / n_i;  with n_i == 0.0: gamma_corr = gamma (THIS PROJECT'S DECISION: the reference
 *     divides by zero there); a negative result becomes 0.0 and is counted
 *   u0 = (nu_i / t_e) (h / k_B), nu_i the block's first frequency;   f = exp(-u0) / u0
 *   coll_ion = ((f (1.55e13 x_sect[a])) / sqrt(t_e)) gbar,  gbar = 0.1, 0.2, 0.3 for ion_charge[i] 0, 1, >= 2
 *   coll_recomb = coll_ion phi_ik
 * Bound-free opacity per point:  n_lte = (phi_ik N_up) n_e;   chi_bf[p] = (n_i - n_lte bfp[p]) x_sect[p];  a negative value becomes
 *   0.0 and is counted.  THIS PROJECT'S DECISION: the reference raises a PlasmaException on a negative value; a stage that feeds nothing
 *   must not fail the update, so the count is reported (tardis_mc_get_continuum_opacity) and the caller decides.
 * Free-free per shell:  q = the serial sum over ALL ion rows, in row order from 0.0, of N_i (ion_charge[i] ion_charge[i]);
 *   ff_opacity_factor = (n_e q) / sqrt(t_e)
 * The opacity at a frequency nu in shell s (tardis_mc_continuum_opacity; csrc/continuum_opacity.hpp holds the __device__ function):
 *   current = the continua c, in ascending c, with nu_min[c] <= nu <= nu_max[c] (a block's first and last frequency)
 *   per current c, on its block b[0 .. n):  hi = clip(searchsorted(b, nu, side="left"), 1, n - 1);  lo = hi - 1
 *     interval = b[hi] - b[lo];  hw = nu - b[lo];  lw = b[hi] - nu
 *     chi_c = ((chi_bf[hi] hw) + (chi_bf[lo] lw)) / interval;   x_c likewise from x_sect
 *     THIS PROJECT'S DECISION: the clip at 1.  The reference indexes [-1] when nu equals a block's first frequency, a wrap-around
 *     artefact; here that frequency takes the block's first interval and gives chi_bf[first point].
 *   chi_bf_tot = the serial sum of chi_c in ascending c, from 0.0
 *   chi_ff = ((FF_OPAC_CONST ff_opacity_factor[s]) / ((nu nu) nu)) (1 - exp((h nu) (-beta_e[s])))
 *   FF_OPAC_CONST = sqrt((2 pi) / ((3 m_e) k_B)) ((4 e^6) / (((3 m_e) h) c)) with e = 4.80320451e-10 esu, e^6 = ((((e e) e) e) e) e,
 *   evaluated once: 3.6923492443190485e+08.
 * Kernels (csrc/continuum_rates.hpp), ONE form each: a thread per shell (t_e, the free-free factor); the LTE Boltzmann kernel and the
 * partition kernels of the plasma stage on t_e (both partition forms add in the same order); a streaming kernel over (point, shell)
 * for bfp and the integrands; a thread per (continuum, shell) that forms phi_ik, walks its block serially and writes the seven rate
 * tables; a streaming kernel for chi_bf.  The clamps are counted per workgroup and the host adds the counts.  The resident chi_bf is
 * [NP][S], the shell fastest -- what the getter returns, and the layout in which a reader in shell s touches two rows per current
 * continuum.  No second form for long blocks is built, hence no tardis_mc_continuum_path.  No atomics: two calls give identical bits.
 * Not covered: continuum events in transport, NLTE
 * ionisation, collisional excitation, p_fb_deactivation (the cooling rates, the free-bound emission CDFs and the k-packet samplers:
 * the section after this one). */
typedef struct TardisMcContinuumData {
    int64_t n_continua;          /* NC >= 1: levels that have a cross-section table */
    const int64_t *level;        /* [NC] indices into the plasma data's levels, strictly ascending */
    const int64_t *block_edge;   /* [NC+1] photo_ion_block_references: 0 .. NP, every block >= 2 points */
    int64_t n_points;            /* NP */
    const double *nu;            /* [NP] Hz, > 0, strictly ascending inside a block; a block's first nu is the threshold nu_i */
    const double *x_sect;        /* [NP] cm^2, finite, >= 0 */
} TardisMcContinuumData;

/* The photo-ionisation data of the resident plasma data; after tardis_mc_set_plasma_data (TARDIS_MC_ERR_STATE before it), dropped by
 * whatever drops the plasma data (tardis_mc_set_opacity, set_line_data, set_plasma_data) and by nothing else -- tardis_mc_set_nlte_data,
 * tardis_mc_set_nlte_collision_data and tardis_mc_set_ionization_options keep them; data == NULL removes them.  The call removes what
 * was installed before it validates: a refused call leaves none.  Everything is checked on the host before anything is indexed or
 * uploaded (tardis_mc_check_continuum_data). */
int tardis_mc_set_continuum_data(TardisMcContext *ctx, const TardisMcContinuumData *data);
/* The host-side check of tardis_mc_set_continuum_data on plain arrays, without a context or a device: n_levels = K and n_ions = I of the
 * plasma data, ion_level_edge [I + 1], element_ion_edge (it runs from 0 to I).  0 or TARDIS_MC_ERR_INVALID_ARGUMENT, the message
 * (tardis_mc_last_error(NULL)) naming the rule and the first offending index: a missing pointer or NC < 1; an edge table that does not
 * run from 0 to NP or a block of fewer than 2 points; a level outside [0, K) or not strictly ascending; a level whose ion is its
 * element's last ion (there is no upper ion); a nu that is not finite and positive or does not ascend strictly inside its block; an
 * x_sect that is not finite or is negative. */
int tardis_mc_check_continuum_data(const TardisMcContinuumData *data, int64_t n_levels, int64_t n_ions, const int64_t *ion_level_edge,
                                   const int64_t *element_ion_edge);
/* The rate coefficients of the last successful tardis_mc_update_plasma, [NC,S] each; any pointer may be NULL.  TARDIS_MC_ERR_STATE
 * unless that update ran the continuum stage and its populations are still resident (whenever tardis_mc_get_plasma answers
 * TARDIS_MC_ERR_STATE: before any update, after a failed one, after tardis_mc_update_opacity / set_opacity). */
int tardis_mc_get_continuum_rates(TardisMcContext *ctx, double *phi_ik, double *alpha_sp, double *gamma, double *alpha_stim, double *gamma_corr,
                                  double *coll_ion, double *coll_recomb);
/* chi_bf [NP,S], ff_opacity_factor [S], the stage's t_electrons [S] and the two clamp counts of that update; any pointer may be NULL.
 * The state rule of tardis_mc_get_continuum_rates. */
int tardis_mc_get_continuum_opacity(TardisMcContext *ctx, double *chi_bf, double *ff_opacity_factor, double *t_electrons,
                                    int64_t *n_negative_chi_bf, int64_t *n_negative_gamma_corr);
/* Device time of the stage in the last tardis_mc_update_plasma, in ms: thermal (t_e, the free-free factor, lbf_e, Z_e), points (bfp and
 * the integrands), rates, opacity (chi_bf).  tardis_mc_last_plasma_update_ms, tardis_mc_last_opacity_update_ms and the other timers keep
 * their outputs: their figures exclude this stage.  TARDIS_MC_ERR_STATE unless the last update ran the stage. */
int tardis_mc_last_continuum_ms(TardisMcContext *ctx, double *out_thermal_ms, double *out_points_ms, double *out_rates_ms, double *out_opacity_ms);

typedef struct TardisMcContinuumQuery {
    int64_t n;  const double *nu;  const int64_t *shell;      /* [n]; nu finite and > 0, shell in [0, S) -- checked on the host */
    double *chi_bf_tot, *chi_ff;  int64_t *n_current;          /* [n] each, any may be NULL */
    double *chi_bf_each, *x_sect_each;                         /* [n][NC], 0.0 where c is not current; either may be NULL (tests, small n) */
} TardisMcContinuumQuery;
/* The continuum opacity of the resident tables at n (frequency, shell) pairs, a thread per query, through the __device__ function of
 * csrc/continuum_opacity.hpp.  TARDIS_MC_ERR_INVALID_ARGUMENT, before the device is touched, for a nu that is not finite and positive
 * or a shell outside [0, S); the state rule of tardis_mc_get_continuum_rates. */
int tardis_mc_continuum_opacity(TardisMcContext *ctx, const TardisMcContinuumQuery *query);

/* ---- the cooling sub-stage behind the continuum stage: cooling rates, free-bound emission CDFs, the k-packet table and its samplers ----
 * What a continuum event needs when a packet's energy becomes thermal: what the k-packet turns into, and at which frequency it comes
 * back.  It restates SpontRecombCoolingRateCoeff, FreeBoundEmissionCDF, FreeBoundCoolingRate, CollIonCooling, FreeFreeCoolingRate,
 * AdiabaticCoolingRate, the cumulative cooling table of the k-packet and the samplers sample_nu_free_bound / sample_nu_free_free.  The
 * sub-stage runs whenever the continuum stage runs, behind its chi_bf kernel and on its tables (bfp, y_sp, phi_ik, coll_ion, t_e) and
 * that update's populations; it writes only its own tables and feeds back into nothing.  Without continuum data no launch of the update
 * changes; with them every output the update had keeps its bits.  Transport kernels do not read any of this yet.
 * The rules of the section above: fp64, no contraction, mcm::exp and mcm::log for the two transcendental functions; every product,
 * quotient, sum and difference a rounding of its own, in exactly the order written; every sum a serial sum from 0.0; the constants of
 * the plasma section and c = 2.99792458e10.
 * Per point p of continuum c (level k, ion i, upper ion i + 1, block [a, b), nu_i = nu[a]), nu = nu[p], shell s:
 *   y_cool[p] = (y_sp[p] (h nu)) (1.0 - nu_i / nu)        (SpontRecombCoolingRateCoeff: 8 pi x h nu^3 / c^2 (1 - nu_i / nu) e^(-h nu / k T_e))
 *   y_em[p] = (((nu nu) nu) x_sect[p]) bfp[p]             (FreeBoundEmissionCDF: the prefactors dropped, only ratios matter)
 * Per (continuum, shell), T the serial trapezoid of the section above:
 *   c_fb_sp = T(y_cool) phi_ik
 *   E[a] = 0.0;  E[j+1] = E[j] + ((nu[j+1] - nu[j]) (y_em[j+1] + y_em[j])) / 2.0;   fb_emission_cdf[p] = E[p] / E[b-1]
 *     THIS PROJECT'S DECISION: where E[b-1] is not positive and finite, the block's CDF is 0.0 at every point but the last and 1.0 at
 *     the last, and the case is counted (n_degenerate_fb_cdf).  The reference produces NaN there.  Such a continuum has
 *     cool_rate_fb == 0.0 wherever bfp underflowed, and is then never chosen.
 *   cool_rate_fb = (c_fb_sp N_up) n_e                                   (FreeBoundCoolingRate)
 *   cool_rate_coll_ion = ((coll_ion n_e) n_i) (h nu_i)                  (CollIonCooling)
 * Per shell, q the free-free sum of the section above, time_explosion that of the resident geometry:
 *   cool_rate_ff = ((C0_FF n_e) sqrt(t_e)) q,  C0_FF = 1.426e-27        (FreeFreeCoolingRate)
 *   cool_rate_adiabatic = (((3.0 n_e) k_B) t_e) / time_explosion        (AdiabaticCoolingRate)
 * The k-packet table k_cdf [2 + 2 NC][S], the shell fastest; its entries in this order: ff, adiabatic, cool_rate_fb[0 .. NC),
 *   cool_rate_coll_ion[0 .. NC).  R[j] = the serial running sum from 0.0;  cool_rate_total = R[last];  k_cdf[j] = R[j] / cool_rate_total,
 *   so the last entry is exactly 1.0.  A successful solve has n_e > 0, so the adiabatic entry makes the total positive.
 *   THIS PROJECT'S DECISION: collisional-excitation cooling is NOT in the table.  It needs a coll_exc_coeff for every line, a data rung
 *   the plasma does not have; it is the next entry to add.
 * The samplers (csrc/kpacket_sample.hpp holds the __device__ functions; z a random number in [0, 1)):
 *   process(shell, z):  j = min(searchsorted(k_cdf[:, s], z, side="right"), last): entry j is chosen iff k_cdf[j-1] <= z < k_cdf[j], so
 *     an entry of zero rate is never chosen.  kind = 0 ff (j = 0), 1 adiabatic (j = 1), 2 fb (continuum j - 2), 3 coll_ion (continuum
 *     j - 2 - NC); continuum = -1 for kinds 0 and 1.
 *   nu_free_bound(c, shell, z), numpy.interp on the block:  hi = clip(searchsorted(cdf_block, z, side="right"), 1, n - 1);  lo = hi - 1
 *     nu = nu[lo] + ((z - cdf[lo]) (nu[hi] - nu[lo])) / (cdf[hi] - cdf[lo]);  for z in [0, 1) the denominator is positive, also in a
 *     degenerate block (there every z gives a frequency of the block's last interval).
 *   nu_free_free(shell, z) = (-((k_B t_e) / h)) log(z);  z == 0.0 gives +inf, as in the reference.  (mcm::log's domain is 0 and the
 *     normal numbers: a subnormal z gives an unspecified finite frequency, on the device and in the oracle alike.)
 * Kernels (csrc/cooling_rates.hpp), ONE form each: a streaming kernel over (point, shell) for the two integrands; a thread per
 * (continuum, shell), the shell fastest, that walks its block twice -- T(y_cool) and E[b-1] first, then E[p] again, in the same order and
 * so with the same bits, written as the quotient -- and writes c_fb_sp, the two rate tables and the normalised CDF; a thread per shell
 * that forms q, the two shell rates and walks the 2 + 2 NC entries twice in the same way.  The degenerate CDFs are counted per workgroup
 * and the host adds the counts.  The tables are [rows][S] with adjacent lanes on adjacent shells; the samplers' bisections read a column
 * and stride by S.  No second form for long blocks is built (the reason of the section above; profiles/cooling_rates.txt has the times).
 * No atomics: two calls give identical bits.
 * Not covered: collisional-excitation cooling and the coll_exc_coeff data it needs; the macro-atom continuum transition probabilities
 * (p_fb_deactivation, the recombination / photo-ionisation / collisional rows); the choice of the absorbing continuum at a bound-free
 * event; NLTE ionisation; any reader of these tables in the propagation kernels. */

/* c_fb_sp, cool_rate_fb, cool_rate_coll_ion [NC,S] and cool_rate_ff, cool_rate_adiabatic, cool_rate_total [S] of the last successful
 * tardis_mc_update_plasma; any pointer may be NULL.  The state rule of tardis_mc_get_continuum_rates: what drops or keeps the continuum
 * data and its tables drops or keeps these. */
int tardis_mc_get_cooling_rates(TardisMcContext *ctx, double *c_fb_sp, double *cool_rate_fb, double *cool_rate_coll_ion, double *cool_rate_ff,
                                double *cool_rate_adiabatic, double *cool_rate_total);
/* fb_emission_cdf [NP,S], k_cdf [2+2NC,S] and the count of degenerate CDFs of that update; any pointer may be NULL.  The state rule of
 * tardis_mc_get_continuum_rates. */
int tardis_mc_get_kpacket_tables(TardisMcContext *ctx, double *fb_emission_cdf, double *k_cdf, int64_t *n_degenerate_fb_cdf);
/* Device time of the sub-stage in the last tardis_mc_update_plasma, in ms, per kernel: points (the two integrands), blocks (c_fb_sp, the
 * two rate tables, the CDFs), table (the shell rates and k_cdf).  Every other timer keeps its outputs: tardis_mc_last_continuum_ms,
 * tardis_mc_last_plasma_update_ms and tardis_mc_last_opacity_update_ms exclude the sub-stage.  TARDIS_MC_ERR_STATE unless the last update
 * ran the continuum stage. */
int tardis_mc_last_cooling_ms(TardisMcContext *ctx, double *out_points_ms, double *out_blocks_ms, double *out_table_ms);

typedef struct TardisMcKpacketQuery {
    int64_t n;  const int64_t *shell;  const double *z_process, *z_nu;   /* [n]; shell in [0, S), both z finite and in [0, 1) -- checked on the host */
    int64_t *kind, *continuum;  double *nu;                               /* [n] each, any may be NULL */
    const int64_t *force_kind, *force_continuum;                          /* [n] or NULL: -1 means sample (tests reach every block with them) */
} TardisMcKpacketQuery;
/* n k-packets on the resident tables, a thread per query, through the __device__ functions of csrc/kpacket_sample.hpp: (kind, continuum)
 * = process(shell, z_process), then nu = nu_free_free(shell, z_nu) for kind 0, nu_free_bound(continuum, shell, z_nu) for kind 2, and 0.0
 * for kinds 1 and 3.  With force_kind[q] in 0 .. 3 the kind is that one and z_process[q] is not used; kinds 2 and 3 then take
 * force_continuum[q], which must lie in [0, NC); wherever no continuum is forced (force_kind[q] of -1, 0 or 1) force_continuum[q] must
 * be -1 (or the array NULL).  TARDIS_MC_ERR_INVALID_ARGUMENT, before the device is touched, for a shell outside [0, S), a z that is not
 * finite or lies outside [0, 1), a force_kind outside [-1, 3] and a forced continuum outside [0, NC); the state rule of
 * tardis_mc_get_continuum_rates. */
int tardis_mc_kpacket_sample(TardisMcContext *ctx, const TardisMcKpacketQuery *query);

/* ---- photo-ionisation and heating estimators from the transport, on the device (csrc/bf_estimators.hpp) ----
 * The continuum stage's gamma and alpha_stim integrate the dilute black body; this is the field the packets actually carried.  The
 * formulas below restate update_bound_free_estimators, and PhotoIonRateCoeff / StimRecombRateCoeff with estimators, of the reference;
 * the reference tree was not at hand, so they are this header's contract, with ONE decision of this project named below.
 * Option "bf_estimators" (0/1, default 0).  With it a propagate call runs on the instantiations that full tracking runs on -- the
 * wave-owner kernel with group sweeps (variant 2) where "track_full" would, else the lane kernel (variant 0); variants 1, 3 and 4 are not
 * instrumented -- and logs one 24-byte record {comov_nu, ed, shell} per move of a packet:
 *   comov_nu = nu doppler_factor,  comov_energy = energy doppler_factor  (the values of the J / nu_bar update of that move)
 *   ed = comov_energy distance,  distance = the trace's distance BEFORE full relativity scales it by the Doppler factor: under partial
 *   relativity ed is bit for bit the term added to J, and ed comov_nu the term added to nu_bar.
 *   THIS PROJECT'S DECISION: a move of length zero writes no record (it would add 0.0 to the four sums and 1 to the statistics only):
 *   the statistics count the moves of positive length.
 * The records go to a pool of chunks with the event log's mechanics (csrc/event_log.hpp: one claim function for both logs); event rows
 * stay tied to "track_full": a call with the estimators on and full tracking off writes segment records only, both may be on together.
 * "segment_log_capacity" (records; 0 = automatic, 96 per packet; the pool's chunks have the event log's size, 128 records, and like that
 * log's pool it holds one more chunk per wave and launch than the capacity asks for), "segment_log_max_bytes" (default 16 GiB; a call over
 * it, or one whose pool would reach 2^32 slots, fails with TARDIS_MC_ERR_INVALID_ARGUMENT like "event_log_max_bytes"), "segment_log_keep" (tests: the
 * records stay readable through tardis_mc_get_segment_log).  With the option off every launch, every instantiation chosen and every
 * per-packet bit is as before.  With it on and no tardis_mc_set_bf_estimators, tardis_mc_propagate fails with TARDIS_MC_ERR_STATE before
 * it launches anything.
 * The accumulate pass runs at the end of every tardis_mc_propagate that logged, on the context's stream behind the last propagation
 * launch (tardis_mc_synchronize covers it), and consumes the log.  Five tables [NC,S], the shell fastest: photo_ion, stim_recomb,
 * bf_heating, stim_recomb_cooling (float64) and statistics (int64).  They accumulate across propagate calls as J does;
 * tardis_mc_reset_estimators zeroes them.  fp64, no contraction, exp = mcm::exp, every operation a rounding of its own in the order
 * written; h and k_B of the plasma section.  Per record (nu, ed, s):
 *   beta_e = 1 / (k_B t_e[s]);   bfac = exp((h nu) (-beta_e))
 * per continuum c that is current (nu_min[c] <= nu <= nu_max[c]), x_c interpolated exactly as tardis_mc_continuum_opacity does (the
 * same __device__ function), nu_i = the block's first frequency:
 *   inc = (ed x_c) / nu;   heat = (ed x_c) (1.0 - nu_i / nu)
 *   photo_ion[c,s] += inc;  stim_recomb[c,s] += inc bfac;  bf_heating[c,s] += heat;  stim_recomb_cooling[c,s] += heat bfac;  statistics[c,s] += 1
 * Every term is non-negative; the order of a cell's sum is not specified (fp64 atomics), the statistics are exact.
 * Kernels: the record slots grouped by shell with the three grouping kernels of csrc/estimator_log.hpp; then a workgroup per (shell,
 * slice of <= 65536 records) that stages batches of records in LDS (the staging thread computes bfac), every thread owning continua
 * whose bounds and five sums it keeps in registers, and one set of fp64 atomics per thread and slice.  The continua are served 256 at a
 * time, a pass over the slice each: bfac is computed once per record and PASS, i.e. ceil(NC / 256) times.  More than 36864 shells are
 * refused (the grouping's LDS histogram).  Measured on an MI355X: profiles/bf_estimators.txt.
 * Rates:  norm[s] = 1.0 / ((time_of_simulation volume[s]) h);  gamma_est = photo_ion norm;  stim_est = stim_recomb norm.
 * Option "continuum_field": 0 (default) the dilute black body; 1: the continuum stage of tardis_mc_update_plasma takes
 * gamma = gamma_est[c,s] and alpha_stim = stim_est[c,s] phi_ik instead of T(y_g) and T(y_st) phi_ik; gamma_corr by the same expression,
 * alpha_sp, coll_*, chi_bf and the cooling sub-stage unchanged; TARDIS_MC_ERR_STATE from tardis_mc_update_plasma when continuum data are
 * installed and no rates are resident.  With the option 0 every output of the update keeps its bits.
 * Not covered: the heating estimators feed no rate yet; tardis_mc_allreduce_estimators does not carry the tables (ranks add their
 * downloads); variants 1, 3 and 4. */
typedef struct TardisMcBfEstimatorSetup {
    const double *t_electrons;   /* [S] K, finite and > 0: an explicit input -- the continuum stage's own t_e is dropped by tardis_mc_update_opacity */
} TardisMcBfEstimatorSetup;
/* Installs t_electrons and the zeroed tables; setup == NULL switches the estimators off and frees the tables.  TARDIS_MC_ERR_STATE
 * without installed continuum data or geometry; TARDIS_MC_ERR_INVALID_ARGUMENT for a temperature that is not finite and positive.
 * Whatever drops the continuum data drops this, and so does a geometry with another number of shells. */
int tardis_mc_set_bf_estimators(TardisMcContext *ctx, const TardisMcBfEstimatorSetup *setup);
/* The host-side check of tardis_mc_set_bf_estimators, without a context or a device: 0 or TARDIS_MC_ERR_INVALID_ARGUMENT, the message
 * (tardis_mc_last_error(NULL)) naming the first offending index. */
int tardis_mc_check_bf_estimator_setup(const TardisMcBfEstimatorSetup *setup, int64_t n_shells);
/* The five tables [NC,S] and the records logged / dropped since the last reset; any pointer may be NULL.  With n_dropped > 0 it returns
 * TARDIS_MC_ERR_STATE after writing the two counts only: raise "segment_log_capacity" or split the packets (the run is deterministic). */
int tardis_mc_get_bf_estimators(TardisMcContext *ctx, double *photo_ion, double *stim_recomb, double *bf_heating, double *stim_recomb_cooling,
                                int64_t *statistics, int64_t *n_records, int64_t *n_dropped);
/* Tests: the records of the last tardis_mc_propagate, in no particular order; needs "segment_log_keep" (else TARDIS_MC_ERR_STATE).
 * *count is always written; the columns (any may be NULL) only when count <= capacity. */
int tardis_mc_get_segment_log(TardisMcContext *ctx, double *nu, double *ed, int64_t *shell, int64_t capacity, int64_t *count);
/* Tests: the accumulate pass alone on n caller-supplied records (checked on the host: nu finite and > 0, ed finite, shell in [0, S))
 * into the resident tables; the records count as logged. */
int tardis_mc_debug_bf_accumulate(TardisMcContext *ctx, int64_t n, const double *nu, const double *ed, const int64_t *shell);
/* Device time of the last accumulate pass in ms: grouping the slots by shell, accumulating.  Excluded from every other timer. */
int tardis_mc_last_bf_estimator_ms(TardisMcContext *ctx, double *out_group_ms, double *out_accumulate_ms);
/* gamma_est and stim_est [NC,S] from the resident tables (volume [S], cm^3; both inputs finite and > 0); resident, and they survive
 * tardis_mc_reset_estimators.  The getter: TARDIS_MC_ERR_STATE before the first call. */
int tardis_mc_bf_estimator_rates(TardisMcContext *ctx, double time_of_simulation, const double *volume);
int tardis_mc_get_bf_estimator_rates(TardisMcContext *ctx, double *gamma_est, double *stim_est);

/* The full r-packet log of the last tardis_mc_propagate (option "track_full"), after tardis_mc_get_results: an exclusive scan of the
 * per-packet row counts into offsets, then the rows scattered packet-major into the caller's columns.  TARDIS_MC_ERR_STATE when the
 * last call ran without full tracking, when a packet of it failed, or when the resident packets were replaced since.  With dropped > 0 only count / dropped / offsets are written: run the call again with
 * event_log_capacity >= count (the run is deterministic). */
int tardis_mc_get_event_log(TardisMcContext *ctx, TardisMcEventLog *log);

/* The v-packet log of the last tardis_mc_propagate, consolidated on the device (csrc/vpacket_log.hpp): one atomic per entry counts the
 * entries per source packet, the event log's scan turns the counts into offsets, and entry k moves to offsets[packet] + seq -- seq is the
 * entry's ordinal within its packet, so nothing is sorted.  The columns stay resident (tardis_mc_vpacket_decomposition reads them) until the
 * next tardis_mc_propagate, tardis_mc_set_packets or tardis_mc_set_config.  tardis_mc_get_results keeps its own host path and outputs.
 * If the call ran without "vpacket_last_interaction" the six last_interaction_* pointers must be NULL (else TARDIS_MC_ERR_STATE); the other
 * columns work either way.  When the device log overflowed (count above vpacket_log_capacity) or count > capacity only count is written and
 * the call returns 0: run again with vpacket_log_capacity >= count (the run is deterministic).  TARDIS_MC_ERR_STATE when the last call did
 * not track v-packets, when a packet of it failed, when the resident packets were replaced since, or when an entry's packet, ordinal or
 * position is out of range (every index is checked on the device before it is used). */
int tardis_mc_get_vpacket_log(TardisMcContext *ctx, TardisMcVpacketLog *log);

/* ---- result streaming (optional).  Registers the caller's per-packet result arrays (output_nus / output_energies and the fourteen li_* arrays of *dst; any may
 * be NULL; the other fields are ignored) as the destination of the NEXT tardis_mc_propagate: a call of the wave-owner kernel that runs as several launches copies the
 * results of the packets handed out so far to these arrays at every launch boundary, beside the next launch, and tardis_mc_get_results -- given the SAME pointers --
 * only copies what is left and the packets that were still in flight when their range was copied.  The arrays must stay valid until tardis_mc_get_results returns.
 * dst = NULL disarms.  Results are identical with and without (tests/test_boundary_gpu.py). */
int tardis_mc_stream_results(TardisMcContext *ctx, const TardisMcResult *dst);
/* What the last tardis_mc_propagate streamed: packets [0, *out_streamed) were copied while the call ran (0: the call did not stream -- one launch, another kernel,
 * fewer packets than the option `stream_min_packets`), *out_resent of them are sent again by tardis_mc_get_results. */
int tardis_mc_streamed_packets(TardisMcContext *ctx, int64_t *out_streamed, int64_t *out_resent);

/* ---- one-shot API: the reference boundary in one call ---------------------------------------------- */
int tardis_mc_run(TardisMcContext *ctx, const TardisMcPackets *packets, const TardisMcGeometry *geometry,
                  const TardisMcOpacity *opacity, const TardisMcConfig *config, TardisMcResult *result);

/* ---- multi-GPU: packets shard by index, one all-reduce of the estimators per iteration (RCCL) ----- */
#define TARDIS_MC_UNIQUE_ID_BYTES 128
int tardis_mc_comm_get_unique_id(uint8_t out_id[TARDIS_MC_UNIQUE_ID_BYTES]);
int tardis_mc_comm_init(TardisMcContext *ctx, int rank, int world_size,
                        const uint8_t id[TARDIS_MC_UNIQUE_ID_BYTES]);
/* In-place sum over ranks of J, nu_bar, j_blue, Edotlu, v-hist (device buffers), on the ctx stream. */
int tardis_mc_allreduce_estimators(TardisMcContext *ctx);
/* Self-check of the communicator (call on every rank after tardis_mc_comm_init): a one-element all-reduce of (rank + 1) must
 * come back as N (N + 1) / 2.  *out_ranks = N on success, 0 otherwise (TARDIS_MC_ERR_COMM / _STATE). */
int tardis_mc_comm_check(TardisMcContext *ctx, int *out_ranks);

/* ---- diagnostics: element-wise device arithmetic, used by the numerics parity tests ------------------
 * op: 0 x+y, 1 x*y, 2 x/y, 3 sqrt(x), 4 log(x) [engine's portable log], 5 exp(x), 6 x*y+x (un-fused),
 *     7 MT19937 doubles of seed (uint32)x[0] (n outputs), 8 floor(x), 9 x/y through the engine's exact 3-fma division;
 *     100 (tests) no arithmetic: the raw 64-byte tracker records the wave-owner kernel left for packets x[0] ... x[0] + n / 8 - 1 of the last
 *     call, 8 doubles each: before_nu, before_mu, before_energy, radius, after_mu, then int32 pairs shell | type, absorb | emit, count | valid.
 *     101 (tests) no arithmetic: n doubles, from its double x[1] on, of the resident prefix-sum table x[0] as the kernels read it (x: two doubles, y unused):
 *         0  the v-packet screening's prefix sums tau_pfx[S][L + 1]            1  its row sums tau_rowsum[S]
 *         2  the block skip's pn[S][L + 1] = {frequency slot, prefix sum}, two doubles per entry
 *         3  its coarse entries ct[S][ceil(L / 8)] = {nu_last, p_end} with the 16 slack entries behind the last row, two doubles per entry
 *         4  its row sums sk_rowsum[S]                                        5  {its margin M, 1.0 if its builder saw a negative or non-finite depth, the padded row length}
 *     TARDIS_MC_ERR_STATE when no propagate call has built that table for the resident opacity state (0, 1: a call that screens v-packets; 2 - 5: a call
 *     whose plan allows the block skip), TARDIS_MC_ERR_INVALID_ARGUMENT for a range that leaves the table. */
int tardis_mc_debug_eval(TardisMcContext *ctx, int op, const double *x, const double *y, double *out, int64_t n);
/* The elimination and back substitution of the blocked form of the NLTE solve on dense systems, for tests: m [n_systems][n][n]
 * row-major, b [n_systems][n]; x [n_systems][n] (rows of a failed system are 0.0) and status [n_systems] (0, 1 + the step of a zero or
 * non-finite pivot, n + 1: x[0] == 0, n + 2: an x that is not finite) come back.  Touches nothing resident, needs no opacity state.
 * TARDIS_MC_ERR_UNSUPPORTED beyond the scratch bound of the global form. */
int tardis_mc_debug_nlte_solve(TardisMcContext *ctx, int64_t n, int64_t n_systems, const double *m, const double *b, double *x, int32_t *status);
/* Plants the line estimators that tardis_mc_source_function reads, for tests: j_blue and edotlu are host arrays [n_lines][n_shells], the layout
 * in which tardis_mc_get_results returns them.  They become copy 0 of the two resident tables and every other copy ("estimator_copies") is zeroed;
 * J, nu_bar and the v-packet histogram keep their values.  Needs a resident opacity state and configuration (TARDIS_MC_ERR_STATE otherwise), allocates
 * the estimators as tardis_mc_reset_estimators would if no call has yet, drops what tardis_mc_reset_estimators drops (the resident source function)
 * and leaves the context, as far as tardis_mc_source_function is concerned, as a tardis_mc_propagate would.  No propagate path reads or calls it. */
int tardis_mc_debug_set_line_estimators(TardisMcContext *ctx, const double *j_blue, const double *edotlu);
/* Memory-system micro-benchmarks used to size the kernels (design input): which = 0 random fp64 atomics (agent
 * scope), 1 same at workgroup scope in a per-XCD slice, 2/3 the same with 16 consecutive doubles per 16 lanes,
 * 4 random 8-byte loads, 5 16-lane-coalesced loads; 15 a wide coalesced copy of the table's first half onto its second (iters
 * passes, n_doubles x 8 bytes of traffic each: the box's streaming rate).  blocks x 256 threads x iters operations; time in ms. */
int tardis_mc_debug_microbench(TardisMcContext *ctx, int which, int64_t n_doubles, int iters, int blocks, double *out_ms);

#ifdef __cplusplus
}
#endif
#endif /* TARDIS_MC_H */
