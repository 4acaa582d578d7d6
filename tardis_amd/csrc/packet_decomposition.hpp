// packet_decomposition.hpp -- the emitted spectrum decomposed by last interaction, from the per-packet results resident after a
// propagate call with the last-interaction tracker on (tardis_mc_packet_decomposition, include/tardis_mc.h).
//
// What the reference's users compute on the host from the tracker's dataframe: emission and absorption by species (SDEC), the
// last-interaction-velocity histogram (LIV) and the per-line packet counts of LastLineInteraction.  One lane per packet with a grid
// stride streams seven 8-byte arrays (output_nu, output_energy, li_interaction_type, li_line_emit_id, li_line_absorb_id, li_before_nu,
// li_shell_id: 56 B per packet), gathers the caller's class of a line from an int32 table (2 MB at 5e5 lines: it stays in L2) and adds
// the packet's luminosity to a few small matrices.
//
// Two accumulation paths, chosen on the host (decomposition_plan.hpp):
//   privatised  every workgroup keeps the double cells and the shell counts in LDS (ds_add_f64 / ds_add_u64) and flushes its non-zero
//               cells once with global atomics -- few cells and many packets would otherwise serialise on a handful of addresses;
//   direct      global fp64 / 64-bit integer atomics straight to the matrices (many cells, e.g. 30-100 species x 1e4 bins).
// The per-line counts ([n_lines]) always go to HBM.  The four scalar counts are kept per lane and reduced per workgroup.
//
// The double sums are sums of non-negative addends in an order that atomics decide: two calls agree to (n - 1) 2^-53 relatively in a
// cell of n addends; a cell without addends is exactly 0.  The integer outputs are exact.
#pragma once

#include "mc_device.hpp"

namespace mc {

// numpy.histogram's bin of x on ascending edges[0..B]: bin k holds edges[k] <= x < edges[k + 1], the last bin is closed on the right,
// a value outside [edges[0], edges[B]] (or NaN) has none (-1).  Starts from the uniform estimate and pins it with the actual edge
// values.  e0 = edges[0], eN = edges[B], inv_delta = B / (eN - e0).
__device__ __forceinline__ int spectrum_bin(const double *__restrict__ edges, int B, double e0, double eN, double inv_delta, double x)
{
    if (!(x >= e0 && x <= eN)) return -1;
    int k = (int)((x - e0) * inv_delta);
    k = k < 0 ? 0 : (k > B - 1 ? B - 1 : k);
    while (k > 0 && x < edges[k]) --k;
    while (k < B - 1 && x >= edges[k + 1]) ++k;
    return k;
}

constexpr int DC_LINE = 2, DC_ESCATTERING = 4, DC_NO_INTERACTION = -1;  // InteractionType, interaction_events.py
constexpr int DC_BLOCK = 256;

struct DecompositionArgs {
    // the resident per-packet results
    const double *out_nu, *out_e, *before_nu;
    const long long *type, *emit_id, *absorb_id, *shell_id;
    long long n_packets;
    // the caller's grouping of the lines (validated on the host: every value in [0, n_classes)), the spectrum grid
    const int *line_class;
    long long n_lines, n_classes;
    const double *edges;
    int n_edges, n_shells;
    double t_sim, nu_start, nu_end;
    // outputs, zeroed by the host
    double *cells;                      // [(2 C + 2) B]: emission [C][B] | absorption [C][B] | no_interaction [B] | electron_scatter [B]
    unsigned long long *shell_packets;  // [(C + 1) S]
    unsigned long long *line_emit, *line_absorb;  // [L]
    unsigned long long *counts;         // {selected, line, electron scatter, no interaction}
};

template <bool PRIV>
__global__ __launch_bounds__(DC_BLOCK) void packet_decomposition_kernel(const DecompositionArgs a)
{
    extern __shared__ double dc_private[];  // the workgroup's four scalar counts; PRIV: then its copy of cells and of shell_packets
    const int B = a.n_edges - 1;
    const long long C = a.n_classes, S = a.n_shells, L = a.n_lines;
    const long long n_cells = (2 * C + 2) * B, n_shell = (C + 1) * S;
    unsigned long long *block_counts = reinterpret_cast<unsigned long long *>(dc_private);
    double *l_cells = dc_private + 4;
    unsigned long long *l_shell = reinterpret_cast<unsigned long long *>(l_cells + n_cells);
    if (threadIdx.x < 4) block_counts[threadIdx.x] = 0;
    if (PRIV) {
        for (long long i = threadIdx.x; i < n_cells; i += DC_BLOCK) l_cells[i] = 0.0;
        for (long long i = threadIdx.x; i < n_shell; i += DC_BLOCK) l_shell[i] = 0;
    }
    __syncthreads();
    auto add_cell = [&](long long idx, double l) {
        if (PRIV) atomicAdd(&l_cells[idx], l); else atomic_add_f64(&a.cells[idx], l);
    };
    auto add_shell = [&](long long idx) {
        if (PRIV) atomicAdd(&l_shell[idx], 1ull); else atomicAdd(&a.shell_packets[idx], 1ull);
    };
    const double e0 = a.edges[0], eN = a.edges[B];
    const double inv_delta = (double)B / (eN - e0);
    unsigned long long n_sel = 0, n_line = 0, n_es = 0, n_none = 0;
    for (long long i = (long long)blockIdx.x * DC_BLOCK + threadIdx.x; i < a.n_packets; i += (long long)gridDim.x * DC_BLOCK) {
        const double e = a.out_e[i], nu = a.out_nu[i], nu_in = a.before_nu[i];
        const long long type = a.type[i], le = a.emit_id[i], la = a.absorb_id[i], sh = a.shell_id[i];
        if (!(e >= 0) || !(nu > a.nu_start && nu < a.nu_end)) continue;  // emitted, inside the strict window
        const double l = e / a.t_sim;
        const int k = spectrum_bin(a.edges, B, e0, eN, inv_delta, nu);
        const bool shell_ok = (unsigned long long)sh < (unsigned long long)S;
        ++n_sel;
        if (type == DC_LINE) {
            ++n_line;
            if ((unsigned long long)le < (unsigned long long)L) {
                const long long c = a.line_class[le];
                if (k >= 0) add_cell(c * B + k, l);
                if (shell_ok) add_shell(c * S + sh);
                atomicAdd(&a.line_emit[le], 1ull);
            }
            if ((unsigned long long)la < (unsigned long long)L) {
                const long long c = a.line_class[la];
                const int k_in = spectrum_bin(a.edges, B, e0, eN, inv_delta, nu_in);
                if (k_in >= 0) add_cell((C + c) * B + k_in, l);
                atomicAdd(&a.line_absorb[la], 1ull);
            }
        } else if (type == DC_ESCATTERING) {
            ++n_es;
            if (k >= 0) add_cell((2 * C + 1) * B + k, l);
            if (shell_ok) add_shell(C * S + sh);
        } else if (type == DC_NO_INTERACTION) {
            ++n_none;
            if (k >= 0) add_cell(2 * C * B + k, l);
        }
    }
    if (n_sel) atomicAdd(&block_counts[0], n_sel);
    if (n_line) atomicAdd(&block_counts[1], n_line);
    if (n_es) atomicAdd(&block_counts[2], n_es);
    if (n_none) atomicAdd(&block_counts[3], n_none);
    __syncthreads();
    if (threadIdx.x < 4 && block_counts[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], block_counts[threadIdx.x]);
    if (PRIV) {
        for (long long i = threadIdx.x; i < n_cells; i += DC_BLOCK) {
            const double v = l_cells[i];
            if (v != 0.0) atomic_add_f64(&a.cells[i], v);
        }
        for (long long i = threadIdx.x; i < n_shell; i += DC_BLOCK) {
            const unsigned long long v = l_shell[i];
            if (v) atomicAdd(&a.shell_packets[i], v);
        }
    }
}

}  // namespace mc
