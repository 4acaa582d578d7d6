// decomposition_plan.hpp -- which accumulation path tardis_mc_packet_decomposition takes: the host's decision as a pure function.
//
// Standard C++ only (no HIP header, no context, no device call): tests/test_packet_decomposition_host.py compiles it with a host
// compiler and pins the rule.  The kernels are in packet_decomposition.hpp.
//
// A workgroup of the privatised path keeps a copy of every small output in LDS: the (2 C + 2) B double cells (emission and absorption
// per class, no interaction, electron scattering) and the (C + 1) S shell counts, 8 bytes each, behind the four scalar counts that
// every workgroup of either path keeps there.  The budget is 64 KiB per workgroup:
// two workgroups fit the 160 KiB of a CU, and no launch attribute is needed for it.  Whatever does not fit goes straight to HBM with
// global atomics (the direct path: the SDEC case of 30-100 species x 1e4 bins, where the cells are many and contention is low).
#pragma once

namespace decomp {

constexpr long long LDS_BUDGET_BYTES = 64 * 1024;
constexpr long long FIXED_BYTES = 4 * 8;  // the four scalar counts of a workgroup (both paths)
constexpr int PATH_PRIVATISED = 0, PATH_DIRECT = 1;

// LDS bytes of one workgroup's private copy, or -1 where that is beyond any budget (a dimension that alone exceeds it: no overflow below)
inline long long private_bytes(long long n_classes, long long n_bins, long long n_shells)
{
    const long long cap = LDS_BUDGET_BYTES / 8;
    if (n_classes < 1 || n_bins < 1 || n_shells < 0) return -1;
    if (n_classes > cap || n_bins > cap || n_shells > cap) return -1;
    return FIXED_BYTES + ((2 * n_classes + 2) * n_bins + (n_classes + 1) * n_shells) * 8;
}

inline int choose_path(long long n_classes, long long n_bins, long long n_shells)
{
    const long long bytes = private_bytes(n_classes, n_bins, n_shells);
    return bytes >= 0 && bytes <= LDS_BUDGET_BYTES ? PATH_PRIVATISED : PATH_DIRECT;
}

}  // namespace decomp
