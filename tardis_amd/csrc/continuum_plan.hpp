// continuum_plan.hpp -- what tardis_mc_set_continuum_data refuses, as a host-only pure function.
//
// Standard C++ only (no HIP header, no context, no device call): tests/test_continuum_host.py drives it through
// tardis_mc_check_continuum_data.  The kernels are in continuum_rates.hpp and continuum_opacity.hpp.
//
// There is ONE form of every continuum kernel (a lane per (continuum, shell) walks its block serially), so there is no path to choose
// and no tardis_mc_continuum_path: photo-ionisation blocks are tens to a few hundred points, the walk is three adds per point on
// loads that do not depend on the running sums, and the stage is measured in profiles/continuum.txt.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>

namespace cont {

// "" or the message: which rule failed and the first offending index.  The edge tables are those of the plasma data (any integer
// type); n_levels = K, n_ions = I.  `level_ion` (may be null) receives the ion of every continuum's level.
template <typename EdgeI, typename EdgeE>
inline std::string check_data(long long n_continua, const int64_t *level, const int64_t *block_edge, long long n_points, const double *nu, const double *x_sect,
                              long long n_levels, long long n_ions, const EdgeI *ion_level_edge, long long n_elements, const EdgeE *element_ion_edge,
                              int *level_ion = nullptr)
{
    char buf[256];
    if (!level || !block_edge || !nu || !x_sect || !ion_level_edge || !element_ion_edge) return "continuum data: a pointer is missing";
    if (n_continua < 1) {
        snprintf(buf, sizeof buf, "continuum data: n_continua = %lld, at least one continuum is needed", n_continua);
        return buf;
    }
    if (n_levels < 1 || n_ions < 1 || n_elements < 1 || n_points > 0x7ffffff0LL || n_continua > 0x7ffffff0LL) return "continuum data: invalid counts";
    if (block_edge[0] != 0 || block_edge[n_continua] != n_points) {
        snprintf(buf, sizeof buf, "continuum data: block_edge must run from 0 to n_points = %lld (it runs from %lld to %lld)", n_points, (long long)block_edge[0],
                 (long long)block_edge[n_continua]);
        return buf;
    }
    for (long long c = 0; c < n_continua; ++c)
        if (block_edge[c + 1] - block_edge[c] < 2 || block_edge[c + 1] > n_points) {
            snprintf(buf, sizeof buf, "continuum data: block %lld has %lld points, a block needs at least 2", c, (long long)(block_edge[c + 1] - block_edge[c]));
            return buf;
        }
    long long i = 0, e = 0;  // (levels ascend: the ion and the element are walked along)
    for (long long c = 0; c < n_continua; ++c) {
        const long long k = level[c];
        if (k < 0 || k >= n_levels) {
            snprintf(buf, sizeof buf, "continuum data: level[%lld] = %lld lies outside [0, %lld)", c, k, n_levels);
            return buf;
        }
        if (c > 0 && k <= level[c - 1]) {
            snprintf(buf, sizeof buf, "continuum data: level[%lld] = %lld does not ascend strictly (level[%lld] = %lld)", c, k, c - 1, (long long)level[c - 1]);
            return buf;
        }
        while (i + 1 < n_ions && (long long)ion_level_edge[i + 1] <= k) ++i;
        while (e + 1 < n_elements && (long long)element_ion_edge[e + 1] <= i) ++e;
        if (i + 1 >= (long long)element_ion_edge[e + 1]) {
            snprintf(buf, sizeof buf, "continuum data: level[%lld] = %lld belongs to ion %lld, the last ion of its element: there is no upper ion", c, k, i);
            return buf;
        }
        if (level_ion) level_ion[c] = (int)i;
    }
    for (long long c = 0; c < n_continua; ++c)
        for (long long p = block_edge[c]; p < block_edge[c + 1]; ++p) {
            if (!(std::isfinite(nu[p]) && nu[p] > 0.0)) {
                snprintf(buf, sizeof buf, "continuum data: nu[%lld] = %g is not finite and positive", p, nu[p]);
                return buf;
            }
            if (p > block_edge[c] && !(nu[p] > nu[p - 1])) {
                snprintf(buf, sizeof buf, "continuum data: nu[%lld] = %g does not ascend strictly inside block %lld", p, nu[p], c);
                return buf;
            }
        }
    for (long long p = 0; p < n_points; ++p)
        if (!(std::isfinite(x_sect[p]) && x_sect[p] >= 0.0)) {
            snprintf(buf, sizeof buf, "continuum data: x_sect[%lld] = %g is not finite and non-negative", p, x_sect[p]);
            return buf;
        }
    return "";
}

}  // namespace cont
