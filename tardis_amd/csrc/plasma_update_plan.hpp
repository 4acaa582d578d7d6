// plasma_update_plan.hpp -- which form of the partition-function kernel of tardis_mc_update_plasma an ion takes: the host's decision as a
// pure function.
//
// Standard C++ only (no HIP header, no context, no device call): tests/test_plasma_update_host.py pins the rule through
// tardis_mc_plasma_update_path.  The kernels are in plasma_update.hpp.
//
// The partition function of an ion of `levels` levels is summed per shell either by one lane (PATH_LANE: the lane walks the ion's
// Boltzmann factors) or by a 16-lane DPP row (PATH_ROW: sixteen consecutive levels per step, the additions carried in level order).  Both
// forms add in the same order, so the choice changes no bit of the result, only the time.  The shape of the problem is that of the
// opacity update's block kernel -- heavy-tailed segment lengths, a serial sum per (segment, shell) over a shell-major table -- so the
// threshold is that kernel's measured one (opacity_update_plan.hpp).  Also here, for the same reason (no device, testable through
// ctypes): check_ionization_options, what tardis_mc_set_ionization_options refuses.  Measured here (profiles/plasma_update.txt): the partition kernel of
// the configs[2] tables (40 ions, the longest of 10 056 levels) takes 1.53 ms with every ion on a lane, 0.288 with every ion on a row and
// 0.293 - 0.301 ms with the row form from 4, 8, 16, 32 or 64 levels; the tardis_example shape 0.092 / 0.023 / 0.026 - 0.033 ms.  The longest
// ion's walk sets the time, the thresholds in between differ by less than the spread: the rule stays the opacity update's.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>
#include "opacity_update_plan.hpp"

namespace plup {

constexpr int PATH_LANE = 0, PATH_ROW = 1;
constexpr long long LONG_ION_LEVELS = opup::LONG_BLOCK_ROWS;  // ions of this many levels or more take a 16-lane row per (ion, shell)
constexpr long long MAX_SHELLS = 1024;                        // the electron-density iteration votes inside one workgroup

// `threshold` < 0: the rule; otherwise ions of `threshold` levels or more take the row form (option plasma_update_long_rows)
inline int choose_path(long long levels, long long threshold = -1)
{
    const long long t = threshold < 0 ? LONG_ION_LEVELS : threshold;
    return levels > 0 && levels >= t ? PATH_ROW : PATH_LANE;
}

// What tardis_mc_set_ionization_options refuses, before anything is indexed: "" or the message.  The edge tables and the charges are
// those of the plasma data (any integer type); they are read only with helium_treatment 1.
template <typename EdgeE, typename EdgeI>
inline std::string check_ionization_options(int helium_treatment, int use_delta_treatment, long long helium_element, double delta_treatment, long long n_elements,
                                            const EdgeE *element_ion_edge, const EdgeI *ion_level_edge, const double *ion_charge)
{
    char buf[256];
    if (helium_treatment != 0 && helium_treatment != 1) {
        snprintf(buf, sizeof buf, "unknown helium_treatment %d (0 none, 1 recomb-nlte)", helium_treatment);
        return buf;
    }
    if (use_delta_treatment && !std::isfinite(delta_treatment)) return "delta_treatment is not finite";
    if (helium_treatment == 0) return "";
    if (n_elements <= 0 || !element_ion_edge || !ion_level_edge || !ion_charge) return "invalid ionization options: the plasma data's tables are missing";
    if (helium_element < 0 || helium_element >= n_elements) {
        snprintf(buf, sizeof buf, "helium_element %lld lies outside [0, %lld)", helium_element, n_elements);
        return buf;
    }
    const long long a = (long long)element_ion_edge[helium_element], b = (long long)element_ion_edge[helium_element + 1];
    if (b - a != 3) {
        snprintf(buf, sizeof buf, "the helium element (element %lld) has %lld ions, not the three He I, He II, He III", helium_element, b - a);
        return buf;
    }
    if (ion_charge[a] != 0.0 || ion_charge[a + 1] != 1.0 || ion_charge[a + 2] != 2.0) {
        snprintf(buf, sizeof buf, "the ions of the helium element carry the charges %g, %g, %g, not 0, 1, 2", ion_charge[a], ion_charge[a + 1], ion_charge[a + 2]);
        return buf;
    }
    const long long last = (long long)ion_level_edge[a + 3] - (long long)ion_level_edge[a + 2];
    if (last != 1) {
        snprintf(buf, sizeof buf, "He III (ion %lld) has %lld levels, not exactly one level", a + 2, last);
        return buf;
    }
    return "";
}

}  // namespace plup
