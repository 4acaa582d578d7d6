// nlte_plan.hpp -- the host's decisions of the NLTE excitation stage of tardis_mc_update_plasma as pure functions: which form of the
// solve kernel a species takes, what the forms cost in LDS and scratch, which species go into which launch, and the check of a
// TardisMcNlteData before anything is indexed.
//
// Standard C++ only (no HIP header, no context, no device call): tests/test_nlte_excitation_host.py pins the rule through
// tardis_mc_nlte_solve_path and the check through tardis_mc_check_nlte_data, tests/test_nlte_plan.py the launches through a shim around
// plan_launches.  The kernels are in nlte_excitation.hpp.
// Likewise the check of a TardisMcNlteCollisionData and the bounds rule of its temperature grid (tests/test_nlte_collision_host.py
// through tardis_mc_check_nlte_collision_data); the collisional rates add to entries the matrix already has, so the working set, the
// LDS limit, the size classes and the 141-level boundary are what they were.
//
// A species of n levels is solved per shell by one workgroup on a column-major n x n fp64 matrix of leading dimension ld = n | 1 (odd:
// a walk along a row then visits 32 different bank pairs) and four vectors of n (b, the multipliers of a step, the pivots, x).  The
// matrix and the vectors live either in the workgroup's LDS (PATH_LDS) or in a slab of HBM per (species, shell) (PATH_GLOBAL); the code
// and the order of every operation are the same, so the choice changes no bit of the result, only the time.  A workgroup may declare
// 163 840 bytes on gfx950: work_bytes(141) = 163 560 fits, work_bytes(142) does not.  Measured (profiles/nlte_excitation.txt, each
// species alone, all 20 shells): the LDS form is ahead at every size that fits -- 0.010 against 0.012 ms at 2 levels, 0.157 / 0.255
// at 61, 0.509 / 0.951 at 125 -- so the rule is "LDS whenever it fits".
// A species in HBM is eliminated either by its one workgroup (FORM_GLOBAL) or by the blocked form (FORM_BLOCKED: panels by one
// workgroup, the trailing update by workgroups all over the chip); choose_form and plan_blocked below, pinned by
// tests/test_nlte_blocked_plan.py.  Same slab, same roundings, same order: same bits again.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace nlte {

constexpr int PATH_LDS = 0, PATH_GLOBAL = 1;
constexpr long long LDS_LIMIT_BYTES = 163840;             // what one workgroup may declare on gfx950
constexpr long long MAX_SCRATCH_BYTES = 1LL << 30;        // all slabs of the global form together, over every shell
// LDS launches go out per size class (dynamic LDS sized for the class's largest species), so that a species of a few levels does not
// cost the occupancy of one of a hundred
constexpr long long LDS_CLASS_LEVELS[] = {8, 16, 32, 64, 96, 141};
constexpr int N_LDS_CLASSES = 6;

inline long long leading_dimension(long long n) { return n | 1; }
// the matrix and the four vectors b, l, pivots, x
inline long long work_bytes(long long n) { return n <= 0 ? 0 : 8 * (leading_dimension(n) * n + 4 * n); }

// species of this many levels or more take the global form under the rule: the first size whose working set no longer fits the LDS
constexpr long long GLOBAL_FORM_LEVELS = 142;

// `threshold` < 0: the rule; otherwise species of `threshold` levels or more take the global form (option nlte_lds_levels).  A species
// that does not fit the LDS takes the global form whatever the option says.
inline int choose_path(long long levels, long long threshold = -1)
{
    const long long t = threshold < 0 ? GLOBAL_FORM_LEVELS : threshold;
    if (levels <= 0) return PATH_LDS;
    return levels >= t || work_bytes(levels) > LDS_LIMIT_BYTES ? PATH_GLOBAL : PATH_LDS;
}

inline int lds_class(long long levels)
{
    for (int c = 0; c < N_LDS_CLASSES; ++c)
        if (levels <= LDS_CLASS_LEVELS[c]) return c;
    return N_LDS_CLASSES - 1;
}

// The launches of the solve kernel for species of levels[sp] levels over n_shells shells and a value of option nlte_lds_levels (`threshold`,
// as in choose_path).  `list`: the order the species are launched in; `slab`, parallel to it: the offset in doubles of a species' first slab
// in the scratch of the global form (0 in the LDS form); a launch covers list[first .. first + count).  The LDS form goes out per size
// class in class order, a class in index order, with the working set of its largest member as dynamic LDS; then one launch of the global
// form in index order, a slab of work_bytes per (species, shell).  refused >= 0: that species' slabs (refused_bytes), alone or with the
// refused_before_bytes of those before it, exceed MAX_SCRATCH_BYTES; nothing else of the plan is to be used then.
struct Launch { int first, count; size_t lds_bytes; bool global; };
struct LaunchPlan {
    std::vector<int> list;
    std::vector<long long> slab;
    std::vector<Launch> launches;
    long long scratch_doubles = 0, refused = -1, refused_bytes = 0, refused_before_bytes = 0;  // (scratch_doubles: all slabs of the global form)
    size_t max_lds_bytes = 0;  // the largest dynamic LDS a launch asks for
};
inline LaunchPlan plan_launches(const std::vector<int> &levels, long long n_shells, long long threshold = -1)
{
    LaunchPlan p;
    const int NS = (int)levels.size();
    for (int c = 0; c < N_LDS_CLASSES; ++c) {
        const int first = (int)p.list.size();
        long long largest = 0;
        for (int sp = 0; sp < NS; ++sp)
            if (choose_path(levels[sp], threshold) == PATH_LDS && lds_class(levels[sp]) == c) { p.list.push_back(sp); largest = std::max<long long>(largest, levels[sp]); }
        if ((int)p.list.size() > first) p.launches.push_back({first, (int)p.list.size() - first, (size_t)work_bytes(largest), false});
        p.max_lds_bytes = std::max(p.max_lds_bytes, (size_t)work_bytes(largest));
    }
    p.slab.assign(p.list.size(), 0);
    const int first = (int)p.list.size();
    for (int sp = 0; sp < NS; ++sp) {
        if (choose_path(levels[sp], threshold) != PATH_GLOBAL) continue;
        p.list.push_back(sp);
        p.slab.push_back(p.scratch_doubles);
        const long long bytes = work_bytes(levels[sp]) * n_shells;
        if (bytes > MAX_SCRATCH_BYTES || p.scratch_doubles * 8 + bytes > MAX_SCRATCH_BYTES) {
            p.refused = sp; p.refused_bytes = bytes; p.refused_before_bytes = p.scratch_doubles * 8;
            return p;
        }
        p.scratch_doubles += bytes / 8;
    }
    if ((int)p.list.size() > first) p.launches.push_back({first, (int)p.list.size() - first, 0, true});
    return p;
}

// The blocked form: a species in HBM whose elimination is spread over the chip (nlte_excitation.hpp).  Panels of PANEL_COLUMNS columns are
// factored by one workgroup per (species, shell); the trailing matrix, with b as its last column, is updated by workgroups that each own
// a strip of TILE_COLUMNS whole columns (a row swap moves entries along a column, so a column has one owner and no workgroup waits on
// another) and walk it in blocks of TILE_ROWS rows.  The slab is the one of the global form: same layout, same bytes, same offsets.
constexpr int FORM_LDS = 0, FORM_GLOBAL = 1, FORM_BLOCKED = 2;
constexpr int PANEL_COLUMNS = 32;                         // NB
constexpr int TILE_COLUMNS = 32, TILE_ROWS = 128;         // a 256-thread workgroup holds 4 x 4 entries per thread in registers
// species of this many levels or more, of those that are not in LDS, take the blocked form under the rule.  Measured
// (profiles/nlte_blocked.txt, each species alone, all 20 shells, one-workgroup / blocked solve in ms): 1.61 / 0.80 at 158 levels,
// 4.04 / 1.43 at 234, 16.5 / 3.45 at 400, 76.7 / 6.78 at 586, 513 / 20.3 at 1071 -- the blocked form is ahead at every measured size,
// by far more than the arms' spread, and 158 is the smallest of them (the synthetic data have no ion of 142 .. 157 levels)
constexpr long long BLOCKED_FORM_LEVELS = 158;

// `lds_threshold` as in choose_path; `blocked_threshold` < 0: the rule, otherwise species of that many levels or more that are not in
// LDS take the blocked form (option nlte_blocked_levels; 0: every one of them).  A species choose_path puts in LDS is never blocked.
inline int choose_form(long long levels, long long lds_threshold = -1, long long blocked_threshold = -1)
{
    if (choose_path(levels, lds_threshold) == PATH_LDS) return FORM_LDS;
    return levels >= (blocked_threshold < 0 ? BLOCKED_FORM_LEVELS : blocked_threshold) ? FORM_BLOCKED : FORM_GLOBAL;
}

inline long long panel_steps(long long n) { return n <= 0 ? 0 : (n + PANEL_COLUMNS - 1) / PANEL_COLUMNS; }
// the strips of the trailing launch of the panel that starts at column c0: the columns right of the panel, and b
inline long long trailing_strips(long long n, long long c0)
{
    if (c0 >= n) return 0;
    const long long right = n - std::min<long long>(n, c0 + PANEL_COLUMNS) + 1;
    return (right + TILE_COLUMNS - 1) / TILE_COLUMNS;
}

// The species of `plan`'s launch of the global form (if it has one), split by choose_form: `single` keeps the one-workgroup kernel,
// `blocked` takes the blocked form; both in the plan's order, each with the slab offsets plan_launches assigned.  The blocked set is
// eliminated in `steps` = ceil(max n / PANEL_COLUMNS) panel steps; step t (c0 = t PANEL_COLUMNS) is one panel launch of
// (panel_x, panel_y) = (blocked species, shells) workgroups and one trailing launch of (trailing_x, trailing_y, trailing_z) = (the most
// strips a blocked species still has, blocked species, shells).  Workgroups past a species' last panel or strip exit.
struct BlockedStep { unsigned panel_x, panel_y, trailing_x, trailing_y, trailing_z; };
struct BlockedPlan {
    std::vector<int> single, blocked;
    std::vector<long long> single_slab, blocked_slab;
    std::vector<BlockedStep> steps;
};
inline BlockedPlan plan_blocked(const LaunchPlan &plan, const std::vector<int> &levels, long long n_shells, long long blocked_threshold = -1)
{
    BlockedPlan b;
    long long largest = 0;
    for (const Launch &l : plan.launches) {
        if (!l.global) continue;
        for (int q = l.first; q < l.first + l.count; ++q) {
            const int sp = plan.list[(size_t)q];
            // (a species of the global launch is not in LDS: a threshold of 0 for choose_path says so again)
            if (choose_form(levels[(size_t)sp], 0, blocked_threshold) == FORM_BLOCKED) {
                b.blocked.push_back(sp); b.blocked_slab.push_back(plan.slab[(size_t)q]);
                largest = std::max<long long>(largest, levels[(size_t)sp]);
            } else { b.single.push_back(sp); b.single_slab.push_back(plan.slab[(size_t)q]); }
        }
    }
    for (long long t = 0; t < panel_steps(largest); ++t) {
        long long strips = 0;
        for (int sp : b.blocked) strips = std::max(strips, trailing_strips(levels[(size_t)sp], t * PANEL_COLUMNS));
        b.steps.push_back({(unsigned)b.blocked.size(), (unsigned)n_shells, (unsigned)strips, (unsigned)b.blocked.size(), (unsigned)n_shells});
    }
    return b;
}

// What tardis_mc_set_nlte_data checks before it indexes anything, on plain arrays: the species against the ions (ion_level_edge[I+1]),
// the edge table, the line ids against the L lines, every line's two levels against its species' ion, and the (lower, upper) pairs of
// a species against each other.  Returns "" when the data are good, else the message.  lower_local / upper_local (may be null) receive
// the local level indices of the NL lines.
template <typename EdgeT, typename LevelT>
inline std::string check_data(long long n_species, const int64_t *species_ion, long long n_nlte_lines, const int64_t *species_line_edge,
                              const int64_t *line_id, long long n_ions, const EdgeT *ion_level_edge, long long n_lines,
                              const LevelT *level_lower, const LevelT *level_upper, std::vector<int> *lower_local = nullptr,
                              std::vector<int> *upper_local = nullptr)
{
    char buf[256];
    auto msg = [&](const char *fmt, long long a = 0, long long b = 0, long long c = 0) { snprintf(buf, sizeof buf, fmt, a, b, c); return std::string(buf); };
    if (n_species <= 0 || n_nlte_lines < 0 || n_species > 0x7ffffff0LL || n_nlte_lines > 0x7ffffff0LL) return msg("invalid NLTE data: %lld species, %lld lines", n_species, n_nlte_lines);
    if (!species_ion || !species_line_edge || (n_nlte_lines > 0 && !line_id)) return msg("invalid NLTE data: a pointer is missing");
    std::vector<char> seen((size_t)n_ions, 0);
    for (long long sp = 0; sp < n_species; ++sp) {
        const long long i = species_ion[sp];
        if (i < 0 || i >= n_ions) return msg("species_ion[%lld] = %lld is no ion of the plasma data", sp, i);
        if (seen[(size_t)i]) return msg("species_ion[%lld] = %lld is repeated", sp, i);
        seen[(size_t)i] = 1;
    }
    if (species_line_edge[0] != 0 || species_line_edge[n_species] != n_nlte_lines) return msg("species_line_edge must run from 0 to n_nlte_lines");
    for (long long sp = 0; sp < n_species; ++sp)
        if (species_line_edge[sp + 1] < species_line_edge[sp]) return msg("species_line_edge decreases at species %lld", sp);
    if (lower_local) lower_local->assign((size_t)n_nlte_lines, 0);
    if (upper_local) upper_local->assign((size_t)n_nlte_lines, 0);
    for (long long sp = 0; sp < n_species; ++sp) {
        const long long k0 = ion_level_edge[species_ion[sp]], k1 = ion_level_edge[species_ion[sp] + 1];
        const long long a = species_line_edge[sp], b = species_line_edge[sp + 1];
        std::vector<std::pair<long long, long long>> pairs;
        pairs.reserve((size_t)(b - a));
        for (long long q = a; q < b; ++q) {
            const long long l = line_id[q];
            if (l < 0 || l >= n_lines) return msg("line_id[%lld] = %lld lies outside the line list", q, l);
            const long long lo = level_lower[l], up = level_upper[l];
            if (lo < k0 || lo >= k1 || up < k0 || up >= k1) return msg("NLTE line %lld (line %lld): its levels are not both inside the ion of species %lld", q, l, sp);
            if (lo == up) return msg("NLTE line %lld (line %lld): lower == upper", q, l);
            pairs.emplace_back(std::min(lo, up) - k0, std::max(lo, up) - k0);  // (u, l) writes the two entries (l, u) writes
            if (lower_local) (*lower_local)[(size_t)q] = (int)(lo - k0);
            if (upper_local) (*upper_local)[(size_t)q] = (int)(up - k0);
        }
        std::sort(pairs.begin(), pairs.end());
        for (size_t q = 1; q < pairs.size(); ++q)
            if (pairs[q] == pairs[q - 1]) return msg("species %lld: the pair of levels (%lld, %lld) is repeated", sp, pairs[q].first, pairs[q].second);
    }
    return std::string();
}

// What tardis_mc_set_nlte_collision_data checks before it indexes anything, on plain arrays: the species count against the installed
// NLTE data's, the temperature grid, the edge table, every pair's two levels against its species' ion (species_levels[sp] levels,
// local indices), lower < upper, the pairs of a species against each other, and delta_e / g_ratio.  C_ul is not inspected: NaN entries
// are data (the interpolation zeroes them).  Returns "" when the data are good, else the message.
inline std::string check_collision_data(long long n_species, long long n_nlte_species, const int64_t *species_levels, long long n_temperatures,
                                        const double *temperatures, long long n_pairs, const int64_t *species_pair_edge, const int64_t *level_lower,
                                        const int64_t *level_upper, const double *delta_e, const double *g_ratio, const double *c_ul)
{
    char buf[256];
    auto msg = [&](const char *fmt, long long a = 0, long long b = 0, long long c = 0) { snprintf(buf, sizeof buf, fmt, a, b, c); return std::string(buf); };
    if (n_species != n_nlte_species) return msg("collision data of %lld species, the NLTE data have %lld", n_species, n_nlte_species);
    if (n_species <= 0 || !species_levels) return msg("invalid collision data: %lld species", n_species);
    if (n_temperatures < 2 || n_temperatures > 0x7ffffff0LL) return msg("collision data need n_temperatures >= 2, not %lld", n_temperatures);
    if (n_pairs < 0 || n_pairs > 0x7ffffff0LL) return msg("invalid collision data: %lld pairs", n_pairs);
    if (!temperatures || !species_pair_edge || (n_pairs > 0 && (!level_lower || !level_upper || !delta_e || !g_ratio || !c_ul)))
        return msg("invalid collision data: a pointer is missing");
    for (long long t = 0; t + 1 < n_temperatures; ++t)
        if (!(temperatures[t] < temperatures[t + 1])) return msg("collision_temperatures must ascend (entry %lld)", t + 1);
    if (!std::isfinite(temperatures[0]) || !std::isfinite(temperatures[n_temperatures - 1])) return msg("collision_temperatures must be finite");
    if (species_pair_edge[0] != 0 || species_pair_edge[n_species] != n_pairs) return msg("species_pair_edge must run from 0 to n_pairs");
    for (long long sp = 0; sp < n_species; ++sp)
        if (species_pair_edge[sp + 1] < species_pair_edge[sp]) return msg("species_pair_edge decreases at species %lld", sp);
    for (long long sp = 0; sp < n_species; ++sp) {
        const long long n = species_levels[sp], a = species_pair_edge[sp], b = species_pair_edge[sp + 1];
        std::vector<std::pair<long long, long long>> pairs;
        pairs.reserve((size_t)(b - a));
        for (long long q = a; q < b; ++q) {
            const long long lo = level_lower[q], up = level_upper[q];
            if (lo < 0 || lo >= n || up < 0 || up >= n) return msg("collision pair %lld: its levels are not both inside the ion of species %lld (%lld levels)", q, sp, n);
            if (lo >= up) return msg("collision pair %lld: lower >= upper (%lld, %lld)", q, lo, up);
            if (!std::isfinite(delta_e[q])) return msg("collision pair %lld: delta_e is not finite", q);
            if (!(g_ratio[q] > 0) || !std::isfinite(g_ratio[q])) return msg("collision pair %lld: g_ratio is not finite and positive", q);
            pairs.emplace_back(lo, up);
        }
        std::sort(pairs.begin(), pairs.end());
        for (size_t q = 1; q < pairs.size(); ++q)
            if (pairs[q] == pairs[q - 1]) return msg("species %lld: the collision pair (%lld, %lld) is repeated", sp, pairs[q].first, pairs[q].second);
    }
    return std::string();
}

// scipy's interp1d bounds error, from the call's t_rad: the first shell whose t_e = link * t_rad[s] lies outside [t_first, t_last]
// (a NaN lies outside), or -1.  A t_e exactly on the first or the last knot is inside.
inline long long first_t_e_outside(double link, long long n_shells, const double *t_rad, double t_first, double t_last)
{
    for (long long s = 0; s < n_shells; ++s) {
        const double t_e = link * t_rad[s];
        if (!(t_e >= t_first && t_e <= t_last)) return s;
    }
    return -1;
}

}  // namespace nlte
