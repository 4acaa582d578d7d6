// mean_opacity_plan.hpp -- the frequency bins of tardis_mc_mean_opacity and the form its shell reduction takes: the host's decisions as
// pure functions.
//
// Standard C++ only (no HIP header, no context, no device call): tests/test_mean_opacity_host.py pins the layout through
// tardis_mc_mean_opacity_bins and the rule through tardis_mc_mean_opacity_path.  The kernels are in mean_opacity.hpp.
//
// Bins (include/tardis_mc.h has the full statement).  The line list is descending; asc[i] = nu[L-1-i].  With m = bin_size,
// e = m - L mod m (1 <= e <= m) pads p[0 .. e] = 1.0, 2.0, ... e + 1.0 Hz are put below the list, p[j] = asc[j-e-1] behind them, and bin b
// runs from low = p[b m] (outside) to high = p[(b+1) m] (inside): members j = b m + 1 .. (b+1) m.  Only bin 0 holds pads.  Refused:
// m < 1, a list that does not lie above its pads, a bin of width 0 (duplicate lines on two consecutive edges).
//
// The shell reduction adds four sums over the bins of a shell in ascending order, either on one lane (PATH_LANE) or carried through a
// 16-lane DPP row, sixteen bins per step (PATH_ROW).  Both add in the same order, so the choice changes no bit, only the time (LONG_BINS
// below has the measurement).
#pragma once
#include <cstdio>
#include <string>

namespace mopl {

constexpr int ERR_INVALID_ARGUMENT = -1;  // (TARDIS_MC_ERR_INVALID_ARGUMENT; the engine asserts the equality)
constexpr int PATH_LANE = 0, PATH_ROW = 1;
// Shells of this many bins or more take the row form.  Measured on the MI355X (profiles/mean_opacity.txt; reduce_ms of 20 shells, lane / row
// form): 0.0144 / 0.0144 ms at 5 bins, 0.0160 / 0.0143 at 9, 0.0194 / 0.0143 at 17, 0.0399 / 0.0165 at 64, 0.50 / 0.066 at 1023, 1.50 / 0.168
// at the 3001 bins of the tardis_example shape, 24.8 / 2.59 at the 50 001 bins of the configs[2] tables.  The row form wins from 17 bins
// upward; below one full step of sixteen lanes the two are within 3 us of each other on a floor of 14 us (two launches), and the row's
// lanes past the end only add zeros: one full step is the threshold.
constexpr long long LONG_BINS = 16;

// `threshold` < 0: the measured rule; otherwise shells of `threshold` bins or more take the row form (option mean_opacity_long_bins)
inline int choose_path(long long n_bins, long long threshold = -1)
{
    const long long t = threshold < 0 ? LONG_BINS : threshold;
    return n_bins > 0 && n_bins >= t ? PATH_ROW : PATH_LANE;
}

struct Layout {
    long long m = 0, e = 0, n_bins = 0, n_lines = 0;
};

// p[j], 0 <= j <= L + e, of the padded ascending sequence (nu: the descending list)
inline double padded_nu(const Layout &lay, const double *nu, long long j)
{
    return j <= lay.e ? (double)(j + 1) : nu[lay.n_lines - 1 - (j - lay.e - 1)];
}
inline double bin_low(const Layout &lay, const double *nu, long long b) { return padded_nu(lay, nu, b * lay.m); }
inline double bin_high(const Layout &lay, const double *nu, long long b) { return padded_nu(lay, nu, (b + 1) * lay.m); }

// The layout of L lines in bins of m, or the refusal: returns n_bins (> 0) or ERR_INVALID_ARGUMENT with `msg` written.  first_degenerate
// (may be null): the first bin of width 0, -1 where there is none (also on the other refusals).
inline long long plan_bins(long long n_lines, const double *nu, long long bin_size, Layout &lay, long long *first_degenerate, std::string &msg)
{
    char buf[256];
    if (first_degenerate) *first_degenerate = -1;
    if (n_lines < 1 || !nu) { msg = "mean opacity: no line list"; return ERR_INVALID_ARGUMENT; }
    if (bin_size < 1) {
        snprintf(buf, sizeof buf, "mean opacity: bin_size %lld, it must be at least 1", bin_size);
        msg = buf;
        return ERR_INVALID_ARGUMENT;
    }
    lay.m = bin_size;
    lay.n_lines = n_lines;
    lay.e = bin_size - n_lines % bin_size;
    lay.n_bins = (n_lines + lay.e) / bin_size;
    const double lowest = nu[n_lines - 1];
    if (!(lowest > (double)(lay.e + 1))) {
        snprintf(buf, sizeof buf, "mean opacity: the lowest line frequency %g Hz does not lie above the %lld pads (1 .. %lld Hz) of bin_size %lld", lowest,
                 lay.e + 1, lay.e + 1, bin_size);
        msg = buf;
        return ERR_INVALID_ARGUMENT;
    }
    for (long long b = 0; b < lay.n_bins; ++b)
        if (bin_high(lay, nu, b) - bin_low(lay, nu, b) == 0.0) {
            if (first_degenerate) *first_degenerate = b;
            snprintf(buf, sizeof buf, "mean opacity: bin %lld of %lld has width 0 at bin_size %lld (duplicate lines at %.17g Hz on both of its edges)", b,
                     lay.n_bins, bin_size, bin_low(lay, nu, b));
            msg = buf;
            return ERR_INVALID_ARGUMENT;
        }
    return lay.n_bins;
}

}  // namespace mopl
