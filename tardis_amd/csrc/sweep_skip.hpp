// sweep_skip.hpp -- lane sweep: whole 8-line blocks proved harmless on a coarse prefix-sum table.
//
// Nearly every line a lane sweep examines is examined only to prove that it does not stop the trace (propagate_wave.hpp, "lane sweep").  That proof
// does not need the line, only an upper bound of what the line could add.  One 16-byte entry per aligned block of BLOCK = 8 lines carries it:
//     ct[s][b] = { nu_last, p_end }      nu_last: the frequency slot of the block's last entry in the interleaved table (-inf for the block that holds
//                                        line L - 1 and for everything behind it); p_end = pfx[s][min(8 b + 8, L)], pfx the double-double prefix sums
//                                        of tau_prefix.hpp rounded once (|pfx - P| <= 2^-53 P).
// A trace that starts at line `start` of block b0 loads N - 1 coarse entries from b0 on together with pn[s][start] = {frequency slot of line `start`, pfx[s][start]} -- the N 16-byte
// loads of a fine step of the instantiation: the width N is the kernel's choice (eight in the sixteen-wave form, ten in the twelve-wave one), nothing below depends
// on it -- and clears block b when
//     X_last < X_b                       X_last = comov_nu - nu_last
//     RN(hi_b + x_last) < tau_event      x_last = RN(K' X_last),   hi_b = RN(RN(p_end_b - pfx[start]) + M)
// in order, stopping at the first block that fails.
//
// Why a cleared block cannot stop the trace.  Let line k lie between `start` and the end of block b, T_k the reference's serial sum of the optical
// depths in front of it and T_k + tau_k (rounded) the one including it.
//   * The list is sorted: X_k <= X_last < X_b, and X_k >= X_start >= 0 (tested on the first line, as every fine step does).  K' > 0 and rounding is
//     monotone: x_k = RN(K' X_k) <= x_last.
//   * tau >= 0 (the host turns the skip off for a table with a negative or non-finite optical depth): the serial sums grow with k, so all of them are
//     at most the one at the end of the block, S, and S <= hi_b (below).
//   * Hence RN(RN(T_k + tau_k) + x_k) <= RN(hi_b + x_last) < tau_event: the lean per-line proof of the fine step (X_k >= 0, X_k < X_b,
//     sum < tau_event; propagate_wave.hpp) holds for every line of the block, which is all the fine step would have established.
//
// The margin.  R: the largest row sum of the table, n <= L the lines between `start` and the end of block b, E their exact sum, d = RN(p_end - pfx[start]).
//     |S - E|  <= 1.01 n 2^-53 E                                  (recursive summation, n 2^-53 < 0.01)
//     |d - E|  <= 2^-53 (P_end + P_start) + 2^-53 |d| <= 2^-51 R  (the two rounded prefixes, the rounded difference)
// so |S - d| <= R (1.01 L 2^-53 + 2^-51), and with
//     M = R (1.02 (L + 16) 2^-53 + 2^-48)
// the rest, more than R 2^-49, pays for the rounding of d + M (at most 2^-53 1.01 R) and of M itself: S <= hi_b, and likewise S >= d - M, i.e.
//     0 <= hi_b - S <= 2 M + 2^-52 R.
//
// After the coarse step the lane takes ordinary fine steps from the first block that was not cleared, with s_tau = hi of the block before it ("interval
// mode").  Serial RN additions of the same non-negative terms to an upper bound stay an upper bound, so the lean per-line proof runs unchanged.  The
// distance between the lane's sum U and the reference's T grows by at most one rounding of each per line, 2 * 2^-53 * 1.01 R, over at most L lines:
//     0 <= U - T <= 2 M + R (2^-52 + 1.01 L 2^-52) < GAP_FACTOR M = 8 M =: g.
// The first line that fails the lean proof is evaluated by lane_exact_line with tau_prev = U.  Its distance to the continuum, RN(RN(tau_event - tau_prev) / chi),
// only grows as tau_prev falls, tau_combined only falls:
//   * code 1 (boundary: d_boundary <= d_trace and d_boundary <= d_cont(U) <= d_cont(T)) and code 0 (d_trace below both, tau_combined(T) <= tau_combined(U)
//     <= tau_event) come out the same for T: taken.  On code 0 the lane goes on, U + tau still an upper bound.
//   * code 3 (line): neither distance test depends on T the other way; the line stops the trace for T as well if
//     RN(RN(RN(U - g) + tau_line) + RN(chi d_trace)) > tau_event, RN(U - g) <= T (the 2^-48 R in M pays for that rounding, too).  The distance is d_trace.
//   * code 2 (electron scattering: the distance is an output and depends on T), a code 3 that fails that check, code 4 and a list that ends on the
//     continuum make the lane FALL BACK: the trace starts again at `start` with s_tau = 0 and the skip off.
// Every decision is a function of the trace's inputs and the tables alone, so a lane suspended in coarse or interval mode is stored as the start of its
// trace and takes the same path again.
//
// What is shared and what is not.  coarse_scan() and interval_take() below are the code the kernel runs, compiled for host and device.  trace(), host only, is a
// RESTATEMENT of the kernel's step logic around them (propagate_wave.hpp, sweep phase under SKIP: the mode bits, the advance after a coarse step, the fall-back,
// the exact evaluation) with the lanes taken one at a time: tests/test_sweep_skip_host.py checks the algorithm on it (tests/test_sweep_skip_widths_host.py: at the
// widths 8, 10 and 12), while the kernel's own glue -- the
// arithmetic on `adv` that sends a fall-back through the go-on path, the toggle of the mode bits in pflags, the suspension that stores the start of the trace --
// is covered by tests/test_sweep_skip_gpu.py and tests/test_sweep_skip_widths_gpu.py against the oracle only.  A change to either copy has to be made in both.
// The host test builds its own prefix sums (one serial two-sum per row); those and the device's pn / ct / margin as the kernel reads them are held to the same exact
// sums and to the layout above by tests/test_prefix_tables_host.py and tests/test_prefix_tables_gpu.py, which also run both copies on tables with a large M.
#pragma once

#if defined(__HIPCC__)
#define SSK_FN __host__ __device__ inline
#else
#define SSK_FN inline
#endif

namespace ssk {

constexpr int BLOCK = 8;        // lines per coarse entry
// The width of a step is the instantiation's: N 16-byte loads, coarse or fine (the same registers) -- N - 1 coarse entries, the N-th load is pn[s][start] =
// {frequency slot of line `start`, pfx[s][start]}; a step that clears all N - 1 goes on from its LAST block (an advance of N - 2 blocks), whose hi the next
// step computes again.  The host restatement takes it from TraceIn::loads (DEFAULT_LOADS where that is 0), at most MAX_LOADS.
constexpr int DEFAULT_LOADS = 10, MAX_LOADS = 16;
constexpr double GAP_FACTOR = 8.0;
// mode bits of a lane's pflags
constexpr int MODE_COARSE = 8, MODE_INTERVAL = 16;
// MODE_START_HELD ("start entry in registers", option sweep_start_held): the trace follows an emission that a hot sector of the walk decided.  The walk's read of
// the emission line's frequency fetched pn[s][emit] and its neighbour pn[s][emit + 1] = pn[s][start] together, so the lane brings {nu_start, p_start} along: the
// prologue of the trace evaluates the start guard of coarse_scan (same operands: comov, xb, nu_start) and gives a trace that fails it no MODE_COARSE -- what
// coarse_scan returning 0 in the first step leads to -- and the coarse steps take p_start from the lane (`held`) and do not issue their N-th load.  Set with
// MODE_COARSE only; cleared when the lane leaves coarse mode, falls back or is suspended (a resumed lane loads the entry as every other trace does).
// trace() restates it (TraceIn::start_held); tests/test_sweep_start_held_host.py holds the held path to the reference's loop and to the load path.
constexpr int MODE_START_HELD = 32;

struct Entry { double nu_last, p_end; };

SSK_FN double margin(int n_lines, double rowsum_max)
{
    return rowsum_max * (1.02 * ((double)n_lines + 16.0) * 0x1p-53 + 0x1p-48);
}

// One coarse step on its N loads (entries 0 .. N - 2 the coarse ones {nu_last, p_end}, entry N - 1 = {nu_start, p_start}): the number of leading
// blocks cleared (0 .. N - 1); hi = the bound of the last cleared block.  None if the first line fails X >= 0 (the reference's "nu difference" error, or a close
// line: to the exact evaluation).
// held (MODE_START_HELD): the start guard has been evaluated already, on the same operands, and held; p_end[N - 1] is the lane's own p_start and nu_last[N - 1] is
// not looked at (the entry was not loaded).
template <int N>
SSK_FN int coarse_scan(const double (&nu_last)[N], const double (&p_end)[N], double comov, double kp, double xb, double tau_event, double m, double &hi,
                       bool held = false)
{
    static_assert(N >= 3, "at least two coarse entries: a full step advances by N - 2 blocks");
    constexpr int STEP = N - 1;
    int c = 0;
    const double p_start = p_end[STEP];
    // (X_start < X_b costs a cleared first block nothing -- X_last >= X_start -- and keeps a trace that starts on the last line of the list or behind it,
    // whose frequency slot holds -inf, out of the coarse entries: behind the row's last block they are the next row's)
    const double x_start = comov - nu_last[STEP];
    bool alive = held || (x_start >= 0.0 && x_start < xb);
    double h_keep = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < STEP; ++k) {
        const double d = p_end[k] - p_start;
        const double h = d + m;
        const double X = comov - nu_last[k];
        const double x = kp * X;
        const double sum = h + x;
        alive = alive && X < xb && sum < tau_event;
        if (alive) { c = k + 1; h_keep = h; }
    }
    hi = h_keep;
    return c;
}

// Interval mode, the first line that failed the lean proof, evaluated with tau_prev = u (code, dist: lane_exact_line's): whether the reference, whose sum
// lies in [u - g, u], comes to the same code and distance.  (g not finite: never -- the tests' "every decision is ambiguous".)
SSK_FN bool interval_take(int code, double u, double g, double tau_line, double chi, double dist, double tau_event)
{
    if (!(g < __builtin_inf())) return false;
    if (code == 1) return true;
    if (code != 3) return false;
    const double lo = u - g;
    const double incl = lo + tau_line;
    const double cd = chi * dist;
    return incl + cd > tau_event;
}

#if !defined(__HIPCC__)
// ---- host statement of the sweep of ONE trace as the kernel runs it (propagate_wave.hpp, sweep phase, SKIP), for the host test.
// nt: the interleaved row {nu, tau} (nu = -inf from line L - 1 on, `slack` entries behind the row); ct: the row's coarse entries; pn: the row's {nu, prefix sum}.
struct TraceIn {
    const double *nt, *ct, *pn;
    int n_lines, start;
    double nu, comov, chi, tau_event, d_boundary, kp, xb, t_exp, m;
    int force_fallback, skip, fine_chunk;
    int loads;  // 16-byte loads of a coarse step (coarse_scan's N); 0: DEFAULT_LOADS
    // MODE_START_HELD: the trace follows an emission whose walk fetched pn[start] = {held_nu, held_p} (start_held != 0: the prologue's guard, no N-th load)
    int start_held;
    double held_nu, held_p;
};
// fb_gap (a trace that fell back on a line): how far tau_event lies below tau_prev + tau_line + chi * distance as the lane's upper bound sees them
// fb_line, fb_u: the line the fall-back happened at (n_lines: behind the list) and the lane's upper bound of the sum in front of it
// start_loads: the coarse steps that loaded pn[start] (their N-th load); guard_failed: a held start entry failed the prologue's guard (no coarse step at all)
struct TraceOut { int code, line; double dist; int fell_back, coarse_steps, fine_steps, interval, fb_code; double fb_gap; int fb_line; double fb_u; int start_loads, guard_failed; };

constexpr double C_LIGHT_ = 2.99792458e10, MISS_ = 1e99, CLOSE_ = 1e-14;
inline int exact_line(int L, double t_exp, int line, double nu_line, double tau_line, double tau_prev, double nu, double comov_nu, double chi, double tau_event,
                      double d_boundary, double &distance)
{   // lane_exact_line (propagate_wave.hpp), line scattering enabled
    const double tau_incl = tau_prev + tau_line;
    const double d_cont = (tau_event - tau_prev) / chi;
    const bool is_last = line == L - 1;
    const double nu_diff = comov_nu - nu_line;
    const double q = nu_diff / nu;
    const bool close = (q < 0 ? -q : q) < CLOSE_;
    const bool err = !is_last && !close && !(nu_diff >= 0);
    const double d_far = q * C_LIGHT_ * t_exp;
    const double d_trace = is_last ? MISS_ : (close ? 0.0 : d_far);
    const double tau_combined = tau_incl + chi * d_trace;
    double dmin = d_trace;
    if (d_boundary < dmin) dmin = d_boundary;
    if (d_cont < dmin) dmin = d_cont;
    const bool stop_b = !err && d_trace != 0 && dmin == d_boundary;
    const bool stop_e = !err && d_trace != 0 && !stop_b && dmin == d_cont;
    const bool stop_l = !err && !stop_b && !stop_e && tau_combined > tau_event;
    distance = stop_b ? d_boundary : (stop_e ? d_cont : d_trace);
    return stop_b ? 1 : (stop_e ? 2 : (stop_l ? 3 : (err ? 4 : 0)));
}

template <int N>
inline int coarse_scan_n(const double *nl, const double *pe, const TraceIn &in, double &hi, bool held)
{
    double a[N], b[N];
    for (int k = 0; k < N; ++k) { a[k] = nl[k]; b[k] = pe[k]; }
    return coarse_scan<N>(a, b, in.comov, in.kp, in.xb, in.tau_event, in.m, hi, held);
}
// (the widths the kernel's instantiations and the tests use)
inline int coarse_scan_any(int n, const double *nl, const double *pe, const TraceIn &in, double &hi, bool held = false)
{
    switch (n) {
    case 8: return coarse_scan_n<8>(nl, pe, in, hi, held);
    case 9: return coarse_scan_n<9>(nl, pe, in, hi, held);
    case 10: return coarse_scan_n<10>(nl, pe, in, hi, held);
    case 12: return coarse_scan_n<12>(nl, pe, in, hi, held);
    default: __builtin_trap();
    }
}

inline TraceOut trace(const TraceIn &in, const double *nu_true)
{
    TraceOut out{};
    const int L = in.n_lines, CH = in.fine_chunk;
    const int LOADS = in.loads ? in.loads : DEFAULT_LOADS, STEP = LOADS - 1, ADVANCE = LOADS - 2;
    int mode = in.skip ? MODE_COARSE : 0;
    int s_line = in.start;
    double s_tau = 0.0;
    if (in.skip && in.start_held) {  // the prologue: coarse_scan's start guard on the entry the lane brought along; p_start waits in s_tau
        const double x_start = in.comov - in.held_nu;
        if (x_start >= 0.0 && x_start < in.xb) { mode |= MODE_START_HELD; s_tau = in.held_p; }
        else { mode = 0; out.guard_failed = 1; }
    }
    const double g = in.force_fallback ? __builtin_inf() : GAP_FACTOR * in.m;
    for (;;) {
        if (mode & MODE_COARSE) {
            ++out.coarse_steps;
            double nl[MAX_LOADS], pe[MAX_LOADS], hi;
            const int b = s_line >> 3;
            for (int k = 0; k < STEP; ++k) { nl[k] = in.ct[2 * (b + k)]; pe[k] = in.ct[2 * (b + k) + 1]; }
            const bool held = (mode & MODE_START_HELD) != 0;
            if (held) { nl[STEP] = 0.0; pe[STEP] = s_tau; }
            else { nl[STEP] = in.pn[2 * in.start]; pe[STEP] = in.pn[2 * in.start + 1]; ++out.start_loads; }
            const int c = coarse_scan_any(LOADS, nl, pe, in, hi, held);
            const bool first = s_line == in.start;
            if (c == STEP) s_line = (b + ADVANCE) << 3;
            else if (c > 0) { s_line = (b + c) << 3; s_tau = hi; mode = MODE_INTERVAL; out.interval = 1; }
            else if (first) { s_tau = 0.0; mode = 0; }
            else { s_line = in.start; s_tau = 0.0; mode = 0; out.fell_back = 1; }
            continue;
        }
        ++out.fine_steps;
        int adv = 0;
        bool alive = true;
        double f_nu = in.nt[2 * s_line], f_tau = in.nt[2 * s_line + 1];
        for (int k = 0; k < CH && alive; ++k) {
            const double nuk = in.nt[2 * (s_line + k)], tk = in.nt[2 * (s_line + k) + 1];
            const double X = in.comov - nuk, x = in.kp * X, tau_n = s_tau + tk, sum = tau_n + x;
            const bool ok = (k > 0 || X >= 0.0) && X < in.xb && sum < in.tau_event;
            if (ok) { s_tau = tau_n; adv = k + 1; }
            else { alive = false; f_nu = nuk; f_tau = tk; }
        }
        if (!alive) {
            const int line = s_line + adv;
            int code;
            double dist;
            if (line < L) {
                code = exact_line(L, in.t_exp, line, line < L - 1 ? f_nu : nu_true[line], f_tau, s_tau, in.nu, in.comov, in.chi, in.tau_event, in.d_boundary, dist);
                if ((mode & MODE_INTERVAL) && code && !interval_take(code, s_tau, g, f_tau, in.chi, dist, in.tau_event)) {
                    out.fb_code = code; out.fb_line = line; out.fb_u = s_tau;
                    out.fb_gap = code == 3 ? ((s_tau + f_tau) + in.chi * dist) - in.tau_event : (s_tau + in.chi * dist) - in.tau_event;
                    code = -1;
                }
                if (!code) { s_tau = s_tau + f_tau; ++adv; }
            } else {
                const double d_cont = (in.tau_event - s_tau) / in.chi;
                const bool cont = d_cont < in.d_boundary;
                dist = cont ? d_cont : in.d_boundary;
                code = (cont ? 2 : 1) | 8;
                if ((mode & MODE_INTERVAL) && cont) { out.fb_code = code; out.fb_line = L; out.fb_u = s_tau; out.fb_gap = (s_tau + in.chi * dist) - in.tau_event; code = -1; }
            }
            if (code < 0) { s_line = in.start; adv = 0; s_tau = 0.0; mode = 0; out.fell_back = 1; }
            else if (code) { out.code = code; out.line = (code & 8) ? 0 : line; out.dist = dist; return out; }
        }
        s_line += adv;
    }
}
#endif

}  // namespace ssk
