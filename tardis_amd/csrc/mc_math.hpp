// mc_math.hpp -- device-side portable log/exp (double-double, nearly correctly rounded) for gfx950.
//
// The reference draws tau_event = -np.log(xi) (modes/homologous_rad_packet_transport.py:84) and weights
// v-packets by math.exp(-tau) (packets/virtual_packet.py:231,372).  ROCm's ocml log/exp are accurate to
// ~1 ulp but are not the correctly rounded value, and neither is any particular libm; to make the per-packet
// results of the kernels reproducible bit for bit on the host, both are evaluated here with an explicit
// algorithm built only from +,-,*,fma and table look-ups (compile with -ffp-contract=off).  The result equals
// the correctly rounded log/exp for all but an estimated ~1e-4 of arguments.  What is asserted, against an 80-digit
// reference from Python's `decimal` that shares nothing with the tables (tests/portable_math_ref.py), for the oracle's copy
// in tests/test_portable_math_host.py and for this one, on the device, in tests/test_portable_math_gpu.py:
//   * every normal result of 16 argument families (whole domain, next to k ln2/64 and (k + 1/2) ln2/64, all residues
//     k & 63, the early returns, the table nodes j/64 and their switches, the sqrt(2) split, next to 1, all powers of
//     two, the kernels' grid k / 2^53) equals the correctly rounded value bit for bit; one true miss is known and listed
//     there by value, exp(2^-53) = 1 instead of 1 + 2^-52;
//   * device == oracle bit for bit on all of them, and every generated constant equals its definition.
//
// Domain of log: x finite and >= 2^-1022, or exactly 0 (-> -inf).  Subnormal, negative, infinite and NaN arguments return
// unspecified finite values.  No caller can produce them: mc::Rng::random() is a multiple of 2^-53 below 1, and the product
// of four pcg_double draws in packet_source.hpp is 0 or at least 2^-212.
// exp: any argument; NaN -> NaN, overflow -> +inf, deep underflow -> 0.  A result below 2^-1022 may differ from the correctly
// rounded value by one unit (about 1 % do): the final ldexp rounds the already rounded 53-bit result a second time.
//
//   log x : x = 2^e m, m in [sqrt(1/2), sqrt(2));  j = round(64 m), c = j/64;
//           log x = e ln2 + ln c + log1p((m - c)/c), ln c and 1/c tabulated in double-double.
//   exp x : k = round(64 x / ln2); r = x - k ln2/64 (double-double); exp x = 2^(k/64) * (1 + expm1(r)).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mc_math_tables.h"

namespace mcm {

__device__ static const double log_tab[MC_LOG_TABLE_LEN][4] = {MC_LOG_TABLE_VALUES};
__device__ static const double log1p_tail[10] = {MC_LOG1P_TAIL_COEFS};
__device__ static const double exp_tab[MC_EXP_TABLE_LEN][2] = {MC_EXP_TABLE_VALUES};
__device__ static const double exp_tail[8] = {MC_EXP_TAIL_COEFS};

__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e)
{
    s = a + b;
    double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// Domain: x == 0 -> -inf; otherwise x finite and >= 2^-1022 (see above; anything else returns an unspecified finite value).
__device__ __forceinline__ double log(double x)
{
    if (x == 0.0) return -__builtin_huge_val();
    uint64_t ix = (uint64_t)__double_as_longlong(x);
    int64_t e = (int64_t)(ix >> 52) - 1023;
    uint64_t mant = ix & 0x000fffffffffffffULL;
    if (mant > 0x6a09e667f3bcdULL) { e += 1; ix = mant | (0x3feULL << 52); }
    else ix = mant | (0x3ffULL << 52);
    double m = __longlong_as_double((long long)ix);
    int j = (int)(m * 64.0 + 0.5);
    const double *t = log_tab[j - 45];
    const double t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
    double u = m - (double)j * 0.015625;
    double qh = u * t0;
    double ql = __builtin_fma(u, t0, -qh) + u * t1;
    double sq = qh * qh;
    double sqe = __builtin_fma(qh, qh, -sq) + 2.0 * qh * ql;
    double sh = -0.5 * sq, sl = -0.5 * sqe;
    double p = log1p_tail[9];
#pragma unroll
    for (int k = 8; k >= 0; --k) p = p * qh + log1p_tail[k];
    double p3 = qh * qh * qh * p;
    double ah = qh + sh;
    double al = (qh - ah) + sh;
    al = al + (ql + sl + p3);
    double ed = (double)e;
    double kh = ed * MC_LN2_HI;
    double kl = ed * MC_LN2_LO;
    double s1, e1, s2, e2;
    two_sum(kh, t2, s1, e1);
    two_sum(s1, ah, s2, e2);
    double low = e1 + e2 + kl + t3 + al;
    return s2 + low;
}

__device__ __forceinline__ double exp(double x)
{
    if (x > 709.782712893384) return __builtin_huge_val();
    if (x < -745.2) return 0.0;
    double kd = x * MC_EXP_INV_LN2_64;
    kd = __builtin_floor(kd + 0.5);
    int64_t k = (int64_t)kd;
    double rh = x - kd * MC_EXP_LN2_64_HI;
    double t1 = kd * MC_EXP_LN2_64_LO;
    double t1e = __builtin_fma(kd, MC_EXP_LN2_64_LO, -t1);
    double r, re;
    two_sum(rh, -t1, r, re);
    double rl = re - t1e - kd * MC_EXP_LN2_64_LOLO;
    double r2 = r * r;
    double r2e = __builtin_fma(r, r, -r2) + 2.0 * r * rl;
    double ep = exp_tail[7];
#pragma unroll
    for (int i = 6; i >= 0; --i) ep = ep * r + exp_tail[i];
    double pl = rl + (0.5 * r2 + (0.5 * r2e + r2 * r * ep));
    int64_t i64 = k & 63;
    int64_t q = (k - i64) / 64;
    double th = exp_tab[i64][0], tl = exp_tab[i64][1];
    double pr = th * r;
    double pre = __builtin_fma(th, r, -pr);
    double s, se;
    two_sum(th, pr, s, se);
    double low = se + pre + th * pl + tl + tl * r;
    double res = s + low;
    return __builtin_ldexp(res, (int)q);
}

}  // namespace mcm
