"""Correctly rounded exp / log from the standard library's `decimal`, and the named argument families on which the
portable exp / log (oracle/portable_math.h, tardis_amd/csrc/mc_math.hpp) are compared with them.

Reference: Decimal(float) is exact, Context.exp / Context.ln are correctly rounded to 80 digits, and float(Decimal) is a
correctly rounded conversion (into the subnormal range too), so the only way the result can miss the correctly rounded
double is a true value within 1e-80 relative of a rounding boundary of binary64; none is known for exp or log.

A family is (x, ref, cls): the arguments, the reference results and the class of every expected result.  Families are
deterministic and cached per process, so the host tests and the device tests of one run evaluate a reference once.

`python tests/portable_math_ref.py [--device]` prints the per-family table that profiles/portable_math.txt records.
"""
import decimal
import functools
import math

import numpy as np

NORMAL, SUBNORMAL, SPECIAL = 0, 1, 2     # |ref| >= 2^-1022 finite; 0 < |ref| < 2^-1022; ref is 0, +-inf or NaN
MIN_NORMAL = 2.0 ** -1022
DBL_MAX = np.finfo(np.float64).max

# the constants of the algorithm, restated (generated tables: MC_EXP_INV_LN2_64) -- only used to lay arguments out
INV_LN2_64 = float.fromhex("0x1.71547652b82fep+6")
LN2_64 = math.log(2.0) / 64.0

# exp: the early returns and the borders of the result classes
EXP_HI_LITERAL = 709.782712893384        # `if (x > 709.782712893384) return inf`
# ln(DBL_MAX) = 709.78271289338399684...: it rounds to the same double as the literal above (asserted below), and that
# double is the largest argument whose exp is finite, so the early return is exact and the two windows coincide.
EXP_LN_DBL_MAX = float.fromhex("0x1.62e42fefa39efp+9")
EXP_LO_LITERAL = -745.2                  # `if (x < -745.2) return 0`
EXP_ZERO_BORDER = -745.1332191019412     # RN(exp x) is 0 up to here and 2^-1074 from the next double on
EXP_SUBNORMAL_BORDER = -708.3964185322641  # RN(exp x) is >= 2^-1022 from here up and subnormal below
THRESHOLDS = (EXP_HI_LITERAL, EXP_LN_DBL_MAX, EXP_LO_LITERAL, EXP_ZERO_BORDER, EXP_SUBNORMAL_BORDER)
WINDOW = 513                             # consecutive doubles on either side of a threshold

FAMILIES = {
    "exp": ("normal", "subnormal", "tiny", "near_k", "half_k", "residues", "thresholds", "special"),
    "log": ("unit", "grid", "wide", "near_one", "nodes", "split", "pow2", "special"),
}


def _context(prec):
    return decimal.Context(prec=prec, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN,
                           traps=[decimal.InvalidOperation, decimal.Overflow])


def _exp1(x, ctx):
    if x != x:
        return math.nan
    if x == 0.0:
        return 1.0
    if math.isinf(x):
        return math.inf if x > 0 else 0.0
    try:
        return float(ctx.exp(decimal.Decimal(x)))
    except (OverflowError, decimal.Overflow):
        return math.inf


def _log1(x, ctx):
    if x != x:
        return math.nan
    if x == 0.0:
        return -math.inf
    if x == 1.0:
        return 0.0
    if math.isinf(x) and x > 0:
        return math.inf
    return float(ctx.ln(decimal.Decimal(x)))


def reference(func, x, prec=80):
    """Correctly rounded exp / log of every element of x (about 80 us each at prec 80)."""
    f, ctx = {"exp": _exp1, "log": _log1}[func], _context(prec)
    return np.array([f(float(v), ctx) for v in np.asarray(x, dtype=np.float64).ravel()], dtype=np.float64)


def ordered(a):
    """Doubles -> integers in the order of the reals (+-0 -> 0), so that a difference is a distance in units of the last place."""
    i = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    return np.where(i < 0, np.int64(-2**63) - i, i)


def bit_distance(a, b):
    """Element-wise distance in representable doubles; NaN against NaN is 0, NaN against a number is 2^62."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    oa, ob = ordered(a), ordered(b)
    same_sign = (oa < 0) == (ob < 0)
    far = np.minimum(np.abs(oa.astype(np.float64) - ob.astype(np.float64)), 2.0**62).astype(np.int64)
    d = np.where(same_sign, np.abs(oa - ob), far)
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na | nb, np.where(na & nb, 0, np.int64(2**62)), d)


def _window(center):
    bits = np.array([center]).view(np.int64)[0]
    return (bits + np.arange(-WINDOW, WINDOW + 1, dtype=np.int64)).view(np.float64)


def _jitter(c, d):
    return c * (1.0 + d * 2.0**-52)


def algorithm_k(x):
    """The k the algorithm picks for x, restated: k = floor(x * (64/ln2) + 0.5)."""
    return np.floor(np.asarray(x) * INV_LN2_64 + 0.5).astype(np.int64)


def _exp_arguments(name):
    rng = np.random.default_rng({"normal": 101, "subnormal": 102, "tiny": 103, "near_k": 104, "half_k": 105,
                                 "residues": 106, "thresholds": 107, "special": 108}[name])
    if name == "normal":
        return rng.uniform(-708.39, 709.78, 20000)
    if name == "subnormal":
        return -rng.uniform(708.4, 745.3, 20000)
    if name == "tiny":
        n = 10000
        with np.errstate(under="ignore"):
            x = rng.random(n) * 10.0 ** rng.integers(-320, 0, n).astype(np.float64)
        x *= np.where(rng.random(n) < 0.5, -1.0, 1.0)
        edge = np.array([2.0**-54, 2.0**-53, 2.0**-1074])
        return np.concatenate([x, edge, -edge])
    if name in ("near_k", "half_k"):
        n = 15000
        k = rng.integers(-65000, 65001, n).astype(np.float64) + (0.5 if name == "half_k" else 0.0)
        return _jitter(k * LN2_64, rng.integers(-4, 5, n))
    if name == "residues":
        res = np.arange(64)
        k = np.concatenate([64 * rng.integers(1, 1000, 64) + res, -64 * rng.integers(1, 1000, 64) + res])
        m = np.array([-1015, -1014, -512, -2, -1, 0, 1, 2, 512, 1014, 1015])
        k = np.concatenate([k, (64 * m[:, None] + np.array([-1, 0, 1])).ravel()]).astype(np.float64)
        return np.concatenate([_jitter(k * LN2_64, d) for d in (0, -1, 1)])
    if name == "thresholds":
        return np.unique(np.concatenate([_window(c) for c in THRESHOLDS]))
    if name == "special":
        return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 710.0, 1e308, -1e308])
    raise KeyError(name)


def _log_arguments(name):
    rng = np.random.default_rng({"unit": 201, "grid": 202, "wide": 203, "near_one": 204, "nodes": 205, "split": 206,
                                 "pow2": 207, "special": 208}[name])
    if name == "unit":
        return rng.random(20000)
    if name == "grid":    # the arguments the kernels produce: multiples of 2^-53 below 1
        k = np.concatenate([np.arange(1, 4097), 2**53 - np.arange(1, 4097), rng.integers(1, 2**53, 10000)])
        return k.astype(np.float64) * 2.0**-53
    if name == "wide":    # the exponent is drawn in binades: every biased exponent 1 ... 2046 is as likely as any other
        n = 20000
        bits = (rng.integers(1, 2047, n).astype(np.uint64) << np.uint64(52)) | rng.integers(0, 2**52, n, dtype=np.uint64)
        return bits.view(np.float64)
    if name == "near_one":
        n = 10000
        a = 1.0 + rng.integers(-10**6, 10**6 + 1, n).astype(np.float64) * 2.0**-53
        b = 1.0 + rng.random(n) * 10.0 ** rng.integers(-15, 0, n).astype(np.float64) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        return np.concatenate([a, b])
    if name == "nodes":   # the table nodes j/64 and the switches (j + 1/2)/64 of j = (int)(64 m + 0.5), across the binades
        j = np.concatenate([np.arange(45, 92), np.arange(45, 92) + 0.5]) / 64.0
        m = _jitter(j[:, None], np.arange(-8, 9)[None, :]).ravel()
        return np.concatenate([np.ldexp(m, e) for e in (-1021, -500, -1, 0, 1, 500, 1022)])
    if name == "split":   # the mantissa at which m moves from [1, sqrt 2] to [sqrt 1/2, 1)
        mant = (0x6a09e667f3bcd + np.arange(-8, 9)).astype(np.uint64)
        return np.concatenate([((np.uint64(e + 1023) << np.uint64(52)) | mant).view(np.float64) for e in (-1022, -1, 0, 1, 1023)])
    if name == "pow2":
        return np.ldexp(1.0, np.arange(-1022, 1024))
    if name == "special":
        return np.array([0.0, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), DBL_MAX, MIN_NORMAL])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def arguments(func, name):
    x = np.ascontiguousarray({"exp": _exp_arguments, "log": _log_arguments}[func](name), dtype=np.float64)
    assert 0 < x.size <= 20000, (func, name, x.size)
    if func == "log":     # the documented domain of the portable log: finite and >= 2^-1022, or exactly 0
        assert np.all(np.isfinite(x) & ((x == 0.0) | (x >= MIN_NORMAL))), name
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def family(func, name):
    """(x, ref, cls) of the named family, read-only and shared by every caller of this process."""
    x = arguments(func, name)
    ref = reference(func, x)
    with np.errstate(invalid="ignore"):
        cls = np.where(np.isfinite(ref) & (np.abs(ref) >= MIN_NORMAL), NORMAL,
                       np.where(np.isfinite(ref) & (ref != 0.0), SUBNORMAL, SPECIAL)).astype(np.int8)
    for a in (ref, cls):
        a.flags.writeable = False
    return x, ref, cls


assert float.fromhex("0x1.62e42fefa39efp+9") == EXP_HI_LITERAL == EXP_LN_DBL_MAX

# True misses of the algorithm by one unit on a normal result, confirmed with a 200-digit reference: argument ->
# (the algorithm's result, the correctly rounded result).  At most 5 per family.
#   exp(2^-53) = 1 + 2^-53 + 2^-107 + ... lies 2^-107 above the tie between 1 and 1 + 2^-52; the low word of the
#   algorithm, se + th * pl = 2^-53 + 2^-107, rounds to 2^-53, and 1 + 2^-53 is then the tie itself: to even, 1.
KNOWN_MISSES = {("exp", "tiny"): {2.0**-53: (1.0, 1.0 + 2.0**-52)}}


def stats(got, ref):
    """(number of arguments, number that differ from the reference, largest bit distance)."""
    d = bit_distance(got, ref)
    return int(d.size), int(np.count_nonzero(d)), int(d.max())


def check(func, name, got):
    """The conditions a result array has to meet against the reference of its family:
      * special results (0, +-inf, NaN) and normal results: equal bit for bit (apart from KNOWN_MISSES);
      * subnormal results: at most one unit away, and at most 2 % of them away at all.  The final ldexp(res, q) rounds an
        already rounded 53-bit `res` again: it goes wrong only if `res` sits exactly on a tie of the shorter subnormal
        significand (chance 2^-s with s dropped bits, about 1.9 % averaged over s = 1 ... 52), and half of the ties fall right."""
    x, ref, cls = family(func, name)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (func, name)
    d = bit_distance(got, ref)
    signs_differ = np.signbit(got) != np.signbit(ref)
    known = KNOWN_MISSES.get((func, name), {})
    assert len(known) <= 5
    exact = cls != SUBNORMAL
    bad = np.flatnonzero(exact & ((d != 0) | (signs_differ & ~np.isnan(ref))))
    bad = [i for i in bad if known.get(float(x[i])) != (float(got[i]), float(ref[i]))]
    assert not bad, (func, name, len(bad), [(float(x[i]).hex(), float(got[i]).hex(), float(ref[i]).hex()) for i in bad[:8]])
    sub = cls == SUBNORMAL
    if sub.any():
        assert d[sub].max() <= 1, (func, name, int(d[sub].max()))
        share = np.count_nonzero(d[sub]) / np.count_nonzero(sub)
        assert share <= 0.02, (func, name, share)
    return stats(got, ref)


def algorithm_j(x):
    """The table node the log picks for x, restated: m in [sqrt 1/2, 1) or [1, sqrt 2] by the mantissa split, j = (int)(64 m + 0.5)."""
    m = np.frexp(x)[0] * 2.0
    m = np.where(m > float.fromhex("0x1.6a09e667f3bcdp+0"), 0.5 * m, m)
    return np.floor(64.0 * m + 0.5).astype(int)


def check_structure(func, name):
    """No family is vacuous: the class counts and the structural coverage the comparison with the reference relies on."""
    x, ref, cls = family(func, name)
    count = lambda c: int(np.count_nonzero(cls == c))
    if func == "exp" and name in ("normal", "tiny", "near_k", "half_k", "residues"):
        assert count(NORMAL) == x.size
    if func == "log" and name in ("unit", "grid", "wide", "near_one", "nodes", "split", "pow2"):
        assert np.all((cls == NORMAL) | (x == 0.0) | (x == 1.0))
    t = x * INV_LN2_64 if name in ("near_k", "half_k") else None
    if (func, name) == ("exp", "subnormal"):    # both sides of the zero border, both sides of the early return
        assert count(SUBNORMAL) > 15000 and np.count_nonzero(ref == 0.0) > 50 and count(NORMAL) == 0
        assert np.count_nonzero(x < EXP_LO_LITERAL) > 20 and np.count_nonzero((x > EXP_LO_LITERAL) & (ref == 0.0)) > 20
    elif (func, name) == ("exp", "thresholds"):
        assert x.size == 4 * (2 * WINDOW + 1)     # two of the five thresholds are one double
        assert np.count_nonzero(np.isinf(ref)) == WINDOW and np.count_nonzero(ref == 0.0) > WINDOW
        assert count(NORMAL) == 2 * WINDOW + 2 and count(SUBNORMAL) == 2 * WINDOW
        for c in THRESHOLDS:
            assert np.count_nonzero(x < c) >= WINDOW and np.count_nonzero(x > c) >= WINDOW and c in x
    elif (func, name) == ("exp", "tiny"):
        assert np.count_nonzero((x != 0) & (np.abs(x) < MIN_NORMAL)) > 50 and (x < 0).any() and (x > 0).any()
    elif (func, name) == ("exp", "residues"):
        k = algorithm_k(x)
        assert set(k[k > 0] & 63) == set(k[k < 0] & 63) == set(range(64))
        assert {-64961, -64960, -64959, -65, -64, -63, -1, 0, 1, 63, 64, 65, 64959, 64960, 64961} <= set(k.tolist())
    elif (func, name) == ("exp", "near_k"):
        assert np.abs(t - np.round(t)).max() < 1e-6 and np.abs(algorithm_k(x)).max() > 64000
    elif (func, name) == ("exp", "half_k"):
        assert np.abs(t - np.floor(t) - 0.5).max() < 1e-6
        up = algorithm_k(x) - np.floor(t).astype(np.int64)     # the rounding switch goes both ways
        assert np.count_nonzero(up == 0) > 1000 and np.count_nonzero(up == 1) > 1000
    elif (func, name) == ("log", "nodes"):
        assert set(algorithm_j(x)) == set(range(45, 92)) and x.min() < 2.0**-1021 and x.max() > 2.0**1022
    elif (func, name) == ("log", "split"):
        mant = x.view(np.uint64) & np.uint64(2**52 - 1)
        for e in (-1022, -1, 0, 1, 1023):
            sel = np.frexp(x)[1] - 1 == e
            assert np.count_nonzero(mant[sel] > 0x6a09e667f3bcd) == 8 and np.count_nonzero(mant[sel] <= 0x6a09e667f3bcd) == 9
    elif (func, name) == ("log", "wide"):
        assert np.frexp(x)[1].min() < -1000 and np.frexp(x)[1].max() > 1000
    elif (func, name) == ("log", "near_one"):
        assert np.count_nonzero(x < 1) > 5000 and np.count_nonzero(x > 1) > 5000 and np.abs(x - 1).min() <= 2.0**-52
    elif (func, name) == ("log", "pow2"):
        assert x.size == 2046
    elif (func, name) == ("log", "grid"):
        assert np.array_equal(x * 2.0**53, np.round(x * 2.0**53)) and x.min() == 2.0**-53 and x.max() == 1 - 2.0**-53


def check_exp_borders(ev):
    """2^-1074 from the double just above -745.1332191019412 on, 0 at it and below; inf just above ln(DBL_MAX)."""
    b = EXP_ZERO_BORDER
    x = _window(b)
    got = ev("exp", x)
    assert np.all(got[x <= b] == 0.0) and np.all(got[x > b] == 2.0**-1074) and not np.signbit(got).any()
    t = EXP_HI_LITERAL
    got = ev("exp", np.array([t, np.nextafter(t, np.inf)]))
    assert got[0] == float.fromhex("0x1.fffffffffff2ap+1023") and got[1] == np.inf
    assert got[0] == reference("exp", [t])[0]


def check_special_values(ev):
    x, ref, cls = family("exp", "special")
    assert np.array_equal(x[[0, 1, 2, 3, 5, 6]], [0.0, -0.0, np.inf, -np.inf, 1.0, -1.0]) and np.isnan(x[4])
    got = ev("exp", x)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == np.inf and got[3] == 0.0 and np.isnan(got[4])
    assert got[5] == math.e and got[6] == ref[6] and abs(got[6] * math.e - 1.0) < 1e-15
    assert np.array_equal(got[7:], [np.inf, np.inf, 0.0]) and not np.signbit(got[[3, 9]]).any()
    x, ref, cls = family("log", "special")
    got = ev("log", x)
    assert got[0] == -np.inf and got[1] == 0.0 and not np.signbit(got[1])
    assert got[2] == -2.0**-53 and got[3] == float.fromhex("0x1.fffffffffffffp-53")
    assert got[4] == EXP_LN_DBL_MAX and got[5] == ref[5] and abs(got[5] - EXP_SUBNORMAL_BORDER) < 1e-12


def _main():
    import argparse
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true", help="evaluate on the GPU (debug_eval ops 5 and 4), not in the oracle")
    args = ap.parse_args()
    if args.device:
        from tardis_amd.engine import Engine
        eng = Engine(0)
        run = {"exp": lambda x: eng.debug_eval(5, x), "log": lambda x: eng.debug_eval(4, x)}
    else:
        from oracle import oracle
        run = {"exp": lambda x: oracle.exp_array(x, 1), "log": lambda x: oracle.log_array(x, 1)}
    print("%-4s %-11s %8s %8s %8s %10s %10s" % ("func", "family", "n", "differ", "max_dist", "subnormal", "sub_differ"))
    for func, names in FAMILIES.items():
        for name in names:
            x, ref, cls = family(func, name)
            got = run[func](x)
            n, nd, md = stats(got, ref)
            sub = cls == SUBNORMAL
            print("%-4s %-11s %8d %8d %8d %10d %10d" % (func, name, n, nd, md, np.count_nonzero(sub),
                                                     np.count_nonzero(bit_distance(got, ref)[sub])))
    if args.device:
        eng.close()


if __name__ == "__main__":
    _main()
