"""Device arithmetic on its whole domain, through Engine.debug_eval (debug_eval_kernel in tardis_mc_hip.hip):
  * mcm::exp / mcm::log (ops 5 / 4) on the argument families of tests/portable_math_ref.py: bit for bit equal to the
    oracle's copy, and -- independently of the shared tables -- the same conditions against the correctly rounded
    `decimal` reference as tests/test_portable_math_host.py asks of the oracle;
  * lanes that take an early return of exp beside lanes that do not, and launches whose size is no multiple of the block;
  * + * / sqrt floor and the unfused a * b + a (ops 0 1 2 3 8 6) against NumPy where IEEE arithmetic is hard: subnormal
    operands and results, overflow, signed zeros, invalid operations, NaN;
  * exact_div behind mid_range (op 9) across the whole guarded range and on both sides of its bounds."""
import ctypes
import decimal

import numpy as np
import pytest

import portable_math_ref as pm

pytestmark = pytest.mark.gpu

CASES = [(f, n) for f, names in pm.FAMILIES.items() for n in names]
OP = {"exp": 5, "log": 4}
TINY, MIN_NORMAL, DBL_MAX = 2.0**-1074, pm.MIN_NORMAL, pm.DBL_MAX


@pytest.fixture(scope="module")
def engine():
    from tardis_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def device_family(engine):
    """The device's results on a whole family, one launch each, evaluated once per module."""
    cache = {}

    def get(func, name):
        if (func, name) not in cache:
            cache[func, name] = engine.debug_eval(OP[func], pm.family(func, name)[0])
        return cache[func, name]
    return get


def same_bits(got, want):
    """Equal bit for bit (the sign of zero included) wherever `want` is a number, NaN wherever it is NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def mismatches(got, want, *operands):
    bad = np.flatnonzero(~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))[:8]
    return [tuple(float(o[i]).hex() for o in operands) + (float(got[i]).hex(), float(want[i]).hex()) for i in bad]


@pytest.mark.parametrize("func,name", CASES)
def test_device_matches_oracle_and_correctly_rounded_reference(engine, oracle, device_family, func, name):
    pm.check_structure(func, name)
    x, ref, cls = pm.family(func, name)
    got = device_family(func, name)
    host = (oracle.exp_array if func == "exp" else oracle.log_array)(x, oracle.MATH_PORTABLE)
    assert same_bits(got, host), mismatches(got, host, x)          # host / device identity, the subnormal range included
    n, differ, dist = pm.check(func, name, got)                    # the comparison that does not share the tables
    print(f"{func} {name}: {n} arguments, {differ} differ from the reference, largest bit distance {dist}")


def test_exp_borders_and_special_values(engine):
    ev = lambda func, x: engine.debug_eval(OP[func], x)
    pm.check_exp_borders(ev)
    pm.check_special_values(ev)


@pytest.fixture(scope="module")
def interleaved(device_family):
    """thresholds, special, subnormal and normal arguments of exp, element by element in a fixed permutation, so that
    lanes which return early (inf above 709.78..., 0 below -745.2, NaN, +-inf) share a wave with lanes that do not;
    with every element's result from its own family's launch."""
    parts = [("thresholds", 4108), ("special", 10), ("subnormal", 7900), ("normal", 7900)]
    x = np.concatenate([pm.family("exp", name)[0][:n] for name, n in parts])
    want = np.concatenate([device_family("exp", name)[:n] for name, n in parts])
    assert x.size == sum(n for _, n in parts) <= 20000
    perm = np.random.default_rng(301).permutation(x.size)
    return x[perm], want[perm]


def test_early_returns_beside_full_evaluations_in_one_wave(engine, interleaved):
    x, want = interleaved
    with np.errstate(invalid="ignore"):
        early = (x > pm.EXP_HI_LITERAL) | (x < pm.EXP_LO_LITERAL)
    per_wave = early[: x.size // 64 * 64].reshape(-1, 64).sum(axis=1)
    assert np.count_nonzero((per_wave > 0) & (per_wave < 64)) > 0.9 * per_wave.size     # nearly every wave is mixed
    got = engine.debug_eval(5, x)
    assert same_bits(got, want), mismatches(got, want, x)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_launch_sizes_off_the_block_size(engine, interleaved, n):
    """The grid is derived from n (256 threads a block).  The device-side output buffer is allocated by the library with
    exactly n elements, so what the kernel does beyond n on the device cannot be observed from here; what can be is the
    caller's buffer: a longer, poisoned `out` must come back untouched beyond n."""
    x, want = interleaved
    assert same_bits(engine.debug_eval(5, x[:n]), want[:n])
    poison = np.uint64(0x7ff8dead0000beef)
    out = np.full(n + 300, poison, dtype=np.uint64)
    xs = np.ascontiguousarray(x[:n])
    rc = engine._L.tardis_mc_debug_eval(engine._h, 5, xs.ctypes.data, None, out.ctypes.data, ctypes.c_int64(n))
    assert rc == 0
    assert same_bits(out[:n].view(np.float64), want[:n]) and np.all(out[n:] == poison)


# ---- plain operators -------------------------------------------------------------------------------------------------

def _wide(rng, n):
    """Doubles of every exponent, subnormal and (rarely) non-finite ones included: random bit patterns."""
    return rng.integers(0, 2**64, n, dtype=np.uint64).view(np.float64)


def _scaled(rng, n, e_lo, e_hi):
    """Random significands and signs with binary exponents in [e_lo, e_hi)."""
    m = 1.0 + rng.integers(0, 2**52, n).astype(np.float64) * 2.0**-52
    return np.ldexp(m, rng.integers(e_lo, e_hi, n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _pairs():
    rng = np.random.default_rng(401)
    v = np.array([0.0, TINY, 3 * TINY, 2.0**-1060, np.nextafter(MIN_NORMAL, 0.0), MIN_NORMAL, np.nextafter(MIN_NORMAL, 1.0),
                  1e-300, 1e-200, 1e-120, 2.0**-537, 2.0**-511, 0.5, 1.0 - 2.0**-53, 1.0, 1.0 + 2.0**-52, 3.0, 1e10,
                  2.0**52, 2.0**511, 2.0**512, 1e200, 2.0**1023, DBL_MAX, np.inf, np.nan])
    v = np.concatenate([v, -v])
    a, b = [np.repeat(v, v.size)], [np.tile(v, v.size)]
    n = 4000
    a.append(_wide(rng, n)), b.append(_wide(rng, n))
    for lo, hi in ((-1080, -1015), (1015, 1030)):      # products and quotients around the subnormal border / overflow
        e1 = rng.integers(-1000, 1000, n)
        e2 = rng.integers(lo, hi, n) - e1
        ok = np.abs(e2) < 1020
        x, y = _scaled(rng, n, 0, 1)[ok], _scaled(rng, n, 0, 1)[ok]
        a.append(np.ldexp(x, e1[ok])), b.append(np.ldexp(y, e2[ok]))      # a * b lands there
        a.append(np.ldexp(x, e1[ok])), b.append(np.ldexp(y, -e2[ok]))     # a / b lands there
    x = _scaled(rng, n, -1074 + 52, -1010)              # sums and differences of tiny numbers, cancellation into subnormals
    a.append(x), b.append(-x * (1.0 + rng.integers(-4, 5, n) * 2.0**-52))
    a.append(_scaled(rng, n, -1022, -1018) * 0.75), b.append(_scaled(rng, n, -1022, -1018) * 0.75)
    # results that round up into the smallest normal
    a.append(np.array([np.nextafter(MIN_NORMAL, 0.0), MIN_NORMAL, np.nextafter(MIN_NORMAL, 0.0), MIN_NORMAL * 2 - TINY, MIN_NORMAL * 2 - TINY]))
    b.append(np.array([1.0 + 2.0**-52, 1.0 - 2.0**-53, TINY, 0.5, 2.0]))
    return np.concatenate(a), np.concatenate(b)


def test_ieee_operators_on_hard_operands(engine):
    a, b = _pairs()
    sub = lambda r: (r != 0) & (np.abs(r) < MIN_NORMAL)
    with np.errstate(all="ignore"):
        want = {0: a + b, 1: a * b, 2: a / b}
        # the family is not vacuous: each hard class occurs in each operator it can occur in
        normal_ops = (np.abs(a) >= MIN_NORMAL) & (np.abs(b) >= MIN_NORMAL) & np.isfinite(a) & np.isfinite(b)
        for op in (0, 1, 2):
            r = want[op]
            assert np.count_nonzero(sub(r)) > 500 and np.count_nonzero(np.isinf(r) & np.isfinite(a) & np.isfinite(b)) > (100 if op else 3)
            assert np.count_nonzero(np.isnan(r) & ~np.isnan(a) & ~np.isnan(b)) >= 2      # inf - inf, inf * 0, 0 / 0, inf / inf
            assert np.count_nonzero((r == 0) & np.signbit(r)) >= 1 and np.count_nonzero((r == 0) & ~np.signbit(r)) > 3
        assert np.count_nonzero(sub(a) | sub(b)) > 500
        assert np.count_nonzero(sub(want[1]) & normal_ops) > 500 and np.count_nonzero(sub(want[2]) & normal_ops) > 500
        assert 1e-200 * 1e-120 in want[1][normal_ops] and 1e-300 / 1e10 in want[2][normal_ops]
        for op in (0, 1, 2):                                  # inexact results that round up into the smallest normal
            assert np.count_nonzero(np.abs(want[op][-5:]) == MIN_NORMAL) >= 1
        assert np.count_nonzero((np.abs(want[1]) == MIN_NORMAL) & (np.abs(a) != MIN_NORMAL) & (np.abs(b) != MIN_NORMAL) & normal_ops) > 0
        assert np.count_nonzero(np.isinf(want[2]) & (b == 0) & (a != 0) & np.isfinite(a)) > 10  # x / 0
    for op in (0, 1, 2):
        got = engine.debug_eval(op, a, b)
        assert same_bits(got, want[op]), (op, mismatches(got, want[op], a, b))


def test_sqrt_and_floor_on_hard_operands(engine):
    rng = np.random.default_rng(402)
    n = rng.integers(1, 2**26, 2000).astype(np.float64)
    squares = np.concatenate([n * n, np.ldexp(n * n, -600), np.ldexp(n * n, 400)])
    x = np.concatenate([[0.0, -0.0, TINY, 3 * TINY, np.nextafter(MIN_NORMAL, 0.0), MIN_NORMAL, 1.0, 2.0, DBL_MAX, np.inf,
                         np.nan, -1.0, -TINY, -np.inf],
                        squares, np.nextafter(squares, 0.0), np.nextafter(squares, np.inf),
                        np.abs(_scaled(rng, 4000, -1070, -1022)), np.abs(_wide(rng, 4000))])
    with np.errstate(all="ignore"):
        want = np.sqrt(x)
    assert np.signbit(want[1]) and want[1] == 0 and want[2] == 2.0**-537 and np.isnan(want[11:14]).all()
    assert np.array_equal(np.sqrt(squares[:2000]), n) and np.count_nonzero((x != 0) & (x < MIN_NORMAL)) > 3000
    got = engine.debug_eval(3, x)
    assert same_bits(got, want), mismatches(got, want, x)

    k = rng.integers(0, 2**51, 1000).astype(np.float64)
    y = np.concatenate([[0.0, -0.0, 0.5, -0.5, np.nextafter(1.0, 0.0), -np.nextafter(1.0, 0.0), 1.0, -1.0, TINY, -TINY,
                         -np.nextafter(MIN_NORMAL, 0.0), -MIN_NORMAL, 2.0**52, 2.0**52 + 1.0, 2.0**53, -(2.0**52), -(2.0**52) - 1.0,
                         2.0**52 - 0.5, -(2.0**52) + 0.5, 2.0**51 + 0.5, 1e300, -1e300, DBL_MAX, -DBL_MAX, np.inf, -np.inf, np.nan],
                        k + 0.5, -k - 0.5, 2.0**52 + k, -(2.0**52) - k, -np.abs(_scaled(rng, 1000, -1070, -1022)),
                        _wide(rng, 4000)])
    with np.errstate(all="ignore"):
        want = np.floor(y)
    assert np.signbit(want[1]) and want[1] == 0 and want[3] == -1.0 and want[9] == -1.0 and want[10] == -1.0
    assert np.all(want[27 + 4000:27 + 5000] == -1.0)          # negative subnormals
    got = engine.debug_eval(8, y)
    assert same_bits(got, want), mismatches(got, want, y)


def test_multiply_add_stays_unfused(engine):
    """a * b + a is two roundings.  The pairs include those where one rounding (an fma) gives another double; that they
    exist here is asserted on the host with an exact product."""
    rng = np.random.default_rng(403)
    n = 3000
    a = np.concatenate([_scaled(rng, n, -3, 4), _scaled(rng, n, -1022, -1016), _scaled(rng, n, 500, 512)])
    b = np.concatenate([_scaled(rng, n, -3, 4), _scaled(rng, n, -4, 0), _scaled(rng, n, 500, 512)])
    pa, pb = _pairs()
    a, b = np.concatenate([a, pa[:2704]]), np.concatenate([b, pb[:2704]])     # and every pair of the special values
    with np.errstate(all="ignore"):
        want = a * b + a
    ctx = decimal.Context(prec=1600, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
    D = decimal.Decimal
    fused = np.array([float(ctx.add(ctx.multiply(D(float(p)), D(float(q))), D(float(p)))) for p, q in zip(a[:2 * n], b[:2 * n])])
    differ = fused != want[:2 * n]
    assert np.count_nonzero(differ[:n]) > 100 and np.count_nonzero(differ[n:]) > 100, (differ[:n].sum(), differ[n:].sum())
    got = engine.debug_eval(6, a, b)
    assert same_bits(got, want), mismatches(got, want, a, b)


# ---- exact_div behind mid_range ------------------------------------------------------------------------------------------

def test_exact_division_across_the_guarded_range(engine):
    """Op 9 is the kernels' division: exact_div (reciprocal and two fmas) once mid_range holds for both operands (or the
    numerator is 0), plain division otherwise.  Adversarial significands as in test_hip_parity.test_exact_division, but
    the exponents span all of (1e-140, 1e140) and a little more, with the neighbours of both bounds on either side."""
    rng = np.random.default_rng(404)
    n = 200_000

    def rand(n, e_lo=-467, e_hi=467):
        m = rng.integers(0, 2**52, n, dtype=np.uint64)
        kind = rng.integers(0, 6, n)
        m = np.where(kind == 1, np.uint64(2**52 - 1) - (m & np.uint64(0xff)), m)
        m = np.where(kind == 2, m & np.uint64(0xff), m)
        m = np.where(kind == 3, m & np.uint64(0xfffff00000000), m)
        e = (rng.integers(e_lo, e_hi, n) + 1023).astype(np.uint64)
        return ((e << np.uint64(52)) | m).view(np.float64) * np.where(rng.random(n) < 0.5, -1.0, 1.0)

    edges = np.array([f(bound, to) for bound in (1e-140, 1e140) for f, to in
                      ((np.nextafter, 0.0), (lambda v, _: v, None), (np.nextafter, np.inf))])
    edges = np.concatenate([edges, -edges])
    m = 500
    e = np.repeat(edges, m)
    a = np.concatenate([rand(n - 4 * e.size - m), e, rand(e.size), e, np.tile(edges, m), np.zeros(m)])
    b = np.concatenate([rand(n - 4 * e.size - m), rand(e.size), e, np.tile(edges, m), e, rand(m)])
    assert a.size == b.size == n
    mid = lambda v: (np.abs(v) > 1e-140) & (np.abs(v) < 1e140)
    fast = (mid(a) | (a == 0)) & mid(b)
    counts = np.count_nonzero(fast), np.count_nonzero(~fast), np.count_nonzero(fast & (a == 0))
    assert counts[0] > 0.85 * n and counts[1] > 5000 and counts[2] > 0.9 * m, counts
    for v in (a, b):                                          # both arms next to both bounds, and binades next to them
        assert np.abs(v[fast & (v != 0)]).min() == np.nextafter(1e-140, 1.0) and np.abs(v[fast]).max() == np.nextafter(1e140, 0.0)
        assert (np.abs(v) == 1e-140).any() and (np.abs(v) == 1e140).any() and np.abs(v).min() < 1e-140 < 1e140 < np.abs(v).max()
    want = a / b
    assert np.isfinite(want).all() and np.all((want == 0) == (a == 0))
    got = engine.debug_eval(9, a, b)
    assert same_bits(got, want), mismatches(got, want, a, b)
