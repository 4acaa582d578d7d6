"""The oracle's portable exp / log (oracle/portable_math.h) against a correctly rounded reference that shares nothing
with it (tests/portable_math_ref.py: the standard library's `decimal` at 80 digits), on argument families laid out on the
places where the algorithm could go wrong.  The device's copy meets the same conditions in tests/test_portable_math_gpu.py.

If a normal-class family ever shows a mismatch: do not loosen the comparison.  Evaluate `reference(func, [x], prec=200)`;
if that confirms a true miss of the algorithm by one unit, enter the argument with its two candidates in
portable_math_ref.KNOWN_MISSES (at most 5 per family -- more means something is wrong, not unlucky)."""
import decimal
import math
import os
import re

import numpy as np
import pytest

import portable_math_ref as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(f, n) for f, names in pm.FAMILIES.items() for n in names]


def host_eval(oracle, func, x):
    return (oracle.exp_array if func == "exp" else oracle.log_array)(x, oracle.MATH_PORTABLE)


def test_families_stay_small():
    assert sum(pm.arguments(f, n).size for f, n in CASES) <= 200_000


@pytest.mark.parametrize("func,name", CASES)
def test_oracle_matches_correctly_rounded_reference(oracle, func, name):
    pm.check_structure(func, name)
    x, ref, cls = pm.family(func, name)
    n, differ, dist = pm.check(func, name, host_eval(oracle, func, x))
    print(f"{func} {name}: {n} arguments, {differ} differ from the reference, largest bit distance {dist}")


def test_known_misses_are_true_misses_by_one_unit(oracle):
    """Every listed argument: a 200-digit reference confirms the correctly rounded candidate, the oracle gives the other
    one, and the two are neighbours."""
    for (func, name), known in pm.KNOWN_MISSES.items():
        assert len(known) <= 5 and name in pm.FAMILIES[func]
        for x, (alg, rn) in known.items():
            assert x in pm.arguments(func, name)
            assert pm.reference(func, [x], prec=200)[0] == rn == pm.reference(func, [x])[0]
            assert host_eval(oracle, func, np.array([x]))[0] == alg and pm.bit_distance(alg, rn) == 1


def test_exp_borders_are_exact(oracle):
    pm.check_exp_borders(lambda func, x: host_eval(oracle, func, x))


def test_special_values(oracle):
    pm.check_special_values(lambda func, x: host_eval(oracle, func, x))


def test_generated_tables_are_identical():
    """tools/gen_log_table.py writes the same text twice; the device and the oracle must not drift apart."""
    with open(os.path.join(ROOT, "oracle", "portable_math_tables.h")) as a, \
            open(os.path.join(ROOT, "tardis_amd", "csrc", "mc_math_tables.h")) as b:
        assert a.read() == b.read()


def test_generated_tables_match_their_definitions():
    """Every constant of the generated header against its definition in tools/gen_log_table.py, evaluated with `decimal` at
    120 digits: a double-double (hi, lo) of v is hi = RN(v), lo = RN(v - hi).  The families above cannot see an error
    below about 2^-62 relative in one table entry (it moves a correctly rounded result for too few arguments); this can."""
    with open(os.path.join(ROOT, "oracle", "portable_math_tables.h")) as f:
        text = f.read().replace("\\\n", " ")
    macro = {}
    for line in text.splitlines():
        if line.startswith("#define "):
            name, _, rest = line[8:].partition(" ")
            macro[name] = [float.fromhex(h) for h in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", rest)]
    ctx = pm._context(120)
    D = decimal.Decimal
    ln2 = ctx.ln(D(2))

    def dd(v, parts=2):
        out = []
        for _ in range(parts):
            out.append(float(v))
            v = ctx.subtract(v, D(out[-1]))
        return out

    def truncated(v, bits):      # floor(v 2^bits) / 2^bits
        return float(ctx.divide(ctx.multiply(v, D(2**bits)).to_integral_value(decimal.ROUND_FLOOR), D(2**bits)))

    want = []
    for j in range(45, 92):
        c = ctx.divide(D(j), D(64))
        want += [1.0, 0.0, 0.0, 0.0] if j == 64 else dd(ctx.divide(D(1), c)) + dd(ctx.ln(c))
    assert "#define MC_LOG_TABLE_LEN 47\n" in text and macro["MC_LOG_TABLE_VALUES"] == want
    hi = truncated(ln2, 42)
    assert macro["MC_LN2_HI"] == [hi] and macro["MC_LN2_LO"] == [float(ctx.subtract(ln2, D(hi)))]
    assert macro["MC_LOG1P_TAIL_COEFS"] == [float(ctx.divide(D((-1) ** k), D(k + 3))) for k in range(10)]
    want = []
    for i in range(64):
        want += dd(ctx.exp(ctx.divide(ctx.multiply(ln2, D(i)), D(64))))
    assert "#define MC_EXP_TABLE_LEN 64\n" in text and macro["MC_EXP_TABLE_VALUES"] == want
    l64 = ctx.divide(ln2, D(64))
    hi = truncated(l64, 38)
    assert macro["MC_EXP_INV_LN2_64"] == [float(ctx.divide(D(64), ln2))] == [pm.INV_LN2_64]
    assert [macro["MC_EXP_LN2_64_HI"][0], macro["MC_EXP_LN2_64_LO"][0], macro["MC_EXP_LN2_64_LOLO"][0]] == [hi] + dd(ctx.subtract(l64, D(hi)))
    assert macro["MC_EXP_TAIL_COEFS"] == [float(ctx.divide(D(1), D(math.factorial(k + 3)))) for k in range(8)]


def test_kernel_arguments_stay_in_the_domain_of_log():
    """The callers of mcm::log: tau_event = -log(rng.random()) in the three propagation kernels and the macro-atom /
    v-packet draws (mc::Rng::random: (a * 2^26 + b) / 2^53, numpy's random_sample), and -log(xi1 xi2 xi3 xi4) of four
    pcg_double draws ((u >> 11) * 2^-53) in packet_source.hpp.  Either is 0 or at least the value below, and normal."""
    assert (0.0 * 67108864.0 + 1.0) / 9007199254740992.0 == 2.0**-53 >= pm.MIN_NORMAL      # mc::Rng::random, a = 0, b = 1
    xi = 1.0 * (1.0 / 9007199254740992.0)                                                  # pcg_double, u >> 11 == 1
    assert ((xi * xi) * xi) * xi == 2.0**-212 >= pm.MIN_NORMAL
