"""CPU check of the wave-wide completion of an MT19937 generation (tardis_amd/csrc/mt_generation.hpp, used by the lane-sweep wave kernel,
tardis_amd/csrc/propagate_wave.hpp): the plain-C++ statement of the rounds, the indices and the rotation by 29 lanes -- the 64 lanes as a loop --
against the sequential in-place twist of mt19937.c (genrand_int32's regeneration loop), for every start word k0 the kernel can hand it, and the
doubles that follow against numpy's legacy stream (oracle.mt19937_random)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M = 624, 397
K0S = list(range(0, N, 8))  # a lane regenerates 8 words per refill: 0, 8, ..., 616

SHIM = """
#include "mt_generation.hpp"
extern "C" void complete_generation(uint32_t *mt, int k0) { mtg::mt_complete_generation_host(mt, k0); }
"""


@pytest.fixture(scope="module")
def complete(tmp_path_factory):
    d = tmp_path_factory.mktemp("mt_generation")
    src, lib = d / "shim.cpp", d / "libmtg.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tardis_amd", "csrc"), str(src), "-o", str(lib)], check=True)
    fn = C.CDLL(str(lib)).complete_generation
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_int]

    def call(mt, k0):
        out = np.ascontiguousarray(mt, dtype=np.uint32).copy()
        fn(out.ctypes.data, k0)
        return out
    return call


def init_genrand(seed):
    mt = np.zeros(N, dtype=np.uint64)
    mt[0] = seed & 0xFFFFFFFF
    for k in range(1, N):
        mt[k] = (1812433253 * (int(mt[k - 1]) ^ (int(mt[k - 1]) >> 30)) + k) & 0xFFFFFFFF
    return mt.astype(np.uint32)


def sequential_twist(mt, first, end):
    """Words [first, end) of mt19937.c's regeneration, in place and in order (a copy is returned)."""
    s = [int(x) for x in mt]
    for k in range(first, end):
        y = (s[k] & 0x80000000) | (s[(k + 1) % N] & 0x7FFFFFFF)
        s[k] = s[(k + M) % N] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
    return np.array(s, dtype=np.uint32)


def tempered_doubles(words):
    y = words.astype(np.uint64)
    y ^= y >> np.uint64(11)
    y ^= (y << np.uint64(7)) & np.uint64(0x9D2C5680)
    y ^= (y << np.uint64(15)) & np.uint64(0xEFC60000)
    y ^= y >> np.uint64(18)
    a, b = y[0::2] >> np.uint64(5), y[1::2] >> np.uint64(6)
    return (a.astype(np.float64) * 67108864.0 + b.astype(np.float64)) / 9007199254740992.0


def _states():
    rng = np.random.default_rng(19937)
    states = [("random %d" % i, rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)) for i in range(3)]
    states.append(("all ones", np.full(N, 0xFFFFFFFF, dtype=np.uint32)))
    states.append(("upper bits only", np.full(N, 0x80000000, dtype=np.uint32)))
    for seed in (0, 1, 23111963, 2 ** 32 - 2):
        states.append(("init_genrand(%d)" % seed, init_genrand(seed)))
        states.append(("init_genrand(%d), second generation" % seed, sequential_twist(init_genrand(seed), 0, N)))
    return states


@pytest.mark.parametrize("name,old", _states(), ids=[n for n, _ in _states()])
def test_completion_equals_the_sequential_twist_for_every_k0(complete, name, old):
    whole = sequential_twist(old, 0, N)
    for k0 in K0S:
        partial = np.concatenate([whole[:k0], old[k0:]])  # words [0, k0) regenerated, the rest as the last generation left them
        assert np.array_equal(sequential_twist(partial, k0, N), whole), k0  # (the yardstick itself: continuing in place gives the whole generation)
        got = complete(partial, k0)
        assert np.array_equal(got, whole), (name, k0, np.flatnonzero(got != whole)[:8])


@pytest.mark.parametrize("seed", [0, 1, 1963, 2 ** 32 - 2])
def test_the_doubles_that_follow_are_numpys(oracle, complete, seed):
    """The kernel's protocol over ten generations: the first one word by word, every later one 8-word refills up to some k0 (another in every
    generation, 0 and 616 among them), the completion from there, then reads only."""
    n_draws = 3000
    want = oracle.mt19937_random(seed, n_draws)
    rng = np.random.default_rng(seed % 1000)
    k0s = [0, 616] + [int(8 * rng.integers(0, 78)) for _ in range(8)]
    mt = sequential_twist(init_genrand(seed), 0, N)
    words = [mt.copy()]
    for k0 in k0s:
        mt = sequential_twist(mt, 0, k0)
        mt = complete(mt, k0)
        words.append(mt.copy())
    got = tempered_doubles(np.concatenate(words))[:n_draws]
    assert len(got) == n_draws
    assert np.array_equal(got, want)
