// mt_generation.hpp -- finishing a generation of an MT19937 state 64 words at a time.
//
// genrand's twist (mt19937.c) replaces the 624 state words in place, one after the other:
//     y = (mt[k] & UPPER) | (mt[(k + 1) % 624] & LOWER);   mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (y & 1 ? MATRIX_A : 0)
// so that word k is a function of the OLD words k and k + 1 (the NEW word 0 for k = 623) and of word k + 397 -- old while k < 227,
// the NEW word k - 227 from there on.  A state whose words [0, k0) are already those of the new generation (k0 a multiple of 8: the
// lanes of the wave kernel regenerate 8 words per refill) is completed here in rounds of 64 words: lane l of round r owns word
// k = k0 + 64 r + l.  Its third input is
//     * a word of memory as it stands before the call: the old mt[k + 397] (k < 227), or the new mt[k - 227] where k - 227 < k0;
//     * else (k - 227 >= k0) a word produced earlier in this call: 227 = 3 * 64 + 35, so it is owned by lane (l + 29) % 64 of round
//       r - 4 (l < 35) or r - 3 (l >= 35) -- a rotation of the wave by ROT lanes, no memory.  Only rounds 0 .. 3 read memory for it.
// Its second input is the first input of the next lane (of lane 0 of the next round for l = 63), word 623 takes the new word 0: from
// memory, or from lane 0 of round 0 when k0 = 0.
// All loads come first, then the rounds; a round's words are stored as soon as they exist (behind every load in program order).
//
// The same statement twice: mt_complete_generation_host() with the 64 lanes as a loop (tests/test_mt_generation.py compares it
// with the sequential twist for every k0) and, for hipcc, mt_complete_generation_wave() with the lanes as lanes.
#pragma once
#include <cstdint>

namespace mtg {

constexpr int N = 624, M = 397, BACK = N - M;  // BACK = 227: word k pairs with the NEW word k - 227 once k >= 227
constexpr int LANES = 64;
constexpr int ROUNDS = (N + LANES - 1) / LANES;                  // 10 (k0 = 0)
constexpr int ROT = LANES - BACK % LANES;                        // 29: lane l takes the word of lane (l + 29) % 64 ...
constexpr int FAR = BACK / LANES + 1, NEAR = BACK / LANES;       // ... of round r - 4 where l < 35, of round r - 3 where l >= 35
constexpr int MEM_ROUNDS = (BACK + LANES - 1) / LANES;           // 4: rounds whose third input (partly) comes from memory
static_assert(ROT == 29 && FAR == 4 && NEAR == 3 && ROUNDS == 10 && MEM_ROUNDS == 4, "");

#if defined(__HIPCC__)
#define MTG_FN __host__ __device__ inline
#else
#define MTG_FN inline
#endif

MTG_FN uint32_t twist(uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
MTG_FN int clamped(int k) { return k < N ? k : N - 1; }
// the third input of word k = k0 + 64 r + l is read from memory (else it is produced in this call: 64 r + l >= 227)
MTG_FN bool third_from_memory(int r, int l) { return LANES * r + l < BACK; }
MTG_FN int third_index(int k) { return k < BACK ? k + M : k - BACK; }
// what lane s offers to the rotation of round r: lanes 29 .. 63 are read by lanes 0 .. 34, which want round r - 4
MTG_FN int offered_round(int r, int s) { return s >= ROT ? r - FAR : r - NEAR; }

// mt[k0 .. 623] <- the new generation; mt[0 .. k0) is new already.  k0 a multiple of 8 in [0, 624).
// Always ROUNDS rounds, straight-line: a lane whose word lies beyond the state (k >= 624) loads word 623 and its third input instead,
// computes on them and stores nothing.
inline void mt_complete_generation_host(uint32_t *mt, int k0)
{
    uint32_t a[ROUNDS + 1][LANES], c[MEM_ROUNDS][LANES], nw[ROUNDS][LANES];
    // ---- loads
    for (int r = 0; r < ROUNDS; ++r)
        for (int l = 0; l < LANES; ++l) a[r][l] = mt[clamped(k0 + LANES * r + l)];
    for (int l = 0; l < LANES; ++l) a[ROUNDS][l] = 0u;
    for (int r = 0; r < MEM_ROUNDS; ++r)
        for (int l = 0; l < LANES; ++l) c[r][l] = mt[third_index(clamped(k0 + LANES * r + l))];
    const uint32_t w0 = mt[0];
    // ---- rounds
    for (int r = 0; r < ROUNDS; ++r) {
        uint32_t offer[LANES];
        for (int s = 0; s < LANES; ++s) {
            const int q = offered_round(r, s);
            offer[s] = q >= 0 ? nw[q][s] : 0u;
        }
        for (int l = 0; l < LANES; ++l) {
            const int k = k0 + LANES * r + l;
            uint32_t b = l < LANES - 1 ? a[r][l + 1] : a[r + 1][0];
            if (k == N - 1) b = k0 == 0 ? nw[0][0] : w0;
            const uint32_t t = third_from_memory(r, l) ? c[r][l] : offer[(l + ROT) % LANES];
            nw[r][l] = twist(a[r][l], b, t);
        }
    }
    // ---- stores
    for (int r = 0; r < ROUNDS; ++r)
        for (int l = 0; l < LANES; ++l) {
            const int k = k0 + LANES * r + l;
            if (k < N) mt[k] = nw[r][l];
        }
}

#if defined(__HIPCC__)
// The wave form: all 64 lanes call it with the same st (a pointer to global memory) and k0.  Vector loads and stores only (the index
// of word 0 is made opaque: a load with a wave-uniform address could become a scalar load, and the scalar cache does not see the
// vector stores that wrote the word).
template <class GPtr> __device__ __forceinline__ void mt_complete_generation_wave(GPtr st, int k0, int lane)
{
    uint32_t a[ROUNDS + 1], c[MEM_ROUNDS], nw[ROUNDS];
    const int kl = k0 + lane;
    // ---- loads
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) a[r] = st[clamped(kl + LANES * r)];
    a[ROUNDS] = 0u;
    unsigned zero = 0u;
    asm volatile("" : "+v"(zero));
    const uint32_t w0 = st[zero];
#pragma unroll
    for (int r = 0; r < MEM_ROUNDS; ++r) c[r] = st[third_index(clamped(kl + LANES * r))];
    // ---- rounds
    const int next = (lane + 1) & (LANES - 1), rot = (lane + ROT) & (LANES - 1);
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        uint32_t b = (uint32_t)__shfl((int)a[r], next);
        if (lane == LANES - 1) b = (uint32_t)__builtin_amdgcn_readlane((int)a[r + 1], 0);
        if (kl + LANES * r == N - 1) b = k0 == 0 ? (uint32_t)__builtin_amdgcn_readlane((int)nw[0], 0) : w0;
        uint32_t t;
        if (r < NEAR) t = c[r < MEM_ROUNDS ? r : 0];  // 64 r + l < 227 for every lane
        else {
            const uint32_t far_w = r >= FAR ? nw[r >= FAR ? r - FAR : 0] : 0u, near_w = nw[r >= NEAR ? r - NEAR : 0];
            t = (uint32_t)__shfl((int)(lane >= ROT ? far_w : near_w), rot);
            if (r < MEM_ROUNDS && third_from_memory(r, lane)) t = c[r < MEM_ROUNDS ? r : 0];
        }
        nw[r] = twist(a[r], b, t);
        if (kl + LANES * r < N) st[kl + LANES * r] = nw[r];  // (behind every load in program order; stored here so that only four rounds' words stay in registers)
    }
}
// The states of the lanes in `todo`, one after the other: lane o's state starts at wave_states + o * STRIDE and is complete up to its k0.
// (Wave-uniform loop; the loads of a state do not wait for the stores of the one before.)
template <int STRIDE, class GPtr> __device__ __forceinline__ void mt_complete_generations_wave(GPtr wave_states, unsigned long long todo, int k0, int lane)
{
    // (say that the pointer and the mask are wave-uniform, whatever the caller computed them from: the address arithmetic below is scalar)
    const unsigned long long base = (unsigned long long)wave_states;
    wave_states = (GPtr)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)base));
    unsigned long long m = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(todo >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)todo);
    for (; m; m &= m - 1ull) {
        const int o = __ffsll((long long)m) - 1;
        mt_complete_generation_wave(wave_states + (size_t)o * (size_t)STRIDE, __builtin_amdgcn_readlane(k0, o), lane);
    }
}
#endif

}  // namespace mtg
