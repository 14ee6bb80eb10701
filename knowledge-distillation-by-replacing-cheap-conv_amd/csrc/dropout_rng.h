// The random-number rule of the library, stated once: which elements a dropout call keeps.  Philox4x32-10 (Salmon et al., "Parallel
// random numbers: as easy as 1, 2, 3", SC'11), counter-based: the mask of a call is a pure function of (seed, offset, idx) and of
// nothing else -- no state, no stored mask, so a backward regenerates its forward's mask from the same pair, and layout, leading
// dimension, dtype, vector width and grid cannot change it.
//   idx = m * C + c (int64): m the pixel index (n*H + h)*W + w, c the logical channel, C the LOGICAL channel count (not a padded one)
//   key = (seed & 0xffffffff, seed >> 32)
//   counter = (q & 0xffffffff, q >> 32, offset & 0xffffffff, offset >> 32), q = idx >> 2
//   element idx uses output word idx & 3 and is kept iff word >= threshold (a uint32: round-down of p * 2^32)
//   y = keep ? x * scale : 0 in fp32
// Plain C++ for the host and the device alike (no HIP calls, no getenv, no globals): csrc/dropout.hip runs it,
// tests/test_dropout_host.py holds a host build to the generator's known answers and to the numpy restatement in tests/_dropoutref.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DROPOUT_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define DROPOUT_FN static inline
#endif

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // the round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // the Weyl increments of the key
constexpr int PHILOX_ROUNDS = 10;
constexpr int DROPOUT_WORDS = 4;        // elements one Philox block decides

struct PhiloxBlock { uint32_t w[4]; };

DROPOUT_FN PhiloxBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < PHILOX_ROUNDS; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    PhiloxBlock b;
    b.w[0] = c0; b.w[1] = c1; b.w[2] = c2; b.w[3] = c3;
    return b;
}

// the block that decides elements 4q .. 4q + 3 of a call
DROPOUT_FN PhiloxBlock dropout_block(uint64_t seed, uint64_t offset, int64_t q)
{
    return philox4x32_10((uint32_t)((uint64_t)q & 0xffffffffu), (uint32_t)((uint64_t)q >> 32), (uint32_t)(offset & 0xffffffffu),
                         (uint32_t)(offset >> 32), (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
}

DROPOUT_FN bool dropout_keep_word(uint32_t word, uint32_t threshold) { return word >= threshold; }

DROPOUT_FN bool dropout_keep(uint64_t seed, uint64_t offset, int64_t idx, uint32_t threshold)
{
    return dropout_keep_word(dropout_block(seed, offset, idx >> 2).w[idx & 3], threshold);
}

DROPOUT_FN float dropout_apply(float x, bool keep, float scale) { return keep ? x * scale : 0.f; }
