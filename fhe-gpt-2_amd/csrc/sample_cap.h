// Capacity of the redraw buffer of the on-device sample_poly_uniform (sample.hip k_uni_redraw),
// host only.  A bulk word of limb l is rejected with probability
//     p_l = (2^64 - max_multiple_l) / 2^64 = ((2^64 - 1) mod q_l + 2) / 2^64        (rlwe.cpp:152),
// independently per word, so the rejects of one draw over `limbs` limbs of n words are a sum of
// binomials with
//     mean = sum_l n p_l,     variance = sum_l n p_l (1 - p_l).
// The buffer holds
//     cap = ceil(mean + 12 sqrt(variance)) + 64
// redrawn words: 12 standard deviations (a tail below 2^-100 by Bernstein's bound for every n p_l) and
// a constant that covers the primes whose mean is far below one word (SEAL's own, 2^k - c 2n + 1:
// p_l ~ c n 2^(1-k), 2^-30 and below).  A draw
// beyond it writes nothing out of bounds: the entry is flagged and counted (mhe_keygen_stats).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

static inline double uniform_reject_probability(uint64_t q)
{
    return ((double)(~0ULL % q) + 2.0) * 0x1p-64;
}

static inline uint32_t uniform_redraw_cap(const uint64_t *q, const int *prime_of_limb, int limbs, size_t n)
{
    double mean = 0, var = 0;
    for (int l = 0; l < limbs; l++)
    {
        const double p = uniform_reject_probability(q[prime_of_limb[l]]);
        mean += (double)n * p;
        var += (double)n * p * (1.0 - p);
    }
    const double cap = std::ceil(mean + 12.0 * std::sqrt(var)) + 64.0;
    const double all = (double)n * limbs; // never more rejects than words
    return (uint32_t)(cap < all ? cap : all);
}
