// Host only: the capacity of the device uniform sampler's redraw buffer (csrc/sample_cap.h), linking
// nothing from the project.  mean + 12 standard deviations + 64 of the reject count, against the
// probabilities worked out here with 128-bit integers.
//   sample_cap_test
#include "sample_cap.h"

#include <cstdio>
#include <vector>

static int g_fail = 0;
static void check(const char *what, bool ok)
{
    std::printf("[%s] %s\n", ok ? "PASS" : "FAIL", what);
    if (!ok) g_fail++;
}

int main()
{
    // rlwe.cpp:152: max_multiple = 2^64 - 1 - ((2^64 - 1) mod q) - 1; a word is rejected when >= it
    // seal50: the shape of SEAL's own primes, 2^50 - c 2n + 1: 2^64 mod q = 2^14 (2^14 - 1), p ~ 2^-36
    const uint64_t heavy = (3ull << 59) + 1, seal50 = (1ull << 50) - (1ull << 14) + 1, small = 97;
    for (uint64_t q : { heavy, seal50, small })
    {
        const unsigned __int128 two64 = (unsigned __int128)1 << 64;
        const uint64_t mm = ~0ULL - (~0ULL % q) - 1;
        const double want = (double)(two64 - mm) / 18446744073709551616.0;
        check("reject probability = (2^64 - max_multiple) / 2^64", std::fabs(uniform_reject_probability(q) - want) <= want * 1e-12);
    }
    check("a prime just above 1.5 * 2^60 rejects one word in 16", std::fabs(uniform_reject_probability(heavy) - 0.0625) < 1e-9);

    const std::vector<uint64_t> q = { seal50, heavy, heavy + 2, small };
    const int seal_only[2] = { 0, 0 }, heavy4[4] = { 1, 2, 1, 2 }, mixed[4] = { 0, 1, 0, 2 };
    // mean + 12 sigma = 1.2e-7 + 12 * 3.5e-4 rounds up to one word
    check("SEAL's primes: one word and the constant", uniform_redraw_cap(q.data(), seal_only, 2, 4096) == 65);
    // 4 limbs of 4096 words at p = 1/16: mean 1024, variance 960
    const uint32_t h4 = uniform_redraw_cap(q.data(), heavy4, 4, 4096);
    check("H4 at n = 4096: ceil(1024 + 12 sqrt(960)) + 64", h4 == (uint32_t)std::ceil(1024 + 12 * std::sqrt(960.0)) + 64);
    const uint32_t mx = uniform_redraw_cap(q.data(), mixed, 4, 4096);
    check("two heavy limbs of four: ceil(512 + 12 sqrt(480)) + 64", mx == (uint32_t)std::ceil(512 + 12 * std::sqrt(480.0)) + 64);
    // 18 heavy limbs at n = 2^16: past the 65536 of the host walk, far below the word count
    std::vector<int> h18(18, 1);
    const uint32_t big = uniform_redraw_cap(q.data(), h18.data(), 18, 65536);
    check("18 heavy limbs at n = 2^16 hold more than 65536 + 12 sigma", big > 73728 + 12 * 262 && big < 80000);
    // never more than the words drawn
    const int tiny[1] = { 3 };
    check("the capacity never exceeds the word count", uniform_redraw_cap(q.data(), tiny, 1, 32) <= 32);
    std::printf(g_fail ? "%d FAILED\n" : "ALL PASSED\n", g_fail);
    return g_fail ? 1 : 0;
}
