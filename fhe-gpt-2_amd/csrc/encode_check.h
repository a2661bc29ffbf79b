// SEAL's "encoded values are too large" check (ckks.h:525-540) as the encoder's host code decides it,
// and the threshold that lets the device take the same decision.  Host only, no HIP: encode.hip
// includes it, tests/cpp/encode_check_test.cpp checks it on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

// the check on the largest coefficient, tb = total_coeff_modulus_bit_count of the bound's level
inline bool size_fits(double max_coeff, int tb)
{
    const int max_bits = static_cast<int>(std::ceil(std::log2(std::max<double>(max_coeff, 1.0)))) + 1;
    return max_bits < tb;
}

// Does l1 >= sum |re| + |im| of the values prove the check?  Each value and its conjugate enter a
// coefficient with unit-modulus weights, fix = scale / n.
inline bool l1_proves_size(double fix, double l1, int tb)
{
    const double bound = fix * 2 * l1 * (1 + 1e-6) + 1;
    return std::isfinite(bound) && size_fits(bound, tb);
}

// The largest finite double size_fits accepts (tb >= 2, so that 1.0 fits).  Non-negative doubles
// order like their bit patterns and size_fits is monotone in them (log2 and ceil are), so this is a
// bisection over the patterns between 1.0 and DBL_MAX with the host's own log2: at most 62 calls,
// whatever the width of the band around 2^(tb-2) that log2 rounds to tb - 2.  The device compares
// the bit pattern of its maximum with this one and so decides as size_fits does for every finite
// maximum.
inline double largest_fitting(int tb)
{
    const auto bits = [](double x) {
        std::uint64_t u;
        std::memcpy(&u, &x, sizeof u);
        return u;
    };
    const auto value = [](std::uint64_t u) {
        double x;
        std::memcpy(&x, &u, sizeof x);
        return x;
    };
    if (size_fits(std::numeric_limits<double>::max(), tb)) return std::numeric_limits<double>::max();
    std::uint64_t lo = bits(1.0), hi = bits(std::numeric_limits<double>::max()); // lo fits, hi does not
    while (hi - lo > 1)
    {
        const std::uint64_t mid = lo + (hi - lo) / 2;
        if (size_fits(value(mid), tb))
            lo = mid;
        else
            hi = mid;
    }
    return value(lo);
}
