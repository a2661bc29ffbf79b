// The encoder's size-check threshold (fhe-gpt-2_amd/csrc/encode_check.h) on the CPU, linking nothing
// from the project: for every tb from 2 to 1100, m = largest_fitting(tb) passes size_fits and the
// next double above it does not (or m is DBL_MAX, when every finite value fits), so a device that
// compares bit patterns with m decides as size_fits does.  Then the verdicts on a band of 4096 ulps on
// either side of 2^(tb-2), where log2 rounds to tb - 2 over a width that grows with tb, compared
// pattern against pattern; and the l1 predicate on both sides of its bound.
//   encode_check_test
#include "encode_check.h"

#include <cstdio>

static std::uint64_t bits(double x)
{
    std::uint64_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}
static double value(std::uint64_t u)
{
    double x;
    std::memcpy(&x, &u, sizeof x);
    return x;
}

int main()
{
    int checked = 0, failed = 0;
    const double top = std::numeric_limits<double>::max(), inf = std::numeric_limits<double>::infinity();
    for (int tb = 2; tb <= 1100; tb++)
    {
        const double m = largest_fitting(tb);
        bool ok = std::isfinite(m) && size_fits(m, tb) && (m == top || !size_fits(std::nextafter(m, inf), tb));
        // the device's decision (pattern <= pattern of m) against the host's, around 2^(tb-2)
        if (tb - 2 <= 1023)
        {
            const std::uint64_t c = bits(std::ldexp(1.0, tb - 2));
            for (std::uint64_t u = c - 4096; ok && u <= c + 4096; u++)
                if (value(u) >= 0) ok = (u <= bits(m)) == size_fits(value(u), tb);
        }
        // far away on both sides, zero and the largest finite double
        for (double x : { 0.0, 0.5, 1.0, std::ldexp(1.0, (tb - 2) / 2), std::ldexp(1.0, std::min(tb - 1, 1023)), top })
            ok = ok && (bits(x) <= bits(m)) == size_fits(x, tb);
        if (!ok) std::printf("tb %d: largest_fitting gives %a\n", tb, m);
        checked++;
        failed += !ok;
    }
    // l1 predicate: fix * 2 * l1 * (1 + 1e-6) + 1 against the same check
    {
        const int tb = 97;
        const double fix = std::ldexp(1.0, 30 - 12);
        const bool ok = l1_proves_size(fix, std::ldexp(1.0, 95 - 19 - 1), tb) &&
                        !l1_proves_size(fix, std::ldexp(1.0, 95 - 19), tb) && !l1_proves_size(fix, inf, tb) &&
                        l1_proves_size(fix, 0.0, tb);
        if (!ok) std::printf("l1_proves_size: wrong verdict around the bound\n");
        checked++;
        failed += !ok;
    }
    std::printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
