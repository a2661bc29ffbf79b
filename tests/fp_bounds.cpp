// Host check of the FP64 forward butterflies of csrc/fparith.h at the entries the ModUp column pass
// (csrc/ntt.h k_modup_col) and the fused key MAC admit: the bounds that fparith.h states under
// "Unreduced lifts", stage by stage, and every residue against exact integer arithmetic.
// The arithmetic is fparith.h's own (MHE_FPARITH_HOST); build with -ffp-contract=off.
// Stand-alone: exit status 0 and a line per prime when everything holds, 1 with the first failures.
#define MHE_FPARITH_HOST
#include "../fhe-gpt-2_amd/csrc/fparith.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned __int128 u128;
typedef uint64_t u64;

static int failures = 0;
#define CHECK(cond, ...)                                                                                               \
    do                                                                                                                 \
    {                                                                                                                  \
        if (!(cond))                                                                                                   \
        {                                                                                                              \
            if (failures++ < 20)                                                                                       \
            {                                                                                                          \
                std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);                                             \
                std::printf(__VA_ARGS__);                                                                              \
                std::printf("\n");                                                                                     \
            }                                                                                                          \
        }                                                                                                              \
    } while (0)

static u64 mulmod(u64 a, u64 b, u64 q) { return (u64)((u128)a * b % q); }
static u64 powmod(u64 a, u64 e, u64 q)
{
    u64 r = 1;
    for (; e; e >>= 1, a = mulmod(a, a, q))
        if (e & 1) r = mulmod(r, a, q);
    return r;
}
static bool is_prime(u64 n)
{
    static const u64 bases[] = { 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37 }; // deterministic below 2^64
    u64 d = n - 1;
    int s = 0;
    while (!(d & 1)) d >>= 1, s++;
    for (u64 a : bases)
    {
        if (a % n == 0) continue;
        u64 x = powmod(a % n, d, n);
        if (x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int r = 1; r < s && comp; r++)
        {
            x = mulmod(x, x, n);
            if (x == n - 1) comp = false;
        }
        if (comp) return false;
    }
    return true;
}
// the largest NTT prime (q = 1 mod 2^17) below 2^bits
static u64 prime_below(int bits)
{
    for (u64 q = ((u64)1 << bits) - ((u64)1 << 17) + 1;; q -= (u64)1 << 17)
        if (is_prime(q)) return q;
}

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static u64 residue(double v, u64 q) // v an integer, |v| < 2^62
{
    long long r = (long long)v % (long long)q;
    return (u64)(r < 0 ? r + (long long)q : r);
}

constexpr int R = 256, STAGES = 8; // one column (or row) pass of n = 2^16

struct Pass
{
    u64 q;
    double qd, qinv;
    std::vector<TwF> tw; // (w, w/q), entries 1 .. R-1 as the passes index them
    std::vector<u64> twi;
    explicit Pass(u64 q_) : q(q_), qd((double)q_), qinv(1.0 / (double)q_), tw(R), twi(R)
    {
        for (int k = 1; k < R; k++)
        {
            u64 w = rnd() % q;
            if (k % 37 == 0) w = q - 1; // the largest twiddle
            if (k % 41 == 0) w = 0;
            if (k % 43 == 0) w = 1;
            twi[k] = w;
            tw[k].x = (double)w;
            tw[k].y = (double)w / qd;
        }
    }
    // Stage s on v (doubles) and on ref (canonical integers): lazy or full butterflies.  `bound` is what
    // every value must stay within after the stage; the product r of every butterfly within 1.5 q.
    void stage(std::vector<double> &v, std::vector<u64> &ref, int s, bool lazy, double bound, const char *what)
    {
        const int gap = R >> (s + 1);
        for (int i = 0; i < R; i++)
        {
            if (i & gap) continue;
            const int k = (1 << s) + (i >> (STAGES - s));
            const double r = fp_mulmod(v[i + gap], tw[k].x, tw[k].y, qd);
            CHECK(std::fabs(r) <= 1.5 * qd, "%s q=%llu stage %d: |r| = %.0f", what, (unsigned long long)q, s, std::fabs(r));
            CHECK(residue(r, q) == mulmod(ref[i + gap], twi[k], q), "%s q=%llu stage %d: product residue", what,
                  (unsigned long long)q, s);
            if (lazy)
                fwd_bfly_f_lazy(v[i], v[i + gap], tw[k], qd);
            else
                fwd_bfly_f(v[i], v[i + gap], tw[k], qd, qinv);
            const u64 t = mulmod(ref[i + gap], twi[k], q), x = ref[i];
            ref[i] = (x + t) % q;
            ref[i + gap] = (x + q - t) % q;
        }
        for (int i = 0; i < R; i++)
        {
            CHECK(v[i] == std::rint(v[i]), "%s q=%llu stage %d: not an integer", what, (unsigned long long)q, s);
            CHECK(std::fabs(v[i]) <= bound, "%s q=%llu stage %d: |v| = %.0f > %.0f", what, (unsigned long long)q, s,
                  std::fabs(v[i]), bound);
            CHECK(residue(v[i], q) == ref[i], "%s q=%llu stage %d: residue", what, (unsigned long long)q, s);
        }
    }
};

// entry vectors of magnitude at most m: all m, alternating m / -m (or m / 0 when unsigned), random
static std::vector<std::vector<double>> entries(double m, bool with_negative)
{
    std::vector<std::vector<double>> out;
    std::vector<double> v(R);
    for (int i = 0; i < R; i++) v[i] = m;
    out.push_back(v);
    for (int i = 0; i < R; i++) v[i] = (i & 1) ? (with_negative ? -m : 0.0) : m;
    out.push_back(v);
    for (int i = 0; i < R; i++) v[i] = (i & 1) ? m : (with_negative ? -m : 0.0);
    out.push_back(v);
    for (int i = 0; i < R; i++) v[i] = ((i / 16) & 1) ? (with_negative ? -m : 0.0) : m;
    out.push_back(v);
    for (int rep = 0; rep < 8; rep++)
    {
        for (int i = 0; i < R; i++)
        {
            const double x = (double)(rnd() % ((u64)m + 1));
            v[i] = (with_negative && (rnd() & 1)) ? -x : x;
        }
        out.push_back(v);
    }
    return out;
}

static std::vector<u64> canon_of(const std::vector<double> &v, u64 q)
{
    std::vector<u64> r(R);
    for (int i = 0; i < R; i++) r[i] = residue(v[i], q);
    return r;
}

// The fused MAC's row pass from what the column pass left (|v| <= m): lazy while the prime is lazy.
static void mac_pass(u64 q, const std::vector<double> &in, double m, bool lazy)
{
    Pass p(q);
    std::vector<double> v = in;
    std::vector<u64> ref = canon_of(v, q);
    const double qd = (double)q;
    for (int s = 0; s < STAGES; s++)
        p.stage(v, ref, s, lazy, lazy ? m + 1.5 * qd * (s + 1) : 2 * qd + 1, lazy ? "mac lazy" : "mac full");
    if (!lazy) return;
    // the lazy MAC multiplies the unreduced digit by a key residue (fp_mulmod_gen: |a| <= 2^51, then
    // |result| <= 1.25 q, which is what lets its sums stay exact)
    for (int i = 0; i < R; i++)
    {
        CHECK(std::fabs(v[i]) <= 2251799813685248.0, "mac lazy exit above 2^51"); // 16q <= 2^51
        const u64 k = (i % 5 == 0) ? q - 1 : rnd() % q;
        const double r = fp_mulmod_gen(v[i], (double)k, qd, 1.0 / qd);
        CHECK(std::fabs(r) <= 1.25 * qd, "q=%llu key product %.0f above 1.25 q", (unsigned long long)q, std::fabs(r));
        CHECK(residue(r, q) == mulmod(ref[i], k, q), "q=%llu key product residue", (unsigned long long)q);
    }
}

static void lazy_prime(u64 q)
{
    const double qd = (double)q, qinv = 1.0 / qd;
    const bool fold = q < ((u64)1 << 46);
    // the largest unreduced lift: a digit prime q_J <= 4q, residue q_J - 1 <= 4q - 1
    for (const auto &in : entries(4 * qd - 1, false))
    {
        Pass p(q);
        std::vector<double> v = in;
        std::vector<u64> ref = canon_of(v, q);
        for (int s = 0; s < STAGES - 1; s++) p.stage(v, ref, s, true, 4 * qd + 1.5 * qd * (s + 1), "lazy");
        std::vector<double> kept = v;
        std::vector<u64> kept_ref = ref;
        // today's exit, every lazy prime: the 8th lazy stage (16q <= 2^51), then a reduction per value
        p.stage(v, ref, STAGES - 1, true, 16 * qd, "lazy");
        std::vector<double> handed(R);
        for (int i = 0; i < R; i++)
        {
            CHECK(std::fabs(v[i]) <= 2251799813685248.0, "lazy exit above 2^51");
            const double back = fp_from_s48(fp_to_s48(v[i], qd, qinv) & 0xFFFFFFFFFFFFull);
            CHECK(std::fabs(back) <= qd / 2 + 1 && residue(back, q) == ref[i], "q=%llu reduced 48-bit exit", (unsigned long long)q);
            CHECK(fp_canon(v[i], qd, qinv) == ref[i], "q=%llu canonical exit", (unsigned long long)q);
            handed[i] = back;
        }
        mac_pass(q, handed, qd / 2 + 1, true);
        if (!fold) continue;
        // the folded exit (q < 2^46): the 8th stage reduces x; the result goes into the slot as it is
        v = kept, ref = kept_ref;
        p.stage(v, ref, STAGES - 1, false, 2 * qd + 1, "folded");
        for (int i = 0; i < R; i++)
        {
            CHECK(std::fabs(v[i]) < 140737488355328.0, "q=%llu folded exit %.0f not below 2^47", (unsigned long long)q, v[i]);
            const double back = fp_from_s48(fp_s48_of(v[i]) & 0xFFFFFFFFFFFFull);
            CHECK(back == v[i], "q=%llu folded exit does not survive the 48-bit slot", (unsigned long long)q);
            handed[i] = back;
        }
        mac_pass(q, handed, 2 * qd + 1, true);
    }
    // the MAC's lazy row pass at the extremes of the folded exit, both signs
    if (fold)
        for (const auto &in : entries(2 * qd + 1, true)) mac_pass(q, in, 2 * qd + 1, true);
}

static void full_prime(u64 q)
{
    const double qd = (double)q, qinv = 1.0 / qd;
    // the largest unreduced lift: a digit prime q_J <= 2q, residue q_J - 1 <= 2q - 1
    for (const auto &in : entries(2 * qd - 1, false))
    {
        Pass p(q);
        std::vector<double> v = in;
        std::vector<u64> ref = canon_of(v, q);
        for (int s = 0; s < STAGES; s++) p.stage(v, ref, s, false, 2 * qd + 1, "full");
        for (int i = 0; i < R; i++) CHECK(fp_canon(v[i], qd, qinv) == ref[i], "q=%llu canonical exit", (unsigned long long)q);
        // handed to the fused MAC as doubles: its non-lazy row pass takes them as they are
        mac_pass(q, v, 2 * qd + 1, false);
    }
    for (const auto &in : entries(2 * qd + 1, true)) mac_pass(q, in, 2 * qd + 1, false);
}

int main()
{
    const int bits[] = { 46, 47, 48, 51 };
    for (int b : bits)
    {
        const u64 q = prime_below(b);
        const int before = failures;
        if (b <= 47)
            lazy_prime(q);
        else
            full_prime(q);
        // a prime below 2^47 also runs non-lazy (the MAC when its sums would not stay exact)
        if (b <= 47) full_prime(q);
        std::printf("q = %llu (below 2^%d): %s\n", (unsigned long long)q, b, failures == before ? "ok" : "FAILED");
    }
    return failures ? 1 : 0;
}
