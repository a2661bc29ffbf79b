// Host check of the scheduled reduction of x in the non-lazy FP64 forward stages (csrc/fparith.h,
// "Scheduled reduction of x"; csrc/ntt.h k_modup_col's non-lazy sweep and k_ks_row_mac's row stages).
//   (a) the header's bounds, propagated in exact integer arithmetic through both kernels' stage
//       sequences and through 64 chained passes: below 2^53 and equal to the header's figures;
//   (b) chains of eight (seven) stages through fparith.h's own fwd_stage_f with the schedule's flag,
//       values pinned to each stage's bound, 0, +-1 and random, twiddles 1, q - 1 and random: every
//       fma(-k, q, h) exact (__int128), every output congruent to the integer butterfly's and within
//       the stage's bound;
//   (c) the fused MAC's digit reduction and fp_mulmod_gen at the row pass's exit bound, and the
//       column pass's exits (fp_to_s48, fp_canon) at theirs.
// The arithmetic is fparith.h's own (MHE_FPARITH_HOST); build with -ffp-contract=off.
// Stand-alone: exit status 0 and a line per prime when everything holds, 1 with the first failures.
#define MHE_FPARITH_HOST
#include "../fhe-gpt-2_amd/csrc/fparith.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

typedef unsigned __int128 u128;
typedef __int128 i128;
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

static u64 residue(i128 v, u64 q)
{
    i128 r = v % (i128)q;
    return (u64)(r < 0 ? r + (i128)q : r);
}

constexpr u64 TWO53 = (u64)1 << 53;

// ---- (a) the header's error model, in integers (every value is one, so floors are bounds)
// |fp_mulmod(y, .)| for |y| <= b: (3 b 2^-54 + 1/2) q
static u64 product_bound(u64 b, u64 q) { return (u64)(((u128)6 * b * q + ((u128)q << 54)) >> 55); }
// |fp_reduce(x)| for |x| <= 2^53: q/2 + 2
static u64 reduce_bound(u64 q) { return (q - 1) / 2 + 2; }
// the bound after a stage that reduces x (R) or not (L), from a bound b on both inputs
static u64 stage_bound(u64 b, u64 q, bool redx) { return (redx ? reduce_bound(q) : b) + product_bound(b, q); }

// A pass of NS stages whose first stage is a = A0 in fp_sched_reduce's numbering: the column pass
// (A0 = -NS) or the row pass (A0 = 0).
struct Bounds
{
    u64 after[8];
};
static Bounds propagate(u64 entry, u64 q, int a0, int ns)
{
    Bounds B{};
    u64 b = entry;
    for (int s = 0; s < ns; s++)
    {
        const bool redx = fp_sched_reduce(a0 + s);
        // what the stage must be given: exact sums and products, an exact fma in fp_mulmod
        CHECK(b < TWO53, "q=%llu stage %d entry bound %llu", (unsigned long long)q, s, (unsigned long long)b);
        // |h - kq| + ulp(h)/2 <= |r| + 2 (ulp(h)/2), h = y w < b q
        const u128 h = (u128)b * q;
        int e = 0;
        while (((u128)1 << (e + 1)) <= h) e++; // 2^e <= h
        const u64 ulp = e >= 52 ? (u64)1 << (e - 52) : 1;
        CHECK(product_bound(b, q) + ulp < TWO53, "q=%llu stage %d: fma not exact at |y| = %llu", (unsigned long long)q, s,
              (unsigned long long)b);
        b = stage_bound(b, q, redx);
        CHECK(b < TWO53, "q=%llu stage %d bound %llu", (unsigned long long)q, s, (unsigned long long)b);
        B.after[s] = b;
    }
    return B;
}

// figure (in 1/scale q, rounded up as the header prints it) against a bound
static bool is_figure(u64 b, u64 q, u64 fig, u64 scale)
{
    return (u128)b * scale <= (u128)fig * q && (u128)b * scale > (u128)(fig - 1) * q;
}
static bool within_figure(u64 b, u64 q, u64 fig, u64 scale) { return (u128)b * scale <= (u128)fig * q; }

// the header's figures for q < 2^51, in q/100
static const u64 COL8_UNRED[8] = { 325, 222, 356, 234, 371, 239, 379, 242 };
static const u64 COL8_RED[8] = { 119, 145, 249, 194, 316, 219, 351, 232 };
static const u64 COL7[7] = { 175, 291, 209, 338, 227, 362, 236 };
// the fixed point, in q/10000, and b_L of the smaller primes in q/100
constexpr u64 FIX_R = 24517, FIX_L = 38710;

// returns the fixed point's b_R
static u64 check_bounds(u64 q, int bits)
{
    const bool top = bits == 51; // the figures are those of the largest prime; smaller ones sit below
    auto fig = [&](u64 b, u64 f, const char *what, int s) {
        CHECK(top ? is_figure(b, q, f, 100) : within_figure(b, q, f, 100), "q=%llu %s stage %d: bound %.4f q, header %.2f q",
              (unsigned long long)q, what, s, (double)b / (double)q, (double)f / 100);
    };
    const Bounds cu = propagate(2 * q + 1, q, -8, 8), cr = propagate((q - 1) / 2 + 1, q, -8, 8);
    const Bounds c7 = propagate(2 * q, q, -7, 7), c6 = propagate(2 * q + 1, q, -6, 6);
    for (int s = 0; s < 8; s++) fig(cu.after[s], COL8_UNRED[s], "column, unreduced lift", s);
    for (int s = 0; s < 8; s++) fig(cr.after[s], COL8_RED[s], "column, reduced lift", s);
    for (int s = 0; s < 7; s++) fig(c7.after[s], COL7[s], "column of 7", s);
    for (int s = 0; s < 6; s++) CHECK(c6.after[s] == cu.after[s], "column of 6 differs from the first 6 of 8");
    // the fixed point of L R L R ...: the integer recurrences are monotone and contract, so they stop
    u64 b_r = reduce_bound(q), b_l = 0;
    for (int it = 0; it < 4096; it++)
    {
        const u64 l = stage_bound(b_r, q, false), r = stage_bound(l, q, true);
        if (l == b_l && r == b_r) break;
        b_l = l, b_r = r;
    }
    CHECK(stage_bound(b_r, q, false) == b_l && stage_bound(b_l, q, true) == b_r, "q=%llu: no fixed point", (unsigned long long)q);
    CHECK(b_l < TWO53, "q=%llu b_L", (unsigned long long)q);
    CHECK(top ? is_figure(b_r, q, FIX_R, 10000) : within_figure(b_r, q, FIX_R, 10000), "q=%llu b_R = %.5f q", (unsigned long long)q,
          (double)b_r / (double)q);
    CHECK(top ? is_figure(b_l, q, FIX_L, 10000) : within_figure(b_l, q, FIX_L, 10000), "q=%llu b_L = %.5f q", (unsigned long long)q,
          (double)b_l / (double)q);
    if (bits == 50) CHECK(is_figure(b_l, q, 218, 100), "b_L below 2^50: %.4f q", (double)b_l / (double)q);
    if (bits == 48) CHECK(is_figure(b_l, q, 163, 100), "b_L below 2^48: %.4f q", (double)b_l / (double)q);
    // 64 chained passes with no reduction between them, of 8 stages each and of 7 stages each (the
    // column pass of 7 ends on R, the row pass of 7 on L, and what reads it reduces first): every bound
    // within the largest prime's fixed point
    for (int ns = 7; ns <= 8; ns++)
    {
        u64 b = 2 * q + 1;
        for (int pass = 0; pass < 64; pass++)
        {
            const int a0 = pass & 1 ? 0 : -ns;
            const Bounds p = propagate(b, q, a0, ns);
            for (int s = 0; s < ns; s++)
                CHECK(within_figure(p.after[s], q, fp_sched_reduce(a0 + s) ? FIX_R : FIX_L, 10000),
                      "q=%llu chained passes of %d, pass %d stage %d: %.4f q", (unsigned long long)q, ns, pass, s,
                      (double)p.after[s] / (double)q);
            b = p.after[ns - 1];
            if (ns == 7 && (pass & 1)) b = reduce_bound(q);
        }
    }
    return b_r;
}

// ---- (b) the arithmetic itself.  fp_mulmod and fp_reduce taken apart, every step against __int128.
struct Prime
{
    u64 q;
    double qd, qinv;
};
static bool exact(double d, i128 want) { return d == std::rint(d) && std::fabs(d) < 1.7e38 && (i128)d == want; }

static double mulmod_checked(const Prime &P, double y, u64 w, const char *what)
{
    const double wd = (double)w, ws = wd / P.qd;
    const double h = y * wd;
    const double l = __builtin_fma(y, wd, -h);
    const double k = fp_rint(y * ws);
    const double f = __builtin_fma(-k, P.qd, h);
    const i128 Y = (i128)y, H = (i128)h, K = (i128)k;
    CHECK(exact(l, Y * (i128)w - H), "%s q=%llu: h + l is not the product", what, (unsigned long long)P.q);
    CHECK(exact(f, H - K * (i128)P.q), "%s q=%llu: fma(-k, q, h) not exact, y = %.0f w = %llu", what, (unsigned long long)P.q, y,
          (unsigned long long)w);
    const double r = f + l;
    CHECK(exact(r, Y * (i128)w - K * (i128)P.q), "%s q=%llu: r is not y w - k q", what, (unsigned long long)P.q);
    CHECK(r == fp_mulmod(y, wd, ws, P.qd), "%s: not fp_mulmod's value", what);
    CHECK((u64)std::fabs(r) <= product_bound((u64)std::fabs(y), P.q), "%s q=%llu: |r| = %.0f above the model's bound for |y| = %.0f",
          what, (unsigned long long)P.q, std::fabs(r), std::fabs(y));
    return r;
}
static double reduce_checked(const Prime &P, double x, const char *what)
{
    const double k = fp_rint(x * P.qinv);
    const double r = __builtin_fma(-k, P.qd, x);
    CHECK(exact(r, (i128)x - (i128)k * (i128)P.q), "%s q=%llu: reduction's fma not exact, x = %.0f", what, (unsigned long long)P.q, x);
    CHECK(r == fp_reduce(x, P.qd, P.qinv), "%s: not fp_reduce's value", what);
    CHECK((u64)std::fabs(r) <= reduce_bound(P.q), "%s q=%llu: |red| = %.0f", what, (unsigned long long)P.q, std::fabs(r));
    return r;
}

static u64 pick_twiddle(u64 q)
{
    switch (rnd() % 8)
    {
    case 0: return 1;
    case 1: return q - 1;
    case 2: return q - 2;
    default: return rnd() % q;
    }
}
// a value of magnitude at most b: +-b, 0, +-1, near b, random
static double pick_value(u64 b)
{
    const u64 r = rnd();
    const double sgn = (r & 1) ? -1.0 : 1.0;
    switch ((r >> 1) % 8)
    {
    case 0:
    case 1: return sgn * (double)b;
    case 2: return 0.0;
    case 3: return sgn;
    case 4: return sgn * (double)(b - (r >> 8) % 1024);
    default: return sgn * (double)((r >> 8) % (b + 1));
    }
}

// One chain: a pair through the NS stages of a pass whose first stage is a = A0.  Stage S goes through
// fparith.h's fwd_stage_f with the schedule's flag as a template argument, as the kernels instantiate
// it; the same butterfly is taken apart beside it.  Between stages either value may be replaced by
// one pinned to the stage's bound (the partner a real transform could bring).
template <int A0, int NS, int S>
static void chain_stage(const Prime &P, const Bounds &B, u64 entry, double x, double y, const char *what)
{
    if constexpr (S < NS)
    {
        constexpr bool REDX = fp_sched_reduce(A0 + S);
        const u64 bin = S == 0 ? entry : B.after[S - 1];
        const u64 w = pick_twiddle(P.q);
        const u64 xr = residue((i128)x, P.q), yr = residue((i128)y, P.q);
        const double r = mulmod_checked(P, y, w, what);
        const double u = REDX ? reduce_checked(P, x, what) : x;
        double v[2] = { x, y };
        const TwF tw = { (double)w, (double)w / P.qd };
        fwd_stage_f<2, false, REDX>(v, 1, [&](int) { return &tw; }, P.qd, P.qinv);
        CHECK(v[0] == u + r && v[1] == u - r, "%s stage %d: fwd_stage_f differs from the butterfly taken apart", what, S);
        const u64 t = mulmod(yr, w, P.q);
        for (int i = 0; i < 2; i++)
        {
            CHECK(exact(v[i], (i128)u + (i ? -(i128)r : (i128)r)), "%s q=%llu stage %d: sum not exact", what, (unsigned long long)P.q, S);
            CHECK((u64)std::fabs(v[i]) <= B.after[S], "%s q=%llu stage %d: |v| = %.0f above %llu (inputs within %llu)", what,
                  (unsigned long long)P.q, S, std::fabs(v[i]), (unsigned long long)B.after[S], (unsigned long long)bin);
            CHECK(residue((i128)v[i], P.q) == (i ? (xr + P.q - t) % P.q : (xr + t) % P.q), "%s q=%llu stage %d: residue", what,
                  (unsigned long long)P.q, S);
        }
        double nx = v[0], ny = v[1];
        const u64 c = rnd() % 8;
        if (c == 0) nx = pick_value(B.after[S]);
        if (c == 1) ny = pick_value(B.after[S]);
        if (c == 2) nx = v[1], ny = v[0];
        if (c == 3) nx = pick_value(B.after[S]), ny = pick_value(B.after[S]);
        chain_stage<A0, NS, S + 1>(P, B, entry, nx, ny, what);
    }
}

constexpr int CHAINS = 25000; // per pass shape: 4 x 25000 = 10^5 chains of eight stages, and the two of seven

// ---- (c) the readers of the two passes' outputs
static void check_exits(const Prime &P, u64 b_col, u64 b_row)
{
    for (int i = 0; i < 20000; i++)
    {
        // the fused MAC: the row pass's output, reduced, times a key residue
        const double d = pick_value(b_row);
        const double dv = reduce_checked(P, d, "mac digit");
        CHECK(std::fabs(dv) <= 2251799813685248.0, "mac digit above 2^51");
        u64 k = pick_twiddle(P.q);
        if (i % 7 == 0) k = 0;
        const double kd = (double)k;
        const double h = dv * kd, l = __builtin_fma(dv, kd, -h), kk = fp_rint(h * P.qinv), f = __builtin_fma(-kk, P.qd, h);
        CHECK(exact(f, (i128)h - (i128)kk * (i128)P.q), "q=%llu fp_mulmod_gen: fma not exact", (unsigned long long)P.q);
        const double r = f + l;
        CHECK(r == fp_mulmod_gen(dv, kd, P.qd, P.qinv), "not fp_mulmod_gen's value");
        CHECK(exact(r, (i128)dv * (i128)k - (i128)kk * (i128)P.q), "q=%llu fp_mulmod_gen: not a k - kk q", (unsigned long long)P.q);
        CHECK(std::fabs(r) <= 1.25 * P.qd, "q=%llu key product %.0f above 1.25 q", (unsigned long long)P.q, std::fabs(r));
        CHECK(residue((i128)r, P.q) == mulmod(residue((i128)d, P.q), k, P.q), "q=%llu key product residue", (unsigned long long)P.q);
        // the column pass's exits: canonical, and (primes below 2^48) the packed 48-bit slot
        const double c = pick_value(b_col);
        CHECK(fp_canon(c, P.qd, P.qinv) == residue((i128)c, P.q), "q=%llu canonical exit", (unsigned long long)P.q);
        if (P.q < ((u64)1 << 48))
        {
            const double back = fp_from_s48(fp_to_s48(c, P.qd, P.qinv) & 0xFFFFFFFFFFFFull);
            CHECK((u64)std::fabs(back) <= reduce_bound(P.q) && residue((i128)back, P.q) == residue((i128)c, P.q),
                  "q=%llu packed exit", (unsigned long long)P.q);
        }
    }
}

int main()
{
    const int bits[] = { 51, 50, 48 };
    for (int bt : bits)
    {
        const u64 q = prime_below(bt);
        const int before = failures;
        const Prime P = { q, (double)q, 1.0 / (double)q };
        const u64 fix_r = check_bounds(q, bt);
        const u64 unred = 2 * q + 1, red = (q - 1) / 2 + 1;
        const Bounds cu = propagate(unred, q, -8, 8), cr = propagate(red, q, -8, 8), c7 = propagate(2 * q, q, -7, 7);
        // what the row pass may be handed: the fixed point's b_R, or (smaller primes, whose fixed point
        // lies below 2q + 1) what the column pass leaves on its way down to it
        u64 b_col = fix_r;
        for (u64 b : { cu.after[7], cu.after[5], cr.after[7], c7.after[6] })
            if (b > b_col) b_col = b;
        CHECK(within_figure(b_col, q, 246, 100), "q=%llu: the column pass leaves %.4f q", (unsigned long long)q, (double)b_col / (double)q);
        const Bounds r8 = propagate(b_col, q, 0, 8), r7 = propagate(b_col, q, 0, 7);
        u64 b_row = 0;
        for (int s = 0; s < 8; s++)
        {
            CHECK(within_figure(r8.after[s], q, s & 1 ? 246 : 388, 100), "q=%llu row pass of 8, stage %d", (unsigned long long)q, s);
            if (s < 7) CHECK(within_figure(r7.after[s], q, s & 1 ? 246 : 388, 100), "q=%llu row pass of 7, stage %d", (unsigned long long)q, s);
            if (r8.after[s] > b_row) b_row = r8.after[s];
        }
        CHECK(b_row < TWO53, "q=%llu: the row pass leaves %llu", (unsigned long long)q, (unsigned long long)b_row);
        for (int i = 0; i < CHAINS; i++)
        {
            chain_stage<-8, 8, 0>(P, cu, unred, pick_value(unred), pick_value(unred), "column, unreduced lift");
            chain_stage<-8, 8, 0>(P, cr, red, pick_value(red), pick_value(red), "column, reduced lift");
            chain_stage<0, 8, 0>(P, r8, b_col, pick_value(b_col), pick_value(b_col), "row");
            chain_stage<0, 8, 0>(P, r8, b_col, pick_value(cu.after[7]), pick_value(cu.after[7]), "row behind the column pass");
            chain_stage<-7, 7, 0>(P, c7, 2 * q, pick_value(2 * q), pick_value(2 * q), "column of 7");
            chain_stage<0, 7, 0>(P, r7, b_col, pick_value(b_col), pick_value(b_col), "row of 7");
        }
        check_exits(P, b_col, b_row);
        std::printf("q = %llu (below 2^%d): %s\n", (unsigned long long)q, bt, failures == before ? "ok" : "FAILED");
    }
    return failures ? 1 : 0;
}
