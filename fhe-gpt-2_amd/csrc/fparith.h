// FP64-FMA modular arithmetic for primes q < 2^51 (gfx950).
//
// gfx950 has no 64x64 integer multiplier: a Shoup product costs 9-10 v_mad_u64_u32 plus
// 64-bit carries, ~35 VALU instructions per Harvey butterfly.  The FP64 pipe runs v_fma_f64 at
// the same rate as v_mad_u64_u32, and for q < 2^51 a residue and a 102-bit product are exact
// in doubles:
//     h = y*w (rounded), l = fma(y, w, -h)      -> y*w = h + l exactly
//     k = rint(y * w')  with w' = w/q           -> quotient estimate, |y*w/q - k| <= 1
//     r = fma(-k, q, h) + l                     -> r = y*w - k*q exactly, |r| <= 1.5q
// so a butterfly is ~11 full-rate FP64 operations.  Values are kept as doubles in the signed
// range |v| <= 2q between stages; the first load converts canonical/lazy u64 residues, the last
// store canonicalises.  Every output that leaves a transform is canonical, so results are the
// same residues SEAL's integer Harvey butterflies produce.
//
// Bounds (q < 2^51, |inputs| <= B = 2q < 2^52):
//   rint(y*w') errs by at most 2*B*2^-53 + 1/2 <= 1, so |r| <= 1.5q; |h - k*q| <= 1.5q + ulp(h)/2
//   <= 1.5q + 2^50 < 2^53, so the fma result is exact; a centered reduction x - rint(x/q)*q of
//   |x| <= 2^53 is within [-q/2 - 1, q/2 + 1].  Forward: x' = red(x) + r, y' = red(x) - r, so
//   |.| <= 2q + 1 is preserved.  Inverse: x' = red(x + y), y' = mulmod(red(x - y), w), |.| <= q.
//   (scripts/ubench_bfly.hip checks 1536 random stages at q ~ 2^51 against the integer path.)
//
// Unreduced lifts (ntt.h k_modup_col; tests/fp_bounds.cpp checks each figure on the host).  The
// ModUp lifts a canonical residue x of the digit's prime, 0 <= x < q_J, to the output prime q
// and runs the 8 stages of the column pass on it:
//   lazy (q < 2^47): x enters as it stands when q_J <= 4q, so |x| < 4q, and reduced (|x| <=
//     q/2 + 1) otherwise.  No stage reduces x, every product is within 1.5q, so after stage s
//     (1..8) |.| <= 4q + 1.5q s, at most 16q <= 2^51 after the 8th: every y that enters
//     fp_mulmod stays within 2^51 (its limit, below), and every sum is an exact integer below
//     2^53.  The exit reduces (fp_to_s48, fp_canon: |x| <= 2^52).
//   lazy, q < 2^46, packed exit: the 8th stage reduces x as fwd_bfly_f does (its x and y are
//     within 4q + 10.5q = 14.5q), so |x'|, |y'| <= q/2 + 1 + 1.5q = 2q + 1 <= 2^47 - 1: a
//     signed 48-bit value with no further reduction (fp_s48_of).  The fused MAC's lazy row pass
//     then starts from |x| <= 2q + 1 <= 4q, ends within 14q + 1 < 16q, and its lazy products
//     take |a| <= 2^51 as before.
//   non-lazy (q < 2^51): x enters as it stands when q_J <= 2q, so |x|, |y| < 2q.  The first
//     stage reduces x itself (|x| <= 2^53) and takes |y| <= 2q into fp_mulmod, the bound B of
//     the paragraph above; from there on |.| <= 2q + 1 as for reduced input.
//
// Scheduled reduction of x (ntt.h k_modup_col's non-lazy sweep and k_ks_row_mac's non-lazy row
// stages; tests/fp_sched.cpp checks each figure on the host).  A non-lazy prime (q < 2^51) need not
// reduce x in every stage: a value that is x in one stage and y in the next is reduced by the
// product, and fp_mulmod stays exact well beyond |y| = 2q + 1 (its comment).  Write R for a stage
// that reduces x (fwd_bfly_f) and L for one that does not (the arithmetic of fwd_bfly_f_lazy).  With
// e(b) = 3 b 2^-54 + 1/2, the quotient error of fp_mulmod for |y| <= b, a stage maps a bound b on
// |x|, |y| to
//     R: q/2 + 2 + e(b) q   (the centred reduction of |x| <= 2^53 is within q/2 + 2)
//     L: b + e(b) q
// and fp_sched_reduce (below) makes the stages alternate, L first in the row pass and R last in the
// column pass, so no two L stages follow each other, not across the two passes either.  For q < 2^51:
//   fixed point: b_R = 2.4517q after an R stage, b_L = 3.8710q after an L stage.  Any entry within
//     b_R keeps every later value within these two, for any number of stages and chained passes:
//     every sum is an exact integer below 3.88q < 2^53, every y that enters fp_mulmod is within
//     3.88q (e <= 1.955, |h - kq| + ulp(h)/2 <= 1.955q + 2^51 < 2^53: the fma is exact), and every x
//     that is reduced is within 2^53.  An L stage needs its inputs within b_R; an R stage takes b_L.
//   column pass of 8 or 6 stages, L R L R ...: from an unreduced lift (|x|, |y| < 2q, or the 2q + 1
//     of the paragraph above) the bounds are 3.25q, 2.22q, 3.56q, 2.34q, 3.71q, 2.39q, 3.79q, 2.42q;
//     from a reduced lift (<= q/2 + 1) 1.19q, 1.45q, 2.49q, 1.94q, 3.16q, 2.19q, 3.51q, 2.32q.
//   column pass of 7 stages, R L R L R L R: from either lift at most 1.75q, 2.91q, 2.09q, 3.38q,
//     2.27q, 3.62q, 2.36q.
//   The column pass leaves |w| <= 2.46q in a slot of doubles (its packed exit, fp_to_s48, reduces
//     |x| <= 2^53 as before); the row pass enters with that, or with a canonical or centred residue,
//     runs L R L R ... and ends within 2.46q (8 or 6 stages) or 3.88q (7 stages).  The fused MAC
//     reduces the digit first (fp_reduce of |x| <= 2^53: within q/2 + 2 <= 2^51, fp_mulmod_gen's
//     condition; its products stay within 1.25q).
//   Primes below 2^50 and 2^48 sit lower: b_L = 2.18q and 1.63q.
// Every output is canonicalised or reduced into its slot as before: the words that leave are the same.
#pragma once
#include <stdint.h>
#ifdef MHE_FPARITH_HOST
// Host build of the same functions (the bound check's stand-alone program): no HIP headers, the
// bit casts through memcpy.
#include <string.h>
#define __device__
#define __forceinline__ inline
struct double2
{
    double x, y;
};
static inline double __longlong_as_double(long long v)
{
    double d;
    memcpy(&d, &v, 8);
    return d;
}
static inline long long __double_as_longlong(double d)
{
    long long v;
    memcpy(&v, &d, 8);
    return v;
}
#else
#include <hip/hip_runtime.h>
#endif

// Twiddle as (w, w/q).
typedef double2 TwF;

__device__ __forceinline__ double fp_rint(double x)
{
    return __builtin_rint(x);
}

// y*w mod q for w in [0, q), ws = fl(w/q); |result| <= 1.5q in both regimes of |y| below.  The
// quotient k = rint(fl(y*ws)) differs from y*w/q by at most |y| 2^-54 (ws < 1 against w/q) +
// |y| 2^-53 (the product's rounding) + 1/2 (rint), and r = y*w - k*q is that many q:
//   non-lazy butterflies, q < 2^51: |y| <= 2q + 1 < 2^52 (the header's B; an unreduced lift is
//     below 2q): at most 0.75 + 0.5 = 1.25;
//   lazy butterflies, q < 2^47: |y| <= 16q <= 2^51: at most 0.375 + 0.5 = 0.875.
// ("Unreduced lifts" in the header says who enters with what.)
__device__ __forceinline__ double fp_mulmod(double y, double w, double ws, double q)
{
    const double h = y * w;
    const double l = __builtin_fma(y, w, -h);
    const double k = fp_rint(y * ws);
    return __builtin_fma(-k, q, h) + l;
}

// a*b mod q in (-1.25q, 1.25q) for a general b in [0, q) (no precomputed b/q) and |a| <= 2^51:
// the quotient estimate rint(fl(a*b) * fl(1/q)) errs by at most 3*2^-53*|ab/q| + 1/2 <= 0.875.
// For |a| <= 2^52 (q < 2^51, a not reduced) it errs by at most 2: |result| <= 2q.
__device__ __forceinline__ double fp_mulmod_gen(double a, double b, double q, double qinv)
{
    const double h = a * b;
    const double l = __builtin_fma(a, b, -h);
    const double k = fp_rint(h * qinv);
    return __builtin_fma(-k, q, h) + l;
}

// centered reduction: x - rint(x/q)*q, |result| <= q/2 + 1 for |x| <= 2^52 and <= q/2 + 2 for
// |x| <= 2^53 (fl(x/q) errs by at most |x/q| 2^-52, which is |x| 2^-52 in the remainder).
__device__ __forceinline__ double fp_reduce(double x, double q, double qinv)
{
    return __builtin_fma(-fp_rint(x * qinv), q, x);
}

// 2^52: a double in [2^52, 2^53) holds the integer d - 2^52 in its 52 mantissa bits
#define FP_TWO52 4503599627370496.0

// canonical [0, q) from |x| <= 2^53, as u64.  The centered residue r is shifted into [2^52, 2^53)
// (r + 2^52, or r + q + 2^52 when negative: exact integers below 2^53), whose mantissa field IS
// the residue -- one add and a mask instead of gfx950's multi-instruction f64 -> u64 conversion.
__device__ __forceinline__ uint64_t fp_canon(double x, double q, double qinv)
{
    const double r = fp_reduce(x, q, qinv); // [-q/2 - 1, q/2 + 1]
    const double d = r + (r < 0 ? q + FP_TWO52 : FP_TWO52);
    return (uint64_t)__double_as_longlong(d) & 0x000FFFFFFFFFFFFFull;
}

// exact double of a u64 < 2^53
__device__ __forceinline__ double fp_from_u64(uint64_t x)
{
    return (double)x;
}

// exact double of a u64 < 2^52 (every canonical residue of a prime below 2^51): the exponent of
// 2^52 OR-ed over x gives 2^52 + x, one subtraction leaves x -- instead of two u32 conversions,
// an ldexp and an add
__device__ __forceinline__ double fp_from_u52(uint64_t x)
{
    return __longlong_as_double((long long)(x | 0x4330000000000000ull)) - FP_TWO52;
}

// The packed ModUp intermediate of the FP path (ntt.h tile16, primes q < 2^48) holds the centred
// residue r = x - rint(x/q) q, |r| <= q/2 + 1 < 2^47, as 48-bit two's complement: r + 1.5 2^52 is a
// double in [2^52, 2^53) whose mantissa is r + 2^51, and its low 48 bits are r mod 2^48 -- one add
// instead of fp_canon's select and add.  Only the low 48 bits of the returned word are meaningful.
__device__ __forceinline__ uint64_t fp_to_s48(double x, double q, double qinv)
{
    const double r = fp_reduce(x, q, qinv);
    return (uint64_t)__double_as_longlong(r + 6755399441055744.0); // 1.5 * 2^52
}

// The same packing of a value already within the slot: |x| < 2^47, an integer (k_modup_col's folded
// exit, "Unreduced lifts" above).
__device__ __forceinline__ uint64_t fp_s48_of(double x)
{
    return (uint64_t)__double_as_longlong(x + 6755399441055744.0); // 1.5 * 2^52
}

// ... and back: flipping bit 47 of r mod 2^48 gives r + 2^47 in [0, 2^48); OR-ed under the exponent
// of 2^52 (one XOR with both) and less 2^52 + 2^47, that is r exactly.
__device__ __forceinline__ double fp_from_s48(uint64_t v48)
{
    return __longlong_as_double((long long)(v48 ^ 0x4330800000000000ull)) - 4644337115725824.0; // 2^52 + 2^47
}

// Forward Cooley-Tukey butterfly (the mathematics of dwthandler.h:122-125).
__device__ __forceinline__ void fwd_bfly_f(double &x, double &y, const TwF w, double q, double qinv)
{
    const double r = fp_mulmod(y, w.x, w.y, q);
    const double u = fp_reduce(x, q, qinv);
    x = u + r;
    y = u - r;
}

// Forward butterfly without reducing x, for q < 2^47: within one pass (<= 8 stages) |x| grows
// from <= 4q by <= 1.5q per stage to <= 16q <= 2^51, which keeps every product's quotient
// estimate within 1 (|y| <= 2^51) -- so the centered reduction of x can be skipped.  What enters
// at up to 4q: an unreduced lift of a digit prime q_J <= 4q (k_modup_col), and that kernel's
// folded exit (<= 2q + 1) read back by the fused MAC ("Unreduced lifts" in the header).
__device__ __forceinline__ void fwd_bfly_f_lazy(double &x, double &y, const TwF w, double q)
{
    const double r = fp_mulmod(y, w.x, w.y, q);
    const double u = x;
    x = u + r;
    y = u - r;
}

// Inverse Gentleman-Sande butterfly (dwthandler.h:230-233).  |x|,|y| <= 2q + 1: the
// difference is reduced first so the product's quotient estimate stays within 1.
__device__ __forceinline__ void inv_bfly_f(double &x, double &y, const TwF w, double q, double qinv)
{
    const double s = x + y, d = x - y;
    x = fp_reduce(s, q, qinv);
    y = fp_mulmod(fp_reduce(d, q, qinv), w.x, w.y, q);
}

// Last inverse stage with n^-1 merged (dwthandler.h:273-314): x' = (u+v) n^-1, y' = (u-v) w_last.
__device__ __forceinline__ void inv_bfly_last_f(double &x, double &y, double ninv, double ninv_s, double lw,
                                                double lws, double q, double qinv)
{
    const double s = x + y, d = x - y;
    x = fp_mulmod(fp_reduce(s, q, qinv), ninv, ninv_s, q);
    y = fp_mulmod(fp_reduce(d, q, qinv), lw, lws, q);
}

// The schedule of the non-lazy primes' x reduction ("Scheduled reduction of x" in the header): does
// stage a reduce x?  a counts from the boundary between the two passes of a transform: stage s of a
// column pass of NS stages is a = s - NS (-NS .. -1), stage s of the row pass is a = s.  Odd stages
// reduce, so the column pass always ends on a reduction and the row pass starts without one.
constexpr bool fp_sched_reduce(int a)
{
    return (a & 1) != 0;
}

// One forward stage over the E values of a lane (pairs (e, e+gap), gap bit clear); LAZY (only
// for q < 2^47) drops the reduction of x.  REDX = false: a non-lazy prime's stage that the schedule
// above leaves without the reduction of x -- the arithmetic of the lazy butterfly under the
// schedule's bounds, not the lazy primes'.
template <int E, bool LAZY, bool REDX = true, class TwOf>
__device__ __forceinline__ void fwd_stage_f(double (&v)[E], int gap, TwOf tw_of, double q, double qinv)
{
#pragma unroll
    for (int e = 0; e < E; e++)
        if (!(e & gap))
        {
            if constexpr (LAZY || !REDX)
                fwd_bfly_f_lazy(v[e], v[e + gap], *tw_of(e), q);
            else
                fwd_bfly_f(v[e], v[e + gap], *tw_of(e), q, qinv);
        }
}

// fwd_stage_f over two value vectors that take the same twiddles (two batch entries of one tile,
// ntt.h k_ks_row_mac NE = 2): each twiddle is read once, into a local, and applied to both.
template <int E, bool LAZY, bool REDX = true, class TwOf>
__device__ __forceinline__ void fwd_stage_f2(double (&v0)[E], double (&v1)[E], int gap, TwOf tw_of, double q, double qinv)
{
#pragma unroll
    for (int e = 0; e < E; e++)
        if (!(e & gap))
        {
            const TwF w = *tw_of(e);
            if constexpr (LAZY || !REDX)
            {
                fwd_bfly_f_lazy(v0[e], v0[e + gap], w, q);
                fwd_bfly_f_lazy(v1[e], v1[e + gap], w, q);
            }
            else
            {
                fwd_bfly_f(v0[e], v0[e + gap], w, q, qinv);
                fwd_bfly_f(v1[e], v1[e + gap], w, q, qinv);
            }
        }
}

template <int E, class TwOf>
__device__ __forceinline__ void inv_stage_f(double (&v)[E], int gap, TwOf tw_of, double q, double qinv)
{
#pragma unroll
    for (int e = 0; e < E; e++)
        if (!(e & gap)) inv_bfly_f(v[e], v[e + gap], *tw_of(e), q, qinv);
}
