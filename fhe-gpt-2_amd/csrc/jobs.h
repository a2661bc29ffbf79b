// Job descriptors of the NTT passes (ntt.h): a job maps the launch's job index y to a view -- the
// source and destination of one limb, its prime and twiddles, and the load / store that fuse the
// step's arithmetic (lifts, epilogues) into the transform.  Kernel arguments, filled on the host by
// the pipelines of keyswitch.h, rotate.h and prodsum.h.
#pragma once

// A batch of jobs of one kind: entry e owns job indices [e * per, (e + 1) * per) of the launch and
// its own buffers (pointers inside j[e]); the shared geometry (level, primes) is the same for all.
template <class Job>
struct JobB
{
    Job j[MHE_MAXB];
    int per; // jobs per entry
    explicit JobB(int per_) : per(per_) {}
    __device__ auto view(int y) const
    {
        const int e = y / per;
        return j[e].view(y - e * per);
    }
};
// The ModDown lift (evaluator.cpp:2466-2524) of the special limb to prime p = q_i, with its constants.
struct ModDownLift
{
    PrimeDev P;
    u64 half, fix;
    bool reduce;
    __device__ u64 lift(u64 s, const PrimeDev &p) const // s in [0, 2P) -> [0, 2p)
    {
        u64 t = barrett64(s + half, P);
        if (reduce) t = barrett64(t, p);
        return t + fix;
    }
    // the integer lift() stands for, from s canonical mod P: s - P when s > P/2, else s
    __device__ double lift_c(u64 s) const { return fp_from_u52(s) - (s > half ? (double)P.q : 0.0); }
};
__device__ __forceinline__ ModDownLift moddown_lift(const PrimeDev *primes, int i, int K)
{
    const PrimeDev p = prime_at(primes, i), P = prime_at(primes, K - 1);
    return ModDownLift{ P, P.q >> 1, p.q - barrett64(P.q >> 1, p), P.q > p.q };
}

// The rescale lift (util/rns.cpp:737-808) of the last limb (prime q_last = q_{L-1}) to prime p = q_i.
struct RescaleLift
{
    u64 ql, half, neg_half;
    bool reduce;
    // lift(s) = finish(shift(s)): s canonical mod q_last -> [0, 2p)
    __device__ u64 shift(u64 s) const { return csub(s + half, ql); }
    __device__ u64 finish(u64 v, const PrimeDev &p) const
    {
        if (reduce) v = barrett64(v, p);
        return v + neg_half;
    }
    __device__ u64 lift(u64 s, const PrimeDev &p) const { return finish(shift(s), p); }
    // the integer lift() stands for: s - q_last when s > q_last/2, else s
    __device__ double lift_c(u64 s) const { return fp_from_u52(s) - (s > half ? (double)ql : 0.0); }
};
__device__ __forceinline__ RescaleLift rescale_lift(const PrimeDev *primes, int i, int L)
{
    const PrimeDev p = prime_at(primes, i);
    const u64 ql = prime_at(primes, L - 1).q;
    return RescaleLift{ ql, ql >> 1, p.q - barrett64(ql >> 1, p), p.q < ql };
}

// The view of a column pass that lifts one source limb to prime p and starts its NTT (ntt.h: k_fwd_col
// loads through lift(), k_icol_lift calls lift() or lift_c() on its own inverse pass's output).
template <class Lift>
struct LiftColView
{
    const u64 *src;
    u64 *dst;
    PrimeDev p;
    Lift lf;
    const Tw *tw;
    bool skip;
    __device__ u64 lift(u64 s) const { return lf.lift(s, p); }
    __device__ double lift_c(u64 s) const { return lf.lift_c(s); }
    __device__ u64 load(u32 x) const { return lift(src[x]); }
    __device__ void store(u32 x, u64 v) const { dst[x] = v; }
};

// The FP64 constants of a prime (fparith.h): q and 1/q.
struct PrimeF
{
    double pd, pi;
};
__device__ __forceinline__ PrimeF prime_f(const PrimeDev &p)
{
    const double pd = (double)p.q;
    return PrimeF{ pd, 1.0 / pd };
}

// Plain transform over [poly][limb][n] with limb l on prime l (optionally src != dst).
struct JobPlain
{
    const u64 *src;
    u64 *dst;
    const PrimeDev *primes;
    const Tw *tw;
    int limbs;
    int log_n;
    int mode; // forward row store: 0 = lazy [0,4q), 1 = full; inverse col store: 0 lazy [0,2q), 1 full
    struct View
    {
        const u64 *src;
        u64 *dst;
        PrimeDev p;
        const Tw *tw;
        int mode;
        bool skip;
        __device__ u64 load(u32 x) const { return src[x]; }
        __device__ void store_fwd(u32 x, u64 v) const
        {
            if (mode) v = csub(csub(v, p.two_q), p.q);
            dst[x] = v;
        }
    };
    __device__ View view(int y) const
    {
        const int l = y % limbs;
        const size_t off = (size_t)y << log_n;
        return View{ src + off, dst + off, primes[l], tw + ((size_t)l << log_n), mode, false };
    }
};

// Views must expose store(); wrappers pick the forward / inverse reduction.
struct JobFwdPlain : JobPlain
{
    struct V2 : View
    {
        __device__ void store(u32 x, u64 v) const { store_fwd(x, v); }
    };
    __device__ V2 view(int y) const { return V2{ JobPlain::view(y) }; }
};

// The forward transform of a batch entry that a kernel earlier in the stream may have rejected
// (mhe_ckks_encode_dev): every job returns when *skip_if != 0; null: always runs.
struct JobFwdPlainIf : JobFwdPlain
{
    const u32 *skip_if;
    __device__ V2 view(int y) const
    {
        V2 v = JobFwdPlain::view(y);
        v.skip = skip_if && *skip_if;
        return v;
    }
};

struct JobInvPlain : JobPlain
{
    struct V2 : View
    {
        __device__ void store(u32 x, u64 v) const
        {
            if (mode) v = csub(v, p.q);
            dst[x] = v;
        }
    };
    __device__ V2 view(int y) const { return V2{ JobPlain::view(y) }; }
};

// Key-switching ModUp, column pass (evaluator.cpp:2386-2408): job y = I*L + J lifts digit J
// (canonical mod q_J, from INTT(target)) to prime I and starts its NTT; I == L is the special
// prime.  I == J is skipped: the MAC reads the input NTT form (evaluator.cpp:2380-2384).
struct JobModUpCol
{
    const u64 *coeff; // [L][n]
    u64 *modup;       // [chunk][L][n] for output primes I0 .. I0+chunk-1
    const PrimeDev *primes;
    const Tw *tw;
    int L, K, log_n, I0;
    int f64 = 0; // limbs of primes below 2^51 leave as doubles (ntt.h MHE_INTER_F64: the fused FP64 MAC reads them)
    struct View
    {
        const u64 *src;
        u64 *dst;
        PrimeDev p;
        const Tw *tw;
        bool reduce;
        bool skip;
        bool f64;
        __device__ u64 load(u32 x) const
        {
            u64 v = src[x];
            return reduce ? barrett64(v, p) : v;
        }
        __device__ void store(u32 x, u64 v) const { dst[x] = f64 ? (u64)__double_as_longlong(fp_from_u52(v)) : v; }
    };
    __device__ View view(int y) const
    {
        const int I = I0 + y / L, J = y % L;
        const int pi = (I == L) ? K - 1 : I;
        View v;
        v.src = coeff + ((size_t)J << log_n);
        v.dst = modup + ((size_t)y << log_n);
        v.p = prime_at(primes, pi);
        v.tw = tw + ((size_t)pi << log_n);
        v.reduce = prime_at(primes, J).q > v.p.q; // key_modulus[J] <= key_modulus[key_index] -> copy
        v.skip = (I == J);
        v.f64 = f64 && v.p.q < (1ull << 51);
        return v;
    }
};

struct JobModUpRow
{
    u64 *modup;
    const PrimeDev *primes;
    const Tw *tw;
    int L, K, log_n, I0;
    struct View
    {
        u64 *buf;
        PrimeDev p;
        const Tw *tw;
        bool skip;
        __device__ u64 load(u32 x) const { return buf[x]; }
        // canonical output keeps the 128-bit MAC safe for any digit count (< 2^8 terms)
        __device__ void store(u32 x, u64 v) const { buf[x] = csub(csub(v, p.two_q), p.q); }
    };
    __device__ View view(int y) const
    {
        const int I = I0 + y / L, J = y % L;
        const int pi = (I == L) ? K - 1 : I;
        return View{ modup + ((size_t)y << log_n), prime_at(primes, pi), tw + ((size_t)pi << log_n), I == J };
    }
};

// The hoisted ModUp's row pass (hoist.h): src [I][J][n] column-pass output -> dst the same layout,
// canonical, each 256-slot block stored in bit-reversed order.  BREV (n = 2^16, 256-slot rows): the
// row pass reads its LDS row bit-reversed and stores contiguously; otherwise the store scatters
// inside the block (out of place: at n < 2^16 a block spans rows of several workgroups).
template <bool BREV>
struct JobModUpRowH
{
    const u64 *src;
    u64 *dst;
    const PrimeDev *primes;
    const Tw *tw;
    int L, K, log_n;
    struct View
    {
        const u64 *src;
        u64 *dst;
        PrimeDev p;
        const Tw *tw;
        bool skip;
        static constexpr bool brev = BREV;
        __device__ u64 load(u32 x) const { return src[x]; }
        __device__ void store(u32 x, u64 v) const
        {
            dst[BREV ? x : ((x & ~255u) | brev8(x & 255u))] = csub(csub(v, p.two_q), p.q);
        }
    };
    __device__ View view(int y) const
    {
        const int I = y / L, J = y % L;
        const int pi = (I == L) ? K - 1 : I;
        const size_t off = (size_t)y << log_n;
        return View{ src + off, dst + off, prime_at(primes, pi), tw + ((size_t)pi << log_n), I == J };
    }
};

// Key-switching ModDown (evaluator.cpp:2466-2524).  t_last = INTT_lazy(acc[k][L]) in [0,2P);
// column pass job y = k*L + i computes ((barrett(t_last + P/2) mod q_i) + fix_i) and starts
// the NTT mod q_i; the row pass epilogue does ct[k][i] += (acc[k][i] + 4q_i - t) * P^-1.
struct JobModDownCol
{
    const u64 *acc; // [2][L+1][n]
    u64 *scratch;   // [2][L][n]
    const PrimeDev *primes;
    const Tw *tw;
    int L, K, log_n;
    int fixed_i = -1; // >= 0: one job per poly, all on limb fixed_i
    using View = LiftColView<ModDownLift>;
    __device__ View view(int y) const
    {
        const int k = fixed_i >= 0 ? y : y / L, i = fixed_i >= 0 ? fixed_i : y % L;
        const Tw *twi = tw + ((size_t)i << log_n); // ahead of the lift's loads: the order the kernels keep
        return View{ acc + ((size_t)(k * (L + 1) + L) << log_n), scratch + ((size_t)y << log_n), prime_at(primes, i),
                     moddown_lift(primes, i, K), twi, false };
    }
};

struct JobModDownRow
{
    u64 *scratch;
    const u64 *acc;
    u64 *ct; // [2][L][n]
    const PrimeDev *primes;
    const Tw *tw;
    const Tw *invq; // [K][K]
    int L, K, log_n;
    int fixed_i = -1; // >= 0: one job per poly, all on limb fixed_i
    int c1_write = 0; // 1: ct[1] = ModDown(acc[1]) instead of += (apply_galois: ct[1] was 0)
    int fp = 0;       // every prime < 2^51: the epilogue in exact FP64 (fparith.h)
    struct View
    {
        u64 *buf;
        const u64 *accp;
        u64 *ctp;
        PrimeDev p;
        const Tw *tw;
        Tw inv;
        bool skip;
        bool replace;
        bool fp;
        PrimeF f;
        double invd;
        __device__ u64 load(u32 x) const { return buf[x]; }
        struct Pre
        {
            u64 a, c;
        };
        __device__ Pre pre(u32 x) const { return Pre{ accp[x], replace ? 0 : ctp[x] }; }
        __device__ void store(u32 x, u64 t, Pre o) const
        {
            if (fp)
            {
                // acc and t canonical: (acc - t) P^-1 in (-1.25p, 1.25p), plus c < p, one
                // canonicalisation (|.| < 2^53): the residue of the integer form
                const double v = fp_mulmod_gen(fp_from_u52(o.a) - fp_from_u52(t), invd, f.pd, f.pi);
                ctp[x] = fp_canon(replace ? v : v + fp_from_u52(o.c), f.pd, f.pi);
                return;
            }
            u64 v = mul_shoup(o.a + p.four_q - t, inv.x, inv.y, p.q);
            ctp[x] = replace ? v : addmod(v, o.c, p.q); // 0 + v = v: the same word
        }
        __device__ void store(u32 x, u64 t) const { store(x, t, pre(x)); }
    };
    __device__ View view(int y) const
    {
        const int k = fixed_i >= 0 ? y : y / L, i = fixed_i >= 0 ? fixed_i : y % L;
        View v;
        v.buf = scratch + ((size_t)y << log_n);
        v.accp = acc + ((size_t)(k * (L + 1) + i) << log_n);
        v.ctp = ct + ((size_t)(k * L + i) << log_n);
        v.p = prime_at(primes, i);
        v.tw = tw + ((size_t)i << log_n);
        v.inv = tw_at(invq, (size_t)(K - 1) * K + i);
        v.skip = false;
        v.replace = c1_write && k == 1;
        v.fp = fp != 0;
        v.f = prime_f(v.p);
        v.invd = (double)v.inv.x;
        return v;
    }
};

// Rescale (util/rns.cpp:737-808): last[s] = INTT(in[s][L-1]) canonical; column pass job
// y = s*(L-1) + i: ((last + half mod q_last) mod q_i) + (q_i - half mod q_i); row pass
// epilogue out[s][i] = (in[s][i] + 4q_i - t) * q_last^-1 mod q_i.
struct JobRescaleCol
{
    const u64 *last; // [size][n]
    u64 *scratch;    // [size][L-1][n]
    const PrimeDev *primes;
    const Tw *tw;
    int L, log_n;
    using View = LiftColView<RescaleLift>;
    __device__ View view(int y) const
    {
        const int s = y / (L - 1), i = y % (L - 1);
        return View{ last + ((size_t)s << log_n), scratch + ((size_t)y << log_n), prime_at(primes, i),
                     rescale_lift(primes, i, L), tw + ((size_t)i << log_n), false };
    }
};

struct JobRescaleRow
{
    u64 *scratch;
    const u64 *in; // [size][L][n]
    u64 *out;      // [size][L-1][n]
    const PrimeDev *primes;
    const Tw *tw;
    const Tw *invq;
    int L, K, log_n;
    int fp = 0; // every prime < 2^51: the epilogue in exact FP64 (fparith.h)
    struct View
    {
        u64 *buf;
        const u64 *inp;
        u64 *outp;
        PrimeDev p;
        const Tw *tw;
        Tw inv;
        bool skip, fp;
        PrimeF f;
        double invd;
        __device__ u64 load(u32 x) const { return buf[x]; }
        using Pre = u64;
        __device__ Pre pre(u32 x) const { return inp[x]; }
        __device__ void store(u32 x, u64 t, u64 in) const
        {
            if (fp) // in and t canonical: (in - t) q_last^-1 in (-1.25p, 1.25p), canonicalised
                outp[x] = fp_canon(fp_mulmod_gen(fp_from_u52(in) - fp_from_u52(t), invd, f.pd, f.pi), f.pd, f.pi);
            else
                outp[x] = mul_shoup(in + p.four_q - t, inv.x, inv.y, p.q);
        }
        __device__ void store(u32 x, u64 t) const { store(x, t, pre(x)); }
    };
    __device__ View view(int y) const
    {
        const int s = y / (L - 1), i = y % (L - 1);
        View v;
        v.buf = scratch + ((size_t)y << log_n);
        v.inp = in + ((size_t)(s * L + i) << log_n);
        v.outp = out + ((size_t)(s * (L - 1) + i) << log_n);
        v.p = prime_at(primes, i);
        v.tw = tw + ((size_t)i << log_n);
        v.inv = tw_at(invq, (size_t)(L - 1) * K + i);
        v.skip = false;
        v.fp = fp != 0;
        v.f = prime_f(v.p);
        v.invd = (double)v.inv.x;
        return v;
    }
};

// ModDown fused with the following rescale (one HMult = multiply + relinearize + rescale).
// With t_i the ModDown lift of INTT(acc_P) and r_i the rescale lift of last = INTT(ct'_{L-1})
// (ct' = ct after ModDown), SEAL computes
//     out_i = ((c_i + (acc_i + 4q - NTT(t_i)) P^-1) + 4q - NTT(r_i)) q_{L-1}^-1   (mod q_i),
// and NTT is linear mod q_i, so the same residues come from ONE forward NTT per limb:
//     out_i = (c_i + acc_i P^-1 - NTT(t_i P^-1 + r_i)) q_{L-1}^-1.
// Column pass job y = k*(L-1) + i builds u_i = t_i P^-1 + r_i (evaluator.cpp:2466-2524 and
// util/rns.cpp:737-808 lifts), the row pass epilogue forms out_i.
struct JobMDRCol
{
    const u64 *acc;  // [2][L+1][n], limb L = INTT_lazy(acc_P) in [0, 2P)
    const u64 *last; // [2][n] = INTT(ct'[k][L-1]), canonical
    u64 *scratch;    // [2][L-1][n]
    const PrimeDev *primes;
    const Tw *tw;
    const Tw *invq; // [K][K]
    int L, K, log_n;
    int fp = 0; // every prime < 2^51 (NttMode::fp): the lift in exact FP64 (fparith.h)
    struct View
    {
        const u64 *accP, *lastp;
        u64 *dst;
        PrimeDev p, P;
        const Tw *tw;
        Tw pinv;
        u64 halfP, fixP, ql, halfL, neg_halfL;
        bool redP, redL, skip, fp;
        PrimeF f;
        double pinvd;
        __device__ u64 load(u32 x) const
        {
            if (fp)
            {
                // accP in [0, 2P) -> a mod P canonical by two conditional subtractions; t + fixP
                // and the rescale lift r + neg_halfL are exact doubles (< 2^52), the product by
                // P^-1 is in (-2p, 2p), the sum below 2^53: one canonicalisation, the same residue
                const u64 t = csub(csub(accP[x] + halfP, 2 * P.q), P.q);
                const u64 r = csub(lastp[x] + halfL, ql);
                const double u = fp_mulmod_gen(fp_from_u52(t + fixP), pinvd, f.pd, f.pi) + fp_from_u52(r + neg_halfL);
                return fp_canon(u, f.pd, f.pi);
            }
            u64 t = barrett64(accP[x] + halfP, P);
            if (redP) t = barrett64(t, p);
            t += fixP;                                  // ModDown lift, [0, 2q)
            u64 r = csub(lastp[x] + halfL, ql);
            if (redL) r = barrett64(r, p);
            r += neg_halfL;                             // rescale lift, [0, 2q)
            const u64 u = mul_shoup(t, pinv.x, pinv.y, p.q) + r; // [0, 3q)
            return csub(csub(u, p.two_q), p.q);
        }
        __device__ void store(u32 x, u64 v) const { dst[x] = v; }
        // k_col_lift2 (FP): the two lifts' centred integers, the same for every output prime -- the
        // special accumulator limb (in [0, 2P)) and the rescale's last limb (canonical mod q_last)
        __device__ void src_c(u32 x, double &ct, double &cr) const
        {
            const u64 a = csub(accP[x], P.q), l = lastp[x];
            ct = fp_from_u52(a) - (a > halfP ? (double)P.q : 0.0);
            cr = fp_from_u52(l) - (l > halfL ? (double)ql : 0.0);
        }
        // t P^-1 + r mod p from them: |.| < 1.25p + 2^50, congruent to load()'s value
        __device__ double lift_f(double ct, double cr) const { return fp_mulmod_gen(ct, pinvd, f.pd, f.pi) + cr; }
    };
    __device__ View view(int y) const
    {
        const int k = y / (L - 1), i = y % (L - 1);
        View v;
        v.accP = acc + ((size_t)(k * (L + 1) + L) << log_n);
        v.lastp = last + ((size_t)k << log_n);
        v.dst = scratch + ((size_t)y << log_n);
        v.p = prime_at(primes, i);
        v.P = prime_at(primes, K - 1);
        v.tw = tw + ((size_t)i << log_n);
        v.pinv = tw_at(invq, (size_t)(K - 1) * K + i);
        v.halfP = v.P.q >> 1;
        v.fixP = v.p.q - barrett64(v.halfP, v.p);
        v.redP = v.P.q > v.p.q;
        v.ql = prime_at(primes, L - 1).q;
        v.halfL = v.ql >> 1;
        v.neg_halfL = v.p.q - barrett64(v.halfL, v.p);
        v.redL = v.p.q < v.ql;
        v.skip = false;
        v.fp = fp != 0;
        v.f = prime_f(v.p);
        v.pinvd = (double)v.pinv.x;
        return v;
    }
};

struct JobMDRRow
{
    u64 *scratch;
    const u64 *acc; // [2][L+1][n]
    const u64 *ct;  // [2][L][n], limbs < L-1 before ModDown
    u64 *out;       // [2][L-1][n]
    const PrimeDev *primes;
    const Tw *tw;
    const Tw *invq;
    int L, K, log_n;
    int fp = 0; // every prime < 2^51: the epilogue in exact FP64 (fparith.h)
    struct View
    {
        u64 *buf;
        const u64 *accp, *ctp;
        u64 *outp;
        PrimeDev p;
        const Tw *tw;
        Tw pinv, qlinv;
        bool skip, fp;
        PrimeF f;
        double pinvd, qlinvd;
        __device__ u64 load(u32 x) const { return buf[x]; }
        struct Pre
        {
            u64 a, c;
        };
        __device__ Pre pre(u32 x) const { return Pre{ accp[x], ctp[x] }; }
        __device__ void store(u32 x, u64 U, Pre o) const
        {
            if (fp)
            {
                // acc_i P^-1 in (-1.25p, 1.25p); c + a - U is an exact integer below 2^53; its
                // centered residue times q_{L-1}^-1, canonicalised: the residue of the integer form
                const double a = fp_mulmod_gen(fp_from_u52(o.a), pinvd, f.pd, f.pi);
                const double v = fp_reduce(fp_from_u52(o.c) + a - fp_from_u52(U), f.pd, f.pi);
                outp[x] = fp_canon(fp_mulmod_gen(v, qlinvd, f.pd, f.pi), f.pd, f.pi);
                return;
            }
            const u64 a = mul_shoup(o.a, pinv.x, pinv.y, p.q); // acc_i P^-1
            const u64 v = o.c + a + p.four_q - U;              // < 6q
            outp[x] = mul_shoup(v, qlinv.x, qlinv.y, p.q);
        }
        __device__ void store(u32 x, u64 U) const { store(x, U, pre(x)); }
    };
    __device__ View view(int y) const
    {
        const int k = y / (L - 1), i = y % (L - 1);
        View v;
        v.buf = scratch + ((size_t)y << log_n);
        v.accp = acc + ((size_t)(k * (L + 1) + i) << log_n);
        v.ctp = ct + ((size_t)(k * L + i) << log_n);
        v.outp = out + ((size_t)(k * (L - 1) + i) << log_n);
        v.p = prime_at(primes, i);
        v.tw = tw + ((size_t)i << log_n);
        v.pinv = tw_at(invq, (size_t)(K - 1) * K + i);
        v.qlinv = tw_at(invq, (size_t)(L - 1) * K + i);
        v.skip = false;
        v.fp = fp != 0;
        v.f = prime_f(v.p);
        v.pinvd = (double)v.pinv.x;
        v.qlinvd = (double)v.qlinv.x;
        return v;
    }
};

// The column pass of a summed HMult tail (mhe_relin_sum_rescale, prodsum.h): JobMDRCol with the
// ModDown lift already taken and summed.  T[k][i] is the sum over a group's terms of the lifted
// special limbs, canonical mod q_i (never summed mod P), so u_i = T_i P^-1 + r_i with r_i the rescale
// lift of last = INTT(S[k][L-1]) exactly as JobMDRCol::View::load lifts it.  Job y = k*(L-1) + i;
// JobMDRRow forms out_i from u_i, acc = A (the summed key products) and ct = C (the summed products).
struct JobProdSumCol
{
    const u64 *T;    // [2][L][n], coefficient form, canonical mod q_i
    const u64 *last; // [2][n] = INTT(S[k][L-1]), canonical
    u64 *scratch;    // [2][L-1][n]
    const PrimeDev *primes;
    const Tw *tw;
    const Tw *invq; // [K][K]
    int L, K, log_n;
    int fp = 0; // every prime < 2^51 (NttMode::fp): the lift in exact FP64 (fparith.h)
    struct View
    {
        const u64 *Tp, *lastp;
        u64 *dst;
        PrimeDev p;
        RescaleLift rs;
        const Tw *tw;
        Tw pinv;
        bool skip, fp;
        PrimeF f;
        double pinvd;
        __device__ u64 load(u32 x) const
        {
            u64 r = rs.shift(lastp[x]); // above the branch: the order the kernels keep
            if (fp)
            {
                // T canonical and the rescale lift r + neg_half are exact doubles (< 2^52), the
                // product by P^-1 is in (-1.25p, 1.25p), the sum below 2^53: one canonicalisation
                const double u = fp_mulmod_gen(fp_from_u52(Tp[x]), pinvd, f.pd, f.pi) + fp_from_u52(r + rs.neg_half);
                return fp_canon(u, f.pd, f.pi);
            }
            r = rs.finish(r, p);                                     // rescale lift, [0, 2q)
            const u64 u = mul_shoup(Tp[x], pinv.x, pinv.y, p.q) + r; // [0, 3q)
            return csub(csub(u, p.two_q), p.q);
        }
        __device__ void store(u32 x, u64 v) const { dst[x] = v; }
    };
    __device__ View view(int y) const
    {
        const int k = y / (L - 1), i = y % (L - 1);
        View v;
        v.Tp = T + ((size_t)(k * L + i) << log_n);
        v.lastp = last + ((size_t)k << log_n);
        v.dst = scratch + ((size_t)y << log_n);
        v.p = prime_at(primes, i);
        v.tw = tw + ((size_t)i << log_n);
        v.pinv = tw_at(invq, (size_t)(K - 1) * K + i);
        v.rs = rescale_lift(primes, i, L);
        v.skip = false;
        v.fp = fp != 0;
        v.f = prime_f(v.p);
        v.pinvd = (double)v.pinv.x;
        return v;
    }
};

// Rescale INTT of the last limb: src limb (L-1) of poly s -> last[s], canonical.
struct JobLastInv
{
    const u64 *in;
    u64 *last;
    const PrimeDev *primes;
    const Tw *itw;
    int L, log_n;
    int lazy;
    struct View
    {
        const u64 *src;
        u64 *dst;
        PrimeDev p;
        const Tw *tw;
        int lazy;
        bool skip;
        __device__ u64 load(u32 x) const { return src[x]; }
        __device__ void store(u32 x, u64 v) const { dst[x] = lazy ? v : csub(v, p.q); }
    };
    __device__ View view(int y) const
    {
        View v;
        v.src = in + ((size_t)(y * L + (L - 1)) << log_n);
        v.dst = last + ((size_t)y << log_n);
        v.p = prime_at(primes, L - 1);
        v.tw = itw + ((size_t)(L - 1) << log_n);
        v.lazy = lazy;
        v.skip = false;
        return v;
    }
};

// Generic job on explicit (src, dst, prime) with a per-job stride: used for the key-switch
// INTT of the target (limb J on prime J) and of the special accumulator limbs.
struct JobStrided
{
    const u64 *src;
    u64 *dst;
    size_t src_stride, dst_stride; // in words, per job
    int prime0;                    // prime index of job 0
    int prime_step;                // 0: all jobs on prime0; 1: job y on prime0 + y
    const PrimeDev *primes;
    const Tw *tw;
    int log_n;
    int mode; // inverse store: 0 lazy, 1 full
    const int *run_if = nullptr; // non-null: every job returns unless *run_if != 0 (hoist.h fallback)
    struct View
    {
        const u64 *src;
        u64 *dst;
        PrimeDev p;
        const Tw *tw;
        int mode;
        bool skip;
        __device__ u64 load(u32 x) const { return src[x]; }
        __device__ void store(u32 x, u64 v) const { dst[x] = mode ? csub(v, p.q) : v; }
    };
    __device__ View view(int y) const
    {
        const int pi = prime0 + prime_step * y;
        return View{ src + y * src_stride, dst + y * dst_stride, primes[pi], tw + ((size_t)pi << log_n), mode,
                     run_if && !*run_if };
    }
};

// ------------------------------------------------------------------------- batched encryption
// Public-key encryption (encrypt.h; rlwe.cpp:220-286 followed by the rescale of util/rns.cpp:737-808)
// at m = L + 1 limbs, dropped prime q_L.  The samples u, e_0, e_1 are planes of one signed byte per
// coefficient (sample.hip k_enc_*), expanded to residues where a job reads them.  With uh = NTT(u),
//     last_j    = INTT_L(uh_L pk_{j,L}) + e_j                        (mod q_L, canonical)
//     out_{j,i} = (uh_i pk_{j,i} + NTT_i(e_j - r_{j,i})) q_L^-1       (mod q_i), i < L,
// r_{j,i} the rescale lift of last_j; plain_i is added to out_{0,i} when the entry has a plaintext.

// Coefficient x of a byte plane: the dword that holds it (four neighbouring lanes read the same one,
// one request per four coefficients) and its byte.
__device__ __forceinline__ int small_at(const u32 *plane, u32 x)
{
    return (int)(signed char)(plane[x >> 2] >> (8 * (x & 3)));
}
__device__ __forceinline__ u64 small_residue(int v, u64 q)
{
    return v >= 0 ? (u64)v : q - (u64)(-v);
}

// Forward NTT of u, column pass: job l expands u to prime l and writes uh[l] (the row pass is
// JobFwdPlain on uh in place, canonical).
struct JobEncU
{
    const u32 *u; // [n] bytes
    u64 *uh;      // [m][n]
    const PrimeDev *primes;
    const Tw *tw;
    int log_n;
    struct View
    {
        const u32 *u;
        u64 *dst;
        PrimeDev p;
        const Tw *tw;
        bool skip;
        __device__ u64 load(u32 x) const { return small_residue(small_at(u, x), p.q); }
        __device__ void store(u32 x, u64 v) const { dst[x] = v; }
    };
    __device__ View view(int l) const
    {
        return View{ u, uh + ((size_t)l << log_n), prime_at(primes, l), tw + ((size_t)l << log_n), false };
    }
};

// Inverse NTT of the dropped limb, job j = poly.  ROW (first pass): loads uh_L pk_{j,L}, stores lazy
// into last[j]; !ROW (column pass, in place): its store adds e_j and canonicalises.
template <bool ROW>
struct JobEncLast
{
    const u64 *uh;  // [m][n]
    const u64 *pk;  // [2][key_limbs][n]
    const u32 *e;   // [2][n] bytes
    u64 *last;      // [2][n]
    const PrimeDev *primes;
    const Tw *itw;
    int L, key_limbs, log_n;
    int fp = 0;
    struct View
    {
        const u64 *a, *b;
        const u32 *e;
        u64 *dst;
        PrimeDev p;
        const Tw *tw;
        bool skip, fp;
        PrimeF f;
        __device__ u64 load(u32 x) const
        {
            if (!ROW) return dst[x];
            if (fp) // canonical operands below 2^51: the product within 1.25q, canonicalised
                return fp_canon(fp_mulmod_gen(fp_from_u52(a[x]), fp_from_u52(b[x]), f.pd, f.pi), f.pd, f.pi);
            return mulmod(a[x], b[x], p);
        }
        __device__ void store(u32 x, u64 v) const
        {
            if (ROW)
            {
                dst[x] = v;
                return;
            }
            const int s = small_at(e, x);      // ahead of the arithmetic on v
            v = csub(v, p.q);                  // [0, 2q) (canonical in FP) -> canonical
            dst[x] = s >= 0 ? addmod(v, (u64)s, p.q) : submod(v, (u64)(-s), p.q);
        }
    };
    __device__ View view(int j) const
    {
        View v;
        v.a = uh + ((size_t)L << log_n);
        v.b = pk + ((size_t)(j * key_limbs + L) << log_n);
        v.e = e + ((size_t)j << (log_n - 2));
        v.dst = last + ((size_t)j << log_n);
        v.p = prime_at(primes, L);
        v.tw = itw + ((size_t)L << log_n);
        v.skip = false;
        v.fp = fp != 0;
        v.f = prime_f(v.p);
        return v;
    }
};

// Lift column pass: job y = j*L + i loads e_j - r_{j,i} (JobRescaleCol's lift of last_j, taken from
// the expanded error) and starts its NTT mod q_i.
struct JobEncLiftCol
{
    const u64 *last; // [2][n] canonical mod q_L
    const u32 *e;    // [2][n] bytes
    u64 *scratch;    // [2][L][n]
    const PrimeDev *primes;
    const Tw *tw;
    int L, log_n;
    int fp = 0;
    struct View : LiftColView<RescaleLift>
    {
        const u32 *e;
        bool fp;
        PrimeF f;
        __device__ u64 load(u32 x) const
        {
            const u64 s = src[x];
            const int v = small_at(e, x);
            if (fp) // |e - lift_c| <= q_L/2 + 21 < 2^51: one canonicalisation
                return fp_canon((double)v - lift_c(s), f.pd, f.pi);
            return small_residue(v, p.q) + p.two_q - lift(s); // the lift in [0, 2q): (0, 3q], a forward input
        }
    };
    __device__ View view(int y) const
    {
        const int j = y / L, i = y % L;
        const PrimeDev p = prime_at(primes, i);
        return View{ { last + ((size_t)j << log_n), scratch + ((size_t)y << log_n), p, rescale_lift(primes, i, L + 1),
                       tw + ((size_t)i << log_n), false },
                     e + ((size_t)j << (log_n - 2)), fp != 0, prime_f(p) };
    }
};

// Row pass: out[j][i] = (uh_i pk_{j,i} + t) q_L^-1 (+ plain_i for j = 0), t the transform of the lift
// column pass.  The product is formed in pre(), with the pass's own loads.
struct JobEncRow
{
    u64 *scratch;     // [2][L][n]
    const u64 *uh;    // [m][n] canonical
    const u64 *pk;    // [2][key_limbs][n]
    const u64 *plain; // [L][n] or null
    u64 *out;         // [2][L][n]
    const PrimeDev *primes;
    const Tw *tw;
    const Tw *invq;
    int L, K, key_limbs, log_n;
    int fp = 0; // every prime < 2^51: the epilogue in exact FP64 (fparith.h)
    struct View
    {
        u64 *buf;
        const u64 *up, *kp, *mp;
        u64 *outp;
        PrimeDev p;
        const Tw *tw;
        Tw inv;
        bool skip, fp;
        PrimeF f;
        double invd;
        __device__ u64 load(u32 x) const { return buf[x]; }
        struct Pre
        {
            u64 a, m; // uh pk: a double's bits within 1.25q (FP) or the canonical residue; the plaintext word
        };
        __device__ Pre pre(u32 x) const
        {
            const u64 u = up[x], k = kp[x], m = mp ? mp[x] : 0;
            if (fp)
                return Pre{ (u64)__double_as_longlong(fp_mulmod_gen(fp_from_u52(u), fp_from_u52(k), f.pd, f.pi)), m };
            return Pre{ mulmod(u, k, p), m };
        }
        __device__ void store(u32 x, u64 t, Pre o) const
        {
            if (fp)
            {
                // t canonical: the sum within 2.25q < 2^53, its centred residue times q_L^-1 within
                // 1.25q, plus m < q, one canonicalisation: the residue of the integer form
                const double s = fp_reduce(__longlong_as_double((long long)o.a) + fp_from_u52(t), f.pd, f.pi);
                outp[x] = fp_canon(fp_mulmod_gen(s, invd, f.pd, f.pi) + fp_from_u52(o.m), f.pd, f.pi);
                return;
            }
            const u64 v = mul_shoup(o.a + t, inv.x, inv.y, p.q); // t in [0, 4q): the sum below 5q
            outp[x] = addmod(v, o.m, p.q);
        }
        __device__ void store(u32 x, u64 t) const { store(x, t, pre(x)); }
    };
    __device__ View view(int y) const
    {
        const int j = y / L, i = y % L;
        View v;
        v.buf = scratch + ((size_t)y << log_n);
        v.up = uh + ((size_t)i << log_n);
        v.kp = pk + ((size_t)(j * key_limbs + i) << log_n);
        v.mp = (j == 0 && plain) ? plain + ((size_t)i << log_n) : nullptr;
        v.outp = out + ((size_t)y << log_n);
        v.p = prime_at(primes, i);
        v.tw = tw + ((size_t)i << log_n);
        v.inv = tw_at(invq, (size_t)L * K + i);
        v.skip = false;
        v.fp = fp != 0;
        v.f = prime_f(v.p);
        v.invd = (double)v.inv.x;
        return v;
    }
};

// ------------------------------------------------------------- symmetric encryption of a batch
// encrypt_zero_symmetric (keygen.h; rlwe.cpp:289-373) over primes 0 .. sample_limbs-1, stored limb k of
// `stored` = keep + keep_last on prime k (k < keep) or on prime sample_limbs-1 (the last stored limb when
// keep_last).  out is [2][stored][n]: c1 = a already holds the uniform sample, the error e is a byte
// plane (sample.hip k_sk_cbd), and
//     c0_k = -(a_k s_k + NTT_k(e)) (+ (q_{K-1} mod q_k) new_key_k on limb k = digit)      (mod q_k).
__device__ __forceinline__ int sk_prime_of(int k, int keep, int sample_limbs)
{
    return k < keep ? k : sample_limbs - 1;
}

// Column pass: job k expands e to the prime of stored limb k (JobEncU's expansion) into scratch[k].
struct JobSkE
{
    const u32 *e; // [n] bytes
    u64 *scratch; // [stored][n]
    const PrimeDev *primes;
    const Tw *tw;
    int keep, sample_limbs, log_n;
    using View = JobEncU::View;
    __device__ View view(int k) const
    {
        const int pi = sk_prime_of(k, keep, sample_limbs);
        return View{ e, scratch + ((size_t)k << log_n), prime_at(primes, pi), tw + ((size_t)pi << log_n), false };
    }
};

// Row pass: pre() forms g - a s with the pass's own loads (g the gadget term, 0 off limb `digit`), the
// store subtracts the transform t of e and writes the canonical word: q - ((a s + t) mod q), 0 for 0,
// plus g -- the words of mhe_multiply_plain, mhe_add, mhe_negate, mhe_multiply_scalar, mhe_add.
struct JobSkRow
{
    u64 *scratch;       // [stored][n]
    const u64 *sk;      // [K][n]
    const u64 *new_key; // [K][n] or null
    u64 *out;           // [2][stored][n]
    const PrimeDev *primes;
    const Tw *tw;
    int keep, stored, sample_limbs, digit, K, log_n;
    int fp = 0; // every prime < 2^51: the epilogue in exact FP64 (fparith.h)
    struct View
    {
        u64 *buf;
        const u64 *ap, *sp, *np;
        u64 *outp;
        PrimeDev p;
        const Tw *tw;
        u64 gad; // q_{K-1} mod q, canonical
        bool skip, fp;
        PrimeF f;
        __device__ u64 load(u32 x) const { return buf[x]; }
        // g - a s: a double's bits within 2.5q (FP) or the canonical residue
        using Pre = u64;
        __device__ Pre pre(u32 x) const
        {
            const u64 a = ap[x], s = sp[x], k = np ? np[x] : 0;
            if (fp)
            {
                // canonical operands below 2^51: each product within 1.25q
                const double g = np ? fp_mulmod_gen(fp_from_u52(k), fp_from_u52(gad), f.pd, f.pi) : 0.0;
                return (u64)__double_as_longlong(g - fp_mulmod_gen(fp_from_u52(a), fp_from_u52(s), f.pd, f.pi));
            }
            const u64 g = np ? mulmod(k, gad, p) : 0;
            return submod(g, mulmod(a, s, p), p.q);
        }
        __device__ void store(u32 x, u64 t, Pre o) const
        {
            if (fp) // t canonical: |g - a s - t| < 3.5q < 2^53, one canonicalisation
                outp[x] = fp_canon(__longlong_as_double((long long)o) - fp_from_u52(t), f.pd, f.pi);
            else // t in [0, 4q) -> canonical
                outp[x] = submod(o, csub(csub(t, p.two_q), p.q), p.q);
        }
        __device__ void store(u32 x, u64 t) const { store(x, t, pre(x)); }
    };
    __device__ View view(int k) const
    {
        const int pi = sk_prime_of(k, keep, sample_limbs);
        View v;
        v.buf = scratch + ((size_t)k << log_n);
        v.ap = out + ((size_t)(stored + k) << log_n);
        v.sp = sk + ((size_t)pi << log_n);
        v.np = (new_key && k == digit) ? new_key + ((size_t)pi << log_n) : nullptr;
        v.outp = out + ((size_t)k << log_n);
        v.p = prime_at(primes, pi);
        v.tw = tw + ((size_t)pi << log_n);
        v.gad = barrett64(prime_at(primes, K - 1).q, v.p);
        v.skip = false;
        v.fp = fp != 0;
        v.f = prime_f(v.p);
        return v;
    }
};
