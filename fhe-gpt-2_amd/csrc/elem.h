// Elementwise, Galois-permutation and mod-raise kernels with their argument structs: one kernel per
// kind for a single launch, and k_elem_b / k_copy16_b / k_galois_b over up to MHE_MAXB entries.
#pragma once

// Elementwise kernels process 2 residues per lane (16-B loads); n is a multiple of 512.
#define ELEM_GRID(total2) dim3((unsigned)(((total2) + 255) / 256))

// Elementwise products in FP64 (csrc/fparith.h) for primes below 2^51, where the integer path's
// 64 x 64 -> 128-bit product and Barrett reduction cost several half- and quarter-rate instructions:
// canonical residues are exact doubles, fp_mulmod_gen leaves a*b mod q in (-1.25q, 1.25q) and
// fp_canon returns the canonical residue, so the words are the integer path's.  fp: the context's
// FP64 mode (MHE_FP=0 keeps every product on the integer path).
__device__ __forceinline__ bool elem_fp(int fp, const PrimeDev &p)
{
    return fp && p.q < (1ull << 51);
}
__device__ __forceinline__ double mulmod_fd(u64 a, u64 b, const PrimeDev &p) // (-1.25q, 1.25q)
{
    return fp_mulmod_gen(fp_from_u52(a), fp_from_u52(b), p.qd, p.qi);
}
__device__ __forceinline__ u64 mulmod_e(u64 a, u64 b, const PrimeDev &p, bool f)
{
    return f ? fp_canon(mulmod_fd(a, b, p), p.qd, p.qi) : mulmod(a, b, p);
}

__device__ __forceinline__ void addsub_at(const u64 *a, const u64 *b, u64 *out, const PrimeDev *primes, int limbs,
                                          int log_n, size_t i2, int op)
{
    const size_t i = i2 * 2;
    const int l = (int)((i >> log_n) % limbs);
    const u64 q = primes[l].q;
    ulonglong2 x = *(const ulonglong2 *)(a + i);
    ulonglong2 r;
    if (op == 0)
    {
        ulonglong2 y = *(const ulonglong2 *)(b + i);
        r.x = addmod(x.x, y.x, q);
        r.y = addmod(x.y, y.y, q);
    }
    else if (op == 1)
    {
        ulonglong2 y = *(const ulonglong2 *)(b + i);
        r.x = submod(x.x, y.x, q);
        r.y = submod(x.y, y.y, q);
    }
    else
    {
        r.x = x.x ? q - x.x : 0;
        r.y = x.y ? q - x.y : 0;
    }
    *(ulonglong2 *)(out + i) = r;
}

__global__ void k_addsub(const u64 *a, const u64 *b, u64 *out, const PrimeDev *primes, int limbs, int log_n,
                         size_t total2, int op)
{
    size_t i2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i2 < total2) addsub_at(a, b, out, primes, limbs, log_n, i2, op);
}

// dyadic product with b broadcast over polys (multiply_plain_ntt)
__device__ __forceinline__ void mulplain_at(const u64 *a, const u64 *b, u64 *out, const PrimeDev *primes, int limbs,
                                            int log_n, size_t i2, int fp)
{
    const size_t i = i2 * 2;
    const size_t limb_words = (size_t)limbs << log_n;
    const int l = (int)((i >> log_n) % limbs);
    const PrimeDev p = primes[l];
    const bool f = elem_fp(fp, p); // uniform: a wave's residues are of one limb
    ulonglong2 x = *(const ulonglong2 *)(a + i);
    ulonglong2 y = *(const ulonglong2 *)(b + i % limb_words);
    ulonglong2 r;
    r.x = mulmod_e(x.x, y.x, p, f);
    r.y = mulmod_e(x.y, y.y, p, f);
    *(ulonglong2 *)(out + i) = r;
}

__global__ void k_mulplain(const u64 *a, const u64 *b, u64 *out, const PrimeDev *primes, int limbs, int log_n,
                           size_t total2, int fp)
{
    size_t i2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i2 < total2) mulplain_at(a, b, out, primes, limbs, log_n, i2, fp);
}

// acc += a * b, b broadcast over polys (multiply_plain_ntt then add_inplace, one pass)
__device__ __forceinline__ void mulplain_add_at(const u64 *a, const u64 *b, u64 *acc, const PrimeDev *primes,
                                                int limbs, int log_n, size_t i2, int fp)
{
    const size_t i = i2 * 2;
    const size_t limb_words = (size_t)limbs << log_n;
    const int l = (int)((i >> log_n) % limbs);
    const PrimeDev p = primes[l];
    ulonglong2 x = *(const ulonglong2 *)(a + i);
    ulonglong2 y = *(const ulonglong2 *)(b + i % limb_words);
    ulonglong2 z = *(const ulonglong2 *)(acc + i);
    ulonglong2 r;
    if (elem_fp(fp, p))
    {
        // canonical acc (< q) + a product in (-1.25q, 1.25q): |.| < 2.25q, exact
        r.x = fp_canon(fp_from_u52(z.x) + mulmod_fd(x.x, y.x, p), p.qd, p.qi);
        r.y = fp_canon(fp_from_u52(z.y) + mulmod_fd(x.y, y.y, p), p.qd, p.qi);
    }
    else
    {
        r.x = addmod(z.x, mulmod(x.x, y.x, p), p.q);
        r.y = addmod(z.y, mulmod(x.y, y.y, p), p.q);
    }
    *(ulonglong2 *)(acc + i) = r;
}

__global__ void k_mulplain_add(const u64 *a, const u64 *b, u64 *acc, const PrimeDev *primes, int limbs, int log_n,
                               size_t total2, int fp)
{
    size_t i2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i2 < total2) mulplain_add_at(a, b, acc, primes, limbs, log_n, i2, fp);
}

// acc = (accumulate ? acc : 0) + sum_k a_k * b_k, up to 16 terms per launch (pointers in the kernel
// arguments); each thread's 2 * cnt loads are independent, so they are all in flight together
#define MHE_SUM_TERMS 16
struct SumPtrs
{
    const u64 *a[MHE_SUM_TERMS];
    const u64 *b[MHE_SUM_TERMS];
};
__global__ void k_mulplain_sum(SumPtrs P, int cnt, u64 *acc, int accumulate, const PrimeDev *primes, int limbs,
                               int log_n, size_t total2, int fp)
{
    size_t i2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i2 >= total2) return;
    const size_t i = i2 * 2;
    const size_t limb_words = (size_t)limbs << log_n;
    const int l = (int)((i >> log_n) % limbs);
    const PrimeDev p = primes[l];
    ulonglong2 z = accumulate ? *(const ulonglong2 *)(acc + i) : ulonglong2{ 0, 0 };
    if (elem_fp(fp, p))
    {
        // FP64 sums: products in (-1.25q, 1.25q), centred by fp_reduce after every second one, so
        // |sum| < q/2 + 1 + 2.5q < 2^53 throughout; one fp_canon at the end
        double sx = fp_from_u52(z.x), sy = fp_from_u52(z.y);
        for (int k = 0; k < cnt; k++)
        {
            const ulonglong2 x = *(const ulonglong2 *)(P.a[k] + i);
            const ulonglong2 y = *(const ulonglong2 *)(P.b[k] + i % limb_words);
            sx += mulmod_fd(x.x, y.x, p);
            sy += mulmod_fd(x.y, y.y, p);
            if (k & 1)
            {
                sx = fp_reduce(sx, p.qd, p.qi);
                sy = fp_reduce(sy, p.qd, p.qi);
            }
        }
        z.x = fp_canon(sx, p.qd, p.qi);
        z.y = fp_canon(sy, p.qd, p.qi);
    }
    else
    {
        for (int k = 0; k < cnt; k++)
        {
            const ulonglong2 x = *(const ulonglong2 *)(P.a[k] + i);
            const ulonglong2 y = *(const ulonglong2 *)(P.b[k] + i % limb_words);
            z.x = addmod(z.x, mulmod(x.x, y.x, p), p.q);
            z.y = addmod(z.y, mulmod(x.y, y.y, p), p.q);
        }
    }
    *(ulonglong2 *)(acc + i) = z;
}

// out = sum_k ct[k] * s^k (Decryptor::decrypt's dot product with the powers of the secret key) by
// Horner over the polys, every intermediate reduced mod q_l: the residues of multiplying the powers
// out and adding term by term.  sk is the key-level secret key, whose first `limbs` limbs lie at the
// same offsets as a poly of the level; out may alias ct[0] (a lane reads its words before it writes).
__global__ void k_decrypt(const u64 *ct, int size, const u64 *sk, u64 *out, const PrimeDev *primes, int limbs,
                          int log_n, size_t total2, int fp)
{
    size_t i2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i2 >= total2) return;
    const size_t i = i2 * 2;
    const size_t ps = (size_t)limbs << log_n;
    const PrimeDev p = primes[(int)(i >> log_n)];
    const bool f = elem_fp(fp, p);
    const ulonglong2 s = *(const ulonglong2 *)(sk + i);
    ulonglong2 z = *(const ulonglong2 *)(ct + (size_t)(size - 1) * ps + i);
    for (int k = size - 2; k >= 0; k--)
    {
        const ulonglong2 x = *(const ulonglong2 *)(ct + (size_t)k * ps + i);
        if (f)
        {
            // canonical x (< q) + a product in (-1.25q, 1.25q): |.| < 2.25q, exact
            z.x = fp_canon(fp_from_u52(x.x) + mulmod_fd(z.x, s.x, p), p.qd, p.qi);
            z.y = fp_canon(fp_from_u52(x.y) + mulmod_fd(z.y, s.y, p), p.qd, p.qi);
        }
        else
        {
            z.x = addmod(x.x, mulmod(z.x, s.x, p), p.q);
            z.y = addmod(x.y, mulmod(z.y, s.y, p), p.q);
        }
    }
    *(ulonglong2 *)(out + i) = z;
}

struct ScalarTab
{
    u64 v[64];
    u64 vq[64];
};

__device__ __forceinline__ void scalar_at(const u64 *a, u64 *out, const PrimeDev *primes, const ScalarTab &s, int limbs,
                                          int log_n, size_t i2, int op)
{
    const size_t i = i2 * 2;
    const int l = (int)((i >> log_n) % limbs);
    const u64 q = primes[l].q;
    ulonglong2 r;
    if (op == 2)
    {
        r.x = r.y = s.v[l];
        *(ulonglong2 *)(out + i) = r;
        return;
    }
    ulonglong2 x = *(const ulonglong2 *)(a + i);
    if (op == 0)
    {
        r.x = mul_shoup(x.x, s.v[l], s.vq[l], q);
        r.y = mul_shoup(x.y, s.v[l], s.vq[l], q);
    }
    else
    {
        r.x = addmod(x.x, s.v[l], q);
        r.y = addmod(x.y, s.v[l], q);
    }
    *(ulonglong2 *)(out + i) = r;
}

__global__ void k_scalar(const u64 *a, u64 *out, const PrimeDev *primes, ScalarTab s, int limbs, int log_n,
                         size_t total2, int op)
{
    size_t i2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i2 < total2) scalar_at(a, out, primes, s, limbs, log_n, i2, op);
}

// ckks_multiply tile loop (evaluator.cpp:714-773) / ckks_square (:1000-1059), fused.
__device__ __forceinline__ void tensor_at(const u64 *a, const u64 *b, u64 *out, const PrimeDev *primes, int limbs,
                                          int log_n, size_t i2, int square, int fp)
{
    const size_t i = i2 * 2;
    const size_t ps = (size_t)limbs << log_n;
    const int l = (int)(i >> log_n);
    const PrimeDev p = primes[l];
    ulonglong2 x0 = *(const ulonglong2 *)(a + i), x1 = *(const ulonglong2 *)(a + ps + i);
    ulonglong2 r0, r1, r2;
    if (elem_fp(fp, p))
    {
        // FP64: each product in (-1.25q, 1.25q), the cross term's two in (-2.5q, 2.5q), exact
        const ulonglong2 y0 = square ? x0 : *(const ulonglong2 *)(b + i), y1 = square ? x1 : *(const ulonglong2 *)(b + ps + i);
        const double qd = p.qd, qi = p.qi;
        r0.x = fp_canon(mulmod_fd(x0.x, y0.x, p), qd, qi);
        r0.y = fp_canon(mulmod_fd(x0.y, y0.y, p), qd, qi);
        r1.x = fp_canon(mulmod_fd(x0.x, y1.x, p) + mulmod_fd(x1.x, y0.x, p), qd, qi);
        r1.y = fp_canon(mulmod_fd(x0.y, y1.y, p) + mulmod_fd(x1.y, y0.y, p), qd, qi);
        r2.x = fp_canon(mulmod_fd(x1.x, y1.x, p), qd, qi);
        r2.y = fp_canon(mulmod_fd(x1.y, y1.y, p), qd, qi);
    }
    else if (square)
    {
        r0.x = mulmod(x0.x, x0.x, p);
        r0.y = mulmod(x0.y, x0.y, p);
        u64 t = mulmod(x0.x, x1.x, p), u = mulmod(x0.y, x1.y, p);
        r1.x = addmod(t, t, p.q);
        r1.y = addmod(u, u, p.q);
        r2.x = mulmod(x1.x, x1.x, p);
        r2.y = mulmod(x1.y, x1.y, p);
    }
    else
    {
        ulonglong2 y0 = *(const ulonglong2 *)(b + i), y1 = *(const ulonglong2 *)(b + ps + i);
        r0.x = mulmod(x0.x, y0.x, p);
        r0.y = mulmod(x0.y, y0.y, p);
        r1.x = addmod(mulmod(x0.x, y1.x, p), mulmod(x1.x, y0.x, p), p.q);
        r1.y = addmod(mulmod(x0.y, y1.y, p), mulmod(x1.y, y0.y, p), p.q);
        r2.x = mulmod(x1.x, y1.x, p);
        r2.y = mulmod(x1.y, y1.y, p);
    }
    *(ulonglong2 *)(out + i) = r0;
    *(ulonglong2 *)(out + ps + i) = r1;
    *(ulonglong2 *)(out + 2 * ps + i) = r2;
}

__global__ void k_tensor(const u64 *a, const u64 *b, u64 *out, const PrimeDev *primes, int limbs, int log_n,
                         size_t total2, int square, int fp)
{
    size_t i2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i2 < total2) tensor_at(a, b, out, primes, limbs, log_n, i2, square, fp);
}

// The same elementwise kernels over up to MHE_MAXB entries of one shape (entry = blockIdx.y): the
// launches that mhe_launch_run coalesces, e.g. the same-numbered adds of the images of a
// seal::FiberBatch
struct ElemPtrs
{
    const u64 *a[MHE_MAXB];
    const u64 *b[MHE_MAXB];
    u64 *out[MHE_MAXB];
};

__global__ void k_elem_b(ElemPtrs P, const PrimeDev *primes, ScalarTab st, int limbs, int log_n, size_t total2,
                         int kind, int op, int fp)
{
    const size_t i2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i2 >= total2) return;
    const int e = blockIdx.y;
    switch (kind)
    {
    case MHE_LK_ADDSUB: addsub_at(P.a[e], P.b[e], P.out[e], primes, limbs, log_n, i2, op); break;
    case MHE_LK_MULPLAIN: mulplain_at(P.a[e], P.b[e], P.out[e], primes, limbs, log_n, i2, fp); break;
    case MHE_LK_MULPLAIN_ADD: mulplain_add_at(P.a[e], P.b[e], P.out[e], primes, limbs, log_n, i2, fp); break;
    case MHE_LK_SCALAR: scalar_at(P.a[e], P.out[e], primes, st, limbs, log_n, i2, op); break;
    case MHE_LK_TENSOR: tensor_at(P.a[e], P.b[e], P.out[e], primes, limbs, log_n, i2, op, fp); break;
    }
}

__global__ void k_copy16_b(ElemPtrs P, size_t count)
{
    const int e = blockIdx.y;
    uint4 *dst = reinterpret_cast<uint4 *>(P.out[e]);
    const uint4 *src = reinterpret_cast<const uint4 *>(P.a[e]);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

// GaloisTool::apply_galois_ntt (util/galois.cpp:192-218) with the permutation of
// generate_table_ntt (util/galois.cpp:18-51) computed on the fly: out[i] = in[tab(i)].
__global__ void k_galois(const u64 *in, u64 *out, u32 elt, int log_n, size_t total)
{
    size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const u32 n = 1u << log_n;
    const u32 i = (u32)(g & (n - 1));
    const size_t base = g - i;
    const u32 reversed = __builtin_bitreverse32(n + i) >> (31 - log_n); // rev over log_n+1 bits
    const u32 idx = (u32)(((u64)elt * reversed) >> 1) & (n - 1);
    const u32 src = __builtin_bitreverse32(idx) >> (32 - log_n);
    out[g] = in[base + src];
}

// The same for up to MHE_MAXB independent (in, out, element) entries, entry = blockIdx.y.
struct GalPtrs
{
    const u64 *in[MHE_MAXB];
    u64 *out[MHE_MAXB];
    u32 elt[MHE_MAXB];
};

__global__ void k_galois_b(GalPtrs P, int log_n, size_t total)
{
    size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const u64 *in = P.in[blockIdx.y];
    u64 *out = P.out[blockIdx.y];
    const u32 elt = P.elt[blockIdx.y];
    const u32 n = 1u << log_n;
    const u32 i = (u32)(g & (n - 1));
    const size_t base = g - i;
    const u32 reversed = __builtin_bitreverse32(n + i) >> (31 - log_n);
    const u32 idx = (u32)(((u64)elt * reversed) >> 1) & (n - 1);
    const u32 src = __builtin_bitreverse32(idx) >> (32 - log_n);
    out[g] = in[base + src];
}

// Bootstrapper::modraise_inplace (ckks_bootstrapping/Bootstrapper.cpp:2894-2948): the single-limb
// coefficient-form polynomial x (mod q_0, canonical) is lifted centered, v = x - q_0 if
// x > q_0/2, and reduced mod every prime of the target level.
__global__ void k_modraise(const u64 *in, u64 *out, const PrimeDev *primes, int limbs, int log_n, size_t total)
{
    size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const size_t n = (size_t)1 << log_n;
    const size_t per_poly = (size_t)limbs << log_n;
    const size_t p = g / per_poly, r = g - p * per_poly;
    const int j = (int)(r >> log_n);
    const size_t i = r & (n - 1);
    const u64 x = in[p * n + i];
    const u64 q0 = primes[0].q, q = primes[j].q;
    u64 v = x % q;
    if (x > (q0 >> 1))
    {
        const u64 mq0 = q - q0 % q; // -q_0 mod q (q for j = 0 reduces to 0 below)
        v += mq0;
        v -= (v >= q) ? q : 0;
    }
    out[g] = v;
}
