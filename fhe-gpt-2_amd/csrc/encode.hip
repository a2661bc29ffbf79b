// CKKS encoding for libmhe.
//
// CKKSEncoder::encode (SEAL/ckks.h:457-640) is a double-precision FFT followed by rounding, an
// RNS reduction and a per-limb NTT.  Bit-exactness with SEAL needs SEAL's exact sequence of
// non-fused double operations (the reference builds its encoder without FMA); IEEE double
// arithmetic is the same on the host and on the GPU, so the whole encode runs on the device,
// compiled with -ffp-contract=off, in SEAL's operation order:
//   * ComplexRoots (util/croots.cpp:17-66): polar(1, 2*PI*i/m) for i <= m/8, 8-fold symmetry,
//     computed once on the host (sincos) and kept in HBM per device;
//   * index map 5^i (ckks.cpp:34-49) computed per slot on the device;
//   * DWTHandler::transform_from_rev over complex<double> with scalar scale/n
//     (util/dwthandler.h:202-314, ckks.h:46-81): the first 12 stages in LDS (4096-point blocks),
//     the remaining stages one launch each;
//   * std::round, then the coefficient's integer value mod q_j (SEAL's 1-word, 2-word and
//     multi-word paths all reduce the same integer, so one per-coefficient decomposition gives
//     their residues).
// The slot values travel through a pinned staging ring, so encode never waits for the device.
// SEAL's "encoded values are too large" check needs max |coeff|: a host bound
// (scale / n) * 2 * sum |v_i| settles it for every ordinary input; only when the bound comes
// within a bit of the limit is the exact device maximum read back (one stream sync).
// mhe_ckks_encode_dev runs the same steps for up to 8 vectors per launch that are already in device
// memory (k_encb_*): no ring and no synchronisation, the size check decided on the device per entry.
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>

extern "C" hipError_t mhe_internal_copy_d2d(void *dst, const void *src, size_t bytes, hipStream_t st);
extern "C" hipError_t mhe_internal_alloc(void **p, size_t bytes, hipStream_t st);
extern "C" hipError_t mhe_internal_free(void *p, hipStream_t st);
#include <vector>

#include "../../include/mhe.h"
#include "arith.h"
#include "encode_check.h" // size_fits, l1_proves_size, largest_fitting

typedef unsigned __int128 u128;
typedef std::complex<double> cd;

// shared with mhe.hip
int mhe_internal_fail(int code, const char *msg);
int mhe_internal_ntt_forward(mhe_ctx *c, uint64_t *data, int polys, int limbs, int full, hipStream_t st);
int mhe_internal_ntt_forward_entries(mhe_ctx *c, uint64_t *const *data, int B, int limbs, const uint32_t *skip_if,
                                     hipStream_t st);
int mhe_internal_primes(mhe_ctx *c, const PrimeDev **dev, const uint64_t **host, int *count, int *log_n);

struct mhe_encoder
{
    int log_n = 0;
    size_t n = 0, slots = 0;
    std::vector<size_t> index_map;
    std::vector<cd> inv_root_powers;
    std::vector<cd> root_powers;

    // device state (lazily created on the first encode of each device)
    // Pinned upload slots, reused round robin.  Reusing a slot waits (under `mu`, so for every
    // thread) until its last upload has run, and that upload sits behind whatever its stream had
    // queued -- with 8 slots, 3 host threads x 8 fibers wrapped the ring within one merged step and
    // every thread stalled behind another stream's key switches.  64 slots (32 MB at n = 2^16) are
    // reused only after ~0.1 s of encodes, when no stream is that far behind.
    static constexpr int kRing = 64;
    struct DevRoots
    {
        int dev;
        double2 *roots; // inv_root_powers [n], root_powers [n] (decode's forward FFT), inverse index map [n] u32
    };
    // decode's RNS constants of one level (the first `q.size()` primes of a chain) on one device:
    // Q, (Q+1)/2, (Q/q_j)^-1 mod q_j and the punctured products Q/q_j, W words each
    struct DecLevel
    {
        int dev;
        std::vector<uint64_t> q;
        uint64_t *consts;
    };
    mutable std::mutex mu;
    mutable std::vector<DevRoots> dev_roots;
    mutable std::vector<DecLevel> dec_levels;
    mutable double *ring = nullptr; // kRing slots of 2 * slots doubles (re, im), pinned
    mutable hipEvent_t ring_ev[kRing] = {};
    mutable int ring_dev = -1;
    mutable unsigned ring_next = 0;
    ~mhe_encoder()
    {
        for (auto &d : dev_roots) (void)hipFree(d.roots);
        for (auto &d : dec_levels) (void)hipFree(d.consts);
        if (ring) (void)hipHostFree(ring);
        for (auto &ev : ring_ev)
            if (ev) (void)hipEventDestroy(ev);
    }
};

namespace
{
u32 rev_bits(u32 x, int bits)
{
    return bits ? (__builtin_bitreverse32(x) >> (32 - bits)) : 0;
}

struct ComplexRoots
{
    size_t m;
    std::vector<cd> roots;
    explicit ComplexRoots(size_t degree) : m(degree), roots(degree / 8 + 1)
    {
        const double PI_ = 3.1415926535897932384626433832795028842;
        for (size_t i = 0; i <= m / 8; i++)
        {
            // std::polar(1, theta) as SEAL's GCC Release build evaluates it: one sincos() call
            // (separate cos()/sin() differ in the last bit for a few angles)
            double sn, cs;
            ::sincos(2 * PI_ * static_cast<double>(i) / static_cast<double>(m), &sn, &cs);
            roots[i] = cd(cs, sn);
        }
    }
    cd get(size_t index) const
    {
        index &= m - 1;
        if (index <= m / 8) return roots[index];
        if (index <= m / 4) return cd(roots[m / 4 - index].imag(), roots[m / 4 - index].real());
        if (index <= m / 2) return -std::conj(get(m / 2 - index));
        if (index <= 3 * m / 4) return -get(index - m / 2);
        return std::conj(get(m - index));
    }
};

// SEAL's ContextData::total_coeff_modulus_bit_count: bit length of prod q_j.
int total_bits(const uint64_t *q, int limbs)
{
    std::vector<u64> prod(limbs + 1, 0);
    prod[0] = 1;
    int words = 1;
    for (int j = 0; j < limbs; j++)
    {
        u64 carry = 0;
        for (int w = 0; w < words; w++)
        {
            u128 t = (u128)prod[w] * q[j] + carry;
            prod[w] = (u64)t;
            carry = (u64)(t >> 64);
        }
        if (carry) prod[words++] = carry;
    }
    return 64 * (words - 1) + (64 - __builtin_clzll(prod[words - 1]));
}

u64 words_mod(const u64 *w, int nw, u64 q)
{
    u128 r = 0;
    for (int k = nw - 1; k >= 0; k--) r = ((r << 64) | w[k]) % q;
    return (u64)r;
}

int scale_fault(double scale, int bound_limbs, int tb)
{
    return mhe_internal_fail(MHE_ERR_ARG, ("scale out of bounds (encoding 2^" + std::to_string(std::log2(scale)) +
                                           " at " + std::to_string(bound_limbs) + " limbs, " + std::to_string(tb) +
                                           " bits)").c_str());
}

// The encoder's complex roots on device `dev`, uploaded once per device (caller holds e->mu):
// inv_root_powers for encode's inverse FFT, root_powers behind them for decode's forward FFT, then
// mhe_ckks_encode_dev's inverse index table (n 32-bit words, at roots + 2n).
int device_roots(const mhe_encoder *e, int dev, const double2 **out)
{
    for (auto &d : e->dev_roots)
        if (d.dev == dev)
        {
            *out = d.roots;
            return MHE_OK;
        }
    const size_t n = e->n;
    // the inverse of index_map: position p of the FFT input holds slot w >> 1, conjugated when w & 1
    std::vector<u32> inv(n);
    for (size_t i = 0; i < e->slots; i++)
    {
        inv[e->index_map[i]] = (u32)(i << 1);
        inv[e->index_map[e->slots | i]] = (u32)(i << 1) | 1;
    }
    double2 *r = nullptr;
    if (hipMalloc((void **)&r, 2 * n * sizeof(double2) + n * sizeof(u32)) != hipSuccess)
        return mhe_internal_fail(MHE_ERR_MEMORY, "encoder roots allocation failed");
    if (hipMemcpy(r, e->inv_root_powers.data(), n * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(r + n, e->root_powers.data(), n * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(r + 2 * n, inv.data(), n * sizeof(u32), hipMemcpyHostToDevice) != hipSuccess)
    {
        (void)hipFree(r);
        return mhe_internal_fail(MHE_ERR_DEVICE, "encoder roots upload failed");
    }
    e->dev_roots.push_back({ dev, r });
    *out = r;
    return MHE_OK;
}
} // namespace

// ---- device encode kernels -------------------------------------------------------------
namespace
{
__device__ __forceinline__ u32 rev_bits_dev(u32 x, int bits)
{
    return __builtin_bitreverse32(x) >> (32 - bits);
}

// cv[index_map[i]] = v_i, cv[index_map[i + slots]] = conj(v_i) (ckks.h:488-497); cv pre-zeroed
__global__ void k_enc_scatter(const double *vals, size_t count, int has_im, double2 *cv, int log_n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const u64 m = (u64)2 << log_n;
    u64 pos = 1, b = 5;
    for (u64 e = i; e; e >>= 1)
    {
        if (e & 1) pos = (pos * b) & (m - 1);
        b = (b * b) & (m - 1);
    }
    const double re = vals[i], im = has_im ? vals[count + i] : 0.0;
    cv[rev_bits_dev((u32)((pos - 1) >> 1), log_n)] = double2{ re, im };
    cv[rev_bits_dev((u32)((m - pos - 1) >> 1), log_n)] = double2{ re, -im };
}

// one butterfly of transform_from_rev in SEAL's operation order (complex products as
// (ac - bd, ad + bc), no contraction); the last stage folds in the scalar
__device__ __forceinline__ void enc_bfly(double2 &x, double2 &y, double2 r, bool last, double scalar)
{
    const double2 u = x, v = y;
    const double2 s = double2{ u.x + v.x, u.y + v.y }, d = double2{ u.x - v.x, u.y - v.y };
    if (last)
    {
        r = double2{ r.x * scalar, r.y * scalar };
        x = double2{ s.x * scalar, s.y * scalar };
    }
    else
        x = s;
    y = double2{ d.x * r.x - d.y * r.y, d.x * r.y + d.y * r.x };
}

constexpr int kEncLogBlock = 12;

// stages 0 .. lb-1 (gap 1 .. 2^(lb-1)) of the 2^lb-point block at `base`, held in LDS by a workgroup
// of 256 lanes; barriers before the first and after every stage
__device__ __forceinline__ void enc_block_stages(double2 *sh, const double2 *roots, size_t base, int log_n, int lb,
                                                 double scalar)
{
    const size_t n = (size_t)1 << log_n, B = (size_t)1 << lb;
    __syncthreads();
    for (int st = 0; st < lb; st++)
    {
        const size_t m = n >> (st + 1), gap = (size_t)1 << st;
        for (size_t t = threadIdx.x; t < B / 2; t += 256)
        {
            const size_t k = t >> st, x = (k << (st + 1)) + (t & (gap - 1));
            const double2 r = roots[n - 2 * m + 1 + (base >> (st + 1)) + k];
            enc_bfly(sh[x], sh[x + gap], r, m == 1, scalar);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_enc_fft_block(double2 *cv, const double2 *roots, int log_n, int lb,
                                                       double scalar)
{
    __shared__ double2 sh[1 << kEncLogBlock];
    const size_t B = (size_t)1 << lb, base = (size_t)blockIdx.x << lb;
    for (size_t t = threadIdx.x; t < B; t += 256) sh[t] = cv[base + t];
    enc_block_stages(sh, roots, base, log_n, lb, scalar);
    for (size_t t = threadIdx.x; t < B; t += 256) cv[base + t] = sh[t];
}

// stages lb .. log_n-1 (gap 2^lb .. 2^(log_n-1)) in one launch: they only pair elements with the same
// low lb bits, so a lane holds the 2^(log_n-lb) <= 16 elements of one such column in registers and
// runs the stages in order -- the same butterflies on the same values as one k_enc_fft_stage launch
// per stage, so the same doubles, in one launch instead of log_n - lb
template <int LR> // log_n - lb
__device__ __forceinline__ void enc_tail_stages(double2 (&v)[1 << LR], const double2 *roots, int log_n, int lb,
                                                double scalar)
{
    constexpr int R = 1 << LR;
    const size_t n = (size_t)1 << log_n;
#pragma unroll
    for (int s = 0; s < LR; s++)
    {
        const int st = lb + s;
        const size_t m = n >> (st + 1);
#pragma unroll
        for (int j = 0; j < R; j++)
            if (!(j & (1 << s)))
            {
                const double2 r = roots[n - 2 * m + 1 + (size_t)(j >> (s + 1))];
                enc_bfly(v[j], v[j + (1 << s)], r, m == 1, scalar);
            }
    }
}

template <int LR>
__global__ __launch_bounds__(256) void k_enc_fft_tail(double2 *cv, const double2 *roots, int log_n, int lb,
                                                      double scalar)
{
    constexpr int R = 1 << LR;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ((size_t)1 << lb)) return;
    double2 v[R];
#pragma unroll
    for (int j = 0; j < R; j++) v[j] = cv[c + ((size_t)j << lb)];
    enc_tail_stages<LR>(v, roots, log_n, lb, scalar);
#pragma unroll
    for (int j = 0; j < R; j++) cv[c + ((size_t)j << lb)] = v[j];
}

// one later stage (gap 2^st) over the whole vector
__global__ void k_enc_fft_stage(double2 *cv, const double2 *roots, int log_n, int st, double scalar)
{
    const size_t n = (size_t)1 << log_n, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n / 2) return;
    const size_t m = n >> (st + 1), gap = (size_t)1 << st, k = t >> st, x = (k << (st + 1)) + (t & (gap - 1));
    enc_bfly(cv[x], cv[x + gap], roots[n - 2 * m + 1 + k], m == 1, scalar);
}

// max |Re cv_i| as ordered bit patterns (non-negative doubles order like their u64 bits)
__global__ void k_enc_absmax(const double2 *cv, size_t n, unsigned long long *mx)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long v = i < n ? (unsigned long long)__double_as_longlong(fabs(cv[i].x)) : 0ull;
    for (int o = 32; o; o >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) atomicMax(mx, v);
}

// round(re) mod p.q, sign applied (ckks.h:545-640)
__device__ __forceinline__ u64 enc_residue(double re, const PrimeDev &p)
{
    double c = round(re);
    const bool neg = signbit(c);
    c = fabs(c);
    u64 r;
    if (c < 0x1p64)
        r = barrett64((u64)c, p);
    else
    {
        u64 w[17];
        int nw = 0;
        while (c >= 1 && nw < 17)
        {
            w[nw++] = (u64)fmod(c, 0x1p64);
            c /= 0x1p64;
        }
        r = 0;
        for (int k = nw - 1; k >= 0; k--) r = barrett128(w[k], r, p);
    }
    return (neg && r) ? p.q - r : r;
}

// out[j][i] = round(Re cv_i) mod q_j
__global__ void k_enc_round_reduce(const double2 *cv, u64 *out, const PrimeDev *primes, int limbs, int log_n)
{
    const size_t n = (size_t)1 << log_n;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n * limbs) return;
    out[g] = enc_residue(cv[g & (n - 1)].x, primes[g >> log_n]);
}

// ---- mhe_ckks_encode_dev: the same steps for up to MHE_MAXB entries per launch (entry =
// blockIdx.y), the values read from device memory
#ifndef MHE_MAXB
#define MHE_MAXB 8 // as ntt.h
#endif

struct EncB
{
    const double *vals[MHE_MAXB]; // count reals or (re, im) pairs; may be null when count is 0
    u64 *out[MHE_MAXB];           // [limbs][n]
    u32 check;                    // bit b: entry b's maximum is taken and compared on the device
};

// the workgroup's part of max |Re cv_i| of one entry, as ordered bit patterns (k_enc_absmax); a NaN
// orders above every finite value and above Inf.  Whole waves call this.
__device__ __forceinline__ void enc_max_fold(unsigned long long v, unsigned long long *mx)
{
    for (int o = 32; o; o >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) atomicMax(mx, v);
}
__device__ __forceinline__ unsigned long long enc_abs_bits(double x)
{
    return (unsigned long long)__double_as_longlong(fabs(x));
}

// k_enc_scatter and k_enc_fft_block in one: position p of the block is read straight from the
// entry's values through the inverse index table (slot w >> 1, conjugated when w & 1; a slot at or
// past count is zero), so cv needs no memset and no scatter pass.  With lb == log_n this kernel runs
// the last stage and folds the entry's maximum in.
__global__ __launch_bounds__(256) void k_encb_fft_block(EncB P, size_t count, int is_complex, const u32 *inv_index,
                                                        double2 *cv, const double2 *roots, int log_n, int lb,
                                                        double scalar, unsigned long long *mx)
{
    __shared__ double2 sh[1 << kEncLogBlock];
    const int b = blockIdx.y;
    const size_t B = (size_t)1 << lb, base = (size_t)blockIdx.x << lb;
    const double *vals = P.vals[b];
    for (size_t t = threadIdx.x; t < B; t += 256)
    {
        const u32 w = inv_index[base + t];
        const size_t slot = w >> 1;
        double2 z = double2{ 0.0, 0.0 };
        if (slot < count)
        {
            const double re = is_complex ? vals[2 * slot] : vals[slot], im = is_complex ? vals[2 * slot + 1] : 0.0;
            z = double2{ re, (w & 1) ? -im : im };
        }
        sh[t] = z;
    }
    enc_block_stages(sh, roots, base, log_n, lb, scalar);
    cv += (size_t)b << log_n;
    for (size_t t = threadIdx.x; t < B; t += 256) cv[base + t] = sh[t];
    if (lb == log_n && ((P.check >> b) & 1)) // uniform per workgroup
    {
        unsigned long long m = 0;
        for (size_t t = threadIdx.x; t < B; t += 256) m = max(m, enc_abs_bits(sh[t].x));
        enc_max_fold(m, mx + b);
    }
}

// k_enc_fft_tail per entry; it always holds the last stage, so the entry's maximum is folded in
template <int LR>
__global__ __launch_bounds__(256) void k_encb_fft_tail(double2 *cv, const double2 *roots, int log_n, int lb,
                                                       double scalar, u32 check, unsigned long long *mx)
{
    constexpr int R = 1 << LR;
    const int b = blockIdx.y;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; // 2^lb is a multiple of 256: no partial workgroup
    cv += (size_t)b << log_n;
    double2 v[R];
#pragma unroll
    for (int j = 0; j < R; j++) v[j] = cv[c + ((size_t)j << lb)];
    enc_tail_stages<LR>(v, roots, log_n, lb, scalar);
    unsigned long long m = 0;
#pragma unroll
    for (int j = 0; j < R; j++)
    {
        cv[c + ((size_t)j << lb)] = v[j];
        m = max(m, enc_abs_bits(v[j].x));
    }
    if ((check >> b) & 1) enc_max_fold(m, mx + b);
}

// k_enc_round_reduce per entry.  A checked entry whose maximum is above max_ok (the bits of the
// largest double SEAL's size check accepts) is rejected: status 1 and its output is left alone.
// One lane writes the entry's status word (status may be null when no entry is checked).
__global__ void k_encb_round_reduce(EncB P, const double2 *cv, const PrimeDev *primes, int limbs, int log_n,
                                    const unsigned long long *mx, unsigned long long max_ok, u32 *status)
{
    const int b = blockIdx.y;
    const bool rejected = ((P.check >> b) & 1) && mx[b] > max_ok;
    if (status && blockIdx.x == 0 && threadIdx.x == 0) status[b] = rejected ? 1u : 0u;
    if (rejected) return;
    const size_t n = (size_t)1 << log_n;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n * limbs) return;
    P.out[b][g] = enc_residue(cv[((size_t)b << log_n) + (g & (n - 1))].x, primes[g >> log_n]);
}
} // namespace

extern "C" __attribute__((visibility("default"))) int mhe_encoder_create(mhe_encoder **out, int log_n)
{
    if (!out || log_n < 2 || log_n > 17) return mhe_internal_fail(MHE_ERR_ARG, "poly_modulus_degree is invalid");
    mhe_encoder *e = new mhe_encoder;
    const size_t n = size_t(1) << log_n, m = n << 1;
    e->log_n = log_n;
    e->n = n;
    e->slots = n >> 1;
    e->index_map.resize(n);
    u64 pos = 1;
    for (size_t i = 0; i < e->slots; i++)
    {
        const u64 index1 = (pos - 1) >> 1, index2 = (m - pos - 1) >> 1;
        e->index_map[i] = rev_bits((u32)index1, log_n);
        e->index_map[e->slots | i] = rev_bits((u32)index2, log_n);
        pos = (pos * 5) & (m - 1);
    }
    e->root_powers.assign(n, cd(0, 0));
    e->inv_root_powers.assign(n, cd(0, 0));
    ComplexRoots cr(m);
    for (size_t i = 1; i < n; i++)
    {
        e->root_powers[i] = cr.get(rev_bits((u32)i, log_n));
        e->inv_root_powers[i] = std::conj(cr.get(rev_bits((u32)(i - 1), log_n) + 1));
    }
    *out = e;
    return MHE_OK;
}

extern "C" __attribute__((visibility("default"))) int mhe_encoder_destroy(mhe_encoder *e)
{
    delete e;
    return MHE_OK;
}

extern "C" __attribute__((visibility("default"))) int mhe_ckks_encode_at(mhe_ctx *c, const mhe_encoder *e,
                                                                        const double *re, const double *im,
                                                                        size_t count, double scale, int bound_limbs,
                                                                        int limbs, uint64_t *out, void *stream)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (!e || e->log_n != log_n) return mhe_internal_fail(MHE_ERR_ARG, "encoder does not match the context");
    if (!re && count > 0) return mhe_internal_fail(MHE_ERR_ARG, "values cannot be null");
    if (count > e->slots) return mhe_internal_fail(MHE_ERR_ARG, "values_size is too large");
    if (limbs < 1 || limbs > bound_limbs || bound_limbs > K || !out)
        return mhe_internal_fail(MHE_ERR_ARG, "parms_id is not valid for encryption parameters");
    const int tb = total_bits(q, bound_limbs);
    if (scale <= 0 || (static_cast<int>(std::log2(scale)) + 1 >= tb)) return scale_fault(scale, bound_limbs, tb);
    const size_t n = e->n;
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return mhe_internal_fail(MHE_ERR_DEVICE, "no device");

    // host bound on max |coeff| (each value and its conjugate enter with unit-modulus weights)
    double l1 = 0;
    for (size_t i = 0; i < count; i++) l1 += std::fabs(re[i]) + (im ? std::fabs(im[i]) : 0.0);
    const double fix = scale / static_cast<double>(n);
    const bool exact_check = !l1_proves_size(fix, l1, tb);

    std::unique_lock<std::mutex> lk(e->mu);
    const double2 *roots = nullptr;
    if (int rc = device_roots(e, dev, &roots)) return rc;
    // staging: [cv: n double2][values: 2 * count doubles][max word]
    const size_t vwords = count * (im ? 2 : 1);
    char *buf = nullptr;
    const size_t bytes = n * sizeof(double2) + vwords * sizeof(double) + sizeof(u64);
    if (mhe_internal_alloc((void **)&buf, bytes, st) != hipSuccess)
        return mhe_internal_fail(MHE_ERR_MEMORY, "encode staging allocation failed");
    double2 *cv = (double2 *)buf;
    double *vals = (double *)(cv + n);
    unsigned long long *mx = (unsigned long long *)(vals + vwords);
    hipError_t err = hipMemsetAsync(cv, 0, n * sizeof(double2), st);
    if (err == hipSuccess && vwords)
    {
        if (e->ring_dev < 0)
        {
            if (hipHostMalloc((void **)&e->ring, mhe_encoder::kRing * 2 * e->slots * sizeof(double)) == hipSuccess)
            {
                e->ring_dev = dev;
                for (auto &ev : e->ring_ev)
                    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) e->ring_dev = -2;
            }
            else
                e->ring_dev = -2;
        }
        if (e->ring_dev == dev)
        {
            const unsigned slot = e->ring_next++ % mhe_encoder::kRing;
            double *h = e->ring + (size_t)slot * 2 * e->slots;
            err = hipEventSynchronize(e->ring_ev[slot]); // the slot's previous upload is done
            if (err == hipSuccess)
            {
                std::memcpy(h, re, count * sizeof(double));
                if (im) std::memcpy(h + count, im, count * sizeof(double));
                err = hipMemcpyAsync(vals, h, vwords * sizeof(double), hipMemcpyHostToDevice, st);
            }
            if (err == hipSuccess) err = hipEventRecord(e->ring_ev[slot], st);
        }
        else
        {
            // another device than the ring's: synchronous upload from the caller's arrays
            err = hipMemcpyAsync(vals, re, count * sizeof(double), hipMemcpyHostToDevice, st);
            if (err == hipSuccess && im)
                err = hipMemcpyAsync(vals + count, im, count * sizeof(double), hipMemcpyHostToDevice, st);
            if (err == hipSuccess) err = hipStreamSynchronize(st);
        }
    }
    lk.unlock();
    if (err == hipSuccess && count)
        hipLaunchKernelGGL(k_enc_scatter, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, vals, count,
                           im ? 1 : 0, cv, log_n);
    if (err == hipSuccess)
    {
        const int lb = std::min(log_n, kEncLogBlock);
        hipLaunchKernelGGL(k_enc_fft_block, dim3((unsigned)(n >> lb)), dim3(256), 0, st, cv, roots, log_n, lb, fix);
        const dim3 tg((unsigned)(((1u << lb) + 255) / 256));
        if (log_n - lb == 4)
            hipLaunchKernelGGL(k_enc_fft_tail<4>, tg, dim3(256), 0, st, cv, roots, log_n, lb, fix);
        else if (log_n - lb == 3)
            hipLaunchKernelGGL(k_enc_fft_tail<3>, tg, dim3(256), 0, st, cv, roots, log_n, lb, fix);
        else if (log_n - lb == 2)
            hipLaunchKernelGGL(k_enc_fft_tail<2>, tg, dim3(256), 0, st, cv, roots, log_n, lb, fix);
        else if (log_n - lb == 1)
            hipLaunchKernelGGL(k_enc_fft_tail<1>, tg, dim3(256), 0, st, cv, roots, log_n, lb, fix);
        else
            for (int s2 = lb; s2 < log_n; s2++)
                hipLaunchKernelGGL(k_enc_fft_stage, dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, st, cv, roots,
                                   log_n, s2, fix);
        err = hipGetLastError();
    }
    if (err == hipSuccess && exact_check)
    {
        // SEAL's check on the exact maximum (ckks.h:525-540)
        unsigned long long h_mx = 0;
        err = hipMemsetAsync(mx, 0, sizeof(u64), st);
        if (err == hipSuccess)
        {
            hipLaunchKernelGGL(k_enc_absmax, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cv, n, mx);
            err = hipMemcpyAsync(&h_mx, mx, sizeof(u64), hipMemcpyDeviceToHost, st);
        }
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err == hipSuccess)
        {
            double max_coeff;
            std::memcpy(&max_coeff, &h_mx, sizeof(double));
            if (!size_fits(max_coeff, tb))
            {
                (void)mhe_internal_free(buf, st);
                return mhe_internal_fail(MHE_ERR_ARG, "encoded values are too large");
            }
        }
    }
    if (err == hipSuccess)
    {
        const size_t total = n * limbs;
        hipLaunchKernelGGL(k_enc_round_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cv, out,
                           primes, limbs, log_n);
        err = hipGetLastError();
    }
    (void)mhe_internal_free(buf, st);
    if (err != hipSuccess) return mhe_internal_fail(MHE_ERR_DEVICE, hipGetErrorString(err));
    return mhe_internal_ntt_forward(c, out, 1, limbs, 1, st);
}

extern "C" __attribute__((visibility("default"))) int mhe_ckks_encode(mhe_ctx *c, const mhe_encoder *e,
                                                                     const double *re, const double *im,
                                                                     size_t count, double scale, int limbs,
                                                                     uint64_t *out, void *stream)
{
    return mhe_ckks_encode_at(c, e, re, im, count, scale, limbs, limbs, out, stream);
}

// 1 when mhe_ckks_encode_dev encodes an entry with this l1 bound unchecked, else 0 (host only)
extern "C" __attribute__((visibility("default"))) int mhe_ckks_encode_l1_proves(mhe_ctx *c, double scale,
                                                                               int bound_limbs, double l1)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (bound_limbs < 1 || bound_limbs > K)
        return mhe_internal_fail(MHE_ERR_ARG, "parms_id is not valid for encryption parameters");
    const double fix = scale / static_cast<double>((size_t)1 << log_n);
    return l1 >= 0 && l1_proves_size(fix, l1, total_bits(q, bound_limbs)) ? 1 : 0;
}

// CKKSEncoder::encode of `entries` vectors that are already in device memory, MHE_MAXB per round:
// per round one memset of the maxima (when an entry is checked), k_encb_fft_block, k_encb_fft_tail,
// k_encb_round_reduce and the two NTT passes.  Stream-ordered: nothing here waits for the device.
extern "C" __attribute__((visibility("default"))) int mhe_ckks_encode_dev(
    mhe_ctx *c, const mhe_encoder *e, int entries, const double *const *values_dev, size_t count, int is_complex,
    double scale, int bound_limbs, int limbs, uint64_t *const *out_dev, const double *l1_bounds, uint32_t *status_dev,
    void *stream)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (!e || e->log_n != log_n) return mhe_internal_fail(MHE_ERR_ARG, "encoder does not match the context");
    // the widest register tail is k_encb_fft_tail<4> (no context has a larger ring)
    if (log_n > kEncLogBlock + 4) return mhe_internal_fail(MHE_ERR_ARG, "poly_modulus_degree is invalid");
    if (entries < 1) return mhe_internal_fail(MHE_ERR_ARG, "entries must be at least 1");
    if (count > 0 && !values_dev) return mhe_internal_fail(MHE_ERR_ARG, "values cannot be null");
    for (int b = 0; b < entries && count > 0; b++)
        if (!values_dev[b]) return mhe_internal_fail(MHE_ERR_ARG, "values cannot be null");
    if (count > e->slots) return mhe_internal_fail(MHE_ERR_ARG, "values_size is too large");
    if (limbs < 1 || limbs > bound_limbs || bound_limbs > K || !out_dev)
        return mhe_internal_fail(MHE_ERR_ARG, "parms_id is not valid for encryption parameters");
    for (int b = 0; b < entries; b++)
        if (!out_dev[b]) return mhe_internal_fail(MHE_ERR_ARG, "parms_id is not valid for encryption parameters");
    const int tb = total_bits(q, bound_limbs);
    if (scale <= 0 || (static_cast<int>(std::log2(scale)) + 1 >= tb)) return scale_fault(scale, bound_limbs, tb);
    const size_t n = e->n;
    // every entry of a round runs inside the same launches: an output may share no byte with another
    // output or with any entry's values
    const size_t ob = (size_t)limbs * n * sizeof(u64), vb = count * (is_complex ? 2 : 1) * sizeof(double);
    for (int i = 0; i < entries; i++)
    {
        const char *o = (const char *)out_dev[i];
        for (int j = 0; j < entries; j++)
        {
            const char *o2 = (const char *)out_dev[j], *v = count ? (const char *)values_dev[j] : nullptr;
            if ((j != i && o < o2 + ob && o2 < o + ob) || (vb && o < v + vb && v < o + ob))
                return mhe_internal_fail(MHE_ERR_ARG, "encode output must not alias another output or an input");
        }
    }
    // entries whose l1 bound does not prove SEAL's size check are checked on the device
    const double fix = scale / static_cast<double>(n);
    std::vector<char> checked(entries);
    bool any_checked = false;
    for (int b = 0; b < entries; b++)
    {
        const bool known = l1_bounds && l1_bounds[b] >= 0; // false for NaN
        checked[b] = !(known && l1_proves_size(fix, l1_bounds[b], tb)); // mhe_ckks_encode_l1_proves
        any_checked |= checked[b] != 0;
    }
    if (any_checked && !status_dev)
        return mhe_internal_fail(MHE_ERR_ARG, "status_dev cannot be null when an entry needs the device size check");
    unsigned long long max_ok = 0;
    if (any_checked)
    {
        const double m = largest_fitting(tb);
        std::memcpy(&max_ok, &m, sizeof m);
    }

    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return mhe_internal_fail(MHE_ERR_DEVICE, "no device");
    const double2 *roots = nullptr;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        if (int rc = device_roots(e, dev, &roots)) return rc;
    }
    const u32 *inv_index = (const u32 *)(roots + 2 * n);
    // staging: [cv: n double2 per entry of a round][max words]; the rounds follow each other on st
    const int R = std::min(entries, MHE_MAXB);
    char *buf = nullptr;
    if (mhe_internal_alloc((void **)&buf, (size_t)R * n * sizeof(double2) + MHE_MAXB * sizeof(u64), st) != hipSuccess)
        return mhe_internal_fail(MHE_ERR_MEMORY, "encode staging allocation failed");
    double2 *cv = (double2 *)buf;
    unsigned long long *mx = (unsigned long long *)(cv + (size_t)R * n);
    const int lb = std::min(log_n, kEncLogBlock);
    const dim3 block(256);
    hipError_t err = hipSuccess;
    int rc = MHE_OK;
    for (int i0 = 0; i0 < entries && err == hipSuccess && rc == MHE_OK; i0 += MHE_MAXB)
    {
        const int B = std::min(MHE_MAXB, entries - i0);
        EncB P{};
        for (int b = 0; b < B; b++)
        {
            P.vals[b] = count ? values_dev[i0 + b] : nullptr;
            P.out[b] = out_dev[i0 + b];
            if (checked[i0 + b]) P.check |= 1u << b;
        }
        if (P.check && (err = hipMemsetAsync(mx, 0, MHE_MAXB * sizeof(u64), st)) != hipSuccess) break;
        hipLaunchKernelGGL(k_encb_fft_block, dim3((unsigned)(n >> lb), (unsigned)B), block, 0, st, P, count,
                           is_complex ? 1 : 0, inv_index, cv, roots, log_n, lb, fix, mx);
        const dim3 tg((unsigned)(((size_t)1 << lb) / 256), (unsigned)B);
        switch (log_n - lb)
        {
        case 0: break;
        case 1: hipLaunchKernelGGL(k_encb_fft_tail<1>, tg, block, 0, st, cv, roots, log_n, lb, fix, P.check, mx); break;
        case 2: hipLaunchKernelGGL(k_encb_fft_tail<2>, tg, block, 0, st, cv, roots, log_n, lb, fix, P.check, mx); break;
        case 3: hipLaunchKernelGGL(k_encb_fft_tail<3>, tg, block, 0, st, cv, roots, log_n, lb, fix, P.check, mx); break;
        default: hipLaunchKernelGGL(k_encb_fft_tail<4>, tg, block, 0, st, cv, roots, log_n, lb, fix, P.check, mx); break;
        }
        u32 *status = status_dev ? status_dev + i0 : nullptr;
        hipLaunchKernelGGL(k_encb_round_reduce, dim3((unsigned)((n * limbs + 255) / 256), (unsigned)B), block, 0, st, P,
                           cv, primes, limbs, log_n, mx, max_ok, status);
        err = hipGetLastError();
        if (err == hipSuccess) rc = mhe_internal_ntt_forward_entries(c, P.out, B, limbs, P.check ? status : nullptr, st);
    }
    (void)mhe_internal_free(buf, st);
    if (rc != MHE_OK) return rc;
    if (err != hipSuccess) return mhe_internal_fail(MHE_ERR_DEVICE, hipGetErrorString(err));
    return MHE_OK;
}

extern "C" __attribute__((visibility("default"))) int mhe_ckks_encode_scalar_at(mhe_ctx *c, double value, double scale,
                                                                               int bound_limbs, int limbs,
                                                                               uint64_t *residues)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (limbs < 1 || limbs > bound_limbs || bound_limbs > K || !residues)
        return mhe_internal_fail(MHE_ERR_ARG, "parms_id is not valid for encryption parameters");
    const int tb = total_bits(q, bound_limbs);
    if (scale <= 0 || (static_cast<int>(std::log2(scale)) >= tb)) return mhe_internal_fail(MHE_ERR_ARG, "scale out of bounds");
    value *= scale;
    const int coeff_bits = static_cast<int>(std::log2(std::fabs(value))) + 2;
    if (coeff_bits >= tb) return mhe_internal_fail(MHE_ERR_ARG, "encoded value is too large");
    const double two64 = std::pow(2.0, 64);
    double coeffd = std::round(value);
    const bool is_neg = std::signbit(coeffd);
    coeffd = std::fabs(coeffd);
    u64 w[64] = { 0 };
    int nw = 1;
    if (coeff_bits <= 64)
        w[0] = static_cast<u64>(std::fabs(coeffd));
    else if (coeff_bits <= 128)
    {
        w[0] = static_cast<u64>(std::fmod(coeffd, two64));
        w[1] = static_cast<u64>(coeffd / two64);
        nw = 2;
    }
    else
    {
        nw = 0;
        while (coeffd >= 1)
        {
            w[nw++] = static_cast<u64>(std::fmod(coeffd, two64));
            coeffd /= two64;
        }
        if (!nw) nw = 1;
    }
    for (int j = 0; j < limbs; j++)
    {
        const u64 r = words_mod(w, nw, q[j]);
        residues[j] = (is_neg && r) ? q[j] - r : r;
    }
    return MHE_OK;
}

extern "C" __attribute__((visibility("default"))) int mhe_ckks_encode_scalar(mhe_ctx *c, double value, double scale,
                                                                            int limbs, uint64_t *residues)
{
    return mhe_ckks_encode_scalar_at(c, value, scale, limbs, limbs, residues);
}

// ------------------------------------------------------------------------------------ decode
// CKKSEncoder::decode (ckks.h:644-761), all of it on the device and stream-ordered, in SEAL's
// operation order (this file is compiled with -ffp-contract=off, see the top):
//   * the inverse NTT of a copy of the plaintext;
//   * k_dec_compose: the sparse-slot mask (ckks.h:704-713), CRT composition
//     (RNSBase::compose_array, util/rns.cpp:354-400 -- its result is the canonical value in
//     [0, Q), so any exact composition gives SEAL's words; here sum_j [x_j (Q/q_j)^-1]_{q_j} Q/q_j
//     reduced mod Q after every term) and SEAL's word-by-word double conversion (ckks.h:715-753).
//     The multi-word accumulator lives in registers: the kernel is instantiated per word-count
//     class W = 1, 2, 4, ..., 64 >= limbs with every word loop unrolled, and the constants are
//     read with wave-uniform (scalar) loads;
//   * DWTHandler::transform_to_rev (util/dwthandler.h:94-190) over double2 with root_powers: the
//     first log_n - 12 stages (gap >= 4096) register-resident in one launch (k_dec_fft_head), the
//     last 12 inside 4096-point blocks in LDS (k_dec_fft_block), k_dec_fft_stage as the fallback;
//   * k_dec_gather: out[i] = res[index_map[i]] with the index map 5^i computed per slot.
// The RNS constants of a level are built on the host once per (encoder, device, primes of the
// level) and stay in device memory.
namespace
{
// a (L words) * s -> out (L words, truncated: every product here is < Q)
void mp_mul_scalar(const u64 *a, size_t L, u64 s, u64 *out)
{
    u64 carry = 0;
    for (size_t k = 0; k < L; k++)
    {
        const u128 p = (u128)a[k] * s + carry;
        out[k] = (u64)p;
        carry = (u64)(p >> 64);
    }
}

u64 inv_mod(u64 a, u64 q)
{
    // extended Euclid on signed 128-bit
    __int128 t = 0, nt = 1, r = q, nr = a % q;
    while (nr)
    {
        const __int128 qq = r / nr, tt = t - qq * nt, rr = r - qq * nr;
        t = nt;
        nt = tt;
        r = nr;
        nr = rr;
    }
    if (t < 0) t += q;
    return (u64)t;
}

// word-count class of a level: the smallest power of two >= limbs (limbs <= 64)
int dec_words(int limbs)
{
    int W = 1;
    while (W < limbs) W <<= 1;
    return W;
}

// Device constants of the level q_0..q_{L-1} (caller holds e->mu), u64 words:
// [Q: W][(Q+1)/2: W][(Q/q_j)^-1 mod q_j: L][Q/q_j: L x W], zero above a value's top word.
int dec_level(const mhe_encoder *e, int dev, const uint64_t *q, int limbs, const u64 **out)
{
    const size_t L = (size_t)limbs, W = (size_t)dec_words(limbs);
    for (auto &d : e->dec_levels)
        if (d.dev == dev && d.q.size() == L && std::memcmp(d.q.data(), q, L * sizeof(u64)) == 0)
        {
            *out = d.consts;
            return MHE_OK;
        }
    std::vector<u64> h(2 * W + L + L * W, 0), tmp(W);
    u64 *Q = &h[0], *thr = &h[W], *inv_punct = &h[2 * W], *punct = &h[2 * W + L];
    Q[0] = 1;
    for (size_t j = 0; j < L; j++)
    {
        mp_mul_scalar(Q, W, q[j], tmp.data());
        std::memcpy(Q, tmp.data(), W * sizeof(u64));
    }
    for (size_t j = 0; j < L; j++)
    {
        u64 *p = &punct[j * W];
        p[0] = 1;
        u64 pm = 1;
        for (size_t k = 0; k < L; k++)
        {
            if (k == j) continue;
            mp_mul_scalar(p, W, q[k], tmp.data());
            std::memcpy(p, tmp.data(), W * sizeof(u64));
            pm = (u64)(((u128)pm * (q[k] % q[j])) % q[j]);
        }
        inv_punct[j] = inv_mod(pm, q[j]);
    }
    std::memcpy(thr, Q, W * sizeof(u64));
    thr[0] += 1; // Q is odd: no carry out of word 0
    for (size_t k = 0; k < W; k++) thr[k] = (thr[k] >> 1) | (k + 1 < W ? thr[k + 1] << 63 : 0);
    u64 *d = nullptr;
    if (hipMalloc((void **)&d, h.size() * sizeof(u64)) != hipSuccess)
        return mhe_internal_fail(MHE_ERR_MEMORY, "decode constants allocation failed");
    if (hipMemcpy(d, h.data(), h.size() * sizeof(u64), hipMemcpyHostToDevice) != hipSuccess)
    {
        (void)hipFree(d);
        return mhe_internal_fail(MHE_ERR_DEVICE, "decode constants upload failed");
    }
    e->dec_levels.push_back({ dev, std::vector<uint64_t>(q, q + L), d });
    *out = d;
    return MHE_OK;
}

// cv[i] = (double(centred CRT value of coefficient i) / scale, 0), or exactly 0 under the sparse
// mask; x: coefficient-form residues [L][n], canonical.
template <int W>
__global__ __launch_bounds__(256) void k_dec_compose(const u64 *x, const u64 *consts, const PrimeDev *primes,
                                                     double2 *cv, int L, int log_n, size_t sparsity, double inv_scale)
{
    const size_t n = (size_t)1 << log_n, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (sparsity > 1 && ((i - 1) & (sparsity - 1)) != sparsity - 1) // i = 0 wraps, as in SEAL
    {
        cv[i] = double2{ 0.0, 0.0 };
        return;
    }
    const const_u64_p Q = (const_u64_p)consts, thr = Q + W, inv_punct = Q + 2 * W, punct = inv_punct + L;
    u64 acc[W];
    if (W == 1)
        acc[0] = x[i];
    else
    {
#pragma unroll
        for (int k = 0; k < W; k++) acc[k] = 0;
        for (int j = 0; j < L; j++)
        {
            const PrimeDev p = prime_at(primes, j);
            const u64 t = mulmod(x[(size_t)j * n + i], inv_punct[j], p);
            const const_u64_p pj = punct + (size_t)j * W;
            // acc += (Q/q_j) * t: both below Q, so the sum is below 2Q (one carry bit above W words)
            u64 carry = 0;
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                u64 lo, hi;
                mul128(pj[k], t, lo, hi);
                u64 s = acc[k] + lo;
                u64 cy = s < lo;
                s += carry;
                cy += s < carry;
                acc[k] = s;
                carry = hi + cy;
            }
            // acc -= Q when acc >= Q
            u64 borrow = 0;
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                const u64 qk = Q[k];
                borrow = (acc[k] < qk) | ((acc[k] == qk) & borrow);
            }
            const u64 mask = (carry | (borrow ^ 1)) ? ~(u64)0 : 0;
            borrow = 0;
#pragma unroll
            for (int k = 0; k < W; k++)
            {
                const u64 qk = Q[k] & mask;
                const u64 d = acc[k] - qk, b1 = acc[k] < qk;
                acc[k] = d - borrow;
                borrow = b1 | (d < borrow);
            }
        }
    }
    // ckks.h:715-753: negative when acc >= (Q+1)/2; every word in turn, zero words skipped
    u64 below = 0;
#pragma unroll
    for (int k = 0; k < W; k++)
    {
        const u64 tk = thr[k];
        below = (acc[k] < tk) | ((acc[k] == tk) & below);
    }
    double v = 0.0, s64 = inv_scale;
    if (!below)
    {
#pragma unroll
        for (int k = 0; k < W; k++)
            if (k < L)
            {
                const u64 qk = Q[k];
                if (acc[k] > qk)
                {
                    const u64 diff = acc[k] - qk;
                    v += diff ? static_cast<double>(diff) * s64 : 0.0;
                }
                else
                {
                    const u64 diff = qk - acc[k];
                    v -= diff ? static_cast<double>(diff) * s64 : 0.0;
                }
                s64 *= 0x1p64;
            }
    }
    else
    {
#pragma unroll
        for (int k = 0; k < W; k++)
            if (k < L)
            {
                v += acc[k] ? static_cast<double>(acc[k]) * s64 : 0.0;
                s64 *= 0x1p64;
            }
    }
    cv[i] = double2{ v, 0.0 };
}

// one butterfly of transform_to_rev: u = x, v = y * r, x = u + v, y = u - v, the complex product
// as (ac - bd, ad + bc) (no contraction)
__device__ __forceinline__ void dec_bfly(double2 &x, double2 &y, double2 r)
{
    const double2 u = x, v = double2{ y.x * r.x - y.y * r.y, y.x * r.y + y.y * r.x };
    x = double2{ u.x + v.x, u.y + v.y };
    y = double2{ u.x - v.x, u.y - v.y };
}

// Stage s of transform_to_rev has m = 2^s groups of gap n >> (s + 1); group g uses roots[m + g].

// stages 0 .. LR-1 (gap n/2 .. 2^lb, LR = log_n - lb) in one launch: they only pair elements with the
// same low lb bits, so a lane holds the 2^LR <= 16 elements of one such column in registers and runs
// the stages in order (the counterpart of k_enc_fft_tail)
template <int LR>
__global__ __launch_bounds__(256) void k_dec_fft_head(double2 *cv, const double2 *roots, int lb)
{
    constexpr int R = 1 << LR;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ((size_t)1 << lb)) return;
    double2 v[R];
#pragma unroll
    for (int j = 0; j < R; j++) v[j] = cv[c + ((size_t)j << lb)];
#pragma unroll
    for (int s = 0; s < LR; s++)
    {
        const int h = R >> (s + 1); // the stage's gap in column elements
#pragma unroll
        for (int j = 0; j < R; j++)
            if (!(j & h)) dec_bfly(v[j], v[j + h], roots[((size_t)1 << s) + (size_t)(j >> (LR - s))]);
    }
#pragma unroll
    for (int j = 0; j < R; j++) cv[c + ((size_t)j << lb)] = v[j];
}

// stages log_n-lb .. log_n-1 (gap 2^(lb-1) .. 1) of one 2^lb-point block in LDS (the counterpart
// of k_enc_fft_block)
__global__ __launch_bounds__(256) void k_dec_fft_block(double2 *cv, const double2 *roots, int log_n, int lb)
{
    __shared__ double2 sh[1 << kEncLogBlock];
    const size_t B = (size_t)1 << lb, base = (size_t)blockIdx.x << lb;
    for (size_t t = threadIdx.x; t < B; t += 256) sh[t] = cv[base + t];
    __syncthreads();
    for (int s2 = 0; s2 < lb; s2++)
    {
        const int sh_k = lb - 1 - s2; // log2 of the stage's gap
        const size_t gap = (size_t)1 << sh_k;
        const size_t first = ((size_t)1 << (log_n - lb + s2)) + ((size_t)blockIdx.x << s2); // root of the block's group 0
        for (size_t t = threadIdx.x; t < B / 2; t += 256)
        {
            const size_t k = t >> sh_k, xi = (k << (sh_k + 1)) + (t & (gap - 1));
            dec_bfly(sh[xi], sh[xi + gap], roots[first + k]);
        }
        __syncthreads();
    }
    for (size_t t = threadIdx.x; t < B; t += 256) cv[base + t] = sh[t];
}

// one stage s over the whole vector
__global__ void k_dec_fft_stage(double2 *cv, const double2 *roots, int log_n, int s)
{
    const size_t n = (size_t)1 << log_n, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n / 2) return;
    const int sh_k = log_n - 1 - s;
    const size_t gap = (size_t)1 << sh_k, k = t >> sh_k, xi = (k << (sh_k + 1)) + (t & (gap - 1));
    dec_bfly(cv[xi], cv[xi + gap], roots[((size_t)1 << s) + k]);
}

// out[i] = cv[index_map[i]], index_map[i] = rev((5^i mod 2n - 1) / 2) (ckks.cpp:34-49)
__global__ void k_dec_gather(const double2 *cv, double2 *out, size_t count, int log_n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const u64 m = (u64)2 << log_n;
    u64 pos = 1, b = 5;
    for (u64 e = i; e; e >>= 1)
    {
        if (e & 1) pos = (pos * b) & (m - 1);
        b = (b * b) & (m - 1);
    }
    out[i] = cv[rev_bits_dev((u32)((pos - 1) >> 1), log_n)];
}

struct DecodeCtx
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
};

// the argument checks of CKKSEncoder::decode; *sparse_slots 0 becomes n/2
int decode_check(mhe_ctx *c, const mhe_encoder *e, const uint64_t *plain, int limbs, double scale,
                 size_t *sparse_slots, const void *dest, DecodeCtx *d)
{
    if (mhe_internal_primes(c, &d->primes, &d->q, &d->K, &d->log_n))
        return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (!e || e->log_n != d->log_n) return mhe_internal_fail(MHE_ERR_ARG, "encoder does not match the context");
    if (limbs < 1 || limbs > d->K || !plain)
        return mhe_internal_fail(MHE_ERR_ARG, "plain is not valid for encryption parameters");
    if (!dest) return mhe_internal_fail(MHE_ERR_ARG, "destination cannot be null");
    if (!*sparse_slots) *sparse_slots = e->slots;
    if (*sparse_slots > e->slots || (*sparse_slots & (*sparse_slots - 1)))
        return mhe_internal_fail(MHE_ERR_ARG, "sparse_slots must be a power of two <= slots");
    if (scale <= 0 || static_cast<int>(std::log2(scale)) >= total_bits(d->q, limbs))
        return mhe_internal_fail(MHE_ERR_ARG, "scale out of bounds");
    return MHE_OK;
}

// checked arguments -> out_dev[sparse_slots] (re, im), enqueued on st
int decode_run(mhe_ctx *c, const mhe_encoder *e, const DecodeCtx &d, const uint64_t *plain, int limbs, double scale,
               size_t sparse_slots, double *out_dev, hipStream_t st)
{
    const size_t n = e->n, L = (size_t)limbs;
    const int log_n = d.log_n;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return mhe_internal_fail(MHE_ERR_DEVICE, "no device");
    const double2 *roots = nullptr;
    const u64 *consts = nullptr;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        if (int rc = device_roots(e, dev, &roots)) return rc;
        if (int rc = dec_level(e, dev, d.q, limbs, &consts)) return rc;
    }
    roots += n; // root_powers
    // staging: [x: L * n words][cv: n double2]
    char *buf = nullptr;
    if (mhe_internal_alloc((void **)&buf, n * L * sizeof(u64) + n * sizeof(double2), st) != hipSuccess)
        return mhe_internal_fail(MHE_ERR_MEMORY, "decode staging allocation failed");
    u64 *x = (u64 *)buf;
    double2 *cv = (double2 *)(x + n * L);
    hipError_t err = mhe_internal_copy_d2d(x, plain, n * L * sizeof(u64), st);
    int rc = err == hipSuccess ? mhe_ntt_inverse(c, x, 1, limbs, 0, st) : MHE_OK;
    if (err == hipSuccess && rc == MHE_OK)
    {
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        const size_t sparsity = e->slots / sparse_slots;
        const double inv_scale = 1.0 / scale;
        switch (dec_words(limbs))
        {
#define MHE_DEC_COMPOSE(w)                                                                                           \
    case w:                                                                                                          \
        hipLaunchKernelGGL(k_dec_compose<w>, grid, block, 0, st, x, consts, d.primes, cv, limbs, log_n, sparsity,    \
                           inv_scale);                                                                               \
        break;
            MHE_DEC_COMPOSE(1)
            MHE_DEC_COMPOSE(2)
            MHE_DEC_COMPOSE(4)
            MHE_DEC_COMPOSE(8)
            MHE_DEC_COMPOSE(16)
            MHE_DEC_COMPOSE(32)
            MHE_DEC_COMPOSE(64)
#undef MHE_DEC_COMPOSE
        }
        const int lb = std::min(log_n, kEncLogBlock);
        const dim3 hg((unsigned)(((1u << lb) + 255) / 256));
        if (log_n - lb == 4)
            hipLaunchKernelGGL(k_dec_fft_head<4>, hg, block, 0, st, cv, roots, lb);
        else if (log_n - lb == 3)
            hipLaunchKernelGGL(k_dec_fft_head<3>, hg, block, 0, st, cv, roots, lb);
        else if (log_n - lb == 2)
            hipLaunchKernelGGL(k_dec_fft_head<2>, hg, block, 0, st, cv, roots, lb);
        else if (log_n - lb == 1)
            hipLaunchKernelGGL(k_dec_fft_head<1>, hg, block, 0, st, cv, roots, lb);
        else
            for (int s = 0; s < log_n - lb; s++)
                hipLaunchKernelGGL(k_dec_fft_stage, dim3((unsigned)((n / 2 + 255) / 256)), block, 0, st, cv, roots, log_n,
                                   s);
        hipLaunchKernelGGL(k_dec_fft_block, dim3((unsigned)(n >> lb)), block, 0, st, cv, roots, log_n, lb);
        hipLaunchKernelGGL(k_dec_gather, dim3((unsigned)((sparse_slots + 255) / 256)), block, 0, st, cv,
                           (double2 *)out_dev, sparse_slots, log_n);
        err = hipGetLastError();
    }
    (void)mhe_internal_free(buf, st);
    if (rc != MHE_OK) return rc;
    if (err != hipSuccess) return mhe_internal_fail(MHE_ERR_DEVICE, hipGetErrorString(err));
    return MHE_OK;
}
} // namespace

extern "C" __attribute__((visibility("default"))) int mhe_ckks_decode_dev(mhe_ctx *c, const mhe_encoder *e,
                                                                         const uint64_t *plain, int limbs,
                                                                         double scale, size_t sparse_slots,
                                                                         double *out_dev, void *stream)
{
    DecodeCtx d;
    if (int rc = decode_check(c, e, plain, limbs, scale, &sparse_slots, out_dev, &d)) return rc;
    return decode_run(c, e, d, plain, limbs, scale, sparse_slots, out_dev, (hipStream_t)stream);
}

// mhe_ckks_decode_dev, then one download of the sparse_slots complex values
extern "C" __attribute__((visibility("default"))) int mhe_ckks_decode(mhe_ctx *c, const mhe_encoder *e,
                                                                     const uint64_t *plain, int limbs, double scale,
                                                                     size_t sparse_slots, double *re, double *im,
                                                                     void *stream)
{
    DecodeCtx d;
    if (int rc = decode_check(c, e, plain, limbs, scale, &sparse_slots, re, &d)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *out = nullptr;
    if (mhe_internal_alloc((void **)&out, 2 * sparse_slots * sizeof(double), st) != hipSuccess)
        return mhe_internal_fail(MHE_ERR_MEMORY, "decode staging allocation failed");
    std::vector<double> z(2 * sparse_slots);
    int rc = decode_run(c, e, d, plain, limbs, scale, sparse_slots, out, st);
    if (rc == MHE_OK)
    {
        hipError_t err = hipMemcpyAsync(z.data(), out, z.size() * sizeof(double), hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) rc = mhe_internal_fail(MHE_ERR_DEVICE, "decode transfer failed");
    }
    (void)mhe_internal_free(out, st);
    if (rc != MHE_OK) return rc;
    for (size_t i = 0; i < sparse_slots; i++)
    {
        re[i] = z[2 * i];
        if (im) im[i] = z[2 * i + 1];
    }
    return MHE_OK;
}

