// On-device sampling of the random polynomials of key generation and encryption, bit-identical
// to SEAL's samplers (SEAL/util/rlwe.cpp) fed by SEAL's default PRNG, Blake2xbPRNG
// (SEAL/randomgen.cpp:185-195): the PRNG stream is 4096-byte buffers, buffer c =
// BLAKE2Xb(out 4096, message = u64 counter c, key = the 64-byte seed).  Every 64-byte block of
// the stream is one independent BLAKE2b compression (csrc/blake2b.h), so a sampler that knows
// where its bytes sit in the stream computes them in parallel:
//
//   sample_poly_uniform (rlwe.cpp:136-162): the whole [limbs][n] u64 array is one bulk draw;
//     a word w >= max_multiple(q_l) is redrawn, in index order, from the words after the bulk.
//     The GPU draws the bulk, reduces the accepted words of the limbs the caller keeps and lists
//     the rejected indices (~q/2^64 of them); the host orders that list and assigns the
//     replacement words from the stream tail (mhe_prng_apply_fixes writes them).
//     mhe_prng_uniform_batch does all of it on the device for a batch of seeds (k_uni_bulk,
//     k_uni_redraw below): the bulk marks its rejects in a bit plane, which keeps their order, and
//     one workgroup per entry walks the tail limb by limb.  The redrawn words pass through a buffer
//     whose capacity the host works out from the primes (sample_cap.h: mean + 12 standard
//     deviations + 64 words).
//   sample_poly_ternary (rlwe.cpp:21-38): one std::uniform_int_distribution<u64>(0, 2) draw per
//     coefficient over a 32-bit adapter; libstdc++ 11 maps a 32-bit word g to (3g) >> 32
//     (Lemire, bits/uniform_int_dist.h:246-270) and redraws only when g == 0 (probability 2^-32
//     per coefficient): then one thread redoes the poly sequentially and records how many bytes the
//     redraws used, so the samples drawn after it (the CBD errors) start at the right byte -- all
//     on the stream, no host round trip.
//   sample_poly_cbd (rlwe.cpp:101-133): 6 bytes per coefficient, x[2], x[5] masked to 5 bits,
//     noise = pop(x0)+pop(x1)+pop(x2) - pop(x3)-pop(x4)-pop(x5).
// Small samples are written as canonical residues over every requested limb (rand + (flag & q));
// the batched encryption's samplers (k_enc_*) write one signed byte per coefficient instead.
#include <hip/hip_runtime.h>

#include "../../include/mhe.h"
#include "arith.h"
#include "blake2b.h"
#include "sample_cap.h"

int mhe_internal_fail(int code, const char *msg);
int mhe_internal_primes(mhe_ctx *c, const PrimeDev **dev, const uint64_t **host, int *count, int *log_n);
int mhe_internal_sample_scratch(mhe_ctx *c, hipStream_t st, size_t bytes, void **scratch, uint64_t **counters);
uint32_t mhe_internal_keygen_cap_limit(mhe_ctx *c);

namespace
{
struct Seed
{
    u64 w[8];
};

// limb l of the sampled array -> output limb slot (-1: not kept), max 64 limbs
struct LimbMap
{
    signed char slot[64];
    int prime[64]; // context prime index of limb l
};

// Every 64-byte block of a 4096-byte buffer is one compression of that buffer's XOF root, and a
// root costs two compressions, so a workgroup first computes the roots of the buffers its blocks
// fall in (threads 0 .. nb-1, into LDS) and every block then costs one compression.
constexpr int kMaxRoots = 8;

// roots of buffers [c0, c0 + nb) (nb <= kMaxRoots) into `roots`; a workgroup-wide barrier follows
__device__ __forceinline__ void load_roots(const Seed &s, u64 c0, int nb, u64 (*roots)[8])
{
    if ((int)threadIdx.x < nb)
    {
        u64 r[8];
        b2b::xof_root(s.w, c0 + threadIdx.x, b2b::kPrngBuffer, r);
#pragma unroll
        for (int k = 0; k < 8; k++) roots[threadIdx.x][k] = r[k];
    }
    __syncthreads();
}

// stream block `blk` from the workgroup's roots (buffer blk >> 6 must be in [c0, c0 + nb))
__device__ __forceinline__ void block_from_roots(const u64 (*roots)[8], u64 c0, u64 blk, u64 (&out)[8])
{
    u64 r[8];
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = roots[(blk >> 6) - c0][k];
    b2b::xof_block(r, (u32)(blk & 63), b2b::kPrngBuffer, 64, out);
}

// 64-byte stream block `blk` (= byte offset / 64) of the PRNG seeded with `s` (root included)
__device__ __forceinline__ void stream_block(const Seed &s, u64 blk, u64 (&out)[8])
{
    u64 root[8];
    b2b::xof_root(s.w, blk >> 6, b2b::kPrngBuffer, root);
    b2b::xof_block(root, (u32)(blk & 63), b2b::kPrngBuffer, 64, out);
}

// Bulk of sample_poly_uniform over `limbs` limbs: one thread per 64-byte block (8 words), a
// workgroup's 256 blocks in 4 buffers.
__global__ __launch_bounds__(256) void k_prng_uniform(Seed s, LimbMap map, u64 *out, const PrimeDev *primes, int limbs,
                                                      int log_n, u64 *rej, u32 *rej_count, u32 rej_cap)
{
    __shared__ u64 roots[kMaxRoots][8];
    const u64 b0 = (u64)blockIdx.x * 256, blk = b0 + threadIdx.x;
    const u64 total = (u64)limbs << log_n;
    const u64 last = ((total / 8 < b0 + 256) ? total / 8 : b0 + 256) - 1;
    load_roots(s, b0 >> 6, (int)((last >> 6) - (b0 >> 6) + 1), roots);
    if (blk * 8 >= total) return;
    u64 w[8];
    block_from_roots(roots, b0 >> 6, blk, w);
#pragma unroll
    for (int k = 0; k < 8; k++)
    {
        const u64 g = blk * 8 + k;
        const int l = (int)(g >> log_n);
        const PrimeDev p = primes[map.prime[l]];
        // max_multiple = (2^64 - 1) - barrett_reduce_64(2^64 - 1, q) - 1 (rlwe.cpp:152)
        const u64 mm = ~0ULL - barrett64(~0ULL, p) - 1;
        if (w[k] >= mm)
        {
            const u32 at = atomicAdd(rej_count, 1u);
            if (at < rej_cap) rej[at] = g;
        }
        else if (map.slot[l] >= 0)
            out[((u64)map.slot[l] << log_n) + (g & (((u64)1 << log_n) - 1))] = barrett64(w[k], p);
    }
}

__global__ void k_prng_apply(const u64 *fix, u32 count, u64 *out)
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[fix[2 * i]] = fix[2 * i + 1];
}

// sample_poly_ternary: coefficients [0, n) from the stream bytes at byte offset `off` (64-aligned).
// A workgroup owns 256 stream blocks (4096 coefficients): one thread per block draws its 16 values
// into LDS, then the workgroup writes them coalesced to the limbs blockIdx.y, blockIdx.y +
// gridDim.y, ... (every y redraws the same values; the limbs split keeps the grid wide).  A zero word
// would be redrawn (Lemire); those are counted in state[1] (by y == 0) and k_prng_ternary_fix redoes
// the poly sequentially.
__global__ __launch_bounds__(256) void k_prng_ternary(Seed s, u64 off, u64 *out, const PrimeDev *primes, int limbs,
                                                      int log_n, u32 *state)
{
    __shared__ u64 roots[kMaxRoots][8];
    __shared__ unsigned char val[256 * 16];
    const u64 n = (u64)1 << log_n;
    const u64 nblk = n / 16, wb0 = (u64)blockIdx.x * 256;
    const u64 wg_end = (wb0 + 256 < nblk ? wb0 + 256 : nblk);
    const u64 first = (off >> 6) + wb0, last = (off >> 6) + wg_end - 1;
    load_roots(s, first >> 6, (int)((last >> 6) - (first >> 6) + 1), roots);
    if (wb0 + threadIdx.x < wg_end)
    {
        u64 w[8];
        block_from_roots(roots, first >> 6, first + threadIdx.x, w);
#pragma unroll
        for (int k = 0; k < 16; k++)
        {
            const u32 g = (u32)(w[k >> 1] >> (32 * (k & 1)));
            if (g == 0 && blockIdx.y == 0) atomicAdd(&state[1], 1u);
            val[threadIdx.x * 16 + k] = (unsigned char)(((u64)g * 3) >> 32); // {0, 1, 2} -> {-1, 0, 1}
        }
    }
    __syncthreads();
    const u32 cnt = (u32)((wg_end - wb0) * 16);
    for (int l = blockIdx.y; l < limbs; l += gridDim.y)
    {
        const u64 q = primes[l].q;
        u64 *o = out + ((u64)l << log_n) + wb0 * 16;
        for (u32 i = threadIdx.x; i < cnt; i += 256)
        {
            const u32 r = val[i];
            o[i] = r == 0 ? q - 1 : r - 1;
        }
    }
}

// The rare redraw path of sample_poly_ternary (probability ~ n 2^-32 per poly): one thread walks
// the stream 4 bytes at a time, skipping zero words as libstdc++ 11's uniform_int_distribution
// does for a 32-bit URBG (threshold 2^32 mod 3 = 1), and records in state[0] how many bytes the
// redraws consumed, which moves the offsets of the samples drawn after it.
__global__ void k_prng_ternary_fix(Seed s, u64 off, u64 *out, const PrimeDev *primes, int limbs, int log_n,
                                   u32 *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (state[1] == 0)
    {
        state[0] = 0;
        return;
    }
    const u64 n = (u64)1 << log_n;
    u64 pos = off, cached = ~0ULL, w[8];
    for (u64 i = 0; i < n; i++)
    {
        u32 g;
        do
        {
            const u64 blk = pos >> 6;
            if (blk != cached)
            {
                stream_block(s, blk, w);
                cached = blk;
            }
            g = (u32)(w[(pos & 63) >> 3] >> (32 * ((pos >> 2) & 1)));
            pos += 4;
        } while (g == 0);
        const u64 r = ((u64)g * 3) >> 32;
        for (int l = 0; l < limbs; l++)
        {
            const u64 q = primes[l].q;
            out[((u64)l << log_n) + i] = r == 0 ? q - 1 : r - 1;
        }
    }
    state[0] = (u32)(pos - off - 4 * n);
}

// sample_poly_cbd: coefficients [0, n) from the bytes at offset off + (*extra when given), a
// multiple of 4.  A workgroup owns kCbdCoeffs coefficients (6 bytes each): it computes the roots
// of the <= 3 buffers and the <= 97 stream blocks those bytes span into LDS (one compression per
// block), forms the noise values in LDS, and writes them coalesced to the limbs blockIdx.y,
// blockIdx.y + gridDim.y, ... (as k_prng_ternary).
constexpr int kCbdCoeffs = 1024;
constexpr int kCbdBlocks = (6 * kCbdCoeffs) / 64 + 1;
__global__ __launch_bounds__(256) void k_prng_cbd(Seed s, u64 off, const u32 *extra, u64 *out, const PrimeDev *primes,
                                                  int limbs, int log_n)
{
    __shared__ u64 roots[kMaxRoots][8];
    __shared__ u64 bytes[kCbdBlocks * 8];
    __shared__ signed char noise[kCbdCoeffs];
    const u64 n = (u64)1 << log_n;
    const u64 c0 = (u64)blockIdx.x * kCbdCoeffs;
    const u64 cnt = (n - c0) < (u64)kCbdCoeffs ? (n - c0) : (u64)kCbdCoeffs;
    const u64 start = off + (extra ? extra[0] : 0) + 6 * c0;
    const u64 b0 = start >> 6, b1 = (start + 6 * cnt - 1) >> 6;
    load_roots(s, b0 >> 6, (int)((b1 >> 6) - (b0 >> 6) + 1), roots);
    if (threadIdx.x <= b1 - b0)
    {
        u64 w[8];
        block_from_roots(roots, b0 >> 6, b0 + threadIdx.x, w);
#pragma unroll
        for (int k = 0; k < 8; k++) bytes[threadIdx.x * 8 + k] = w[k];
    }
    __syncthreads();
    const u32 skip = (u32)(start - 64 * b0);
    auto byte_at = [&](u32 i) -> u32 {
        i += skip;
        return (u32)(bytes[i >> 3] >> (8 * (i & 7))) & 0xff;
    };
    for (u32 k = threadIdx.x; k < cnt; k += 256)
    {
        const u32 c = 6 * k;
        noise[k] = (signed char)(__popc(byte_at(c)) + __popc(byte_at(c + 1)) + __popc(byte_at(c + 2) & 0x1f) -
                                 __popc(byte_at(c + 3)) - __popc(byte_at(c + 4)) - __popc(byte_at(c + 5) & 0x1f));
    }
    __syncthreads();
    for (int l = blockIdx.y; l < limbs; l += gridDim.y)
    {
        const u64 q = primes[l].q;
        u64 *o = out + ((u64)l << log_n) + c0;
        for (u32 k = threadIdx.x; k < cnt; k += 256)
        {
            const int v = noise[k];
            o[k] = v >= 0 ? (u64)v : q - (u64)(-v);
        }
    }
}

// ------------------------------------------------------------------ batched encryption samples
// The three small polys of a public-key encryption (encrypt_zero_asymmetric, rlwe.cpp:220-286) for a
// batch of entries, one signed byte per coefficient: small[entry][3][n], entries `pitch` bytes apart,
// = u (ternary, stream byte 0), e_0 and e_1 (CBD, bytes 4n and 10n plus what the entry's ternary
// redraws consumed).  The residues
// mod each prime are expanded where they are used (jobs.h, the encryption jobs).  The entry comes
// from the grid; its seed and its redraw state[entry][2] (as k_prng_ternary's) are its own.
constexpr int MHE_SAMPLE_MAXB = 8; // entries per launch: ntt.h MHE_MAXB (encrypt.h asserts it fits)
struct SeedB
{
    Seed s[MHE_SAMPLE_MAXB];
};

// k_prng_ternary for entry blockIdx.y: a thread's 16 values leave as one 16-byte store.
__global__ __launch_bounds__(256) void k_enc_ternary(SeedB sb, signed char *small, size_t pitch, int log_n, u32 *state)
{
    __shared__ u64 roots[kMaxRoots][8];
    const int ent = blockIdx.y;
    const u64 n = (u64)1 << log_n;
    const u64 nblk = n / 16, wb0 = (u64)blockIdx.x * 256;
    const u64 wg_end = (wb0 + 256 < nblk ? wb0 + 256 : nblk);
    load_roots(sb.s[ent], wb0 >> 6, (int)(((wg_end - 1) >> 6) - (wb0 >> 6) + 1), roots);
    if (wb0 + threadIdx.x >= wg_end) return;
    u64 w[8];
    block_from_roots(roots, wb0 >> 6, wb0 + threadIdx.x, w);
    u32 pk[4] = { 0, 0, 0, 0 }, zeros = 0;
#pragma unroll
    for (int k = 0; k < 16; k++)
    {
        const u32 g = (u32)(w[k >> 1] >> (32 * (k & 1)));
        zeros += g == 0;
        const u32 v = (u32)(((u64)g * 3) >> 32) - 1u; // {0, 1, 2} -> {-1, 0, 1}
        pk[k >> 2] |= (v & 0xffu) << (8 * (k & 3));
    }
    if (zeros) atomicAdd(&state[2 * ent + 1], zeros);
    uint4 *o = reinterpret_cast<uint4 *>(small + (size_t)ent * pitch) + wb0 + threadIdx.x;
    *o = make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

// k_prng_ternary_fix per entry (workgroup = entry): returns at once for an entry without a zero word.
__global__ void k_enc_ternary_fix(SeedB sb, signed char *small, size_t pitch, int log_n, u32 *state)
{
    const int ent = blockIdx.x;
    if (threadIdx.x != 0) return;
    if (state[2 * ent + 1] == 0)
    {
        state[2 * ent] = 0;
        return;
    }
    const u64 n = (u64)1 << log_n;
    signed char *o = small + (size_t)ent * pitch;
    u64 pos = 0, cached = ~0ULL, w[8];
    for (u64 i = 0; i < n; i++)
    {
        u32 g;
        do
        {
            const u64 blk = pos >> 6;
            if (blk != cached)
            {
                stream_block(sb.s[ent], blk, w);
                cached = blk;
            }
            g = (u32)(w[(pos & 63) >> 3] >> (32 * ((pos >> 2) & 1)));
            pos += 4;
        } while (g == 0);
        o[i] = (signed char)((int)(((u64)g * 3) >> 32) - 1);
    }
    state[2 * ent] = (u32)(pos - 4 * n);
}

// k_prng_cbd's noise values of coefficients [c0, c0 + cnt) (cnt <= kCbdCoeffs, a multiple of 4) from
// the stream bytes at `start` on, one signed byte each: a thread's 4 values leave as one dword of o.
__device__ __forceinline__ void cbd_bytes_wg(const Seed &s, u64 start, u64 cnt, u32 *o)
{
    __shared__ u64 roots[kMaxRoots][8];
    __shared__ u64 bytes[kCbdBlocks * 8];
    const u64 b0 = start >> 6, b1 = (start + 6 * cnt - 1) >> 6;
    load_roots(s, b0 >> 6, (int)((b1 >> 6) - (b0 >> 6) + 1), roots);
    if (threadIdx.x <= b1 - b0)
    {
        u64 w[8];
        block_from_roots(roots, b0 >> 6, b0 + threadIdx.x, w);
#pragma unroll
        for (int k = 0; k < 8; k++) bytes[threadIdx.x * 8 + k] = w[k];
    }
    __syncthreads();
    const u32 skip = (u32)(start - 64 * b0);
    auto byte_at = [&](u32 i) -> u32 {
        i += skip;
        return (u32)(bytes[i >> 3] >> (8 * (i & 7))) & 0xff;
    };
    if (4 * threadIdx.x >= cnt) return;
    u32 pk = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        const u32 c = 6 * (4 * threadIdx.x + k);
        const int v = __popc(byte_at(c)) + __popc(byte_at(c + 1)) + __popc(byte_at(c + 2) & 0x1f) -
                      __popc(byte_at(c + 3)) - __popc(byte_at(c + 4)) - __popc(byte_at(c + 5) & 0x1f);
        pk |= ((u32)v & 0xffu) << (8 * k);
    }
    o[threadIdx.x] = pk;
}

// k_prng_cbd for error poly j = blockIdx.y of entry blockIdx.z, from byte 4n + 6n j + the entry's
// extra bytes.
__global__ __launch_bounds__(256) void k_enc_cbd(SeedB sb, signed char *small, size_t pitch, int log_n, const u32 *state)
{
    const int j = blockIdx.y, ent = blockIdx.z;
    const u64 n = (u64)1 << log_n;
    const u64 c0 = (u64)blockIdx.x * kCbdCoeffs;
    const u64 cnt = (n - c0) < (u64)kCbdCoeffs ? (n - c0) : (u64)kCbdCoeffs; // a multiple of 4
    const u64 start = 4 * n + 6 * n * (u64)j + state[2 * ent] + 6 * c0;
    cbd_bytes_wg(sb.s[ent], start, cnt, reinterpret_cast<u32 *>(small + (size_t)ent * pitch + (size_t)(1 + j) * n + c0));
}

// The error of a symmetric encryption (encrypt_zero_symmetric, rlwe.cpp:289-373) of entry blockIdx.y:
// CBD from stream byte 64 (the first 64 bytes seed the PRNG of a), plane small + entry * pitch.
__global__ __launch_bounds__(256) void k_sk_cbd(SeedB sb, signed char *small, size_t pitch, int log_n)
{
    const int ent = blockIdx.y;
    const u64 n = (u64)1 << log_n;
    const u64 c0 = (u64)blockIdx.x * kCbdCoeffs;
    const u64 cnt = (n - c0) < (u64)kCbdCoeffs ? (n - c0) : (u64)kCbdCoeffs;
    cbd_bytes_wg(sb.s[ent], 64 + 6 * c0, cnt, reinterpret_cast<u32 *>(small + (size_t)ent * pitch + c0));
}

// ------------------------------------------------------ sample_poly_uniform, all on the device
// For a batch of entries (seed, output) that share the limb maps.  state[entry][2] (zeroed before the
// bulk): [0] nonzero when the bulk rejected a word, [1] nonzero when the redraw buffer overflowed.
struct UniB
{
    Seed s[MHE_SAMPLE_MAXB];
    u64 *out[MHE_SAMPLE_MAXB];
};

// k_prng_uniform for entry blockIdx.y.  Thread t of a workgroup owns words 8t .. 8t+7 of the
// workgroup's 2048 (all in one limb: n >= 8) and leaves their reject bits as byte `blk` of the entry's
// bit plane: bit g of the plane is word g of the stream, so the plane holds the rejects in stream order.
__global__ __launch_bounds__(256) void k_uni_bulk(UniB ub, LimbMap map, const PrimeDev *primes, int limbs, int log_n,
                                                  unsigned char *flags, size_t flag_pitch, u32 *state)
{
    __shared__ u64 roots[kMaxRoots][8];
    const int ent = blockIdx.y;
    const u64 b0 = (u64)blockIdx.x * 256, blk = b0 + threadIdx.x;
    const u64 total = (u64)limbs << log_n;
    const u64 last = ((total / 8 < b0 + 256) ? total / 8 : b0 + 256) - 1;
    load_roots(ub.s[ent], b0 >> 6, (int)((last >> 6) - (b0 >> 6) + 1), roots);
    if (blk * 8 >= total) return;
    u64 w[8];
    block_from_roots(roots, b0 >> 6, blk, w);
    const int l = (int)((blk * 8) >> log_n);
    const PrimeDev p = primes[map.prime[l]];
    const u64 mm = ~0ULL - barrett64(~0ULL, p) - 1; // max_multiple (rlwe.cpp:152)
    const int slot = map.slot[l];
    u64 *o = ub.out[ent] + ((u64)(slot < 0 ? 0 : slot) << log_n) + ((blk * 8) & (((u64)1 << log_n) - 1));
    u32 rej = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
    {
        if (w[k] >= mm)
            rej |= 1u << k;
        else if (slot >= 0)
            o[k] = barrett64(w[k], p);
    }
    flags[(size_t)ent * flag_pitch + blk] = (unsigned char)rej;
    if (rej) state[2 * ent] = 1; // every writer stores the same word
}

// Exclusive prefix sum of v over the workgroup's 256 threads (thread order); total = the sum.
__device__ __forceinline__ u32 wg_excl_scan(u32 v, u32 *sh, u32 &total)
{
    // four waves of 64 lanes (gfx950)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u32 x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const u32 y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) sh[wv] = x;
    __syncthreads();
    u32 off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
        const u32 s = sh[i];
        off += i < wv ? s : 0;
        tot += s;
    }
    __syncthreads(); // sh is free again
    total = tot;
    return off + x - v;
}

// The redraws of sample_poly_uniform (rlwe.cpp:153-157) for entry blockIdx.x, one workgroup: returns
// at once when the bulk rejected nothing (SEAL's own primes in practice).  The rejects are consumed in
// stream order, so limb by limb, and max_multiple changes only between limbs.  Per limb:
//   need   = the set bits of the limb's part of the bit plane;
//   draw   the first `need` tail words below the limb's max_multiple, 2048 tail words per round (a
//          thread per stream block, a workgroup scan for their ranks), into val[rank]; the tail
//          position moves past the last word taken, so a word rejected here is skipped for good;
//   apply  (kept limbs) the plane again, 2048 bits per round: the r-th set bit of the limb takes
//          val[rank0 + r].
// A rank at or beyond cap is neither written nor read: the entry's flag is raised and counted.
// counters: [0] redrawn words, [1] overflowed entries (device totals, mhe_keygen_stats).
__global__ __launch_bounds__(256) void k_uni_redraw(UniB ub, LimbMap map, const PrimeDev *primes, int limbs, int log_n,
                                                    const unsigned char *flags, size_t flag_pitch, u64 *val,
                                                    size_t val_pitch, u32 cap, u32 *state,
                                                    unsigned long long *counters)
{
    const int ent = blockIdx.x, tid = threadIdx.x;
    if (state[2 * ent] == 0) return; // uniform per workgroup
    __shared__ u64 roots[kMaxRoots][8];
    __shared__ u32 sh[4];
    __shared__ u64 s_last;
    const Seed &seed = ub.s[ent];
    const unsigned char *fl = flags + (size_t)ent * flag_pitch;
    u64 *vals = val + (size_t)ent * val_pitch;
    const u32 n8 = 1u << (log_n - 3); // plane bytes per limb
    u64 pos = (u64)limbs << log_n;    // next tail word
    u32 rank0 = 0;
    for (int l = 0; l < limbs; l++)
    {
        const unsigned char *fll = fl + (size_t)l * n8;
        u32 c = 0, need;
        for (u32 i = tid; i < n8; i += 256) c += __popc(fll[i]);
        wg_excl_scan(c, sh, need);
        if (need == 0) continue;
        const PrimeDev p = primes[map.prime[l]];
        const u64 mm = ~0ULL - barrett64(~0ULL, p) - 1;
        u32 got = 0;
        while (got < need)
        {
            // blocks b0 .. b0 + 255 span at most 5 buffers
            const u64 b0 = pos >> 3, blk = b0 + tid;
            load_roots(seed, b0 >> 6, (int)(((b0 + 255) >> 6) - (b0 >> 6) + 1), roots);
            u64 w[8];
            block_from_roots(roots, b0 >> 6, blk, w);
            u32 ok = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) ok |= (blk * 8 + k >= pos && w[k] < mm) ? 1u << k : 0;
            u32 taken;
            u32 a = got + wg_excl_scan(__popc(ok), sh, taken);
#pragma unroll
            for (int k = 0; k < 8; k++)
                if ((ok >> k) & 1)
                {
                    if (a < need)
                    {
                        if (rank0 + a < cap) vals[rank0 + a] = barrett64(w[k], p);
                        if (a == need - 1) s_last = blk * 8 + k;
                    }
                    a++;
                }
            __syncthreads(); // s_last, and the roots before the next round replaces them
            if (got + taken >= need)
            {
                pos = s_last + 1;
                got = need;
            }
            else
            {
                pos = (b0 + 256) << 3;
                got += taken;
            }
            __syncthreads(); // s_last is read before a later round writes it
        }
        const int slot = map.slot[l];
        if (slot >= 0)
        {
            // the barriers above order this workgroup's stores to vals before these loads
            u64 *o = ub.out[ent] + ((u64)slot << log_n);
            u32 base = rank0;
            for (u32 c0 = 0; c0 < n8; c0 += 256)
            {
                const u32 i = c0 + tid;
                const u32 f = i < n8 ? fll[i] : 0;
                u32 cnt;
                u32 r = base + wg_excl_scan(__popc(f), sh, cnt);
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if ((f >> k) & 1)
                    {
                        if (r < cap) o[(u64)i * 8 + k] = vals[r];
                        r++;
                    }
                base += cnt;
            }
        }
        rank0 += need;
    }
    if (tid == 0)
    {
        atomicAdd(&counters[0], (unsigned long long)rank0);
        if (rank0 > cap)
        {
            state[2 * ent + 1] = 1;
            atomicAdd(&counters[1], 1ull);
        }
    }
}

int launch_check(const char *what)
{
    if (hipGetLastError() != hipSuccess) return mhe_internal_fail(MHE_ERR_DEVICE, what);
    return MHE_OK;
}
} // namespace

#define MHE_EXPORT extern "C" __attribute__((visibility("default")))

// The samples of B <= MHE_SAMPLE_MAXB encryptions (encrypt.h): small [B][3][n] signed bytes, entry e at
// small + e * pitch (both multiples of 16), state [B][2] device words.  Three launches and one memset,
// no host synchronisation.
int mhe_internal_encrypt_samples(mhe_ctx *c, int B, const uint64_t (*seeds)[8], signed char *small, uint32_t *state,
                                 size_t pitch, hipStream_t st)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (!seeds || !small || !state || B < 1 || B > MHE_SAMPLE_MAXB || log_n < 5 || (((uintptr_t)small | pitch) & 15) ||
        (B > 1 && pitch < 3 * ((size_t)1 << log_n)))
        return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
    SeedB sb{};
    for (int e = 0; e < B; e++)
        for (int i = 0; i < 8; i++) sb.s[e].w[i] = seeds[e][i];
    const u64 n = (u64)1 << log_n;
    if (hipMemsetAsync(state, 0, 8 * (size_t)B, st) != hipSuccess)
        return mhe_internal_fail(MHE_ERR_DEVICE, "sampling state reset failed");
    hipLaunchKernelGGL(k_enc_ternary, dim3((unsigned)((n / 16 + 255) / 256), (unsigned)B), dim3(256), 0, st, sb, small,
                       pitch, log_n, state);
    hipLaunchKernelGGL(k_enc_ternary_fix, dim3((unsigned)B), dim3(64), 0, st, sb, small, pitch, log_n, state);
    hipLaunchKernelGGL(k_enc_cbd, dim3((unsigned)((n + kCbdCoeffs - 1) / kCbdCoeffs), 2, (unsigned)B), dim3(256), 0, st,
                       sb, small, pitch, log_n, (const u32 *)state);
    return launch_check("sampling kernel launch failed");
}

// Scratch of the on-device sample_poly_uniform for B entries: state [MHE_SAMPLE_MAXB][2] words, then
// per entry a reject bit plane of limbs * n bits and `cap` redrawn words (sample_cap.h).
namespace
{
struct UniLayout
{
    size_t flag_pitch, flags_at, val_at, bytes;
    u32 cap;
};
UniLayout uni_layout(mhe_ctx *c, const uint64_t *q, int B, int limbs, const int *prime_of_limb, int log_n)
{
    UniLayout u;
    u.cap = uniform_redraw_cap(q, prime_of_limb, limbs, (size_t)1 << log_n);
    const u32 limit = mhe_internal_keygen_cap_limit(c); // mhe_debug_keygen_cap: the overflow side under test
    if (limit && limit < u.cap) u.cap = limit;
    u.flag_pitch = ((((size_t)limbs << log_n) / 8) + 255) & ~(size_t)255;
    u.flags_at = 256;
    u.val_at = u.flags_at + (size_t)B * u.flag_pitch;
    u.bytes = u.val_at + (size_t)B * u.cap * sizeof(u64);
    return u;
}
bool uni_maps_ok(int K, int log_n, int limbs, const int *prime_of_limb, const int *slot_of_limb)
{
    if (!prime_of_limb || !slot_of_limb || limbs < 1 || limbs > 64 || log_n < 5) return false;
    for (int l = 0; l < limbs; l++)
        if (prime_of_limb[l] < 0 || prime_of_limb[l] >= K || slot_of_limb[l] < -1 || slot_of_limb[l] > 63) return false;
    return true;
}
} // namespace

size_t mhe_internal_uniform_scratch_bytes(mhe_ctx *c, int B, int limbs, const int *prime_of_limb)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return 0;
    return uni_layout(c, q, B, limbs, prime_of_limb, log_n).bytes;
}

// sample_poly_uniform of B <= MHE_SAMPLE_MAXB entries into out[e] (the maps checked by the caller,
// scratch of mhe_internal_uniform_scratch_bytes for at least B entries): the state reset and two launches.
int mhe_internal_uniform_group(mhe_ctx *c, int B, const uint64_t (*seeds)[8], int limbs, const int *prime_of_limb,
                               const int *slot_of_limb, uint64_t *const *out, void *scratch, uint64_t *counters,
                               hipStream_t st)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (B < 1 || B > MHE_SAMPLE_MAXB || !scratch || !counters)
        return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
    const UniLayout u = uni_layout(c, q, B, limbs, prime_of_limb, log_n);
    UniB ub{};
    LimbMap m;
    for (int e = 0; e < B; e++)
    {
        for (int i = 0; i < 8; i++) ub.s[e].w[i] = seeds[e][i];
        ub.out[e] = out[e];
    }
    for (int l = 0; l < 64; l++)
    {
        m.slot[l] = l < limbs ? (signed char)slot_of_limb[l] : -1;
        m.prime[l] = l < limbs ? prime_of_limb[l] : 0;
    }
    u32 *state = static_cast<u32 *>(scratch);
    unsigned char *flags = static_cast<unsigned char *>(scratch) + u.flags_at;
    u64 *val = reinterpret_cast<u64 *>(static_cast<unsigned char *>(scratch) + u.val_at);
    if (hipMemsetAsync(state, 0, 8 * (size_t)MHE_SAMPLE_MAXB, st) != hipSuccess)
        return mhe_internal_fail(MHE_ERR_DEVICE, "sampling state reset failed");
    const u64 blocks = ((u64)limbs << log_n) / 8;
    hipLaunchKernelGGL(k_uni_bulk, dim3((unsigned)((blocks + 255) / 256), (unsigned)B), dim3(256), 0, st, ub, m, primes,
                       limbs, log_n, flags, u.flag_pitch, state);
    hipLaunchKernelGGL(k_uni_redraw, dim3((unsigned)B), dim3(256), 0, st, ub, m, primes, limbs, log_n,
                       (const unsigned char *)flags, u.flag_pitch, val, (size_t)u.cap, u.cap, state,
                       reinterpret_cast<unsigned long long *>(counters));
    return launch_check("uniform sampling kernel launch failed");
}

// The error planes of B symmetric encryptions (keygen.h): small + e * pitch, n signed bytes each.
int mhe_internal_sk_errors(mhe_ctx *c, int B, const uint64_t (*seeds)[8], signed char *small, size_t pitch, hipStream_t st)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (!seeds || !small || B < 1 || B > MHE_SAMPLE_MAXB || log_n < 5 || (((uintptr_t)small | pitch) & 3) ||
        (B > 1 && pitch < ((size_t)1 << log_n)))
        return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
    SeedB sb{};
    for (int e = 0; e < B; e++)
        for (int i = 0; i < 8; i++) sb.s[e].w[i] = seeds[e][i];
    const u64 n = (u64)1 << log_n;
    hipLaunchKernelGGL(k_sk_cbd, dim3((unsigned)((n + kCbdCoeffs - 1) / kCbdCoeffs), (unsigned)B), dim3(256), 0, st, sb,
                       small, pitch, log_n);
    return launch_check("sampling kernel launch failed");
}

MHE_EXPORT int mhe_prng_uniform_batch(mhe_ctx *c, int count, const uint64_t (*seeds)[8], int limbs,
                                      const int *prime_of_limb, const int *slot_of_limb, uint64_t *const *out,
                                      void *stream)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (count < 1 || !seeds || !out || !uni_maps_ok(K, log_n, limbs, prime_of_limb, slot_of_limb))
        return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
    for (int i = 0; i < count; i++)
        if (!out[i]) return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
    hipStream_t st = (hipStream_t)stream;
    const int Bmax = count < MHE_SAMPLE_MAXB ? count : MHE_SAMPLE_MAXB;
    void *scratch;
    uint64_t *counters;
    int r = mhe_internal_sample_scratch(c, st, uni_layout(c, q, Bmax, limbs, prime_of_limb, log_n).bytes, &scratch, &counters);
    if (r) return r;
    for (int b0 = 0; b0 < count; b0 += MHE_SAMPLE_MAXB)
    {
        const int B = count - b0 < MHE_SAMPLE_MAXB ? count - b0 : MHE_SAMPLE_MAXB;
        if ((r = mhe_internal_uniform_group(c, B, seeds + b0, limbs, prime_of_limb, slot_of_limb, out + b0, scratch,
                                            counters, st)))
            return r;
    }
    return MHE_OK;
}

MHE_EXPORT int mhe_prng_uniform_bulk(mhe_ctx *c, const uint64_t seed[8], int limbs, const int *prime_of_limb,
                                     const int *slot_of_limb, uint64_t *out, uint64_t *rej, uint32_t *rej_count,
                                     uint32_t rej_cap, void *stream)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (!seed || !prime_of_limb || !slot_of_limb || !out || !rej || !rej_count || limbs < 1 || limbs > 64)
        return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
    Seed s;
    LimbMap m;
    for (int i = 0; i < 8; i++) s.w[i] = seed[i];
    for (int l = 0; l < 64; l++)
    {
        m.slot[l] = l < limbs ? (signed char)slot_of_limb[l] : -1;
        m.prime[l] = l < limbs ? prime_of_limb[l] : 0;
        if (l < limbs && (prime_of_limb[l] < 0 || prime_of_limb[l] >= K))
            return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
    }
    hipStream_t st = (hipStream_t)stream;
    const u64 blocks = ((u64)limbs << log_n) / 8;
    hipLaunchKernelGGL(k_prng_uniform, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, s, m, out, primes,
                       limbs, log_n, rej, rej_count, rej_cap);
    return launch_check("uniform sampling kernel launch failed");
}

MHE_EXPORT int mhe_prng_apply_fixes(mhe_ctx *c, const uint64_t *fixes_dev, uint32_t count, uint64_t *out, void *stream)
{
    if (!c || (count && (!fixes_dev || !out))) return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
    if (!count) return MHE_OK;
    hipLaunchKernelGGL(k_prng_apply, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, fixes_dev, count,
                       out);
    return launch_check("sampling fix-up launch failed");
}

MHE_EXPORT int mhe_prng_small(mhe_ctx *c, const uint64_t seed[8], uint64_t byte_offset, int kind, int limbs,
                              uint64_t *out, uint32_t *state_dev, void *stream)
{
    const PrimeDev *primes;
    const uint64_t *q;
    int K, log_n;
    if (mhe_internal_primes(c, &primes, &q, &K, &log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    if (!seed || !out || limbs < 1 || limbs > K || (byte_offset & 63) || log_n < 5)
        return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
    Seed s;
    for (int i = 0; i < 8; i++) s.w[i] = seed[i];
    hipStream_t st = (hipStream_t)stream;
    const u64 n = (u64)1 << log_n;
    if (kind == MHE_SAMPLE_TERNARY)
    {
        if (!state_dev) return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
        if (hipMemsetAsync(state_dev, 0, 8, st) != hipSuccess)
            return mhe_internal_fail(MHE_ERR_DEVICE, "sampling state reset failed");
        hipLaunchKernelGGL(k_prng_ternary, dim3((unsigned)((n / 16 + 255) / 256), (unsigned)(limbs < 8 ? limbs : 8)),
                           dim3(256), 0, st, s, byte_offset, out, primes, limbs, log_n, state_dev);
        hipLaunchKernelGGL(k_prng_ternary_fix, dim3(1), dim3(64), 0, st, s, byte_offset, out, primes, limbs, log_n,
                           state_dev);
    }
    else if (kind == MHE_SAMPLE_CBD)
        hipLaunchKernelGGL(k_prng_cbd, dim3((unsigned)((n + kCbdCoeffs - 1) / kCbdCoeffs), (unsigned)(limbs < 4 ? limbs : 4)),
                           dim3(256), 0, st, s, byte_offset, (const u32 *)state_dev, out, primes, limbs, log_n);
    else
        return mhe_internal_fail(MHE_ERR_ARG, "unknown distribution");
    return launch_check("sampling kernel launch failed");
}
