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
// Each sampler has two kernels, which differ only in where a value goes: the single-seed kernels
// (k_prng_*) write canonical residues over every requested limb (rand + (flag & q)), the batched ones
// (k_enc_*, k_sk_cbd, k_uni_bulk; the entry comes from the grid) one signed byte per coefficient, or
// the uniform words with a bit plane of the rejects.  What is computed exists once, in the device
// functions both kernels of a pair call (ternary_wg, ternary_walk, cbd_bytes_wg, expand_residues,
// uniform_bulk_wg); a kernel keeps its addressing and its store.
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

// A batch of entries, at most MHE_SAMPLE_MAXB per launch: the entry comes from the grid; its seed, its
// plane of signed bytes (small + entry * pitch) and its state words are its own.
constexpr int MHE_SAMPLE_MAXB = 8; // ntt.h MHE_MAXB (encrypt.h asserts it fits)
struct SeedB
{
    Seed s[MHE_SAMPLE_MAXB];
};
struct UniB
{
    SeedB sb;
    u64 *out[MHE_SAMPLE_MAXB];
};

// a small signed value as a canonical residue mod q
__device__ __forceinline__ u64 small_residue(int v, u64 q)
{
    return v >= 0 ? (u64)v : q - (u64)(-v);
}

// Signed bytes val[0, cnt) in LDS as residues of limbs blockIdx.y, blockIdx.y + gridDim.y, ... (every
// y computes the same values; the limbs split keeps the grid wide), coalesced; `out` is the
// workgroup's first coefficient in limb 0.
__device__ __forceinline__ void expand_residues(const signed char *val, u32 cnt, u64 *out, const PrimeDev *primes,
                                                int limbs, int log_n)
{
    for (int l = blockIdx.y; l < limbs; l += gridDim.y)
    {
        const u64 q = primes[l].q;
        u64 *o = out + ((u64)l << log_n);
        for (u32 i = threadIdx.x; i < cnt; i += 256) o[i] = small_residue(val[i], q);
    }
}

// ------------------------------------------------------------------------ sample_poly_ternary
// libstdc++ 11's uniform_int_distribution(0, 2) of a nonzero 32-bit word (Lemire), less one
__device__ __forceinline__ int ternary_of(u32 g)
{
    return (int)(((u64)g * 3) >> 32) - 1;
}

// Coefficients [0, n) from the stream bytes at byte offset `off` (64-aligned).  Workgroup blockIdx.x
// owns 256 stream blocks (4096 coefficients) and thread t the 16 values of block t of those: they
// come back as signed bytes in pk, with the number of zero words among the 16 -- those would be
// redrawn, so a poly that has one is redone by ternary_walk.  False: the block is past the poly.
__device__ __forceinline__ bool ternary_wg(const Seed &s, u64 off, int log_n, u32 (&pk)[4], u32 &zeros)
{
    __shared__ u64 roots[kMaxRoots][8];
    const u64 nblk = ((u64)1 << log_n) / 16, wb0 = (u64)blockIdx.x * 256;
    const u64 wg_end = (wb0 + 256 < nblk ? wb0 + 256 : nblk);
    const u64 first = (off >> 6) + wb0, last = (off >> 6) + wg_end - 1;
    load_roots(s, first >> 6, (int)((last >> 6) - (first >> 6) + 1), roots);
    if (wb0 + threadIdx.x >= wg_end) return false;
    u64 w[8];
    block_from_roots(roots, first >> 6, first + threadIdx.x, w);
    zeros = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) pk[k] = 0;
#pragma unroll
    for (int k = 0; k < 16; k++)
    {
        const u32 g = (u32)(w[k >> 1] >> (32 * (k & 1)));
        zeros += g == 0;
        pk[k >> 2] |= ((u32)ternary_of(g) & 0xffu) << (8 * (k & 3));
    }
    return true;
}

// Residues over `limbs` limbs; the zero words are counted in state[1] (by y == 0).
__global__ __launch_bounds__(256) void k_prng_ternary(Seed s, u64 off, u64 *out, const PrimeDev *primes, int limbs,
                                                      int log_n, u32 *state)
{
    __shared__ uint4 val[256];
    u32 pk[4], zeros;
    if (ternary_wg(s, off, log_n, pk, zeros))
    {
        if (zeros && blockIdx.y == 0) atomicAdd(&state[1], zeros);
        val[threadIdx.x] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    }
    __syncthreads();
    const u64 n = (u64)1 << log_n, c0 = (u64)blockIdx.x * 4096;
    expand_residues(reinterpret_cast<const signed char *>(val), (u32)((n - c0) < 4096 ? (n - c0) : 4096), out + c0,
                    primes, limbs, log_n);
}

// u of entry blockIdx.y (stream byte 0): a thread's 16 values leave as one 16-byte store; the zero
// words are counted in state[entry][1].
__global__ __launch_bounds__(256) void k_enc_ternary(SeedB sb, signed char *small, size_t pitch, int log_n, u32 *state)
{
    const int ent = blockIdx.y;
    u32 pk[4], zeros;
    if (!ternary_wg(sb.s[ent], 0, log_n, pk, zeros)) return;
    if (zeros) atomicAdd(&state[2 * ent + 1], zeros);
    uint4 *o = reinterpret_cast<uint4 *>(small + (size_t)ent * pitch) + (u64)blockIdx.x * 256 + threadIdx.x;
    *o = make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

// The rare redraw path (probability ~ n 2^-32 per poly): one thread walks the stream 4 bytes at a
// time from byte `off`, skipping zero words as libstdc++ 11's uniform_int_distribution does for a
// 32-bit URBG (threshold 2^32 mod 3 = 1), and hands value i to put(i, v).  Returns how many bytes
// the redraws consumed, which moves the offsets of the samples drawn after this one.
template <class Put>
__device__ __forceinline__ u32 ternary_walk(const Seed &s, u64 off, u64 n, Put put)
{
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
        put(i, ternary_of(g));
    }
    return (u32)(pos - off - 4 * n);
}

// Both fix kernels return at once for a poly without a zero word (state[1] == 0) and leave the bytes
// consumed in state[0].
__global__ void k_prng_ternary_fix(Seed s, u64 off, u64 *out, const PrimeDev *primes, int limbs, int log_n,
                                   u32 *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (state[1] == 0)
    {
        state[0] = 0;
        return;
    }
    state[0] = ternary_walk(s, off, (u64)1 << log_n, [&](u64 i, int v) {
        for (int l = 0; l < limbs; l++) out[((u64)l << log_n) + i] = small_residue(v, primes[l].q);
    });
}

// workgroup = entry
__global__ void k_enc_ternary_fix(SeedB sb, signed char *small, size_t pitch, int log_n, u32 *state)
{
    const int ent = blockIdx.x;
    if (threadIdx.x != 0) return;
    if (state[2 * ent + 1] == 0)
    {
        state[2 * ent] = 0;
        return;
    }
    signed char *o = small + (size_t)ent * pitch;
    state[2 * ent] = ternary_walk(sb.s[ent], 0, (u64)1 << log_n, [&](u64 i, int v) { o[i] = (signed char)v; });
}

// ---------------------------------------------------------------------------- sample_poly_cbd
// A workgroup owns kCbdCoeffs coefficients (6 bytes each): it computes the roots of the <= 3 buffers
// and the <= 97 stream blocks those bytes span into LDS (one compression per block).
constexpr int kCbdCoeffs = 1024;
constexpr int kCbdBlocks = (6 * kCbdCoeffs) / 64 + 1;

// Workgroup blockIdx.x's noise values, coefficients [c0, c0 + cnt) of a poly whose bytes start at
// stream byte `first` (a multiple of 4), one signed byte each: a thread's 4 values leave as one dword
// of o (global or LDS).  Returns cnt, a multiple of 4: n is a power of two from 2^12 to 2^16 in every
// context, and the entry points refuse n < 32.
__device__ __forceinline__ u32 cbd_bytes_wg(const Seed &s, u64 first, int log_n, u32 *o)
{
    __shared__ u64 roots[kMaxRoots][8];
    __shared__ u64 bytes[kCbdBlocks * 8];
    const u64 n = (u64)1 << log_n, c0 = (u64)blockIdx.x * kCbdCoeffs;
    const u32 cnt = (u32)((n - c0) < (u64)kCbdCoeffs ? (n - c0) : (u64)kCbdCoeffs);
    const u64 start = first + 6 * c0;
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
    if (4 * threadIdx.x >= cnt) return cnt;
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
    return cnt;
}

// Residues over `limbs` limbs, from the bytes at off + (*extra when given).
__global__ __launch_bounds__(256) void k_prng_cbd(Seed s, u64 off, const u32 *extra, u64 *out, const PrimeDev *primes,
                                                  int limbs, int log_n)
{
    __shared__ u32 noise[kCbdCoeffs / 4];
    const u32 cnt = cbd_bytes_wg(s, off + (extra ? extra[0] : 0), log_n, noise);
    __syncthreads();
    expand_residues(reinterpret_cast<const signed char *>(noise), cnt, out + (u64)blockIdx.x * kCbdCoeffs, primes, limbs,
                    log_n);
}

// The errors of a public-key encryption (encrypt_zero_asymmetric, rlwe.cpp:220-286): small[entry][3][n]
// = u (k_enc_ternary), e_0, e_1; e_j (j = blockIdx.y) of entry blockIdx.z from byte 4n + 6n j + what
// the entry's ternary redraws consumed.  The residues mod each prime are expanded where they are used
// (jobs.h, the encryption jobs).
__global__ __launch_bounds__(256) void k_enc_cbd(SeedB sb, signed char *small, size_t pitch, int log_n, const u32 *state)
{
    const int j = blockIdx.y, ent = blockIdx.z;
    const u64 n = (u64)1 << log_n;
    signed char *e = small + (size_t)ent * pitch + (size_t)(1 + j) * n;
    cbd_bytes_wg(sb.s[ent], 4 * n + 6 * n * (u64)j + state[2 * ent], log_n,
                 reinterpret_cast<u32 *>(e + (size_t)blockIdx.x * kCbdCoeffs));
}

// The error of a symmetric encryption (encrypt_zero_symmetric, rlwe.cpp:289-373) of entry blockIdx.y:
// from stream byte 64 (the first 64 bytes seed the PRNG of a), plane small + entry * pitch.
__global__ __launch_bounds__(256) void k_sk_cbd(SeedB sb, signed char *small, size_t pitch, int log_n)
{
    signed char *e = small + (size_t)blockIdx.y * pitch;
    cbd_bytes_wg(sb.s[blockIdx.y], 64, log_n, reinterpret_cast<u32 *>(e + (size_t)blockIdx.x * kCbdCoeffs));
}

// ------------------------------------------------------------------------ sample_poly_uniform
// max_multiple = (2^64 - 1) - barrett_reduce_64(2^64 - 1, q) - 1 (rlwe.cpp:152)
__device__ __forceinline__ u64 max_multiple(const PrimeDev &p)
{
    return ~0ULL - barrett64(~0ULL, p) - 1;
}

// The bulk over `limbs` limbs: one thread per 64-byte stream block `blk` (8 words, all in one limb:
// n >= 8), a workgroup's 256 blocks in 4 buffers.  A word below its limb's max_multiple is reduced into
// the limb's slot of `out` when the limb is kept; the others are bits of rej (bit k: word 8 blk + k).
// False: the block is past the bulk.
__device__ __forceinline__ bool uniform_bulk_wg(const Seed &s, const LimbMap &map, u64 *out, const PrimeDev *primes,
                                                int limbs, int log_n, u64 &blk, u32 &rej)
{
    __shared__ u64 roots[kMaxRoots][8];
    const u64 b0 = (u64)blockIdx.x * 256;
    const u64 total = (u64)limbs << log_n;
    const u64 last = ((total / 8 < b0 + 256) ? total / 8 : b0 + 256) - 1;
    load_roots(s, b0 >> 6, (int)((last >> 6) - (b0 >> 6) + 1), roots);
    blk = b0 + threadIdx.x;
    if (blk * 8 >= total) return false;
    u64 w[8];
    block_from_roots(roots, b0 >> 6, blk, w);
    const int l = (int)((blk * 8) >> log_n);
    const PrimeDev p = primes[map.prime[l]];
    const u64 mm = max_multiple(p);
    const int slot = map.slot[l];
    u64 *o = out + ((u64)(slot < 0 ? 0 : slot) << log_n) + ((blk * 8) & (((u64)1 << log_n) - 1));
    rej = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
    {
        if (w[k] >= mm)
            rej |= 1u << k;
        else if (slot >= 0)
            o[k] = barrett64(w[k], p);
    }
    return true;
}

// The rejected indices go to a list of at most rej_cap entries, in no order (the host sorts it);
// rej_count counts them all.
__global__ __launch_bounds__(256) void k_prng_uniform(Seed s, LimbMap map, u64 *out, const PrimeDev *primes, int limbs,
                                                      int log_n, u64 *rej, u32 *rej_count, u32 rej_cap)
{
    u64 blk;
    u32 m;
    if (!uniform_bulk_wg(s, map, out, primes, limbs, log_n, blk, m)) return;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if ((m >> k) & 1)
        {
            const u32 at = atomicAdd(rej_count, 1u);
            if (at < rej_cap) rej[at] = blk * 8 + k;
        }
}

__global__ void k_prng_apply(const u64 *fix, u32 count, u64 *out)
{
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[fix[2 * i]] = fix[2 * i + 1];
}

// All of sample_poly_uniform on the device, for a batch of entries (seed, output) that share the limb
// maps.  state[entry][2] (zeroed before the bulk): [0] nonzero when the bulk rejected a word, [1]
// nonzero when the redraw buffer overflowed.  Entry blockIdx.y's reject bits are byte `blk` of its bit
// plane: bit g of the plane is word g of the stream, so the plane holds the rejects in stream order.
__global__ __launch_bounds__(256) void k_uni_bulk(UniB ub, LimbMap map, const PrimeDev *primes, int limbs, int log_n,
                                                  unsigned char *flags, size_t flag_pitch, u32 *state)
{
    const int ent = blockIdx.y;
    u64 blk;
    u32 rej;
    if (!uniform_bulk_wg(ub.sb.s[ent], map, ub.out[ent], primes, limbs, log_n, blk, rej)) return;
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
    const Seed &seed = ub.sb.s[ent];
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
        const u64 mm = max_multiple(p);
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

// ---------------------------------------------------------------------------------- host side
int bad_args()
{
    return mhe_internal_fail(MHE_ERR_ARG, "invalid sampling arguments");
}

int launch_check(const char *what)
{
    if (hipGetLastError() != hipSuccess) return mhe_internal_fail(MHE_ERR_DEVICE, what);
    return MHE_OK;
}

// what a sampler needs of the context
struct Primes
{
    const PrimeDev *dev;
    const uint64_t *q;
    int K, log_n;
};
int primes_of(mhe_ctx *c, Primes &P)
{
    if (mhe_internal_primes(c, &P.dev, &P.q, &P.K, &P.log_n)) return mhe_internal_fail(MHE_ERR_ARG, "context is not valid");
    return MHE_OK;
}

Seed seed_of(const uint64_t w[8])
{
    Seed s;
    for (int i = 0; i < 8; i++) s.w[i] = w[i];
    return s;
}
SeedB seeds_of(int B, const uint64_t (*seeds)[8])
{
    SeedB sb{};
    for (int e = 0; e < B; e++) sb.s[e] = seed_of(seeds[e]);
    return sb;
}

// the maps of `limbs` sampled limbs over a context of K primes into m; false when they are not valid
bool limb_map(int K, int limbs, const int *prime_of_limb, const int *slot_of_limb, LimbMap &m)
{
    if (!prime_of_limb || !slot_of_limb || limbs < 1 || limbs > 64) return false;
    for (int l = 0; l < 64; l++)
    {
        if (l < limbs && (prime_of_limb[l] < 0 || prime_of_limb[l] >= K || slot_of_limb[l] < -1 || slot_of_limb[l] > 63))
            return false;
        m.slot[l] = l < limbs ? (signed char)slot_of_limb[l] : -1;
        m.prime[l] = l < limbs ? prime_of_limb[l] : 0;
    }
    return true;
}

// Scratch of the on-device sample_poly_uniform for B entries: state [MHE_SAMPLE_MAXB][2] words, then
// per entry a reject bit plane of limbs * n bits and `cap` redrawn words (sample_cap.h).
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
} // namespace

#define MHE_EXPORT extern "C" __attribute__((visibility("default")))

// The samples of B <= MHE_SAMPLE_MAXB encryptions (encrypt.h): small [B][3][n] signed bytes, entry e at
// small + e * pitch (both multiples of 16), state [B][2] device words.  Three launches and one memset,
// no host synchronisation.
int mhe_internal_encrypt_samples(mhe_ctx *c, int B, const uint64_t (*seeds)[8], signed char *small, uint32_t *state,
                                 size_t pitch, hipStream_t st)
{
    Primes P;
    if (int r = primes_of(c, P)) return r;
    const int log_n = P.log_n;
    if (!seeds || !small || !state || B < 1 || B > MHE_SAMPLE_MAXB || log_n < 5 || (((uintptr_t)small | pitch) & 15) ||
        (B > 1 && pitch < 3 * ((size_t)1 << log_n)))
        return bad_args();
    const SeedB sb = seeds_of(B, seeds);
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

size_t mhe_internal_uniform_scratch_bytes(mhe_ctx *c, int B, int limbs, const int *prime_of_limb)
{
    Primes P;
    if (primes_of(c, P)) return 0;
    return uni_layout(c, P.q, B, limbs, prime_of_limb, P.log_n).bytes;
}

// sample_poly_uniform of B <= MHE_SAMPLE_MAXB entries into out[e] (scratch of
// mhe_internal_uniform_scratch_bytes for at least B entries): the state reset and two launches.
int mhe_internal_uniform_group(mhe_ctx *c, int B, const uint64_t (*seeds)[8], int limbs, const int *prime_of_limb,
                               const int *slot_of_limb, uint64_t *const *out, void *scratch, uint64_t *counters,
                               hipStream_t st)
{
    Primes P;
    if (int r = primes_of(c, P)) return r;
    LimbMap m;
    if (B < 1 || B > MHE_SAMPLE_MAXB || !scratch || !counters || !limb_map(P.K, limbs, prime_of_limb, slot_of_limb, m))
        return bad_args();
    const int log_n = P.log_n;
    const UniLayout u = uni_layout(c, P.q, B, limbs, prime_of_limb, log_n);
    UniB ub{ seeds_of(B, seeds), {} };
    for (int e = 0; e < B; e++) ub.out[e] = out[e];
    u32 *state = static_cast<u32 *>(scratch);
    unsigned char *flags = static_cast<unsigned char *>(scratch) + u.flags_at;
    u64 *val = reinterpret_cast<u64 *>(static_cast<unsigned char *>(scratch) + u.val_at);
    if (hipMemsetAsync(state, 0, 8 * (size_t)MHE_SAMPLE_MAXB, st) != hipSuccess)
        return mhe_internal_fail(MHE_ERR_DEVICE, "sampling state reset failed");
    const u64 blocks = ((u64)limbs << log_n) / 8;
    hipLaunchKernelGGL(k_uni_bulk, dim3((unsigned)((blocks + 255) / 256), (unsigned)B), dim3(256), 0, st, ub, m, P.dev,
                       limbs, log_n, flags, u.flag_pitch, state);
    hipLaunchKernelGGL(k_uni_redraw, dim3((unsigned)B), dim3(256), 0, st, ub, m, P.dev, limbs, log_n,
                       (const unsigned char *)flags, u.flag_pitch, val, (size_t)u.cap, u.cap, state,
                       reinterpret_cast<unsigned long long *>(counters));
    return launch_check("uniform sampling kernel launch failed");
}

// The error planes of B symmetric encryptions (keygen.h): small + e * pitch, n signed bytes each.
int mhe_internal_sk_errors(mhe_ctx *c, int B, const uint64_t (*seeds)[8], signed char *small, size_t pitch, hipStream_t st)
{
    Primes P;
    if (int r = primes_of(c, P)) return r;
    const int log_n = P.log_n;
    if (!seeds || !small || B < 1 || B > MHE_SAMPLE_MAXB || log_n < 5 || (((uintptr_t)small | pitch) & 3) ||
        (B > 1 && pitch < ((size_t)1 << log_n)))
        return bad_args();
    const u64 n = (u64)1 << log_n;
    hipLaunchKernelGGL(k_sk_cbd, dim3((unsigned)((n + kCbdCoeffs - 1) / kCbdCoeffs), (unsigned)B), dim3(256), 0, st,
                       seeds_of(B, seeds), small, pitch, log_n);
    return launch_check("sampling kernel launch failed");
}

MHE_EXPORT int mhe_prng_uniform_batch(mhe_ctx *c, int count, const uint64_t (*seeds)[8], int limbs,
                                      const int *prime_of_limb, const int *slot_of_limb, uint64_t *const *out,
                                      void *stream)
{
    Primes P;
    if (int r = primes_of(c, P)) return r;
    LimbMap m; // filled again per group
    if (count < 1 || !seeds || !out || P.log_n < 5 || !limb_map(P.K, limbs, prime_of_limb, slot_of_limb, m))
        return bad_args();
    for (int i = 0; i < count; i++)
        if (!out[i]) return bad_args();
    hipStream_t st = (hipStream_t)stream;
    const int Bmax = count < MHE_SAMPLE_MAXB ? count : MHE_SAMPLE_MAXB;
    void *scratch;
    uint64_t *counters;
    int r = mhe_internal_sample_scratch(c, st, uni_layout(c, P.q, Bmax, limbs, prime_of_limb, P.log_n).bytes, &scratch,
                                        &counters);
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
    Primes P;
    if (int r = primes_of(c, P)) return r;
    LimbMap m;
    if (!seed || !out || !rej || !rej_count || !limb_map(P.K, limbs, prime_of_limb, slot_of_limb, m)) return bad_args();
    const u64 blocks = ((u64)limbs << P.log_n) / 8;
    hipLaunchKernelGGL(k_prng_uniform, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       seed_of(seed), m, out, P.dev, limbs, P.log_n, rej, rej_count, rej_cap);
    return launch_check("uniform sampling kernel launch failed");
}

MHE_EXPORT int mhe_prng_apply_fixes(mhe_ctx *c, const uint64_t *fixes_dev, uint32_t count, uint64_t *out, void *stream)
{
    if (!c || (count && (!fixes_dev || !out))) return bad_args();
    if (!count) return MHE_OK;
    hipLaunchKernelGGL(k_prng_apply, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, fixes_dev, count,
                       out);
    return launch_check("sampling fix-up launch failed");
}

MHE_EXPORT int mhe_prng_small(mhe_ctx *c, const uint64_t seed[8], uint64_t byte_offset, int kind, int limbs,
                              uint64_t *out, uint32_t *state_dev, void *stream)
{
    Primes P;
    if (int r = primes_of(c, P)) return r;
    const int log_n = P.log_n;
    if (!seed || !out || limbs < 1 || limbs > P.K || (byte_offset & 63) || log_n < 5) return bad_args();
    const Seed s = seed_of(seed);
    hipStream_t st = (hipStream_t)stream;
    const u64 n = (u64)1 << log_n;
    if (kind == MHE_SAMPLE_TERNARY)
    {
        if (!state_dev) return bad_args();
        if (hipMemsetAsync(state_dev, 0, 8, st) != hipSuccess)
            return mhe_internal_fail(MHE_ERR_DEVICE, "sampling state reset failed");
        hipLaunchKernelGGL(k_prng_ternary, dim3((unsigned)((n / 16 + 255) / 256), (unsigned)(limbs < 8 ? limbs : 8)),
                           dim3(256), 0, st, s, byte_offset, out, P.dev, limbs, log_n, state_dev);
        hipLaunchKernelGGL(k_prng_ternary_fix, dim3(1), dim3(64), 0, st, s, byte_offset, out, P.dev, limbs, log_n,
                           state_dev);
    }
    else if (kind == MHE_SAMPLE_CBD)
        hipLaunchKernelGGL(k_prng_cbd, dim3((unsigned)((n + kCbdCoeffs - 1) / kCbdCoeffs), (unsigned)(limbs < 4 ? limbs : 4)),
                           dim3(256), 0, st, s, byte_offset, (const u32 *)state_dev, out, P.dev, limbs, log_n);
    else
        return mhe_internal_fail(MHE_ERR_ARG, "unknown distribution");
    return launch_check("sampling kernel launch failed");
}
