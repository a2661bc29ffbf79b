// libmhe: MI355X-native RNS-CKKS evaluator kernels behind the C ABI of include/mhe.h.
//
// Data layout in HBM: [poly][limb][n] u64, identical to SEAL's
// Ciphertext::data() so host<->device moves are single memcpys.  Per-context tables:
//   primes[K]        PrimeDev constants
//   tw[K][n]         (psi^rev(j), Shoup quotient)       -- NTTTables::root_powers_
//   itw[K][n]        (psi^-rev(j), Shoup quotient)      -- same transform as SEAL's scrambled
//                                                          inv_root_powers_, bit-reversed index
//   invq[K][K]       (q_j^-1 mod q_i, Shoup)            -- RNSTool::inv_q_last_mod_q for every j
// Scratch workspaces are per stream (see Workspace).
//
// This file holds the errors, the host number theory, the context and workspace, the elementwise
// path, the job builders and the C ABI; it is the one translation unit of mhe.o and includes the NTT
// (ntt.h), hoisting (hoist.h), job descriptors (jobs.h), elementwise kernels (elem.h) and the device
// allocator (devalloc.h) once each, and further down, where what they build on is defined, the
// key-switch and rescale pipelines (keyswitch.h) and the rotation pipelines (rotate.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <atomic>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/mhe.h"
#include "arith.h"
#include "ntt.h"
#include "hoist.h"
#include "jobs.h"
#include "elem.h"
#include "devalloc.h"

#define MHE_EXPORT extern "C" __attribute__((visibility("default")))

typedef unsigned __int128 u128;

// ============================================================================ errors
static thread_local std::string g_err;

static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do                                                                                         \
    {                                                                                          \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(MHE_ERR_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

#define HIP_LAUNCH_CHECK()                                                                     \
    do                                                                                         \
    {                                                                                          \
        hipError_t e_ = hipGetLastError();                                                     \
        if (e_ != hipSuccess) return fail(MHE_ERR_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)

// ===================================================================== host number theory
// (product code: the engine builds its own tables; it never calls the test oracle)
namespace host
{
static u64 mulmod(u64 a, u64 b, u64 q)
{
    return (u64)((u128)a * b % q);
}

static u64 powmod(u64 b, u64 e, u64 q)
{
    u64 r = 1 % q;
    b %= q;
    while (e)
    {
        if (e & 1) r = mulmod(r, b, q);
        b = mulmod(b, b, q);
        e >>= 1;
    }
    return r;
}

// try_invert_uint_mod (util/numth.h:145)
static bool invmod(u64 a, u64 q, u64 &out)
{
    __int128 r0 = q, r1 = a % q, s0 = 0, s1 = 1;
    if (r1 == 0) return false;
    while (r1)
    {
        __int128 qt = r0 / r1, r2 = r0 - qt * r1, s2 = s0 - qt * s1;
        r0 = r1;
        r1 = r2;
        s0 = s1;
        s1 = s2;
    }
    if (r0 != 1) return false;
    __int128 v = s0 % (__int128)q;
    if (v < 0) v += q;
    out = (u64)v;
    return true;
}

// is_prime (util/numth.cpp:179-277): deterministic Miller-Rabin bases for 64-bit inputs.
static bool is_prime(u64 v)
{
    if (v < 2) return false;
    static const u64 sm[] = { 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37 };
    for (u64 p : sm)
    {
        if (v == p) return true;
        if (v % p == 0) return false;
    }
    u64 d = v - 1;
    int r = 0;
    while (!(d & 1))
    {
        d >>= 1;
        r++;
    }
    for (u64 a : sm)
    {
        u64 x = powmod(a, d, v);
        if (x == 1 || x == v - 1) continue;
        bool ok = false;
        for (int i = 0; i < r - 1; i++)
        {
            x = mulmod(x, x, v);
            if (x == v - 1)
            {
                ok = true;
                break;
            }
        }
        if (!ok) return false;
    }
    return true;
}

// try_minimal_primitive_root (util/numth.cpp:398-424): smallest primitive degree-th root.
static u64 minimal_primitive_root(u64 degree, u64 q)
{
    u64 quo = (q - 1) / degree;
    if (quo * degree != q - 1) return 0;
    u64 root = 0;
    for (u64 c = 2; c < q && !root; c++)
    {
        u64 g = powmod(c, quo, q);
        if (g && powmod(g, degree >> 1, q) == q - 1) root = g;
    }
    if (!root) return 0;
    u64 gsq = mulmod(root, root, q), cur = root, best = root;
    for (u64 i = 0; i < degree; i++)
    {
        if (cur < best) best = cur;
        cur = mulmod(cur, gsq, q);
    }
    return best;
}

static u64 shoup(u64 w, u64 q)
{
    return (u64)(((u128)w << 64) / q);
}

static u32 rev_bits(u32 x, int bits)
{
    return bits ? (__builtin_bitreverse32(x) >> (32 - bits)) : 0;
}
} // namespace host

// ============================================================================= context
// Per batch entry (a key switch / rescale of one ciphertext inside a batched launch).
struct WsEntry
{
    u64 *coeff = nullptr; // [L][n]        INTT(target); the rescale's / ModDown's INTT'd last limbs
    u64 *modup = nullptr; // [L+1][L][n]   lifted + NTT'd digits; reused by mod-down/rescale
    u64 *acc = nullptr;   // [2][L+1][n]   key inner products
    u64 *ct3 = nullptr;   // [3][L][n]     tensor output of a batched HMult
};

// One grow-on-demand device buffer of a stream's scratch.  p and the growth are guarded by the
// workspace's lock; bytes is read by mhe_scratch_bytes without it.
struct Scratch
{
    u64 *p = nullptr;
    std::atomic<size_t> bytes{ 0 };
    // Replaces the buffer by one of nbytes, draining st first (its queued kernels may still use the
    // old one); consults mhe_debug_fail_alloc.  On failure the buffer is empty.
    int grow(mhe_ctx *c, hipStream_t st, size_t nbytes);
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// The group accumulators of a grouped sum (groupsum.h) for MHE_MAXB groups in flight at up to `limbs`
// limbs, (words * limbs + 2) n words per group slot: the sum of the key products A [2][L+1][n], the sum
// of the lifted special limbs T [2][L][n] and, with words = 6, the caller's own sum [2][L][n] behind them.
// Allocated by the first call, grown when a call needs a higher level (get_groupsum).
struct SumPool
{
    int words;
    Scratch buf;
    int limbs = 0;
    u64 *at(int slot, int part, int L, size_t n) const // part 0: A, 1: T, 2: the caller's
    {
        return buf.p + ((size_t)slot * ((size_t)words * limbs + 2) + (part ? 2 * (L + 1) + 2 * L * (part - 1) : 0)) * n;
    }
};

struct Workspace
{
    int max_limbs = 0;
    int entries = 0;      // batch entries the scratch is sized for (<= MHE_MAXB)
    Scratch base;
    WsEntry e[MHE_MAXB];
    u64 *tmp = nullptr;   // [L][n]        permuted c1 for Galois
    // hoisted rotations (hoist.h): the ModUp of up to MHE_MAXB inputs, [K][K-1][n] each, and one
    // zero-coefficient flag per input
    Scratch hoist_base;
    int hoist_entries = 0;
    int hoist_limbs = 0; // the hoisting buffers' level (per-input ModUp of up to this many limbs)
    u64 *hoist[MHE_MAXB] = {};
    u64 *hacc[MHE_MAXB * MHE_HOIST_R] = {}; // [2][K][n] key products of each hoisted rotation
    int *flags = nullptr;
    SumPool rotsum{ 4 };  // mhe_rotate_sum: A and T
    SumPool prodsum{ 6 }; // mhe_relin_sum_rescale: A, T and the sum C of the products' first two polys
    Scratch sample;       // the on-device sample_poly_uniform's state, reject bit planes and redrawn words (sample.hip)
    // kernel timing (mhe_ctx_set_timing): event pairs recorded around the two dominant
    // key-switch kernels on this stream, read back by mhe_kernel_time
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[2];
    size_t ev_used[2] = { 0, 0 };
    std::mutex mu; // growth of this stream's buffers
    // frees everything the stream owns on the device (the caller has drained the stream)
    void release()
    {
        base.release();
        hoist_base.release();
        rotsum.buf.release();
        prodsum.buf.release();
        sample.release();
        if (flags) (void)hipFree(flags);
        flags = nullptr;
        for (auto &v : ev)
        {
            for (auto &e : v)
            {
                (void)hipEventDestroy(e.first);
                (void)hipEventDestroy(e.second);
            }
            v.clear();
        }
    }
};

enum TimedKernel
{
    TK_KS_ROW_MAC = 0, // k_ks_row_mac: fused ModUp row pass + key inner products
    TK_MODUP_COL = 1   // k_modup_col / ModUp column pass
};

// Per-level operation counts (mhe_op_counts, include/mhe.h MHE_OPK_*): what a workload asked of the
// engine, by kind and level -- the op mix a CPU cost model multiplies by per-op CPU timings.
#define MHE_OPK_KINDS 8
#define MHE_OPK_LEVELS 64

struct mhe_ctx
{
    std::atomic<unsigned long long> opc[MHE_OPK_KINDS][MHE_OPK_LEVELS] = {};
    std::atomic<unsigned long long> key_bytes{ 0 }; // key-switching key bytes read since reset (mhe_key_traffic)
    std::atomic<unsigned long long> key_bytes_prep{ 0 }; // the same slices' bytes in the prepared key format
    int device = 0;
    int log_n = 0;
    size_t n = 0;
    int K = 0;
    std::vector<u64> q;
    std::vector<PrimeDev> primes_h;
    PrimeDev *primes = nullptr;
    Tw *tw = nullptr;
    Tw *itw = nullptr;
    Tw *invq = nullptr;
    TwF *twf = nullptr; // FP64 twiddles (w, w/q), [K][n] forward then [K][n] inverse
    NttMode nm;         // FP64 butterflies when every prime is < 2^51 (MHE_FP=0 forces integer)
    // the two ModUp key-switch kernels when only the special prime is >= 2^51 (the GPT-2 chain's
    // 60-bit P): FP64 per output prime below 2^51, integer for P (fp = 2: mixed; MHE_KS_MIX=0: off)
    NttMode nm_ks;
    int ks_fused = 1; // fused row-pass + key-MAC kernel (MHE_KS_FUSED=0: separate row pass + MAC)
    int timing = 0;      // record HIP events around the key-switch kernels (mhe_ctx_set_timing)
    int hmult_fused = 1; // HMult: ModDown fused with the rescale (MHE_HMULT_FUSED=0: separate)
    int ks_share = 1;    // batched key switches sharing one key: XCD-grouped entries (MHE_KS_SHARE=0: off)
    // shared-key launches at n = 2^16 (FP64): two entries per workgroup (k_ks_row_mac NE = 2; MHE_KS_PAIR=0: one)
    int ks_pair = 1;
    std::atomic<unsigned long long> ks_paired{ 0 }, ks_single{ 0 }; // mhe_ks_pair_stats
    // ModUp column pass: output-prime groups per digit.  -1: by the launch's size (ntt.h modup_groups);
    // MHE_KS_COLGROUPS=n: n groups; 0: one job per (I, J) (the generic column pass)
    int ks_colgroups = -1;
    // k_modup_col launches and the sum of their group counts IG (mhe_modup_stats)
    std::atomic<unsigned long long> modup_launches{ 0 }, modup_ig_sum{ 0 };
    int ks_pack = 1; // n = 2^16: ModUp intermediate of primes < 2^48 stored in 48 bits (MHE_KS_PACK=0: 64 bits)
    int icol_fused = 1; // ModDown / rescale: inverse column pass fused into the lift column pass (MHE_ICOL_FUSED=0: separate)
    int galois_fused = 1; // apply_galois: one permutation launch, c1 written by the ModDown (MHE_GALOIS_FUSED=0: SEAL's order with a zero fill)
    // read by every thread's rotations, written by mhe_ctx_set_hoist at any time: atomic
    std::atomic<int> ks_hoist{ 1 }; // batched rotations of one input share their ModUp (hoist.h); mhe_ctx_set_hoist / MHE_KS_HOIST=0 turn it off
    std::atomic<int> hoist_check{ 0 }; // recompute every hoisted rotation by the classic path and compare (mhe_ctx_set_hoist)
    std::atomic<int> fail_switch{ 0 }; // mhe_debug_fail_switch: the n-th next batched key switch fails (0: off)
    std::atomic<unsigned long long> hoist_rot{ 0 }, hoist_mac{ 0 }, hoist_bad{ 0 }; // mhe_hoist_stats
    std::atomic<unsigned long long> rotsum_sums{ 0 }, rotsum_terms{ 0 };             // mhe_rotsum_stats
    std::atomic<unsigned long long> prodsum_sums{ 0 }, prodsum_terms{ 0 };           // mhe_prodsum_stats
    std::atomic<unsigned long long> enc_entries{ 0 }, enc_groups{ 0 };               // mhe_encrypt_stats
    std::atomic<unsigned long long> kg_entries{ 0 }, kg_groups{ 0 };                 // mhe_keygen_stats
    std::atomic<unsigned> kg_cap_limit{ 0 }; // mhe_debug_keygen_cap: an upper limit on the redraw buffer's capacity (0: none)
    unsigned long long id = 0;            // this context's number among all ever created (mhe_keygen_overflows)
    unsigned long long *kg_dev = nullptr; // device totals: [0] redrawn uniform words, [1] overflowed entries (sample.hip)
    std::atomic<int> fail_alloc{ 0 }; // mhe_debug_fail_alloc: the n-th next allocation fails (0: off)
    TwF *cmodf = nullptr; // [K][K]: (q_j mod q_i, (q_j mod q_i) / q_i) as doubles, j major (hoist.h)
    std::mutex mask_mu;
    std::map<u32, u64 *> masks; // Galois element -> NTT of its negation mask, [K][n] (hoist.h)
    std::mutex mu;
    std::map<hipStream_t, Workspace> ws;
};

// Key limbs a prepared key converts: format 1 (doubles) every prime below 2^51, the FP64 path's;
// format 2 (48-bit planes) every prime below 2^48 (ntt.h KEY_PREP_MIN, KEY_PACK_TAG).
static bool key_limb_packed(const mhe_ctx *c, int limb, int key_limbs, int fmt)
{
    const int pi = (limb == key_limbs - 1) ? c->K - 1 : limb;
    return c->q[pi] < (fmt == 2 ? (1ull << 48) : (1ull << 51));
}

// The prepared format of `key` (0: SEAL's layout, 1 doubles, 2 48-bit planes), from the last word of
// its first slot that either format converts (host sync: only prepare / unprepare and the
// separate-MAC debugging path ask).
static int key_tagged(mhe_ctx *c, const u64 *key, int key_limbs, hipStream_t st, int *tagged)
{
    *tagged = 0;
    for (int fmt = 2; fmt >= 1; fmt--)
        for (int l = 0; l < key_limbs; l++)
            if (key_limb_packed(c, l, key_limbs, fmt))
            {
                u64 w = 0;
                HIP_TRY(hipMemcpyAsync(&w, key + (size_t)l * c->n + c->n - 1, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                const int f = key_slot_format(w);
                if (f == fmt)
                {
                    *tagged = f;
                    return MHE_OK;
                }
                break; // this format's first slot is not in it
            }
    return MHE_OK;
}

// Events around a launch of kernel kind k on stream st when timing is on.
static hipEvent_t *timing_slot(mhe_ctx *c, Workspace *w, int k, hipStream_t st)
{
    if (!c->timing) return nullptr;
    auto &v = w->ev[k];
    if (w->ev_used[k] == v.size())
    {
        std::pair<hipEvent_t, hipEvent_t> e{};
        if (hipEventCreate(&e.first) != hipSuccess || hipEventCreate(&e.second) != hipSuccess) return nullptr;
        v.push_back(e);
    }
    hipEvent_t *pair = &v[w->ev_used[k]++].first;
    (void)hipEventRecord(pair[0], st);
    return pair;
}

static void timing_end(hipEvent_t *pair, hipStream_t st)
{
    if (pair) (void)hipEventRecord(pair[1], st);
}

// Scratch allocation (hipMalloc) that, when the device reports out of memory, first gives the
// blocks the engine's caching allocator holds back to the device (devalloc.h release_cached_blocks:
// synchronises the device) and retries once.  Freed ciphertext / key buffers stay cached for reuse at
// their own sizes; a plain hipMalloc cannot use them.
static hipError_t scratch_alloc(void **p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return e;
    (void)hipGetLastError();
    release_cached_blocks();
    e = hipMalloc(p, bytes);
    if (e != hipSuccess)
    {
        (void)hipGetLastError();
        g_alloc_failures.fetch_add(1);
    }
    else
        g_alloc_retries.fetch_add(1);
    return e;
}

// mhe_debug_fail_alloc's countdown: true for the allocation it designates
static bool injected_alloc_failure(mhe_ctx *c)
{
    int v = c->fail_alloc.load();
    while (v > 0)
        if (c->fail_alloc.compare_exchange_weak(v, v - 1))
        {
            if (v == 1) g_alloc_failures.fetch_add(1);
            return v == 1;
        }
    return false;
}

int Scratch::grow(mhe_ctx *c, hipStream_t st, size_t nbytes)
{
    HIP_TRY(hipSetDevice(c->device));
    if (p)
    {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipFree(p));
    }
    p = nullptr;
    bytes = 0;
    if (injected_alloc_failure(c) || scratch_alloc((void **)&p, nbytes) != hipSuccess)
    {
        p = nullptr;
        return fail(MHE_ERR_MEMORY, "workspace allocation failed");
    }
    bytes = nbytes;
    return MHE_OK;
}

// The scratch of stream st, for ciphertexts of up to `limbs` limbs and `entries` batch entries.
// The context lock only guards the map; growing one stream's scratch (which drains that stream
// first: its queued kernels may still use the old buffers) holds that workspace's own lock, so
// other threads' streams are not held up by the drain.
static Workspace &ws_of(mhe_ctx *c, hipStream_t st)
{
    std::lock_guard<std::mutex> g(c->mu);
    return c->ws[st];
}

static int get_ws(mhe_ctx *c, hipStream_t st, int limbs, Workspace **out, int entries = 1)
{
    Workspace &w = ws_of(c, st);
    std::lock_guard<std::mutex> g(w.mu);
    if (w.max_limbs < limbs || w.entries < entries)
    {
        const int E = std::max(entries, w.entries);
        const size_t n = c->n, L = std::max(limbs, w.max_limbs);
        const size_t Lc = L < 3 ? 3 : L;
        const size_t per = Lc * n + (L + 1) * L * n + 2 * (L + 1) * n + 3 * L * n;
        size_t words = (size_t)E * per + L * n;
        w.max_limbs = 0;
        w.entries = 0;
        int r = w.base.grow(c, st, words * sizeof(u64));
        if (r) return r;
        for (int i = 0; i < E; i++)
        {
            w.e[i].coeff = w.base.p + (size_t)i * per;
            w.e[i].modup = w.e[i].coeff + Lc * n;
            w.e[i].acc = w.e[i].modup + (L + 1) * L * n;
            w.e[i].ct3 = w.e[i].acc + 2 * (L + 1) * n;
        }
        w.tmp = w.base.p + (size_t)E * per;
        w.max_limbs = (int)L;
        w.entries = E;
    }
    *out = &w;
    return MHE_OK;
}

// ======================================================================= dispatch helpers
static bool valid_ctx(mhe_ctx *c)
{
    return c && c->primes;
}

static hipStream_t S(void *s)
{
    return (hipStream_t)s;
}

static int check_limbs(mhe_ctx *c, int limbs, int lo)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    if (limbs < lo || limbs > c->K - 1) return fail(MHE_ERR_ARG, "encrypted is not valid for encryption parameters");
    return MHE_OK;
}

// Do the word ranges [a, a + aw) and [b, b + bw) share a word?  The batched entry points run every
// entry inside the same kernels, so an output that overlaps another entry's operand would be read
// and written by one launch in an order that depends on the grid (not the order of count calls).
static bool ranges_overlap(const u64 *a, size_t aw, const u64 *b, size_t bw)
{
    return a < b + bw && b < a + aw;
}

// Does output i (ow words) share a word with one of the nin inputs (iw words each) or with another
// of the nout outputs?
static bool output_overlaps(u64 *const *out, int i, int nout, size_t ow, const u64 *const *in, int nin, size_t iw)
{
    for (int j = 0; j < nin; j++)
        if (ranges_overlap(out[i], ow, in[j], iw)) return true;
    for (int j = 0; j < nout; j++)
        if (j != i && ranges_overlap(out[i], ow, out[j], ow)) return true;
    return false;
}

static int check_galois_elt(mhe_ctx *c, u32 elt)
{
    if (!(elt & 1) || elt >= 2 * c->n) return fail(MHE_ERR_ARG, "Galois element is not valid");
    return MHE_OK;
}

static void count_op(mhe_ctx *c, int kind, int L, unsigned long long k)
{
    if (kind >= 0 && kind < MHE_OPK_KINDS && L >= 0 && L < MHE_OPK_LEVELS) c->opc[kind][L].fetch_add(k, std::memory_order_relaxed);
}

static int check_poly_args(mhe_ctx *c, const void *a, int polys, int limbs)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    if (!a || polys < 1 || limbs < 1 || limbs > c->K) return fail(MHE_ERR_ARG, "invalid polynomial arguments");
    return MHE_OK;
}

// MHE_ALLOC_TRACE: the operand p of the calling entry point, [polys][limbs][n] words.  Nothing is
// read through c unless it is valid, and nothing at all when tracing is off.
static void trace_operand(const char *fn, mhe_ctx *c, const char *what, const void *p, size_t polys, size_t limbs)
{
    if (trace_on() && valid_ctx(c)) trace_range(fn, what, p, (polys * limbs) << c->log_n);
}
#define TR(what, p, polys, limbs) trace_operand(__func__, c, what, p, (size_t)(polys), (size_t)(limbs))

// ------------------------------------------------------------------- elementwise launches
// The unit of work of the elementwise family and the d2d copy is the mhe_launch descriptor
// (include/mhe.h).  An entry point fills one and hands it to elem_entry: elem_check validates it,
// the calling thread's hook (mhe_set_launch_hook) may take it, otherwise elem_launch runs it as a
// group of one.  mhe_launch_run runs groups of same-shaped descriptors through the same functions.
static thread_local mhe_launch_hook tl_hook = nullptr;
static thread_local void *tl_hook_user = nullptr;

static mhe_launch elem_desc(int kind, int op, const u64 *a, const u64 *b, u64 *out, int polys, int limbs, void *stream)
{
    mhe_launch l{};
    l.kind = kind;
    l.op = op;
    l.a = a;
    l.b = b;
    l.out = out;
    l.polys = polys;
    l.limbs = limbs;
    l.stream = stream;
    return l;
}

// The argument checks of the descriptor's entry point, with its return code and message.
static int elem_check(mhe_ctx *c, const mhe_launch &l)
{
    bool b_used = true;
    switch (l.kind)
    {
    case MHE_LK_COPY: return valid_ctx(c) ? MHE_OK : fail(MHE_ERR_ARG, "invalid argument");
    case MHE_LK_ADDSUB: b_used = l.op < 2; break; // negate
    case MHE_LK_MULPLAIN:
    case MHE_LK_MULPLAIN_ADD: break;
    case MHE_LK_SCALAR: b_used = false; break;
    case MHE_LK_TENSOR: b_used = !l.op; break; // square
    default: return fail(MHE_ERR_ARG, "unknown launch kind");
    }
    const bool set = l.kind == MHE_LK_SCALAR && l.op == 2; // a unused: out stands in for it
    int r = check_poly_args(c, set ? l.out : l.a, l.kind == MHE_LK_TENSOR ? 2 : l.polys, l.limbs);
    if (r) return r;
    if (!l.out || (b_used && !l.b)) return fail(MHE_ERR_ARG, "invalid polynomial arguments");
    if (l.kind == MHE_LK_SCALAR)
        for (int i = 0; i < l.limbs; i++)
            if (l.scalars[i] >= c->q[i]) return fail(MHE_ERR_ARG, "scalar must be less than modulus");
    return MHE_OK;
}

// Op counts of B descriptors of l's shape (a tensor product counts once, the others per poly).
static void elem_count(mhe_ctx *c, const mhe_launch &l, int B)
{
    if (l.kind == MHE_LK_COPY) return;
    const int opk = l.kind == MHE_LK_ADDSUB ? MHE_OPK_ADDSUB
                    : l.kind == MHE_LK_SCALAR ? MHE_OPK_SCALAR
                    : l.kind == MHE_LK_TENSOR ? MHE_OPK_TENSOR
                                              : MHE_OPK_MULPLAIN;
    const unsigned long long k = (unsigned long long)B * (l.kind == MHE_LK_TENSOR ? 1 : l.polys);
    count_op(c, opk, l.limbs, k);
    if (l.kind == MHE_LK_MULPLAIN_ADD) count_op(c, MHE_OPK_ADDSUB, l.limbs, k);
}

static void scalar_tab(mhe_ctx *c, const mhe_launch &l, ScalarTab &t)
{
    for (int i = 0; i < l.limbs; i++)
    {
        t.v[i] = l.scalars[i];
        t.vq[i] = host::shoup(l.scalars[i], c->q[i]);
    }
}

// Can B > 1 descriptors of one shape run as one batched launch?  Copies move 16 bytes per lane.
static bool elem_batchable(mhe_launch *const *g, int B)
{
    if (g[0]->kind != MHE_LK_COPY) return true;
    uintptr_t bits = g[0]->bytes;
    for (int k = 0; k < B; k++) bits |= (uintptr_t)g[k]->a | (uintptr_t)g[k]->out;
    return (bits & 15) == 0;
}

// Counts and launches a group of B <= MHE_MAXB checked descriptors of one shape (same_shape; B > 1:
// elem_batchable): one descriptor by the kernel of its kind, several by k_elem_b / k_copy16_b.
static int elem_launch(mhe_ctx *c, mhe_launch *const *g, int B)
{
    const mhe_launch &l = *g[0];
    const hipStream_t st = S(l.stream);
    const int log_n = c->log_n, fp = c->nm.fp ? 1 : 0;
    // a tensor product covers one pair of 2-poly ciphertexts ([limbs] residues per output poly)
    const size_t total2 = ((size_t)(l.kind == MHE_LK_TENSOR ? 1 : l.polys) * l.limbs << log_n) / 2;
    const dim3 grid = ELEM_GRID(total2), block(256);
    elem_count(c, l, B);
    if (B == 1)
        switch (l.kind)
        {
        case MHE_LK_ADDSUB:
            hipLaunchKernelGGL(k_addsub, grid, block, 0, st, l.a, l.b, l.out, c->primes, l.limbs, log_n, total2, l.op);
            break;
        case MHE_LK_MULPLAIN:
            hipLaunchKernelGGL(k_mulplain, grid, block, 0, st, l.a, l.b, l.out, c->primes, l.limbs, log_n, total2, fp);
            break;
        case MHE_LK_MULPLAIN_ADD:
            hipLaunchKernelGGL(k_mulplain_add, grid, block, 0, st, l.a, l.b, l.out, c->primes, l.limbs, log_n, total2, fp);
            break;
        case MHE_LK_SCALAR:
        {
            ScalarTab t;
            scalar_tab(c, l, t);
            hipLaunchKernelGGL(k_scalar, grid, block, 0, st, l.a, l.out, c->primes, t, l.limbs, log_n, total2, l.op);
            break;
        }
        case MHE_LK_TENSOR:
            hipLaunchKernelGGL(k_tensor, grid, block, 0, st, l.a, l.op ? l.a : l.b, l.out, c->primes, l.limbs, log_n,
                               total2, l.op ? 1 : 0, fp);
            break;
        case MHE_LK_COPY:
        {
            void *dst = l.out, *stream = l.stream;
            const void *src = l.a;
            const size_t bytes = l.bytes;
            HIP_TRY(mhe_internal_copy_d2d(dst, src, bytes, S(stream)));
            return MHE_OK;
        }
        }
    else
    {
        ElemPtrs P{};
        for (int k = 0; k < B; k++)
        {
            P.a[k] = g[k]->a;
            P.b[k] = g[k]->b;
            P.out[k] = g[k]->out;
        }
        if (l.kind == MHE_LK_COPY)
        {
            const size_t cnt = l.bytes / 16;
            if (!cnt) return MHE_OK;
            const unsigned cgrid = (unsigned)std::min<size_t>((cnt + 255) / 256, 4096);
            hipLaunchKernelGGL(k_copy16_b, dim3(cgrid, (unsigned)B), block, 0, st, P, cnt);
        }
        else
        {
            ScalarTab t{};
            if (l.kind == MHE_LK_SCALAR) scalar_tab(c, l, t);
            hipLaunchKernelGGL(k_elem_b, dim3(grid.x, (unsigned)B), block, 0, st, P, c->primes, t, l.limbs, log_n, total2,
                               l.kind, l.op, fp);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MHE_ERR_DEVICE, std::string(B == 1 ? "kernel launch: " : "") + hipGetErrorString(e));
    return MHE_OK;
}

static int elem_entry(mhe_ctx *c, mhe_launch &l)
{
    int r = elem_check(c, l);
    if (r) return r;
    if (tl_hook)
    {
        l.rc = -1;
        tl_hook(c, &l, tl_hook_user); // gets it run (mhe_launch_run) and sets l.rc
        return l.rc;
    }
    mhe_launch *g = &l;
    return elem_launch(c, &g, 1);
}

// ----------------------------------------------------------------------------- job builders
// Plain transform of [polys][limbs][n] on the context's tables (limb l on prime l).
static JobFwdPlain fwd_plain(mhe_ctx *c, const u64 *src, u64 *dst, int limbs, int mode)
{
    return JobFwdPlain{ { src, dst, c->primes, c->tw, limbs, c->log_n, mode } };
}

static JobInvPlain inv_plain(mhe_ctx *c, const u64 *src, u64 *dst, int limbs, int mode)
{
    return JobInvPlain{ { src, dst, c->primes, c->itw, limbs, c->log_n, mode } };
}

// The two special accumulator limbs of the key products acc [2][L+1][n]: inverse NTT in place, lazy.
static JobStrided special_limbs(mhe_ctx *c, u64 *acc, int L)
{
    u64 *p = acc + (size_t)L * c->n;
    const size_t stride = (size_t)(L + 1) * c->n;
    return JobStrided{ p, p, stride, stride, c->K - 1, 0, c->primes, c->itw, c->log_n, 0 };
}

// Forward NTT of [polys][limbs] (limb l on prime l).
static int run_ntt_fwd(mhe_ctx *c, const u64 *src, u64 *dst, int polys, int limbs, int full, hipStream_t st)
{
    count_op(c, MHE_OPK_NTT, limbs, (unsigned long long)polys);
    fwd_col(fwd_plain(c, src, dst, limbs, 0), c->log_n, polys * limbs, c->nm, st);
    fwd_row(fwd_plain(c, dst, dst, limbs, full), c->log_n, polys * limbs, c->nm, st);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

static int run_ntt_inv(mhe_ctx *c, const u64 *src, u64 *dst, int polys, int limbs, int full, hipStream_t st)
{
    count_op(c, MHE_OPK_NTT, limbs, (unsigned long long)polys);
    inv_row(inv_plain(c, src, dst, limbs, 0), c->log_n, polys * limbs, c->nm, st);
    inv_col(inv_plain(c, dst, dst, limbs, full), c->log_n, polys * limbs, c->nm, st);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

// ------------------------------------------------------------- key switch and rescale pipelines
#include "keyswitch.h"

// ================================================================ internal (encode.hip)
int mhe_internal_fail(int code, const char *msg)
{
    return fail(code, msg);
}

int mhe_internal_ntt_forward(mhe_ctx *c, uint64_t *data, int polys, int limbs, int full, hipStream_t st)
{
    return run_ntt_fwd(c, data, data, polys, limbs, full, st);
}

// Full forward NTT in place of B <= MHE_MAXB plaintexts [limbs][n] in one pair of launches; entry
// e's workgroups return when the device word skip_if[e] is nonzero (skip_if null: all run).
int mhe_internal_ntt_forward_entries(mhe_ctx *c, uint64_t *const *data, int B, int limbs, const uint32_t *skip_if,
                                     hipStream_t st)
{
    if (B < 1 || B > MHE_MAXB) return fail(MHE_ERR_ARG, "forward NTT: batch size out of range");
    count_op(c, MHE_OPK_NTT, limbs, (unsigned long long)B);
    JobB<JobFwdPlainIf> col(limbs), row(limbs);
    for (int e = 0; e < B; e++)
    {
        const u32 *flag = skip_if ? skip_if + e : nullptr;
        col.j[e] = JobFwdPlainIf{ fwd_plain(c, data[e], data[e], limbs, 0), flag };
        row.j[e] = JobFwdPlainIf{ fwd_plain(c, data[e], data[e], limbs, 1), flag };
    }
    fwd_col(col, c->log_n, B * limbs, c->nm, st);
    fwd_row(row, c->log_n, B * limbs, c->nm, st);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

int mhe_internal_primes(mhe_ctx *c, const PrimeDev **dev, const uint64_t **host, int *count, int *log_n)
{
    if (!valid_ctx(c)) return MHE_ERR_ARG;
    *dev = c->primes;
    *host = c->q.data();
    *count = c->K;
    *log_n = c->log_n;
    return MHE_OK;
}

// The sampling scratch of stream st with at least `bytes` bytes (grown here, before the caller's first
// launch), and the context's device counters of the uniform sampler.
int mhe_internal_sample_scratch(mhe_ctx *c, hipStream_t st, size_t bytes, void **scratch, uint64_t **counters)
{
    if (!valid_ctx(c) || !bytes) return fail(MHE_ERR_ARG, "invalid sampling arguments");
    Workspace &w = ws_of(c, st);
    std::lock_guard<std::mutex> g(w.mu);
    if (w.sample.bytes < bytes)
    {
        int r = w.sample.grow(c, st, bytes);
        if (r) return r;
    }
    *scratch = w.sample.p;
    *counters = reinterpret_cast<uint64_t *>(c->kg_dev);
    return MHE_OK;
}

uint32_t mhe_internal_keygen_cap_limit(mhe_ctx *c)
{
    return c->kg_cap_limit.load();
}

// ================================================================================ C ABI
MHE_EXPORT const char *mhe_last_error(void)
{
    return g_err.c_str();
}

MHE_EXPORT int mhe_version(void)
{
    return 1;
}

MHE_EXPORT int mhe_coeff_modulus_create(uint64_t n, const int *bit_sizes, int count, uint64_t *out)
{
    if (!bit_sizes || !out || count <= 0 || count > 64 || (n & (n - 1)) || n < 2)
        return fail(MHE_ERR_ARG, "bit_sizes is invalid");
    std::map<int, std::vector<u64>> table;
    std::map<int, int> cnt;
    for (int i = 0; i < count; i++)
    {
        if (bit_sizes[i] < 2 || bit_sizes[i] > 60) return fail(MHE_ERR_ARG, "bit_sizes is invalid");
        cnt[bit_sizes[i]]++;
    }
    for (auto &kv : cnt)
    {
        const int bits = kv.first;
        const u64 factor = 2 * n;
        u64 value = ((u64)1 << bits) - factor + 1, lower = (u64)1 << (bits - 1);
        std::vector<u64> &v = table[bits];
        while ((int)v.size() < kv.second && value > lower)
        {
            if (host::is_prime(value)) v.push_back(value);
            value -= factor;
        }
        if ((int)v.size() < kv.second) return fail(MHE_ERR_ARG, "failed to find enough qualifying primes");
    }
    for (int i = 0; i < count; i++)
    {
        auto &v = table[bit_sizes[i]];
        out[i] = v.back();
        v.pop_back();
    }
    return MHE_OK;
}

MHE_EXPORT uint32_t mhe_galois_elt_from_step(int log_n, int step)
{
    const u64 n = (u64)1 << log_n, m = 2 * n;
    if (step == 0) return (uint32_t)(m - 1);
    u64 pos = (u64)(step < 0 ? -(long long)step : step);
    if (pos >= (n >> 1)) return 0;
    u64 s = step < 0 ? (n >> 1) - pos : pos;
    u64 elt = 1;
    while (s--) elt = (elt * 5) & (m - 1); // generator_ = 5 (util/galois.h:169)
    return (uint32_t)elt;
}

MHE_EXPORT int mhe_ctx_create(mhe_ctx **out, int log_n, const uint64_t *moduli, int count, int device)
{
    if (!out) return fail(MHE_ERR_ARG, "ctx is null");
    *out = nullptr;
    if (log_n < 12 || log_n > 16) return fail(MHE_ERR_ARG, "poly_modulus_degree is invalid");
    if (!moduli || count < 2 || count > 64) return fail(MHE_ERR_ARG, "coeff_modulus is invalid");
    const size_t n = (size_t)1 << log_n;
    for (int i = 0; i < count; i++)
    {
        u64 q = moduli[i];
        if (q < 2 || q >= ((u64)1 << 61) || (q - 1) % (2 * n) != 0 || !host::is_prime(q))
            return fail(MHE_ERR_ARG, "coeff_modulus is not NTT-friendly prime");
    }
    mhe_ctx *c = new (std::nothrow) mhe_ctx;
    if (!c) return fail(MHE_ERR_MEMORY, "out of memory");
    c->device = device;
    c->log_n = log_n;
    c->n = n;
    c->K = count;
    c->q.assign(moduli, moduli + count);
    if (const char *f = getenv("MHE_KS_FUSED")) c->ks_fused = atoi(f);
    if (const char *f = getenv("MHE_HMULT_FUSED")) c->hmult_fused = atoi(f);
    if (const char *f = getenv("MHE_KS_SHARE")) c->ks_share = atoi(f);
    if (const char *f = getenv("MHE_KS_PAIR")) c->ks_pair = atoi(f);
    if (const char *f = getenv("MHE_KS_COLGROUPS")) c->ks_colgroups = std::max(0, atoi(f));
    if (const char *f = getenv("MHE_KS_PACK")) c->ks_pack = atoi(f);
    if (const char *f = getenv("MHE_GALOIS_FUSED")) c->galois_fused = atoi(f);
    if (const char *f = getenv("MHE_ICOL_FUSED")) c->icol_fused = atoi(f);
    if (const char *f = getenv("MHE_KS_HOIST")) c->ks_hoist = atoi(f);
    std::vector<Tw> tw((size_t)count * n), itw((size_t)count * n), invq((size_t)count * count);
    c->primes_h.resize(count);
    for (int k = 0; k < count; k++)
    {
        const u64 q = moduli[k];
        PrimeDev &p = c->primes_h[k];
        p.q = q;
        p.two_q = 2 * q;
        p.four_q = 4 * q;
        p.qd = (double)q;
        p.qi = 1.0 / (double)q;
        u128 ratio = (~(u128)0) / q;
        p.r0 = (u64)ratio;
        p.r1 = (u64)(ratio >> 64);
        // NTTTables::initialize (util/ntt.cpp:30-89)
        u64 psi = host::minimal_primitive_root(2 * n, q), ipsi = 0, ninv = 0;
        if (!psi || !host::invmod(psi, q, ipsi) || !host::invmod(n % q, q, ninv))
        {
            delete c;
            return fail(MHE_ERR_ARG, "invalid modulus");
        }
        Tw *t = &tw[(size_t)k * n], *it = &itw[(size_t)k * n];
        u64 pw = 1, ipw = 1;
        for (size_t i = 0; i < n; i++)
        {
            const u32 r = host::rev_bits((u32)i, log_n);
            t[r].x = pw;
            t[r].y = host::shoup(pw, q);
            it[r].x = ipw;
            it[r].y = host::shoup(ipw, q);
            pw = host::mulmod(pw, psi, q);
            ipw = host::mulmod(ipw, ipsi, q);
        }
        p.ninv = ninv;
        p.ninv_q = host::shoup(ninv, q);
        p.last_w = host::mulmod(it[1].x, ninv, q);
        p.last_wq = host::shoup(p.last_w, q);
    }
    for (int j = 0; j < count; j++)
        for (int i = 0; i < count; i++)
        {
            u64 inv = 0;
            if (i != j) host::invmod(moduli[j] % moduli[i], moduli[i], inv);
            invq[(size_t)j * count + i].x = inv;
            invq[(size_t)j * count + i].y = host::shoup(inv, moduli[i]);
        }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess)
    {
        hipMemPool_t pool;
        if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess)
        {
            uint64_t threshold = UINT64_MAX;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &threshold);
        }
    }
    if (e == hipSuccess) e = hipMalloc(&c->primes, sizeof(PrimeDev) * count);
    if (e == hipSuccess) e = hipMalloc(&c->tw, sizeof(Tw) * tw.size());
    if (e == hipSuccess) e = hipMalloc(&c->itw, sizeof(Tw) * itw.size());
    if (e == hipSuccess) e = hipMalloc(&c->invq, sizeof(Tw) * invq.size());
    if (e == hipSuccess) e = hipMemcpy(c->primes, c->primes_h.data(), sizeof(PrimeDev) * count, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->tw, tw.data(), sizeof(Tw) * tw.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->itw, itw.data(), sizeof(Tw) * itw.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->invq, invq.data(), sizeof(Tw) * invq.size(), hipMemcpyHostToDevice);
    // FP64 arithmetic (fparith.h) needs q < 2^51 for every prime of the chain; with only the last
    // (special) prime above, the ModUp kernels still run FP64 for every other output prime
    bool fp = true, fp_data = true;
    for (int k = 0; k < count; k++) fp = fp && moduli[k] < ((u64)1 << 51);
    for (int k = 0; k + 1 < count; k++) fp_data = fp_data && moduli[k] < ((u64)1 << 51);
    if (const char *f = getenv("MHE_FP"))
        if (atoi(f) == 0) fp = fp_data = false;
    bool mix = !fp && fp_data && count > 1;
    if (const char *f = getenv("MHE_KS_MIX")) mix = mix && atoi(f) != 0;
    if (e == hipSuccess && fp)
    {
        // hoisted rotations (hoist.h): q_j mod q_i and its quotient by q_i
        std::vector<TwF> cm((size_t)count * count);
        for (int j = 0; j < count; j++)
            for (int i = 0; i < count; i++)
            {
                const u64 r = moduli[j] % moduli[i];
                cm[(size_t)j * count + i] = make_double2((double)r, (double)r / (double)moduli[i]);
            }
        e = hipMalloc(&c->cmodf, sizeof(TwF) * cm.size());
        if (e == hipSuccess) e = hipMemcpy(c->cmodf, cm.data(), sizeof(TwF) * cm.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && (fp || mix))
    {
        std::vector<TwF> twf((size_t)2 * count * n);
        for (int k = 0; k < count; k++)
        {
            const double qd = (double)moduli[k];
            for (size_t i = 0; i < n; i++)
            {
                const size_t o = (size_t)k * n + i;
                twf[o] = make_double2((double)tw[o].x, (double)tw[o].x / qd);
                twf[(size_t)count * n + o] = make_double2((double)itw[o].x, (double)itw[o].x / qd);
            }
        }
        e = hipMalloc(&c->twf, sizeof(TwF) * twf.size());
        if (e == hipSuccess) e = hipMemcpy(c->twf, twf.data(), sizeof(TwF) * twf.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess)
        {
            NttMode m;
            m.fp = fp ? 1 : 2;
            m.dfwd = (long long)((const char *)c->twf - (const char *)c->tw);
            m.dinv = (long long)((const char *)(c->twf + (size_t)count * n) - (const char *)c->itw);
            if (fp) c->nm = m;
            c->nm_ks = m;
        }
    }
    if (e == hipSuccess) e = hipMalloc(&c->kg_dev, 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(c->kg_dev, 0, 2 * sizeof(unsigned long long));
    if (e != hipSuccess)
    {
        (void)hipFree(c->kg_dev);
        (void)hipFree(c->cmodf);
        (void)hipFree(c->twf);
        (void)hipFree(c->primes);
        (void)hipFree(c->tw);
        (void)hipFree(c->itw);
        (void)hipFree(c->invq);
        c->primes = nullptr;
        delete c;
        return fail(MHE_ERR_DEVICE, std::string("mhe_ctx_create: ") + hipGetErrorString(e));
    }
    static std::atomic<unsigned long long> serial{ 0 };
    c->id = ++serial;
    mhe_internal_ctx_count(+1);
    *out = c;
    return MHE_OK;
}

MHE_EXPORT int mhe_ctx_destroy(mhe_ctx *c)
{
    if (!c) return MHE_OK;
    (void)hipSetDevice(c->device);
    for (auto &kv : c->masks) (void)hipFree(kv.second);
    for (auto &kv : c->ws) kv.second.release();
    (void)hipFree(c->primes);
    (void)hipFree(c->tw);
    (void)hipFree(c->itw);
    (void)hipFree(c->invq);
    (void)hipFree(c->twf);
    (void)hipFree(c->cmodf);
    (void)hipFree(c->kg_dev);
    delete c;
    mhe_internal_ctx_count(-1);
    return MHE_OK;
}

MHE_EXPORT int mhe_ctx_reserve(mhe_ctx *c, int max_limbs, void *stream)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    Workspace *w;
    return get_ws(c, S(stream), max_limbs < c->K - 1 ? c->K - 1 : max_limbs, &w);
}

MHE_EXPORT int mhe_malloc(mhe_ctx *c, void **dptr, size_t bytes)
{
    if (!valid_ctx(c) || !dptr) return fail(MHE_ERR_ARG, "invalid argument");
    HIP_TRY(hipSetDevice(c->device));
    if (hipMalloc(dptr, bytes ? bytes : 1) != hipSuccess) return fail(MHE_ERR_MEMORY, "device allocation failed");
    return MHE_OK;
}

MHE_EXPORT int mhe_malloc_async(mhe_ctx *c, void **dptr, size_t bytes, void *stream)
{
    if (!valid_ctx(c) || !dptr) return fail(MHE_ERR_ARG, "invalid argument");
    const size_t kGuard = trace_on() ? ((size_t)16 << 20) : 0;
    if (injected_alloc_failure(c)) return fail(MHE_ERR_MEMORY, "device allocation failed");
    if (mhe_internal_alloc(dptr, (bytes ? bytes : 1) + kGuard, S(stream)) != hipSuccess)
        return fail(MHE_ERR_MEMORY, "device allocation failed");
    if (trace_on())
    {
        (void)hipMemsetAsync((char *)*dptr + (bytes ? bytes : 1), 0xAB, kGuard, S(stream));
        std::lock_guard<std::mutex> g(g_trace_mu);
        const uintptr_t a = (uintptr_t)*dptr, e = a + (bytes ? bytes : 1);
        auto it = g_live.upper_bound(a);
        if (it != g_live.begin())
        {
            auto pv = std::prev(it);
            if (pv->first + pv->second > a)
                fprintf(stderr, "[alloc-trace] overlap: new [%#lx,+%zu) inside live [%#lx,+%zu)\n", (unsigned long)a,
                        bytes, (unsigned long)pv->first, pv->second);
        }
        if (it != g_live.end() && it->first < e)
            fprintf(stderr, "[alloc-trace] overlap: new [%#lx,+%zu) covers live [%#lx,+%zu)\n", (unsigned long)a, bytes,
                    (unsigned long)it->first, it->second);
        g_live[a] = bytes ? bytes : 1;
    }
    return MHE_OK;
}

MHE_EXPORT int mhe_free_async(mhe_ctx *c, void *dptr, void *stream)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "invalid argument");
    if (trace_on() && dptr)
    {
        std::lock_guard<std::mutex> g(g_trace_mu);
        auto it = g_live.find((uintptr_t)dptr);
        if (it == g_live.end())
            fprintf(stderr, "[alloc-trace] free of unknown or already freed pointer %p\n", dptr);
        else
        {
            const size_t kGuard = (size_t)16 << 20;
            std::vector<unsigned char> gbuf(kGuard);
            (void)hipStreamSynchronize(S(stream));
            (void)hipMemcpy(gbuf.data(), (char *)dptr + it->second, kGuard, hipMemcpyDeviceToHost);
            size_t first = kGuard, last = 0;
            for (size_t i = 0; i < kGuard; i++)
                if (gbuf[i] != 0xAB)
                {
                    first = std::min(first, i);
                    last = i;
                }
            if (first < kGuard)
                fprintf(stderr, "[alloc-trace] OVERRUN of allocation %p (%zu bytes = %zu words): guard bytes [%zu, %zu] written\n",
                        dptr, it->second, it->second / 8, first, last);
            g_live.erase(it);
        }
    }
    HIP_TRY(mhe_internal_free(dptr, S(stream)));
    return MHE_OK;
}

MHE_EXPORT int mhe_free(mhe_ctx *c, void *dptr)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "invalid argument");
    HIP_TRY(hipFree(dptr));
    return MHE_OK;
}

MHE_EXPORT int mhe_memcpy_h2d(mhe_ctx *c, void *dst, const void *src, size_t bytes, void *stream)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "invalid argument");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(stream)));
    return MHE_OK;
}

MHE_EXPORT int mhe_memcpy_d2h(mhe_ctx *c, void *dst, const void *src, size_t bytes, void *stream)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "invalid argument");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream)));
    return MHE_OK;
}

MHE_EXPORT int mhe_memcpy_d2d(mhe_ctx *c, void *dst, const void *src, size_t bytes, void *stream)
{
    trace_range(__func__, "dst", dst, bytes / 8);
    trace_range(__func__, "src", src, bytes / 8);
    TRC(0, 0, 0, 0);
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "invalid argument");
    if (!bytes || dst == src) return MHE_OK;
    mhe_launch l = elem_desc(MHE_LK_COPY, 0, (const u64 *)src, nullptr, (u64 *)dst, 0, 0, stream);
    l.bytes = bytes;
    return elem_entry(c, l);
}

static bool same_shape(const mhe_launch &x, const mhe_launch &y)
{
    if (x.kind != y.kind || x.op != y.op || x.polys != y.polys || x.limbs != y.limbs || x.bytes != y.bytes ||
        x.stream != y.stream)
        return false;
    if (x.kind == MHE_LK_SCALAR)
        for (int l = 0; l < x.limbs; l++)
            if (x.scalars[l] != y.scalars[l]) return false;
    return true;
}

MHE_EXPORT int mhe_set_launch_hook(mhe_launch_hook hook, void *user)
{
    tl_hook = hook;
    tl_hook_user = user;
    return MHE_OK;
}

MHE_EXPORT int mhe_launch_run(mhe_ctx *c, mhe_launch *const *ls, int count)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    if (count < 0 || (count && !ls)) return fail(MHE_ERR_ARG, "invalid argument");
    // every descriptor is checked before the first launch; one that fails keeps its entry point's rc
    // and takes part in no launch
    std::vector<char> done((size_t)count, 0);
    int first_err = MHE_OK;
    for (int i = 0; i < count; i++)
        if ((ls[i]->rc = elem_check(c, *ls[i])))
        {
            done[i] = 1;
            if (!first_err) first_err = ls[i]->rc;
        }
    for (int i = 0; i < count; i++)
    {
        if (done[i]) continue;
        // entries of i's shape, in order, up to MHE_MAXB per launch
        mhe_launch *grp[MHE_MAXB];
        int B = 0;
        for (int j = i; j < count && B < MHE_MAXB; j++)
            if (!done[j] && same_shape(*ls[i], *ls[j]))
            {
                grp[B++] = ls[j];
                done[j] = 1;
            }
        // one batched launch, or (a lone descriptor, copies that are not 16-byte aligned) one by one
        const int step = (B > 1 && elem_batchable(grp, B)) ? B : 1;
        for (int k = 0; k < B; k += step)
        {
            const int rc = elem_launch(c, grp + k, step);
            for (int j = k; j < k + step; j++) grp[j]->rc = rc;
            if (rc && !first_err) first_err = rc;
        }
    }
    return first_err;
}

MHE_EXPORT int mhe_ctx_set_timing(mhe_ctx *c, int on)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    c->timing = on ? 1 : 0;
    return MHE_OK;
}

MHE_EXPORT int mhe_trim(mhe_ctx *c)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    HIP_TRY(hipSetDevice(c->device));
    release_cached_blocks();
    return MHE_OK;
}

MHE_EXPORT int mhe_debug_fail_switch(mhe_ctx *c, int nth)
{
    if (!valid_ctx(c) || nth < 0) return fail(MHE_ERR_ARG, "invalid argument");
    c->fail_switch.store(nth);
    return MHE_OK;
}

MHE_EXPORT int mhe_alloc_stats(uint64_t *retries, uint64_t *failures, int reset)
{
    if (!retries || !failures) return fail(MHE_ERR_ARG, "invalid argument");
    *retries = reset ? g_alloc_retries.exchange(0) : g_alloc_retries.load();
    *failures = reset ? g_alloc_failures.exchange(0) : g_alloc_failures.load();
    return MHE_OK;
}

MHE_EXPORT int mhe_debug_fail_alloc(mhe_ctx *c, int nth)
{
    if (!valid_ctx(c) || nth < 0) return fail(MHE_ERR_ARG, "invalid argument");
    c->fail_alloc.store(nth);
    return MHE_OK;
}

MHE_EXPORT int mhe_scratch_bytes(mhe_ctx *c, uint64_t *workspace, uint64_t *hoisting, uint64_t *masks, int *streams)
{
    if (!valid_ctx(c) || !workspace || !hoisting || !masks || !streams) return fail(MHE_ERR_ARG, "invalid argument");
    {
        std::lock_guard<std::mutex> g(c->mu);
        *workspace = *hoisting = 0;
        for (auto &kv : c->ws)
        {
            *workspace += kv.second.base.bytes + kv.second.rotsum.buf.bytes + kv.second.prodsum.buf.bytes;
            *hoisting += kv.second.hoist_base.bytes;
        }
        *streams = (int)c->ws.size();
    }
    std::lock_guard<std::mutex> g(c->mask_mu);
    *masks = (uint64_t)c->masks.size() * c->K * c->n * sizeof(u64);
    return MHE_OK;
}

MHE_EXPORT int mhe_kernel_time(mhe_ctx *c, int kernel, double *total_ms, int *launches)
{
    if (!valid_ctx(c) || kernel < 0 || kernel > 1 || !total_ms || !launches) return fail(MHE_ERR_ARG, "invalid argument");
    std::lock_guard<std::mutex> g(c->mu);
    double ms = 0;
    int cnt = 0;
    for (auto &kv : c->ws)
    {
        Workspace &w = kv.second;
        for (size_t i = 0; i < w.ev_used[kernel]; i++)
        {
            float t = 0;
            HIP_TRY(hipEventSynchronize(w.ev[kernel][i].second));
            HIP_TRY(hipEventElapsedTime(&t, w.ev[kernel][i].first, w.ev[kernel][i].second));
            ms += t;
            cnt++;
        }
        w.ev_used[kernel] = 0;
    }
    *total_ms = ms;
    *launches = cnt;
    return MHE_OK;
}

MHE_EXPORT int mhe_stream_create(mhe_ctx *c, void **stream)
{
    if (!valid_ctx(c) || !stream) return fail(MHE_ERR_ARG, "invalid argument");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return MHE_OK;
}

MHE_EXPORT int mhe_stream_destroy(mhe_ctx *c, void *stream)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "invalid argument");
    {
        std::lock_guard<std::mutex> g(c->mu);
        auto it = c->ws.find(S(stream));
        if (it != c->ws.end())
        {
            (void)hipStreamSynchronize(S(stream));
            it->second.release();
            c->ws.erase(it);
        }
    }
    HIP_TRY(hipStreamDestroy(S(stream)));
    return MHE_OK;
}

MHE_EXPORT int mhe_stream_sync(mhe_ctx *c, void *stream)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "invalid argument");
    HIP_TRY(hipStreamSynchronize(S(stream)));
    return MHE_OK;
}

MHE_EXPORT int mhe_op_counts(mhe_ctx *c, int kind, uint64_t *counts, int levels, int reset)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    if (kind < 0 || kind >= MHE_OPK_KINDS || !counts || levels < 1) return fail(MHE_ERR_ARG, "invalid argument");
    for (int l = 0; l < levels; l++)
        counts[l] = l < MHE_OPK_LEVELS ? (reset ? c->opc[kind][l].exchange(0) : c->opc[kind][l].load()) : 0;
    if (reset)
        for (int l = levels; l < MHE_OPK_LEVELS; l++) c->opc[kind][l].store(0);
    return MHE_OK;
}

MHE_EXPORT int mhe_key_traffic(mhe_ctx *c, uint64_t *bytes, int reset)
{
    if (!valid_ctx(c) || !bytes) return fail(MHE_ERR_ARG, "invalid argument");
    *bytes = reset ? c->key_bytes.exchange(0) : c->key_bytes.load();
    return MHE_OK;
}

// Format 1 (doubles): prepare (dir 1) or unprepare (dir 0) the limb slots of a key in place: a slot
// of a prime below 2^51 holds its residues as doubles (-0.0 for zero, so every word is >=
// KEY_PREP_MIN); other slots keep SEAL's layout.  blockIdx.y: digit * 2 * key_limbs + poly *
// key_limbs + limb.
__global__ void k_key_pack(u64 *__restrict__ key, const unsigned char *__restrict__ packed, int key_limbs, int log_n,
                           int dir)
{
    const size_t n = (size_t)1 << log_n;
    const int slot = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !packed[slot % key_limbs]) return;
    u64 *d = key + (size_t)slot * n;
    const u64 v = d[i];
    d[i] = dir ? (v ? (u64)__double_as_longlong((double)v) : 0x8000000000000000ull) : key_word_u(v);
}

// Format 2 (48-bit planes): pack (dir 1) or unpack (dir 0) the slots of one digit: src is a copy of
// the digit's 2 x key_limbs slots, dst the key's.  A slot of a prime below 2^48: a 32-bit plane [n]
// then a 16-bit plane [n] (natural order) and KEY_PACK_TAG in the last word; other slots copied.
__global__ void k_key_pack48(const u64 *__restrict__ src, u64 *__restrict__ dst, const unsigned char *__restrict__ packed,
                             int key_limbs, int log_n, int dir)
{
    const size_t n = (size_t)1 << log_n;
    const int slot = blockIdx.y; // poly * key_limbs + limb
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 *s = src + (size_t)slot * n;
    u64 *d = dst + (size_t)slot * n;
    if (!packed[slot % key_limbs])
    {
        d[i] = s[i];
        return;
    }
    if (dir)
    {
        const u64 v = s[i];
        reinterpret_cast<u32 *>(d)[i] = (u32)v;
        reinterpret_cast<unsigned short *>(reinterpret_cast<u32 *>(d) + n)[i] = (unsigned short)(v >> 32);
        if (i == n - 1) d[n - 1] = KEY_PACK_TAG; // in the slot's unused last quarter
    }
    else
    {
        const u32 lo = reinterpret_cast<const u32 *>(s)[i];
        const unsigned short hi = reinterpret_cast<const unsigned short *>(reinterpret_cast<const u32 *>(s) + n)[i];
        d[i] = (u64)lo | ((u64)hi << 32);
    }
}

static int key_pack_run(mhe_ctx *c, u64 *key, int digits, int key_limbs, int dir, int fmt, hipStream_t st)
{
    const size_t n = c->n, slots1 = 2 * (size_t)key_limbs;
    std::vector<unsigned char> pk(key_limbs);
    for (int l = 0; l < key_limbs; l++) pk[l] = key_limb_packed(c, l, key_limbs, fmt) ? 1 : 0;
    HIP_TRY(hipSetDevice(c->device));
    u64 *tmp = nullptr; // format 2: one digit's copy, then the limb table
    const size_t tmp_words = fmt == 2 ? slots1 * n : 0;
    if (hipMalloc(&tmp, tmp_words * sizeof(u64) + 256 + (size_t)key_limbs) != hipSuccess)
        return fail(MHE_ERR_MEMORY, "key prepare: scratch allocation failed");
    unsigned char *pkd = reinterpret_cast<unsigned char *>(tmp + tmp_words);
    int rc = MHE_OK;
    if (hipMemcpyAsync(pkd, pk.data(), key_limbs, hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(MHE_ERR_DEVICE, "key prepare: copy");
    if (fmt == 2)
    {
        for (int J = 0; J < digits && rc == MHE_OK; J++)
        {
            u64 *dg = key + (size_t)J * slots1 * n;
            if (hipMemcpyAsync(tmp, dg, slots1 * n * sizeof(u64), hipMemcpyDeviceToDevice, st) != hipSuccess)
            {
                rc = fail(MHE_ERR_DEVICE, "key prepare: copy");
                break;
            }
            hipLaunchKernelGGL(k_key_pack48, dim3((unsigned)((n + 255) / 256), (unsigned)slots1), dim3(256), 0, st, tmp,
                               dg, pkd, key_limbs, c->log_n, dir);
            if (hipGetLastError() != hipSuccess) rc = fail(MHE_ERR_DEVICE, "key prepare: launch");
        }
    }
    else
    {
        // grid.y is at most 65535 slots per launch: whole groups of key_limbs slots each, so the
        // kernel's slot % key_limbs stays the limb
        const size_t slots = slots1 * (size_t)digits, per = (65535 / (size_t)key_limbs) * (size_t)key_limbs;
        for (size_t s0 = 0; s0 < slots && rc == MHE_OK;)
        {
            const size_t cnt = std::min(per, slots - s0);
            hipLaunchKernelGGL(k_key_pack, dim3((unsigned)((n + 255) / 256), (unsigned)cnt), dim3(256), 0, st,
                               key + s0 * n, pkd, key_limbs, c->log_n, dir);
            if (hipGetLastError() != hipSuccess) rc = fail(MHE_ERR_DEVICE, "key prepare: launch");
            s0 += cnt;
        }
    }
    // the scratch is freed only after the stream has used it
    if (hipStreamSynchronize(st) != hipSuccess && rc == MHE_OK) rc = fail(MHE_ERR_DEVICE, "key prepare: sync");
    (void)hipFree(tmp);
    return rc;
}

// the format mhe_key_prepare makes: MHE_KEY_FMT=2 chooses the 48-bit planes, default doubles
static int default_key_format()
{
    static const int f = [] {
        const char *e = getenv("MHE_KEY_FMT");
        return (e && atoi(e) == 2) ? 2 : 1;
    }();
    return f;
}

MHE_EXPORT int mhe_key_prepare_as(mhe_ctx *c, uint64_t *key, int digits, int key_limbs, int format, void *s)
{
    if (!valid_ctx(c) || !key || digits < 1 || key_limbs < 2 || key_limbs > c->K || digits > key_limbs - 1 ||
        (format != MHE_KEY_FMT_DOUBLE && format != MHE_KEY_FMT_PACK48))
        return fail(MHE_ERR_ARG, "invalid argument");
    int tagged = 0;
    int r = key_tagged(c, key, key_limbs, S(s), &tagged);
    if (r) return r;
    if (tagged) return fail(MHE_ERR_ARG, "key prepare: key is already prepared");
    return key_pack_run(c, key, digits, key_limbs, 1, format, S(s));
}

MHE_EXPORT int mhe_key_prepare(mhe_ctx *c, uint64_t *key, int digits, int key_limbs, void *s)
{
    return mhe_key_prepare_as(c, key, digits, key_limbs, default_key_format(), s);
}

MHE_EXPORT int mhe_key_unprepare(mhe_ctx *c, uint64_t *key, int digits, int key_limbs, void *s)
{
    if (!valid_ctx(c) || !key || digits < 1 || key_limbs < 2 || key_limbs > c->K || digits > key_limbs - 1)
        return fail(MHE_ERR_ARG, "invalid argument");
    int tagged = 0;
    int r = key_tagged(c, key, key_limbs, S(s), &tagged);
    if (r) return r;
    if (!tagged) return fail(MHE_ERR_ARG, "key unprepare: key is not prepared");
    return key_pack_run(c, key, digits, key_limbs, 0, tagged, S(s));
}

MHE_EXPORT int mhe_key_traffic_prepared(mhe_ctx *c, uint64_t *bytes, int reset)
{
    if (!valid_ctx(c) || !bytes) return fail(MHE_ERR_ARG, "invalid argument");
    *bytes = reset ? c->key_bytes_prep.exchange(0) : c->key_bytes_prep.load();
    return MHE_OK;
}

MHE_EXPORT int mhe_key_is_prepared(mhe_ctx *c, const uint64_t *key, int key_limbs, int *prepared, void *s)
{
    if (!valid_ctx(c) || !key || !prepared || key_limbs < 2 || key_limbs > c->K) return fail(MHE_ERR_ARG, "invalid argument");
    return key_tagged(c, key, key_limbs, S(s), prepared);
}

MHE_EXPORT int mhe_stream_wait(mhe_ctx *c, void *waiter, void *waitee)
{
    // device-side ordering: work enqueued on `waiter` after this call starts after everything
    // enqueued on `waitee` before it (no host blocking)
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "invalid argument");
    if (waiter == waitee) return MHE_OK;
    HIP_TRY(hipSetDevice(c->device)); // the event must belong to the engine's device
    // A ring of events per thread and device, re-recorded in turn: a stream wait captures the
    // event's state at the call, so a later record of the same event does not move it.  (Creating
    // and destroying an event per wait cost host time, and destroying one still pending crashed
    // under rocprofv3's API tracing in multi-stream runs, profiles/r04d.)
    struct Ring
    {
        int device = -1;
        hipEvent_t ev[64] = {};
        unsigned next = 0;
    };
    static thread_local Ring ring[8];
    Ring &r = ring[c->device & 7];
    if (r.device != c->device)
    {
        for (auto &e : r.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        r.device = c->device;
    }
    hipEvent_t ev = r.ev[r.next++ & 63];
    hipError_t e = hipEventRecord(ev, S(waitee));
    if (e == hipSuccess) e = hipStreamWaitEvent(S(waiter), ev, 0);
    if (e != hipSuccess) return fail(MHE_ERR_DEVICE, hipGetErrorString(e));
    return MHE_OK;
}

MHE_EXPORT int mhe_ntt_forward(mhe_ctx *c, uint64_t *data, int polys, int limbs, int lazy, void *stream)
{
    TR("data", data, polys, limbs);
    TRC(0, 0, 0, 0);
    int r = check_poly_args(c, data, polys, limbs);
    if (r) return r;
    return run_ntt_fwd(c, data, data, polys, limbs, lazy ? 0 : 1, S(stream));
}

MHE_EXPORT int mhe_ntt_inverse(mhe_ctx *c, uint64_t *data, int polys, int limbs, int lazy, void *stream)
{
    TR("data", data, polys, limbs);
    TRC(0, 0, 0, 0);
    int r = check_poly_args(c, data, polys, limbs);
    if (r) return r;
    return run_ntt_inv(c, data, data, polys, limbs, lazy ? 0 : 1, S(stream));
}

static int launch_addsub(mhe_ctx *c, const u64 *a, const u64 *b, u64 *out, int polys, int limbs, int op, void *st)
{
    mhe_launch l = elem_desc(MHE_LK_ADDSUB, op, a, b, out, polys, limbs, st);
    return elem_entry(c, l);
}

MHE_EXPORT int mhe_add(mhe_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, int polys, int limbs, void *s)
{
    TR("out", out, polys, limbs); TR("a", a, polys, limbs); TR("b", b, polys, limbs);
    TRC(0, 0, 0, 0);
    return launch_addsub(c, a, b, out, polys, limbs, 0, s);
}

MHE_EXPORT int mhe_sub(mhe_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, int polys, int limbs, void *s)
{
    TR("out", out, polys, limbs); TR("a", a, polys, limbs); TR("b", b, polys, limbs);
    TRC(0, 0, 0, 0);
    return launch_addsub(c, a, b, out, polys, limbs, 1, s);
}

MHE_EXPORT int mhe_negate(mhe_ctx *c, const uint64_t *a, uint64_t *out, int polys, int limbs, void *s)
{
    TR("out", out, polys, limbs); TR("a", a, polys, limbs);
    TRC(0, 0, 0, 0);
    return launch_addsub(c, a, nullptr, out, polys, limbs, 2, s);
}

MHE_EXPORT int mhe_multiply_plain(mhe_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, int polys,
                                  int limbs, void *s)
{
    TR("out", out, polys, limbs); TR("a", a, polys, limbs); TR("b", b, 1, limbs);
    TRC(0, 0, 0, 0);
    mhe_launch l = elem_desc(MHE_LK_MULPLAIN, 0, a, b, out, polys, limbs, s);
    return elem_entry(c, l);
}

MHE_EXPORT int mhe_multiply_plain_add(mhe_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *acc, int polys,
                                      int limbs, void *s)
{
    mhe_launch l = elem_desc(MHE_LK_MULPLAIN_ADD, 0, a, b, acc, polys, limbs, s);
    return elem_entry(c, l);
}

MHE_EXPORT int mhe_multiply_plain_sum(mhe_ctx *c, int count, const uint64_t *const *a, const uint64_t *const *b,
                                      uint64_t *out, int accumulate, int polys, int limbs, void *s)
{
    if (count < 1 || !a || !b || !out) return fail(MHE_ERR_ARG, "invalid polynomial arguments");
    for (int k = 0; k < count; k++)
    {
        int r = check_poly_args(c, a[k], polys, limbs);
        if (r) return r;
        if (!b[k]) return fail(MHE_ERR_ARG, "invalid polynomial arguments");
    }
    count_op(c, MHE_OPK_MULPLAIN, limbs, (unsigned long long)polys * count);
    count_op(c, MHE_OPK_ADDSUB, limbs, (unsigned long long)polys * (count - 1 + (accumulate ? 1 : 0)));
    const size_t total2 = ((size_t)polys * limbs << c->log_n) / 2;
    for (int k0 = 0; k0 < count; k0 += MHE_SUM_TERMS)
    {
        const int cnt = std::min(MHE_SUM_TERMS, count - k0);
        SumPtrs P{};
        for (int k = 0; k < cnt; k++)
        {
            P.a[k] = a[k0 + k];
            P.b[k] = b[k0 + k];
        }
        hipLaunchKernelGGL(k_mulplain_sum, ELEM_GRID(total2), dim3(256), 0, S(s), P, cnt, out,
                           (accumulate || k0 > 0) ? 1 : 0, c->primes, limbs, c->log_n, total2, c->nm.fp ? 1 : 0);
        HIP_LAUNCH_CHECK();
    }
    return MHE_OK;
}

MHE_EXPORT int mhe_decrypt(mhe_ctx *c, const uint64_t *ct, int size, const uint64_t *sk, uint64_t *out, int limbs,
                           void *s)
{
    TR("out", out, 1, limbs); TR("ct", ct, size, limbs); TR("sk", sk, 1, limbs);
    TRC(0, 0, 0, 0);
    int r = check_poly_args(c, ct, size, limbs);
    if (r) return r;
    if (size < 2 || !sk || !out) return fail(MHE_ERR_ARG, "invalid polynomial arguments");
    // the op mix of the sequence this replaces: s^2..s^(size-1) and the size - 1 products c_k s^k
    // as plaintext products, and size - 1 additions
    count_op(c, MHE_OPK_MULPLAIN, limbs, (unsigned long long)(2 * size - 3));
    count_op(c, MHE_OPK_ADDSUB, limbs, (unsigned long long)(size - 1));
    const size_t total2 = ((size_t)limbs << c->log_n) / 2;
    hipLaunchKernelGGL(k_decrypt, ELEM_GRID(total2), dim3(256), 0, S(s), ct, size, sk, out, c->primes, limbs, c->log_n,
                       total2, c->nm.fp ? 1 : 0);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

// op 2 (set): a is out.  The table is copied into the descriptor once limbs is known to be in range.
static int launch_scalar(mhe_ctx *c, const u64 *a, const u64 *scalars, u64 *out, int polys, int limbs, int op,
                         void *s)
{
    int r = check_poly_args(c, a, polys, limbs);
    if (r) return r;
    if (!scalars) return fail(MHE_ERR_ARG, "invalid polynomial arguments");
    mhe_launch l = elem_desc(MHE_LK_SCALAR, op, a, nullptr, out, polys, limbs, s);
    std::copy(scalars, scalars + limbs, l.scalars);
    return elem_entry(c, l);
}

MHE_EXPORT int mhe_multiply_scalar(mhe_ctx *c, const uint64_t *a, const uint64_t *scalars, uint64_t *out, int polys,
                                   int limbs, void *s)
{
    TR("out", out, polys, limbs); TR("a", a, polys, limbs);
    TRC(0, 0, 0, 0);
    return launch_scalar(c, a, scalars, out, polys, limbs, 0, s);
}

MHE_EXPORT int mhe_add_scalar(mhe_ctx *c, const uint64_t *a, const uint64_t *scalars, uint64_t *out, int polys,
                              int limbs, void *s)
{
    TR("out", out, polys, limbs); TR("a", a, polys, limbs);
    TRC(0, 0, 0, 0);
    return launch_scalar(c, a, scalars, out, polys, limbs, 1, s);
}

MHE_EXPORT int mhe_set_scalar(mhe_ctx *c, const uint64_t *scalars, uint64_t *out, int polys, int limbs, void *s)
{
    return launch_scalar(c, out, scalars, out, polys, limbs, 2, s);
}

// the tensor product inside HMult: operands from the pipeline, not offered to the hook
static int launch_tensor(mhe_ctx *c, const u64 *a, const u64 *b, u64 *out3, int L, int square, hipStream_t st)
{
    mhe_launch l = elem_desc(MHE_LK_TENSOR, square, a, b, out3, 2, L, st), *g = &l;
    return elem_launch(c, &g, 1);
}

MHE_EXPORT int mhe_ct_multiply(mhe_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out3, int limbs, void *s)
{
    TR("out3", out3, 3, limbs); TR("a", a, 2, limbs); TR("b", b, 2, limbs);
    TRC(0, 0, 0, 0);
    mhe_launch l = elem_desc(MHE_LK_TENSOR, 0, a, b, out3, 2, limbs, s);
    return elem_entry(c, l);
}

MHE_EXPORT int mhe_ct_square(mhe_ctx *c, const uint64_t *a, uint64_t *out3, int limbs, void *s)
{
    TR("out3", out3, 3, limbs); TR("a", a, 2, limbs);
    TRC(0, 0, 0, 0);
    mhe_launch l = elem_desc(MHE_LK_TENSOR, 1, a, a, out3, 2, limbs, s);
    return elem_entry(c, l);
}

MHE_EXPORT int mhe_switch_key(mhe_ctx *c, uint64_t *ct, const uint64_t *target, const uint64_t *key, int key_limbs,
                              int limbs, void *s)
{
    TR("ct", ct, 2, limbs); TR("target", target, 1, limbs); TR("key", key, 2 * limbs, key_limbs);
    TRC(0, 0, 0, 0);
    int r = check_limbs(c, limbs, 1);
    if (r) return r;
    if (!ct || !target || !key) return fail(MHE_ERR_ARG, "target_iter");
    return run_switch_key(c, ct, target, key, key_limbs, limbs, S(s));
}

MHE_EXPORT int mhe_relinearize(mhe_ctx *c, uint64_t *ct3, const uint64_t *key, int key_limbs, int limbs, void *s)
{
    TR("ct3", ct3, 3, limbs); TR("key", key, 2 * limbs, key_limbs);
    TRC(0, 0, 0, 0);
    int r = check_limbs(c, limbs, 1);
    if (r) return r;
    if (!ct3 || !key) return fail(MHE_ERR_ARG, "relin_keys is not valid for encryption parameters");
    return run_switch_key(c, ct3, ct3 + ((size_t)2 * limbs << c->log_n), key, key_limbs, limbs, S(s));
}

static int launch_galois(mhe_ctx *c, const u64 *in, u32 elt, u64 *out, int polys, int limbs, hipStream_t st)
{
    int r = check_galois_elt(c, elt);
    if (r) return r;
    count_op(c, MHE_OPK_GALOIS, limbs, (unsigned long long)polys);
    size_t total = (size_t)polys * limbs << c->log_n;
    hipLaunchKernelGGL(k_galois, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, out, elt, c->log_n,
                       total);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

MHE_EXPORT int mhe_permute_galois(mhe_ctx *c, const uint64_t *in, uint32_t elt, uint64_t *out, int polys, int limbs,
                                  void *s)
{
    TR("out", out, polys, limbs); TR("in", in, polys, limbs);
    TRC(0, 0, 0, 0);
    int r = check_poly_args(c, in, polys, limbs);
    if (r) return r;
    if (!out || out == in) return fail(MHE_ERR_ARG, "result cannot point to the same value as operand");
    return launch_galois(c, in, elt, out, polys, limbs, S(s));
}

MHE_EXPORT int mhe_apply_galois(mhe_ctx *c, uint64_t *ct, uint32_t elt, const uint64_t *key, int key_limbs, int limbs,
                                void *s)
{
    TR("ct", ct, 2, limbs); TR("key", key, 2 * limbs, key_limbs);
    TRC(0, 0, 0, 0);
    int r = check_limbs(c, limbs, 1);
    if (r) return r;
    if (!ct || !key) return fail(MHE_ERR_ARG, "Galois key not present");
    hipStream_t st = S(s);
    Workspace *w;
    r = get_ws(c, st, c->K - 1, &w);
    if (r) return r;
    const size_t ps = (size_t)limbs << c->log_n;
    // evaluator.cpp:2193-2214: c0 <- perm(c0) (via tmp), tmp <- perm(c1), c1 <- 0, then KS(tmp)
    r = launch_galois(c, ct, elt, w->tmp, 1, limbs, st);
    if (r) return r;
    HIP_TRY(mhe_internal_copy_d2d(ct, w->tmp, ps * sizeof(u64), st));
    r = launch_galois(c, ct + ps, elt, w->tmp, 1, limbs, st);
    if (r) return r;
    if (!c->galois_fused) HIP_TRY(hipMemsetAsync(ct + ps, 0, ps * sizeof(u64), st));
    return run_switch_key(c, ct, w->tmp, key, key_limbs, limbs, st, nullptr, c->galois_fused); // c1 <- 0 + KS_1
}

MHE_EXPORT int mhe_apply_galois_to(mhe_ctx *c, const uint64_t *in, uint64_t *out, uint32_t elt, const uint64_t *key,
                                   int key_limbs, int limbs, void *s)
{
    TR("out", out, 2, limbs); TR("in", in, 2, limbs);
    TRC(0, 0, 0, 0);
    int r = check_limbs(c, limbs, 1);
    if (r) return r;
    if (!in || !out || !key) return fail(MHE_ERR_ARG, "Galois key not present");
    if (in == out) return fail(MHE_ERR_ARG, "result cannot point to the same value as operand");
    hipStream_t st = S(s);
    Workspace *w;
    r = get_ws(c, st, c->K - 1, &w);
    if (r) return r;
    const size_t ps = (size_t)limbs << c->log_n;
    // evaluator.cpp:2193-2214: out0 <- perm(c0), out1 <- perm(c1) (one launch), then the key switch
    // of out1 with out0 += KS_0 and out1 = KS_1 (SEAL zeroes c1 and adds; same words)
    if (c->galois_fused)
    {
        r = launch_galois(c, in, elt, out, 2, limbs, st);
        if (r) return r;
        return run_switch_key(c, out, out + ps, key, key_limbs, limbs, st, nullptr, 1);
    }
    r = launch_galois(c, in, elt, out, 1, limbs, st);
    if (r) return r;
    r = launch_galois(c, in + ps, elt, w->tmp, 1, limbs, st);
    if (r) return r;
    HIP_TRY(hipMemsetAsync(out + ps, 0, ps * sizeof(u64), st));
    return run_switch_key(c, out, w->tmp, key, key_limbs, limbs, st);
}

// ------------------------------- what rotate-and-sum and relinearize-sum-rescale share
#include "groupsum.h"

// ------------------------------------------ batched rotations, hoisting and rotate-and-sum
#include "rotate.h"

// ------------------------------------------------- sums of relinearized products, rescaled
#include "prodsum.h"

// ------------------------------------------------------- public-key encryption of a batch
#include "encrypt.h"

// ---------------------------------------- symmetric encryption of a batch: key-switching keys
#include "keygen.h"

MHE_EXPORT int mhe_rescale_batch(mhe_ctx *c, int count, const uint64_t *const *in, uint64_t *const *out, int size,
                                 int limbs, void *s)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    if (limbs < 2) return fail(MHE_ERR_RANGE, "end of modulus switching chain reached");
    if (limbs > c->K || size < 1 || size > 3 || count < 0 || (count && (!in || !out)))
        return fail(MHE_ERR_ARG, "encrypted is not valid for encryption parameters");
    const size_t iw = ((size_t)size * limbs) << c->log_n, ow = ((size_t)size * (limbs - 1)) << c->log_n;
    for (int i = 0; i < count; i++)
    {
        if (!in[i] || !out[i]) return fail(MHE_ERR_ARG, "encrypted is not valid for encryption parameters");
        // an output may share no word with any entry's input or with another output: the last pass
        // writes out[i] while other workgroups of the same launch still read their inputs
        if (output_overlaps(out, i, count, ow, in, count, iw))
            return fail(MHE_ERR_ARG, "rescale output must not alias its input");
    }
    for (int i0 = 0; i0 < count; i0 += MHE_MAXB)
    {
        const int B = std::min(MHE_MAXB, count - i0);
        int r = run_rescale_batch(c, in + i0, out + i0, B, size, limbs, S(s));
        if (r) return r;
    }
    return MHE_OK;
}

MHE_EXPORT int mhe_switch_key_batch(mhe_ctx *c, int count, uint64_t *const *ct, const uint64_t *const *target,
                                    const uint64_t *const *keys, const int *key_limbs, int limbs, void *s)
{
    int r = check_limbs(c, limbs, 1);
    if (r) return r;
    if (count < 0 || (count && (!ct || !target || !keys || !key_limbs))) return fail(MHE_ERR_ARG, "invalid argument");
    for (int i = 0; i < count; i++)
    {
        if (!ct[i] || !target[i] || !keys[i]) return fail(MHE_ERR_ARG, "target_iter");
        // every key before the first launch: the switches work in place, chunk by chunk
        if ((r = check_key_limbs(c, key_limbs[i], limbs))) return r;
    }
    for (int i0 = 0; i0 < count; i0 += MHE_MAXB)
    {
        const int B = std::min(MHE_MAXB, count - i0);
        KsJob jobs[MHE_MAXB];
        for (int e = 0; e < B; e++) jobs[e] = KsJob{ ct[i0 + e], target[i0 + e], keys[i0 + e], key_limbs[i0 + e], nullptr };
        if ((r = run_switch_key_batch(c, jobs, B, limbs, S(s)))) return r;
    }
    return MHE_OK;
}

MHE_EXPORT int mhe_rescale_to_next(mhe_ctx *c, const uint64_t *in, uint64_t *out, int size, int limbs, void *s)
{
    TR("out", out, size, (limbs - 1)); TR("in", in, size, limbs);
    TRC(0, 0, 0, 0);
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    if (limbs < 2) return fail(MHE_ERR_RANGE, "end of modulus switching chain reached");
    if (limbs > c->K || size < 1 || size > 3 || !in || !out)
        return fail(MHE_ERR_ARG, "encrypted is not valid for encryption parameters");
    if (in == out) return fail(MHE_ERR_ARG, "rescale output must not alias its input");
    return run_rescale(c, in, out, size, limbs, S(s));
}

MHE_EXPORT int mhe_modraise(mhe_ctx *c, const uint64_t *in, uint64_t *out, int size, int limbs, void *s)
{
    TR("out", out, size, limbs); TR("in", in, size, 1);
    TRC(0, 0, 0, 0);
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    if (!in || !out || size < 1 || limbs < 1 || limbs > c->K) return fail(MHE_ERR_ARG, "invalid polynomial arguments");
    const size_t total = ((size_t)size * limbs) << c->log_n;
    hipLaunchKernelGGL(k_modraise, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S(s), in, out, c->primes,
                       limbs, c->log_n, total);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

MHE_EXPORT int mhe_mod_switch_drop(mhe_ctx *c, const uint64_t *in, uint64_t *out, int size, int limbs, void *s)
{
    TR("out", out, size, (limbs - 1)); TR("in", in, size, limbs);
    TRC(0, 0, 0, 0);
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    if (limbs < 2) return fail(MHE_ERR_RANGE, "end of modulus switching chain reached");
    if (!in || !out || size < 1) return fail(MHE_ERR_ARG, "invalid polynomial arguments");
    const size_t src_pitch = ((size_t)limbs << c->log_n) * sizeof(u64);
    const size_t dst_pitch = ((size_t)(limbs - 1) << c->log_n) * sizeof(u64);
    if (in != out)
    {
        for (int p = 0; p < size; p++)
            HIP_TRY(mhe_internal_copy_d2d((char *)out + p * dst_pitch, (const char *)in + p * src_pitch, dst_pitch,
                                          S(s)));
        return MHE_OK;
    }
    // In place: component p moves down by p limbs.  One copy per limb, ascending: every copy's
    // source and destination are disjoint (they are p*n words apart), and a destination never
    // covers a source that a later copy still has to read.
    const size_t limb_bytes = sizeof(u64) << c->log_n;
    for (int p = 1; p < size; p++)
        for (int l = 0; l + 1 < limbs; l++)
            HIP_TRY(mhe_internal_copy_d2d((char *)out + p * dst_pitch + l * limb_bytes,
                                          (const char *)in + p * src_pitch + l * limb_bytes, limb_bytes, S(s)));
    return MHE_OK;
}

MHE_EXPORT int mhe_hmult_batch(mhe_ctx *c, int count, const uint64_t *const *a, const uint64_t *const *b,
                               const uint64_t *key, int key_limbs, uint64_t *const *out, int limbs, void *s)
{
    // mhe_hmult of every entry, MHE_MAXB per key switch: the tensor products into per-entry
    // scratch, then one batched key switch (all entries share the relinearization key, so
    // k_ks_row_mac reads it once per XCD) with the fused rescale tail -- bit-identical to count
    // mhe_hmult calls
    int r = check_limbs(c, limbs, 2);
    if (r) return r;
    if (count < 0 || (count && (!a || !b || !out)) || !key) return fail(MHE_ERR_ARG, "invalid argument");
    if ((r = check_key_limbs(c, key_limbs, limbs))) return r;
    const size_t iw = (size_t)2 * limbs * c->n, ow = (size_t)2 * (limbs - 1) * c->n;
    for (int i = 0; i < count; i++)
    {
        if (!a[i] || !b[i] || !out[i]) return fail(MHE_ERR_ARG, "invalid argument");
        // out[i] may overlap its own operands (they are consumed by the tensor product before the
        // tail writes out[i]) but no other entry's operands (a later chunk reads them after this
        // chunk's tail) and no other output
        for (int j = 0; j < count; j++)
        {
            if (j == i) continue;
            if (ranges_overlap(out[i], ow, out[j], ow)) return fail(MHE_ERR_ARG, "outputs must be distinct");
            if (ranges_overlap(out[i], ow, a[j], iw) || ranges_overlap(out[i], ow, b[j], iw))
                return fail(MHE_ERR_ARG, "result cannot point to the same value as another entry's operand");
        }
    }
    hipStream_t st = S(s);
    const size_t n = c->n;
    for (int i0 = 0; i0 < count; i0 += MHE_MAXB)
    {
        const int B = std::min(MHE_MAXB, count - i0);
        Workspace *w;
        if ((r = get_ws(c, st, c->K - 1, &w, B))) return r;
        KsJob jobs[MHE_MAXB];
        for (int e = 0; e < B; e++)
        {
            const int i = i0 + e;
            if ((r = launch_tensor(c, a[i], b[i], w->e[e].ct3, limbs, a[i] == b[i], st))) return r;
            jobs[e] = KsJob{ w->e[e].ct3, w->e[e].ct3 + ((size_t)2 * limbs * n), key, key_limbs,
                             c->hmult_fused ? out[i] : nullptr };
        }
        if ((r = run_switch_key_batch(c, jobs, B, limbs, st))) return r;
        if (!c->hmult_fused)
        {
            const u64 *in[MHE_MAXB];
            u64 *o[MHE_MAXB];
            for (int e = 0; e < B; e++)
            {
                in[e] = w->e[e].ct3;
                o[e] = out[i0 + e];
            }
            if ((r = run_rescale_batch(c, in, o, B, 2, limbs, st))) return r;
        }
    }
    return MHE_OK;
}

MHE_EXPORT int mhe_hmult(mhe_ctx *c, const uint64_t *a, const uint64_t *b, const uint64_t *key, int key_limbs,
                         uint64_t *out, int limbs, void *s)
{
    int r = check_limbs(c, limbs, 2);
    if (r) return r;
    if (!a || !b || !key || !out) return fail(MHE_ERR_ARG, "invalid argument");
    return mhe_hmult_batch(c, 1, &a, &b, key, key_limbs, &out, limbs, s); // one entry: the same launches
}
