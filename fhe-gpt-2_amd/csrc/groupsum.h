// Grouped sums of key switches: what mhe_rotate_sum (rotate.h) and mhe_relin_sum_rescale (prodsum.h)
// share -- the accumulate kernel, the group accumulators' scratch, and the steps between the key
// products and the callers' tails.  The launches of a call are planned by groupsum_plan.h.  Included
// by mhe.hip once, after keyswitch.h.
//
// Entry e's key switch leaves acc^e [2][L+1][n].  Every special limb goes through its own inverse NTT
// ([0, 2P)) and SEAL's integer lift to each data prime (evaluator.cpp:2466-2524); everything after the
// lift is linear mod q_i, so per group
//     A = m sum_e acc^e,   T = m sum_e lift(acc^e[L]),   X = m sum_e x^e      (m = 2 when doubled)
// are formed first (sums of canonical residues mod q_i: the special limbs are never added mod P) and
// the ModDown runs once per group.  x^e is the caller's extra summand.
#pragma once

#include "groupsum_plan.h"

struct GroupSumPtrs
{
    const u64 *acc[MHE_MAXB]; // entry: key products [2][L+1][n], special limbs in coefficient form
    const u64 *x[MHE_MAXB];   // entry: the extra summand [xpolys][L][n]
    int zof[MHE_MAXB];        // entry: its group among the chunk's
    u64 *A[MHE_MAXB];         // group: sum of the key products [2][L+1][n] (limbs 0 .. L-1 used)
    u64 *T[MHE_MAXB];         // group: sum of the lifted special limbs [2][L][n], coefficient form
    u64 *X[MHE_MAXB];         // group: sum of the extra summands [xpolys][L][n]
    int first[MHE_MAXB];      // group: its first chunk (A and T written, not added to)
    int firstx[MHE_MAXB];     // group: X written, not added to
    int twice[MHE_MAXB];      // group: the sum is doubled (each chunk's share is, which is the same words)
    int B;                    // entries in the chunk
    int xpolys;               // polys of the extra summand, 1 or 2
};

// grid (n / 512, 2 * L, groups in the chunk); one lane owns two adjacent words of (group, k, i): no
// atomics, no LDS, 16-byte accesses.  Every operand is a canonical residue, so the order of the
// additions does not change a word.
__global__ __launch_bounds__(256) void k_groupsum_acc(GroupSumPtrs P, const PrimeDev *__restrict__ primes, int L, int K,
                                                      int log_n)
{
    const int z = blockIdx.z, k = blockIdx.y / L, i = blockIdx.y - k * L;
    const size_t x = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t n = (size_t)1 << log_n;
    const PrimeDev p = prime_at(primes, i);
    const ModDownLift md = moddown_lift(primes, i, K);
    const u64 q = p.q;
    const bool ext = k < P.xpolys; // uniform over the workgroup
    const size_t oa = (size_t)(k * (L + 1) + i) * n + x, os = (size_t)(k * (L + 1) + L) * n + x;
    const size_t ot = (size_t)(k * L + i) * n + x; // T, and the extra summand and its sum
    auto ld = [](const u64 *s) { return *(const ulonglong2 *)s; };
    auto add = [q](ulonglong2 &s, ulonglong2 v) {
        s.x = addmod(s.x, v.x, q);
        s.y = addmod(s.y, v.y, q);
    };
    // the prior sums, read ahead of the loop (zero where this chunk writes: adding it changes nothing)
    ulonglong2 a0{ 0, 0 }, t0{ 0, 0 }, d0{ 0, 0 };
    if (!P.first[z])
    {
        a0 = ld(P.A[z] + oa);
        t0 = ld(P.T[z] + ot);
    }
    if (ext && !P.firstx[z]) d0 = ld(P.X[z] + ot);
    ulonglong2 a{ 0, 0 }, t{ 0, 0 }, d{ 0, 0 };
    for (int e = 0; e < P.B; e++)
    {
        if (P.zof[e] != z) continue; // uniform over the workgroup
        const ulonglong2 se = ld(P.acc[e] + os);
        add(a, ld(P.acc[e] + oa));
        add(t, ulonglong2{ csub(md.lift(se.x, p), q), csub(md.lift(se.y, p), q) }); // lift() is in [0, 2q)
        if (ext) add(d, ld(P.x[e] + ot));
    }
    if (P.twice[z])
    {
        add(a, a);
        add(t, t);
        add(d, d);
    }
    add(a, a0);
    add(t, t0);
    add(d, d0);
    *(ulonglong2 *)(P.A[z] + oa) = a;
    *(ulonglong2 *)(P.T[z] + ot) = t;
    if (ext) *(ulonglong2 *)(P.X[z] + ot) = d;
}

// The scratch of a grouped sum on stream st: the workspace for `entries` batch entries and the pool's
// accumulators of MHE_MAXB groups at L limbs (grown, after draining the stream, when a call needs a
// higher level).
static int get_groupsum(mhe_ctx *c, hipStream_t st, int entries, int L, SumPool Workspace::*pool, Workspace **out)
{
    Workspace *w;
    int r = get_ws(c, st, c->K - 1, &w, entries);
    if (r) return r;
    std::lock_guard<std::mutex> g(w->mu);
    SumPool &sp = w->*pool;
    if (sp.limbs < L)
    {
        sp.limbs = 0;
        if ((r = sp.buf.grow(c, st, (size_t)MHE_MAXB * ((size_t)sp.words * L + 2) * c->n * sizeof(u64)))) return r;
        sp.limbs = L;
    }
    *out = w;
    return MHE_OK;
}

// The accumulate kernel's pointers of a chunk, but for what the caller knows: x, X, firstx and twice.
static GroupSumPtrs groupsum_ptrs(const GroupSumChunk &ch, const Workspace *w, const SumPool &sp, int xpolys, int L, size_t n)
{
    GroupSumPtrs gp{};
    gp.B = (int)ch.entries.size();
    gp.xpolys = xpolys;
    for (int e = 0; e < gp.B; e++)
    {
        gp.acc[e] = w->e[e].acc;
        gp.zof[e] = ch.zof[e];
    }
    for (int z = 0; z < ch.Z(); z++)
    {
        gp.A[z] = sp.at(ch.slot[z], 0, L, n);
        gp.T[z] = sp.at(ch.slot[z], 1, L, n);
        gp.first[z] = ch.first[z];
    }
    return gp;
}

// A chunk: the key switch of every entry's target up to the key products (evaluator.cpp:2281-2463),
// each entry's special limbs through their own inverse NTT, [0, 2P), then the chunk folded into its Z
// groups' accumulators.
static int groupsum_fold(mhe_ctx *c, Workspace *w, const KsJob *jobs, const GroupSumPtrs &gp, int Z, int L, hipStream_t st)
{
    int special_inv_done = 0;
    if (int r = run_switch_key_batch(c, jobs, gp.B, L, st, 0, &special_inv_done)) return r;
    JobB<JobStrided> sj(2);
    for (int e = 0; e < gp.B; e++) sj.j[e] = special_limbs(c, w->e[e].acc, L);
    if (!special_inv_done) inv_row(sj, c->log_n, 2 * gp.B, c->nm, st);
    inv_col(sj, c->log_n, 2 * gp.B, c->nm, st);
    hipLaunchKernelGGL(k_groupsum_acc, dim3((unsigned)(c->n / 512), (unsigned)(2 * L), (unsigned)Z), dim3(256), 0, st, gp,
                       c->primes, L, c->K, c->log_n);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

// The adds of the sequence a round replaces, per group: one less than its terms, `extra` more, and
// one more where twice[group] (twice may be null).
static void groupsum_count_adds(mhe_ctx *c, const GroupSumRound &r, int L, int extra, const int *twice)
{
    for (int z = 0; z < r.G; z++)
    {
        const int more = extra + ((twice && twice[r.g0 + z]) ? 1 : 0);
        count_op(c, MHE_OPK_ADDSUB, L, 2ull * (unsigned long long)(r.terms[z] - 1 + more));
    }
}

// mhe_rotsum_stats / mhe_prodsum_stats over the context's counters cs (sums) and ct (terms)
template <class Counter>
static int groupsum_stats(mhe_ctx *c, Counter cs, Counter ct, uint64_t *sums, uint64_t *terms, int reset)
{
    if (!valid_ctx(c) || !sums || !terms) return fail(MHE_ERR_ARG, "invalid argument");
    *sums = reset ? (c->*cs).exchange(0) : (c->*cs).load();
    *terms = reset ? (c->*ct).exchange(0) : (c->*ct).load();
    return MHE_OK;
}
