// Sums of relinearized products with the rescale fused behind them (host side and the accumulate
// kernel): mhe_relin_sum_rescale and its counters.  Included by mhe.hip once, after rotate.h.
//
// Term e of a group has the size-3 product (d0, d1, d2)^e; its key switch leaves acc^e [2][L+1][n].
// Every special limb goes through its own inverse NTT and SEAL's integer lift to each data prime
// (evaluator.cpp:2466-2524); everything after the lift is linear mod q_i, so per group
//     C = m sum_e d^e,   A = m sum_e acc^e,   T = m sum_e lift(acc^e[L])      (m = 2 when doubled)
// are formed first (sums of canonical residues mod q_i: the special limbs are never added mod P) and
// the ModDown and the rescale then run once per group through one forward NTT per limb, as the fused
// HMult tail does for one product (jobs.h JobMDRCol / JobMDRRow, JobProdSumCol here).
#pragma once

struct ProdSumPtrs
{
    const u64 *acc[MHE_MAXB]; // entry: key products [2][L+1][n], special limbs in coefficient form
    const u64 *ct3[MHE_MAXB]; // entry: the product [3][L][n] (polys 0 and 1 read)
    u64 *A[MHE_MAXB];         // group: sum of the key products [2][L+1][n] (limbs 0 .. L-1 used)
    u64 *T[MHE_MAXB];         // group: sum of the lifted special limbs [2][L][n], coefficient form
    u64 *C[MHE_MAXB];         // group: sum of the products' polys 0 and 1 [2][L][n]
    int zof[MHE_MAXB];        // entry: its group among the chunk's
    int B;                    // entries in the chunk
    int first[MHE_MAXB];      // group: its first chunk (A, T and C written, not added to)
    int twice[MHE_MAXB];      // group: the sum is doubled (each chunk's share is, which is the same words)
};

// grid (n / 512, 2 * L, groups in the chunk); one lane owns two adjacent words of (group, k, i).
// k_rotsum_acc's shape (rotate.h, left as it is): no atomics, no LDS, 16-byte accesses.
__global__ __launch_bounds__(256) void k_prodsum_acc(ProdSumPtrs P, const PrimeDev *__restrict__ primes, int L, int K,
                                                     int log_n)
{
    const int z = blockIdx.z, k = blockIdx.y / L, i = blockIdx.y - k * L;
    const size_t x = ((size_t)blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t n = (size_t)1 << log_n;
    JobModDownCol::View v; // the ModDown column pass's lift, with its constants
    v.p = prime_at(primes, i);
    v.P = prime_at(primes, K - 1);
    v.half = v.P.q >> 1;
    v.fix = v.p.q - barrett64(v.half, v.p);
    v.reduce = v.P.q > v.p.q;
    const u64 q = v.p.q;
    const size_t oa = (size_t)(k * (L + 1) + i) * n + x, os = (size_t)(k * (L + 1) + L) * n + x;
    const size_t ot = (size_t)(k * L + i) * n + x; // T and C, and polys 0 / 1 of a product
    ulonglong2 a{ 0, 0 }, t{ 0, 0 }, d{ 0, 0 };
    for (int e = 0; e < P.B; e++)
    {
        if (P.zof[e] != z) continue; // uniform over the workgroup
        const ulonglong2 ae = *(const ulonglong2 *)(P.acc[e] + oa);
        const ulonglong2 se = *(const ulonglong2 *)(P.acc[e] + os);
        const ulonglong2 de = *(const ulonglong2 *)(P.ct3[e] + ot);
        a.x = addmod(a.x, ae.x, q);
        a.y = addmod(a.y, ae.y, q);
        t.x = addmod(t.x, csub(v.lift(se.x), q), q); // lift() is in [0, 2q)
        t.y = addmod(t.y, csub(v.lift(se.y), q), q);
        d.x = addmod(d.x, de.x, q);
        d.y = addmod(d.y, de.y, q);
    }
    if (P.twice[z])
    {
        a.x = addmod(a.x, a.x, q);
        a.y = addmod(a.y, a.y, q);
        t.x = addmod(t.x, t.x, q);
        t.y = addmod(t.y, t.y, q);
        d.x = addmod(d.x, d.x, q);
        d.y = addmod(d.y, d.y, q);
    }
    if (!P.first[z])
    {
        const ulonglong2 a0 = *(const ulonglong2 *)(P.A[z] + oa);
        const ulonglong2 t0 = *(const ulonglong2 *)(P.T[z] + ot);
        const ulonglong2 d0 = *(const ulonglong2 *)(P.C[z] + ot);
        a.x = addmod(a.x, a0.x, q);
        a.y = addmod(a.y, a0.y, q);
        t.x = addmod(t.x, t0.x, q);
        t.y = addmod(t.y, t0.y, q);
        d.x = addmod(d.x, d0.x, q);
        d.y = addmod(d.y, d0.y, q);
    }
    *(ulonglong2 *)(P.A[z] + oa) = a;
    *(ulonglong2 *)(P.T[z] + ot) = t;
    *(ulonglong2 *)(P.C[z] + ot) = d;
}

// The scratch of mhe_relin_sum_rescale on stream st: the workspace for `entries` batch entries and
// A, T and C of MHE_MAXB groups at L limbs, (6L + 2) n words per group slot (grown, after draining the
// stream, when a call needs a higher level).
static int get_prodsum(mhe_ctx *c, hipStream_t st, int entries, int L, Workspace **out)
{
    Workspace *w;
    int r = get_ws(c, st, c->K - 1, &w, entries);
    if (r) return r;
    std::lock_guard<std::mutex> g(w->mu);
    if (w->ps_limbs < L)
    {
        w->ps_limbs = 0;
        if ((r = w->ps_base.grow(c, st, (size_t)MHE_MAXB * (6 * (size_t)L + 2) * c->n * sizeof(u64)))) return r;
        w->ps_limbs = L;
    }
    *out = w;
    return MHE_OK;
}

MHE_EXPORT int mhe_prodsum_stats(mhe_ctx *c, uint64_t *sums, uint64_t *terms, int reset)
{
    if (!valid_ctx(c) || !sums || !terms) return fail(MHE_ERR_ARG, "invalid argument");
    *sums = reset ? c->prodsum_sums.exchange(0) : c->prodsum_sums.load();
    *terms = reset ? c->prodsum_terms.exchange(0) : c->prodsum_terms.load();
    return MHE_OK;
}

// The sequence the merged path replaces, one entry at a time (the separate-MAC debugging path):
// relinearize a copy of each product, add, double, rescale.
static int prodsum_one_by_one(mhe_ctx *c, int count, const u64 *const *ct3, const int *group, int groups,
                              const int *twice, const u64 *key, int key_limbs, u64 *const *out, int L, hipStream_t st)
{
    const size_t ps = (size_t)L << c->log_n;
    u64 *buf = nullptr;
    if (injected_alloc_failure(c) || mhe_internal_alloc((void **)&buf, 4 * ps * sizeof(u64), st) != hipSuccess)
        return fail(MHE_ERR_MEMORY, "device allocation failed");
    u64 *sum = buf, *tmp = buf + 2 * ps;
    int r = MHE_OK;
    for (int i = 0; i < count && !r; i++)
    {
        const bool first = i == 0 || group[i] != group[i - 1], last = i + 1 == count || group[i + 1] != group[i];
        u64 *dst = first ? sum : tmp;
        if (mhe_internal_copy_d2d(dst, ct3[i], 2 * ps * sizeof(u64), st) != hipSuccess)
            r = fail(MHE_ERR_DEVICE, "device copy failed");
        if (!r) r = run_switch_key(c, dst, ct3[i] + 2 * ps, key, key_limbs, L, st);
        if (!r && !first) r = launch_addsub(c, sum, tmp, sum, 2, L, 0, st);
        if (!r && last && twice && twice[group[i]]) r = launch_addsub(c, sum, sum, sum, 2, L, 0, st);
        if (!r && last) r = run_rescale(c, sum, out[group[i]], 2, L, st);
    }
    (void)groups;
    (void)mhe_internal_free(buf, st);
    return r;
}

MHE_EXPORT int mhe_relin_sum_rescale(mhe_ctx *c, int count, const uint64_t *const *ct3, const int *group, int groups,
                                     const int *twice, const uint64_t *key, int key_limbs, uint64_t *const *out,
                                     int limbs, void *s)
{
    int r = check_limbs(c, limbs, 1);
    if (r) return r;
    if (limbs < 2) return fail(MHE_ERR_RANGE, "end of modulus switching chain reached");
    if (count < 0 || groups < 0 || (count && (!ct3 || !group)) || (groups && !out) || !key)
        return fail(MHE_ERR_ARG, "invalid argument");
    hipStream_t st = S(s);
    const int L = limbs;
    const size_t n = c->n, ps = (size_t)L << c->log_n;
    // group[] non-decreasing from 0 to groups - 1 without a gap: no group is empty
    for (int i = 0, prev = 0; i < count; prev = group[i++])
        if (group[i] != prev && !(i > 0 && group[i] == prev + 1)) return fail(MHE_ERR_ARG, "invalid argument");
    if ((count ? group[count - 1] + 1 : 0) != groups) return fail(MHE_ERR_ARG, "invalid argument");
    for (int i = 0; i < count; i++)
        if (!ct3[i]) return fail(MHE_ERR_ARG, "invalid argument");
    for (int g = 0; g < groups; g++)
        if (!out[g]) return fail(MHE_ERR_ARG, "invalid argument");
    if ((r = check_key_limbs(c, key_limbs, limbs))) return r;
    // outputs must be disjoint from every input and from each other (a round's outputs are written
    // while later rounds still read their products)
    for (int g = 0; g < groups; g++)
        if (output_overlaps(out, g, groups, 2 * (ps - n), ct3, count, 3 * ps))
            return fail(MHE_ERR_ARG, "result cannot point to the same value as operand");
    if (!count) return MHE_OK;
    if (!c->ks_fused) return prodsum_one_by_one(c, count, ct3, group, groups, twice, key, key_limbs, out, L, st);
    Workspace *w;
    bool doubled = false;
    for (int g = 0; twice && g < groups; g++) doubled = doubled || twice[g];
    if (count == groups && !doubled && c->hmult_fused)
    {
        // every sum a single product, none doubled: nothing to add, so each product takes the fused
        // HMult tail as it is (run_moddown's hm branch: the same one forward NTT per limb, without the
        // pass over A, T and C; it measured ahead of the accumulate kernel at this shape, DESIGN.md
        // §17).  The tail works on a copy of the product's first two polys: the input stays const.
        if ((r = get_ws(c, st, c->K - 1, &w, std::min(count, MHE_MAXB)))) return r;
        for (int b0 = 0; b0 < count; b0 += MHE_MAXB)
        {
            const int B = std::min(MHE_MAXB, count - b0);
            KsJob jobs[MHE_MAXB];
            for (int e = 0; e < B; e++)
            {
                HIP_TRY(mhe_internal_copy_d2d(w->e[e].ct3, ct3[b0 + e], 2 * ps * sizeof(u64), st));
                jobs[e] = KsJob{ w->e[e].ct3, ct3[b0 + e] + 2 * ps, key, key_limbs, out[b0 + e] };
            }
            if ((r = run_switch_key_batch(c, jobs, B, L, st))) return r; // counts the switches and rescales
        }
        c->prodsum_sums += (unsigned long long)groups;
        c->prodsum_terms += (unsigned long long)count;
        return MHE_OK;
    }
    // all scratch before the first launch: a failed growth leaves every output as it was
    if ((r = get_prodsum(c, st, std::min(count, MHE_MAXB), L, &w))) return r;
    const size_t per = (6 * (size_t)w->ps_limbs + 2) * n;
    auto A_of = [&](int slot) { return w->ps_base.p + (size_t)slot * per; };
    auto T_of = [&](int slot) { return A_of(slot) + 2 * (size_t)(L + 1) * n; };
    auto C_of = [&](int slot) { return T_of(slot) + 2 * ps; };
    const int log_n = c->log_n, fp = c->nm.fp ? 1 : 0;
    // rounds of at most MHE_MAXB groups: their entries (all of one key: a launch of them shares the
    // key stream) in chunks of at most MHE_MAXB that cut across groups, then the tail once per group
    int i0 = 0;
    for (int g0 = 0; g0 < groups; g0 += MHE_MAXB)
    {
        const int G = std::min(MHE_MAXB, groups - g0);
        int i1 = i0;
        while (i1 < count && group[i1] < g0 + G) i1++;
        bool started[MHE_MAXB] = {}; // the round's groups that a chunk has written
        for (int b0 = i0; b0 < i1; b0 += MHE_MAXB)
        {
            const int B = std::min(MHE_MAXB, i1 - b0);
            KsJob jobs[MHE_MAXB];
            ProdSumPtrs pp{};
            int Z = 0, zslot[MHE_MAXB];
            pp.B = B;
            for (int e = 0; e < B; e++)
            {
                const int i = b0 + e;
                jobs[e] = KsJob{ nullptr, ct3[i] + 2 * ps, key, key_limbs, nullptr };
                pp.acc[e] = w->e[e].acc;
                pp.ct3[e] = ct3[i];
                const int slot = group[i] - g0;
                int z = 0;
                while (z < Z && zslot[z] != slot) z++;
                if (z == Z)
                {
                    zslot[Z++] = slot;
                    pp.A[z] = A_of(slot);
                    pp.T[z] = T_of(slot);
                    pp.C[z] = C_of(slot);
                    pp.first[z] = started[slot] ? 0 : 1; // the group's first chunk
                    pp.twice[z] = (twice && twice[group[i]]) ? 1 : 0;
                    started[slot] = true;
                }
                pp.zof[e] = z;
            }
            // the key switch of every entry's d2 up to the key products (evaluator.cpp:2281-2463)
            int special_inv_done = 0;
            if ((r = run_switch_key_batch(c, jobs, B, L, st, 0, &special_inv_done))) return r;
            // each entry's special limbs through their own inverse NTT, [0, 2P)
            JobB<JobStrided> sj;
            sj.per = 2;
            for (int e = 0; e < B; e++) sj.j[e] = special_limbs(c, w->e[e].acc, L);
            if (!special_inv_done) inv_row(sj, log_n, 2 * B, c->nm, st);
            inv_col(sj, log_n, 2 * B, c->nm, st);
            hipLaunchKernelGGL(k_prodsum_acc, dim3((unsigned)(n / 512), (unsigned)(2 * L), (unsigned)Z), dim3(256), 0, st,
                               pp, c->primes, L, c->K, log_n);
            HIP_LAUNCH_CHECK();
        }
        // the round's groups, group z in entry slot z of the workspace.  Limb L-1 only:
        // C += (A - NTT(T)) P^-1 (the sum S of the sequence), last = INTT(S[L-1]); then limbs
        // 0 .. L-2: out = (C + A P^-1 - NTT(T P^-1 + r)) q_{L-1}^-1 through one forward NTT each
        JobB<JobStrided> tc;
        tc.per = 2;
        JobB<JobModDownRow> dr;
        dr.per = 2;
        JobB<JobLastInv> li;
        li.per = 2;
        JobB<JobStrided> j2;
        j2.per = 2;
        JobB<JobProdSumCol> pc;
        pc.per = 2 * (L - 1);
        JobB<JobMDRRow> mr;
        mr.per = 2 * (L - 1);
        for (int z = 0; z < G; z++)
        {
            const WsEntry &e = w->e[z];
            tc.j[z] = JobStrided{ T_of(z) + (size_t)(L - 1) * n, e.modup, ps, n, L - 1, 0, c->primes, c->tw, log_n, 0 };
            dr.j[z] = JobModDownRow{ e.modup, A_of(z), C_of(z), c->primes, c->tw, c->invq, L, c->K, log_n, L - 1 };
            dr.j[z].fp = fp;
            li.j[z] = JobLastInv{ C_of(z), e.coeff, c->primes, c->itw, L, log_n, 1 };
            j2.j[z] = JobStrided{ e.coeff, e.coeff, n, n, L - 1, 0, c->primes, c->itw, log_n, 1 };
            pc.j[z] = JobProdSumCol{ T_of(z), e.coeff, e.modup, c->primes, c->tw, c->invq, L, c->K, log_n, fp };
            mr.j[z] = JobMDRRow{ e.modup, A_of(z), C_of(z), out[g0 + z], c->primes, c->tw, c->invq, L, c->K, log_n, fp };
        }
        fwd_col(tc, log_n, 2 * G, c->nm, st);
        fwd_row(dr, log_n, 2 * G, c->nm, st);
        inv_row(li, log_n, 2 * G, c->nm, st);
        inv_col(j2, log_n, 2 * G, c->nm, st);
        fwd_col(pc, log_n, 2 * (L - 1) * G, c->nm, st);
        fwd_row(mr, log_n, 2 * (L - 1) * G, c->nm, st);
        HIP_LAUNCH_CHECK();
        // the op mix of the sequence this replaces: the adds of each sum and one rescale per group
        for (int z = 0; z < G; z++)
        {
            int terms = 0;
            for (int i = i0; i < i1; i++) terms += group[i] == g0 + z;
            const int dbl = (twice && twice[g0 + z]) ? 1 : 0;
            count_op(c, MHE_OPK_ADDSUB, L, 2ull * (unsigned long long)(terms - 1 + dbl));
        }
        count_op(c, MHE_OPK_RESCALE, L, 2ull * (unsigned long long)G);
        i0 = i1;
    }
    c->prodsum_sums += (unsigned long long)groups;
    c->prodsum_terms += (unsigned long long)count;
    return MHE_OK;
}
