// Sums of relinearized products with the rescale fused behind them (host side): mhe_relin_sum_rescale
// and its counters.  Included by mhe.hip once, after groupsum.h and rotate.h.
//
// A grouped sum (groupsum.h) whose term e has the size-3 product (d0, d1, d2)^e: the key switch of d2
// leaves acc^e, the extra summand is (d0, d1)^e, and its sum is C.  The ModDown and the rescale then
// run once per group through the fused HMult tail (keyswitch.h run_hmult_tail; JobProdSumCol).
#pragma once

MHE_EXPORT int mhe_prodsum_stats(mhe_ctx *c, uint64_t *sums, uint64_t *terms, int reset)
{
    return groupsum_stats(c, &mhe_ctx::prodsum_sums, &mhe_ctx::prodsum_terms, sums, terms, reset);
}

// The sequence the merged path replaces, one entry at a time (the separate-MAC debugging path):
// relinearize a copy of each product, add, double, rescale.
static int prodsum_one_by_one(mhe_ctx *c, int count, const u64 *const *ct3, const int *group, const int *twice,
                              const u64 *key, int key_limbs, u64 *const *out, int L, hipStream_t st)
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
    if (!check_groups(group, count, groups)) return fail(MHE_ERR_ARG, "invalid argument");
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
    if (!c->ks_fused) return prodsum_one_by_one(c, count, ct3, group, twice, key, key_limbs, out, L, st);
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
    if ((r = get_groupsum(c, st, std::min(count, MHE_MAXB), L, &Workspace::prodsum, &w))) return r;
    const SumPool &sp = w->prodsum;
    const int log_n = c->log_n, fp = c->nm.fp ? 1 : 0;
    // rounds of at most MHE_MAXB groups: their entries (all of one key: a launch of them shares the
    // key stream) in chunks of at most MHE_MAXB that cut across groups, then the tail once per group
    for (const GroupSumRound &round : plan_group_sums<const void *>(count, group, groups, MHE_MAXB, nullptr))
    {
        for (const GroupSumChunk &ch : round.chunks)
        {
            KsJob jobs[MHE_MAXB];
            GroupSumPtrs gp = groupsum_ptrs(ch, w, sp, 2, L, n);
            for (int e = 0; e < gp.B; e++)
            {
                jobs[e] = KsJob{ nullptr, ct3[ch.entries[e]] + 2 * ps, key, key_limbs, nullptr };
                gp.x[e] = ct3[ch.entries[e]];
            }
            for (int z = 0; z < ch.Z(); z++)
            {
                gp.X[z] = sp.at(ch.slot[z], 2, L, n);
                gp.firstx[z] = ch.first[z];
                gp.twice[z] = (twice && twice[round.g0 + ch.slot[z]]) ? 1 : 0;
            }
            if ((r = groupsum_fold(c, w, jobs, gp, ch.Z(), L, st))) return r; // the key switches of the d2
        }
        // the round's groups, group z in entry slot z of the workspace.  Limb L-1 only:
        // C += (A - NTT(T)) P^-1 (the sum S of the sequence), last = INTT(S[L-1]); then limbs
        // 0 .. L-2: out = (C + A P^-1 - NTT(T P^-1 + r)) q_{L-1}^-1 through one forward NTT each
        TailSlot ts[MHE_MAXB];
        for (int z = 0; z < round.G; z++) ts[z] = TailSlot{ sp.at(z, 0, L, n), sp.at(z, 2, L, n), out[round.g0 + z] };
        run_hmult_tail(
            c, w, ts, round.G, L, st,
            [&] {
                JobB<JobStrided> tc(2);
                for (int z = 0; z < round.G; z++)
                    tc.j[z] = JobStrided{ sp.at(z, 1, L, n) + (size_t)(L - 1) * n, w->e[z].modup, ps, n, L - 1, 0, c->primes,
                                          c->tw, log_n, 0 };
                fwd_col(tc, log_n, 2 * round.G, c->nm, st);
            },
            [&] {
                JobB<JobProdSumCol> pc(2 * (L - 1));
                for (int z = 0; z < round.G; z++)
                    pc.j[z] = JobProdSumCol{ sp.at(z, 1, L, n), w->e[z].coeff, w->e[z].modup, c->primes, c->tw, c->invq, L,
                                             c->K, log_n, fp };
                fwd_col(pc, log_n, 2 * (L - 1) * round.G, c->nm, st);
            });
        HIP_LAUNCH_CHECK();
        // the op mix of the sequence this replaces: the adds of each sum and one rescale per group
        groupsum_count_adds(c, round, L, 0, twice);
        count_op(c, MHE_OPK_RESCALE, L, 2ull * (unsigned long long)round.G);
    }
    c->prodsum_sums += (unsigned long long)groups;
    c->prodsum_terms += (unsigned long long)count;
    return MHE_OK;
}
