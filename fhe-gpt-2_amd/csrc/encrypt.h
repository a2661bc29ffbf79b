// Public-key encryption of a batch on the device (host side): mhe_encrypt_pk_batch and its counters.
// Included by mhe.hip once, after prodsum.h.
//
// SEAL's encrypt_zero_asymmetric (rlwe.cpp:220-286) at m = L + 1 limbs followed by the rescale by
// prime L (util/rns.cpp:737-808) computes, with uh = NTT(u),
//     c_j       = uh pk_j + NTT(e_j)
//     out_{j,i} = (c_{j,i} - NTT_i(r_{j,i})) q_L^-1,  r_{j,i} the rescale lift of INTT(c_{j,L}).
// The NTT is linear mod q_i and e_j is drawn in coefficient form, so
//     last_j    = INTT_L(uh_L pk_{j,L}) + e_j                       (mod q_L)
//     out_{j,i} = (uh_i pk_{j,i} + NTT_i(e_j - r_{j,i})) q_L^-1      (mod q_i), i < L
// with one forward NTT per output limb, none of e over the m limbs, and c never written.  The samples
// travel as one signed byte per coefficient (sample.hip k_enc_*; jobs.h, the encryption jobs).
// Launches per group of up to MHE_MAXB entries: the state reset, three sampling kernels, the two
// passes of NTT(u), the two inverse passes of the dropped limb, the lift column pass, the row pass.
#pragma once

int mhe_internal_encrypt_samples(mhe_ctx *c, int B, const uint64_t (*seeds)[8], signed char *small, uint32_t *state,
                                 size_t pitch, hipStream_t st);
static_assert(MHE_MAXB <= 8, "sample.hip MHE_SAMPLE_MAXB");

MHE_EXPORT int mhe_encrypt_stats(mhe_ctx *c, uint64_t *entries, uint64_t *launch_groups, int reset)
{
    if (!valid_ctx(c) || !entries || !launch_groups) return fail(MHE_ERR_ARG, "invalid argument");
    *entries = reset ? c->enc_entries.exchange(0) : c->enc_entries.load();
    *launch_groups = reset ? c->enc_groups.exchange(0) : c->enc_groups.load();
    return MHE_OK;
}

MHE_EXPORT int mhe_encrypt_pk_batch(mhe_ctx *c, int count, const uint64_t (*seeds)[8], const uint64_t *pk,
                                    int key_limbs, const uint64_t *const *plain, uint64_t *const *out, int limbs,
                                    void *s)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    // the public key lives at the key level: limb l of each poly on prime l of the context
    if (key_limbs != c->K) return fail(MHE_ERR_ARG, "public key is not valid for encryption parameters");
    if (limbs < 1 || limbs > key_limbs - 1) return fail(MHE_ERR_ARG, "parms_id is not valid for encryption parameters");
    if (count < 1 || !seeds || !pk || !out) return fail(MHE_ERR_ARG, "invalid argument");
    const int L = limbs, m = L + 1, K = c->K, log_n = c->log_n, fp = c->nm.fp ? 1 : 0;
    const size_t n = c->n, ow = 2 * (size_t)L * n;
    for (int i = 0; i < count; i++)
    {
        if (!out[i]) return fail(MHE_ERR_ARG, "invalid argument");
        // an output may share no word with the key, a plaintext or another output: the last pass
        // writes it while other workgroups of the launch still read theirs
        if (ranges_overlap(out[i], ow, pk, 2 * (size_t)K * n))
            return fail(MHE_ERR_ARG, "result cannot point to the same value as operand");
        for (int k = 0; k < count; k++)
            if ((k != i && ranges_overlap(out[i], ow, out[k], ow)) ||
                (plain && plain[k] && ranges_overlap(out[i], ow, plain[k], (size_t)L * n)))
                return fail(MHE_ERR_ARG, "result cannot point to the same value as operand");
    }
    hipStream_t st = S(s);
    // all scratch before the first launch: a failed growth leaves every output as it was
    Workspace *w;
    int r = get_ws(c, st, K - 1, &w, std::min(count, MHE_MAXB));
    if (r) return r;
    // per entry: uh [m][n] in acc, last [2][n] and the byte planes [3][n] in coeff (3n words at
    // least), the lifts' transforms [2][L][n] in modup; the redraw states [B][2] in tmp
    u32 *state = reinterpret_cast<u32 *>(w->tmp);
    const size_t pitch = w->entries > 1 ? (size_t)(w->e[1].coeff - w->e[0].coeff) * sizeof(u64) : 0;
    for (int b0 = 0; b0 < count; b0 += MHE_MAXB)
    {
        const int B = std::min(MHE_MAXB, count - b0);
        signed char *small0 = reinterpret_cast<signed char *>(w->e[0].coeff + 2 * n);
        if ((r = mhe_internal_encrypt_samples(c, B, seeds + b0, small0, state, pitch, st))) return r;
        JobB<JobEncU> uc(m);
        JobB<JobFwdPlain> ur(m);
        JobB<JobEncLast<true>> lr(2);
        JobB<JobEncLast<false>> lc(2);
        JobB<JobEncLiftCol> fc(2 * L);
        JobB<JobEncRow> fr(2 * L);
        for (int e = 0; e < B; e++)
        {
            const WsEntry &we = w->e[e];
            u64 *uh = we.acc, *last = we.coeff;
            const u32 *small = reinterpret_cast<const u32 *>(we.coeff + 2 * n);
            const u32 *err = small + n / 4;
            uc.j[e] = JobEncU{ small, uh, c->primes, c->tw, log_n };
            ur.j[e] = fwd_plain(c, uh, uh, m, 1);
            lr.j[e] = JobEncLast<true>{ uh, pk, err, last, c->primes, c->itw, L, key_limbs, log_n, fp };
            lc.j[e] = JobEncLast<false>{ uh, pk, err, last, c->primes, c->itw, L, key_limbs, log_n, fp };
            fc.j[e] = JobEncLiftCol{ last, err, we.modup, c->primes, c->tw, L, log_n, fp };
            fr.j[e] = JobEncRow{ we.modup, uh, pk, plain ? plain[b0 + e] : nullptr, out[b0 + e], c->primes, c->tw, c->invq,
                                 L, K, key_limbs, log_n, fp };
        }
        fwd_col(uc, log_n, m * B, c->nm, st);
        fwd_row(ur, log_n, m * B, c->nm, st);
        inv_row(lr, log_n, 2 * B, c->nm, st);
        inv_col(lc, log_n, 2 * B, c->nm, st);
        fwd_col(fc, log_n, 2 * L * B, c->nm, st);
        fwd_row(fr, log_n, 2 * L * B, c->nm, st);
        HIP_LAUNCH_CHECK();
        // the op mix of the sequence this replaces (Encryptor::encrypt_zero_at + encrypt_plain): the
        // NTTs of u and (e_0, e_1), two plaintext products and two additions at m limbs, the rescale
        // of two polys, and the plaintext's addition at L
        int plains = 0;
        for (int e = 0; e < B; e++) plains += plain && plain[b0 + e];
        count_op(c, MHE_OPK_NTT, m, 3ull * B);
        count_op(c, MHE_OPK_MULPLAIN, m, 2ull * B);
        count_op(c, MHE_OPK_ADDSUB, m, 2ull * B);
        count_op(c, MHE_OPK_RESCALE, m, 2ull * B);
        count_op(c, MHE_OPK_ADDSUB, L, (unsigned long long)plains);
        c->enc_entries += (unsigned long long)B;
        c->enc_groups += 1;
    }
    return MHE_OK;
}
