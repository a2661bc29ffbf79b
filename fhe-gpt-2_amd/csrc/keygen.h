// Symmetric encryption of a batch on the device (host side): mhe_encrypt_sk_batch, the digits of a
// key-switching key or a public key, and the counters of the path.  Included by mhe.hip once, after
// encrypt.h.
//
// SEAL's encrypt_zero_symmetric (rlwe.cpp:289-373) draws a = c1 uniform from the PRNG seeded with the
// first 64 bytes of the bootstrap stream, e as CBD from byte 64 of that stream, and sets
// c0 = -(a s + NTT(e)); generate_one_kswitch_key (keygenerator.cpp:384-414) adds (q_{K-1} mod q_j)
// new_key_j to limb j of digit j's c0.  Here a is sampled straight into the kept limbs of the output
// (sample.hip: k_uni_bulk, k_uni_redraw), e stays one signed byte per coefficient (k_sk_cbd) that the
// column pass expands for the kept limbs only (jobs.h JobSkE), and the row pass's epilogue forms c0
// (JobSkRow).  Launches per group of up to MHE_MAXB entries: the state reset, the two kernels of the
// uniform sampler, the error bytes, the column pass, the row pass.
#pragma once

size_t mhe_internal_uniform_scratch_bytes(mhe_ctx *c, int B, int limbs, const int *prime_of_limb);
int mhe_internal_uniform_group(mhe_ctx *c, int B, const uint64_t (*seeds)[8], int limbs, const int *prime_of_limb,
                               const int *slot_of_limb, uint64_t *const *out, void *scratch, uint64_t *counters,
                               hipStream_t st);
int mhe_internal_sk_errors(mhe_ctx *c, int B, const uint64_t (*seeds)[8], signed char *small, size_t pitch, hipStream_t st);
// the public seed of a = the first 64 bytes of the bootstrap stream (seal/random.cpp stream_prefix_seed)
#include "blake2b.h"

MHE_EXPORT int mhe_keygen_stats(mhe_ctx *c, uint64_t *entries, uint64_t *launch_groups, uint64_t *redrawn_words,
                                uint64_t *overflows, int reset)
{
    if (!valid_ctx(c) || !entries || !launch_groups || !redrawn_words || !overflows)
        return fail(MHE_ERR_ARG, "invalid argument");
    // the device totals are written by kernels of any stream: wait for all of them
    unsigned long long dev[2] = { 0, 0 };
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dev, c->kg_dev, sizeof(dev), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(c->kg_dev, 0, sizeof(dev)));
    *entries = reset ? c->kg_entries.exchange(0) : c->kg_entries.load();
    *launch_groups = reset ? c->kg_groups.exchange(0) : c->kg_groups.load();
    *redrawn_words = dev[0];
    *overflows = dev[1];
    return MHE_OK;
}

MHE_EXPORT int mhe_debug_keygen_cap(mhe_ctx *c, uint32_t cap)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "invalid argument");
    c->kg_cap_limit = cap;
    return MHE_OK;
}

MHE_EXPORT int mhe_keygen_overflows(mhe_ctx *c, void *s, uint64_t *overflows, uint64_t *ctx_id)
{
    if (!valid_ctx(c) || !overflows || !ctx_id) return fail(MHE_ERR_ARG, "invalid argument");
    *ctx_id = c->id;
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, c->kg_dev + 1, sizeof(v), hipMemcpyDeviceToHost, S(s)));
    HIP_TRY(hipStreamSynchronize(S(s)));
    *overflows = v;
    return MHE_OK;
}

MHE_EXPORT int mhe_encrypt_sk_batch(mhe_ctx *c, int count, const uint64_t (*seeds)[8], const uint64_t *sk,
                                    int sample_limbs, int keep, int keep_last, const uint64_t *const *new_key,
                                    const int *digit, uint64_t *const *out, void *s)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    const int K = c->K, log_n = c->log_n, fp = c->nm.fp ? 1 : 0;
    if (sample_limbs < 1 || sample_limbs > K) return fail(MHE_ERR_ARG, "parms_id is not valid for encryption parameters");
    if (keep_last != 0 && keep_last != 1) return fail(MHE_ERR_ARG, "invalid argument");
    if (keep < 0 || keep + keep_last < 1 || keep > sample_limbs - keep_last)
        return fail(MHE_ERR_ARG, "kept limbs out of range");
    if (count < 1 || !seeds || !sk || !out) return fail(MHE_ERR_ARG, "invalid argument");
    if (keep_last && sample_limbs != K) return fail(MHE_ERR_ARG, "the last limb is kept at the key level only");
    const int stored = keep + keep_last;
    const size_t n = c->n, ow = 2 * (size_t)stored * n, kw = (size_t)K * n;
    for (int i = 0; i < count; i++)
    {
        if (!out[i]) return fail(MHE_ERR_ARG, "invalid argument");
        const u64 *nk = new_key ? new_key[i] : nullptr;
        if (nk && sample_limbs != K) return fail(MHE_ERR_ARG, "a key-switching key digit is made at the key level only");
        if (nk && (!digit || digit[i] < 0 || digit[i] >= keep)) return fail(MHE_ERR_ARG, "digit out of range");
        // an output may share no word with the secret key, a new key or another output: the passes
        // write it while other workgroups of the launch still read theirs
        if (ranges_overlap(out[i], ow, sk, kw)) return fail(MHE_ERR_ARG, "result cannot point to the same value as operand");
        for (int k = 0; k < count; k++)
            if ((k != i && ranges_overlap(out[i], ow, out[k], ow)) ||
                (new_key && new_key[k] && ranges_overlap(out[i], ow, new_key[k], kw)))
                return fail(MHE_ERR_ARG, "result cannot point to the same value as operand");
    }
    hipStream_t st = S(s);
    // a over primes 0 .. sample_limbs-1; the kept ones land in c1's stored slots, the others are drawn
    // (their rejects consume tail words) and dropped
    int prime_of[64], slot_of[64];
    if (sample_limbs > 64) return fail(MHE_ERR_ARG, "parms_id is not valid for encryption parameters");
    for (int l = 0; l < sample_limbs; l++)
    {
        prime_of[l] = l;
        slot_of[l] = l < keep ? l : (keep_last && l == sample_limbs - 1) ? keep : -1;
    }
    // all scratch before the first launch: a failed growth leaves every output as it was
    const int Bmax = std::min(count, MHE_MAXB);
    Workspace *w;
    int r = get_ws(c, st, std::max(K - 1, 1), &w, Bmax);
    if (r) return r;
    void *uni;
    uint64_t *counters;
    if ((r = mhe_internal_sample_scratch(c, st, mhe_internal_uniform_scratch_bytes(c, Bmax, sample_limbs, prime_of), &uni,
                                         &counters)))
        return r;
    // per entry: the error bytes [n] in coeff (3n words at least), NTT(e)'s column pass [stored][n] in
    // modup (K (K-1) n words, or 2n at K = 1)
    const size_t pitch = w->entries > 1 ? (size_t)(w->e[1].coeff - w->e[0].coeff) * sizeof(u64) : 0;
    for (int b0 = 0; b0 < count; b0 += MHE_MAXB)
    {
        const int B = std::min(MHE_MAXB, count - b0);
        u64 *a_out[MHE_MAXB];
        for (int e = 0; e < B; e++) a_out[e] = out[b0 + e] + (size_t)stored * n;
        // a is drawn from the stream that the bootstrap stream's first 64 bytes seed (rlwe.cpp:317-318),
        // e from the bootstrap stream itself
        uint64_t pub[MHE_MAXB][8];
        for (int e = 0; e < B; e++)
        {
            uint64_t root[8];
            b2b::xof_root(seeds[b0 + e], 0, b2b::kPrngBuffer, root);
            b2b::xof_block(root, 0, b2b::kPrngBuffer, 64, pub[e]);
        }
        if ((r = mhe_internal_uniform_group(c, B, pub, sample_limbs, prime_of, slot_of, a_out, uni, counters, st))) return r;
        if ((r = mhe_internal_sk_errors(c, B, seeds + b0, reinterpret_cast<signed char *>(w->e[0].coeff), pitch, st)))
            return r;
        JobB<JobSkE> ec(stored);
        JobB<JobSkRow> er(stored);
        int gadgets = 0;
        for (int e = 0; e < B; e++)
        {
            const WsEntry &we = w->e[e];
            const u64 *nk = new_key ? new_key[b0 + e] : nullptr;
            gadgets += nk != nullptr;
            ec.j[e] = JobSkE{ reinterpret_cast<const u32 *>(we.coeff), we.modup, c->primes, c->tw, keep, sample_limbs, log_n };
            er.j[e] = JobSkRow{ we.modup, sk, nk, out[b0 + e], c->primes, c->tw, keep, stored, sample_limbs,
                                nk ? digit[b0 + e] : -1, K, log_n, fp };
        }
        fwd_col(ec, log_n, stored * B, c->nm, st);
        fwd_row(er, log_n, stored * B, c->nm, st);
        HIP_LAUNCH_CHECK();
        // the op mix of the sequence this replaces (seal/keys.cpp make_kswitch_key_seq), all at
        // sample_limbs limbs: the NTT of e, a s, the addition and the negation, and for a key digit
        // the scalar product of the new key and its addition
        count_op(c, MHE_OPK_NTT, sample_limbs, (unsigned long long)B);
        count_op(c, MHE_OPK_MULPLAIN, sample_limbs, (unsigned long long)B);
        count_op(c, MHE_OPK_ADDSUB, sample_limbs, 2ull * B + (unsigned long long)gadgets);
        count_op(c, MHE_OPK_SCALAR, sample_limbs, (unsigned long long)gadgets);
        c->kg_entries += (unsigned long long)B;
        c->kg_groups += 1;
    }
    return MHE_OK;
}
