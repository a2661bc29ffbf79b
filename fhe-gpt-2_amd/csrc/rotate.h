// The rotation pipelines (host side): batched rotations with hoisting (hoist.h kernels, hoist_plan.h
// launch plan) and rotate-and-sum, with their entry points of the C ABI.  Included by mhe.hip once,
// after keyswitch.h and the single-rotation entry points.
#pragma once

#include "hoist_plan.h"

// One rotation of a list: input and key present, the element a unit mod 2N, the key's limbs in range.
static int check_rotation(mhe_ctx *c, const u64 *in, u32 elt, const u64 *key, int key_limbs, int limbs)
{
    if (!in || !key) return fail(MHE_ERR_ARG, "Galois key not present");
    int r = check_galois_elt(c, elt);
    if (r) return r;
    return check_key_limbs(c, key_limbs, limbs);
}

// out_e <- perm_e(in_e) for the B entries of gp, both polys at L limbs, one launch
// (evaluator.cpp:2193-2214).  count: the permutations are part of what the caller was asked for
// (mhe_op_counts), not of a check.
static int permute_batch(mhe_ctx *c, const GalPtrs &gp, int B, int L, hipStream_t st, bool count)
{
    const size_t total = (size_t)2 * L << c->log_n;
    if (count) count_op(c, MHE_OPK_GALOIS, L, 2ull * B);
    hipLaunchKernelGGL(k_galois_b, dim3((unsigned)((total + 255) / 256), (unsigned)B), dim3(256), 0, st, gp, c->log_n,
                       total);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

// ------------------------------------------------------------------ hoisted rotations (hoist.h)
// The ModUp buffers of up to `entries` hoisted inputs on stream st ([K][K-1][n] each: every level),
// the key products of up to MHE_MAXB * MHE_HOIST_R of their rotations and the inputs' flags.
static int get_hoist(mhe_ctx *c, hipStream_t st, int entries, int ws_entries, int L, Workspace **out)
{
    Workspace *w;
    int r = get_ws(c, st, c->K - 1, &w, std::max(entries, ws_entries));
    if (r) return r;
    std::lock_guard<std::mutex> g(w->mu);
    // per input [L+1][L][n] (the pass's level), the key products of up to MHE_MAXB * MHE_HOIST_R
    // rotations at that level; grown (after draining the stream) when a pass needs more
    if (w->hoist_entries < entries || w->hoist_limbs < L)
    {
        const int E = std::max(entries, w->hoist_entries), HL = std::max(L, w->hoist_limbs);
        w->hoist_entries = 0;
        w->hoist_limbs = 0;
        const size_t per = (size_t)(HL + 1) * HL * c->n, pacc = (size_t)2 * (HL + 1) * c->n;
        const int na = MHE_MAXB * MHE_HOIST_R;
        if ((r = w->hoist_base.grow(c, st, ((size_t)E * per + (size_t)na * pacc) * sizeof(u64)))) return r;
        for (int i = 0; i < E; i++) w->hoist[i] = w->hoist_base.p + (size_t)i * per;
        for (int i = 0; i < na; i++) w->hacc[i] = w->hoist_base.p + (size_t)E * per + (size_t)i * pacc;
        w->hoist_entries = E;
        w->hoist_limbs = HL;
    }
    if (!w->flags && hipMalloc(&w->flags, MHE_MAXB * sizeof(int)) != hipSuccess)
        return fail(MHE_ERR_MEMORY, "workspace allocation failed");
    *out = w;
    return MHE_OK;
}

// M^g = NTT of Galois element g's negation mask under every prime of the context, [K][n]
// canonical; built once per element on stream st (which then waits for it: other streams use the
// table without an event).
static int get_mask(mhe_ctx *c, u32 elt, hipStream_t st, const u64 **out)
{
    std::lock_guard<std::mutex> g(c->mask_mu);
    auto it = c->masks.find(elt);
    if (it != c->masks.end())
    {
        *out = it->second;
        return MHE_OK;
    }
    u64 *m = nullptr;
    const size_t total = (size_t)c->K * c->n;
    HIP_TRY(hipSetDevice(c->device));
    if (hipMalloc(&m, total * sizeof(u64)) != hipSuccess) return fail(MHE_ERR_MEMORY, "Galois mask allocation failed");
    hipLaunchKernelGGL(k_negmask, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, m, elt, c->K, c->log_n);
    fwd_col(fwd_plain(c, m, m, c->K, 0), c->log_n, c->K, c->nm, st);
    fwd_row(fwd_plain(c, m, m, c->K, 1), c->log_n, c->K, c->nm, st);
    HIP_LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(st));
    c->masks[elt] = m;
    *out = m;
    return MHE_OK;
}

// f(std::integral_constant<int, R>) for the rotation count R of a hoisted MAC launch
// (k_ks_hoist_mac<R>, k_ks_hoist_mac_sh<R>: 1 .. MHE_HOIST_R)
template <class F> static void with_rotation_count(int R, F f)
{
    switch (R)
    {
#define HM(r) case r: f(std::integral_constant<int, r>{}); break;
        HM(1) HM(2) HM(3) HM(4) HM(5) HM(6) HM(7) HM(8)
#undef HM
    }
}

static bool hoist_ok(const mhe_ctx *c)
{
    return c->ks_hoist && c->ks_fused && c->galois_fused && c->ks_colgroups != 0 && c->nm.fp == 1 && c->nm_ks.fp == 1 &&
           c->cmodf;
}

// counts words that differ between a and b (mhe_ctx_set_hoist's check); first[0] = lowest index
__global__ void k_cmp_words(const u64 *__restrict__ a, const u64 *__restrict__ b, size_t total,
                            unsigned long long *bad)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total || a[i] == b[i]) return;
    atomicAdd(bad, 1ull);
    atomicMin(bad + 1, (unsigned long long)i);
}

// The check of a hoisted pass: every rotation again by SEAL's order (permutation, then the classic
// key switch of the permuted c1) into scratch, compared word for word with the hoisted output.
static int hoist_check_pass(mhe_ctx *c, const u64 *const *in, int count, const int *ent_in, u64 *const *out,
                            const u32 *elts, const u64 *const *keys, const int *key_limbs, int L, hipStream_t st,
                            const int *flags)
{
    const size_t ps = (size_t)L * c->n;
    u64 *tmp = nullptr;
    unsigned long long *cnt = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    if (hipMalloc(&tmp, (size_t)MHE_MAXB * 2 * ps * sizeof(u64)) != hipSuccess)
        return fail(MHE_ERR_MEMORY, "hoist check: allocation failed");
    if (hipMalloc(&cnt, 2 * MHE_MAXB * sizeof(unsigned long long) + MHE_MAXB * sizeof(int)) != hipSuccess)
    {
        (void)hipFree(tmp);
        return fail(MHE_ERR_MEMORY, "hoist check: allocation failed");
    }
    int *fl = reinterpret_cast<int *>(cnt + 2 * MHE_MAXB);
    int r = MHE_OK;
    for (int i0 = 0; i0 < count && r == MHE_OK; i0 += MHE_MAXB)
    {
        const int B = std::min(MHE_MAXB, count - i0);
        GalPtrs gp{};
        KsJob jobs[MHE_MAXB];
        std::vector<unsigned long long> init(2 * MHE_MAXB);
        for (int e = 0; e < B; e++)
        {
            const int i = i0 + e;
            u64 *t = tmp + (size_t)e * 2 * ps;
            gp.in[e] = in[ent_in[i]];
            gp.out[e] = t;
            gp.elt[e] = elts[i];
            jobs[e] = KsJob{ t, t + ps, keys[i], key_limbs[i], nullptr };
            init[2 * e] = 0;
            init[2 * e + 1] = ~0ull;
        }
        HIP_TRY(hipMemcpyAsync(cnt, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        for (int e = 0; e < B; e++)
            HIP_TRY(hipMemcpyAsync(fl + e, flags + ent_in[i0 + e], sizeof(int), hipMemcpyDeviceToDevice, st));
        if ((r = permute_batch(c, gp, B, L, st, false))) break;
        if ((r = run_switch_key_batch(c, jobs, B, L, st, 1, nullptr, 0))) break; // the one-entry key MAC
        for (int e = 0; e < B; e++)
            hipLaunchKernelGGL(k_cmp_words, dim3((unsigned)((2 * ps + 255) / 256)), dim3(256), 0, st,
                               tmp + (size_t)e * 2 * ps, out[i0 + e], 2 * ps, cnt + 2 * e);
        HIP_LAUNCH_CHECK();
        std::vector<unsigned long long> got(2 * MHE_MAXB);
        std::vector<int> hf(MHE_MAXB);
        HIP_TRY(hipMemcpyAsync(got.data(), cnt, got.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hf.data(), fl, MHE_MAXB * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int e = 0; e < B; e++)
        {
            if (!got[2 * e]) continue;
            c->hoist_bad += got[2 * e];
            const unsigned long long f = got[2 * e + 1];
            fprintf(stderr,
                    "[hoist check] stream %p L %d entry %d/%d (input %d, elt %u, key %p, key_limbs %d, zero flag %d): "
                    "%llu words differ, first at poly %llu limb %llu slot %llu\n",
                    (void *)st, L, i0 + e, count, ent_in[i0 + e], elts[i0 + e], (const void *)keys[i0 + e],
                    key_limbs[i0 + e], hf[e], got[2 * e], f / ps, (f % ps) / c->n, f % c->n);
        }
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(tmp);
    (void)hipFree(cnt);
    return r;
}

// Rotations of H <= MHE_MAXB inputs at L limbs, entry i rotating input ent_in[i] (index into in)
// by elts[i] into out[i]: ModUp of every input once (INTT -> column pass -> row pass, canonical
// D in the hoist buffers, plus the zero scan), then per chunk of entries the permutation of c0 /
// c1 into out, the hoisted key MAC (hoist.h), the classic ModUp + MAC for flagged inputs only
// (their kernels return at once otherwise), and the ModDown (c1 written).
static int run_galois_hoisted(mhe_ctx *c, const u64 *const *in, int H, int count, const int *ent_in,
                              u64 *const *out, const u32 *elts, const u64 *const *keys, const int *key_limbs, int L,
                              hipStream_t st)
{
    Workspace *w;
    int r = get_hoist(c, st, H, std::min(count, MHE_MAXB), L, &w); // step 3 uses up to MHE_MAXB entry slots
    if (r) return r;
    const int log_n = c->log_n;
    const size_t n = c->n, ps = (size_t)L * n;
    std::vector<const u64 *> masks(count);
    std::vector<u32> elt_inv(count);
    for (int i = 0; i < count; i++)
    {
        if ((r = get_mask(c, elts[i], st, &masks[i]))) return r;
        u64 inv = 0;
        host::invmod(elts[i], 2 * n, inv); // odd: a unit mod 2N
        elt_inv[i] = (u32)inv;
    }
    // 1. ModUp of each input's c1: INTT into entry slot h's coeff, the zero scan, the column pass
    //    (64-bit, natural order), the row pass into hoist[h]
    {
        const u64 *c1[MHE_MAXB];
        for (int h = 0; h < H; h++) c1[h] = in[h] + ps;
        intt_targets(c, w, c1, H, L, nullptr, st);
        HIP_TRY(hipMemsetAsync(w->flags, 0, MHE_MAXB * sizeof(int), st));
        for (int h = 0; h < H; h++)
            hipLaunchKernelGGL(k_zero_scan, dim3((unsigned)((ps + 255) / 256)), dim3(256), 0, st, w->e[h].coeff, log_n, ps,
                               w->flags + h);
        KsPtrs kp{};
        for (int h = 0; h < H; h++)
        {
            kp.coeff[h] = w->e[h].coeff;
            kp.inter[h] = w->e[h].modup;
        }
        ks_modup_col(c, kp, H, L, 0, st);
        auto row = [&](auto brev) {
            JobB<JobModUpRowH<decltype(brev)::value>> rj((L + 1) * L);
            for (int h = 0; h < H; h++) rj.j[h] = { w->e[h].modup, w->hoist[h], c->primes, c->tw, L, c->K, log_n };
            fwd_row(rj, log_n, H * (L + 1) * L, c->nm, st);
        };
        if (log_n == 16)
            row(std::true_type{});
        else
            row(std::false_type{});
        HIP_LAUNCH_CHECK();
    }
    // 2. the hoisted key MACs, as planned (hoist_plan.h); rotation i's key products go to w->hacc[i]
    for (const HoistLaunch &hl : plan_hoist_macs(H, count, ent_in, reinterpret_cast<const void *const *>(keys), key_limbs,
                                                 elts, MHE_MAXB, MHE_HOIST_R))
    {
        const int Z = (int)hl.items.size(), R = (int)hl.items[0].second.size();
        // times, launches and counts the kernel instance of R rotations that `launch` starts
        auto run = [&](auto launch) {
            hipEvent_t *tm = timing_slot(c, w, TK_KS_ROW_MAC, st);
            with_rotation_count(R, launch);
            c->hoist_mac++;
            timing_end(tm, st);
        };
        if (hl.shared)
        {
            HoistShared hs{};
            hs.Z = Z;
            for (int r0 = 0; r0 < R; r0++)
            {
                const int i = hl.items[0].second[r0]; // every item lists these keys and elements
                hs.key[r0] = keys[i];
                hs.mask[r0] = masks[i];
                hs.einv[r0] = elt_inv[i];
                hs.key_limbs[r0] = key_limbs[i];
            }
            for (int z = 0; z < Z; z++)
            {
                const int h = hl.items[z].first;
                hs.D[z] = w->hoist[h];
                hs.c1[z] = in[h] + ps;
                hs.flag[z] = w->flags + h;
                for (int r0 = 0; r0 < R; r0++) hs.acc[z][r0] = w->hacc[hl.items[z].second[r0]];
            }
            const int per_wg = R <= 4 ? 8 : 4; // 4 lane groups x items per lane
            const dim3 grid((unsigned)(n / 256), (unsigned)(L + 1), (unsigned)((Z + per_wg - 1) / per_wg));
            run([&](auto rc) {
                hipLaunchKernelGGL((k_ks_hoist_mac_sh<decltype(rc)::value>), grid, dim3(1024), 0, st, hs, c->primes, c->cmodf,
                                   L, c->K, log_n);
            });
        }
        else
        {
            HoistPtrs hp{};
            for (int z = 0; z < Z; z++)
            {
                const int h = hl.items[z].first;
                hp.D[z] = w->hoist[h];
                hp.c1[z] = in[h] + ps;
                hp.flag[z] = w->flags + h;
                hp.R[z] = R;
                for (int r0 = 0; r0 < R; r0++)
                {
                    const int i = hl.items[z].second[r0];
                    hp.key[z][r0] = keys[i];
                    hp.mask[z][r0] = masks[i];
                    hp.acc[z][r0] = w->hacc[i];
                    hp.einv[z][r0] = elt_inv[i];
                    hp.key_limbs[z][r0] = key_limbs[i];
                }
            }
            const dim3 grid((unsigned)(n / 256), (unsigned)(L + 1), (unsigned)Z);
            run([&](auto rc) {
                hipLaunchKernelGGL((k_ks_hoist_mac<decltype(rc)::value>), grid, dim3(256), 0, st, hp, c->primes, c->cmodf, L,
                                   c->K, log_n);
            });
        }
    }
    HIP_LAUNCH_CHECK();
    // 3. per MHE_MAXB rotations: c0 / c1 permuted into out, the classic ModUp + MAC of flagged
    //    inputs (their kernels return at once otherwise), the ModDown (c1 written)
    const int pack = (c->ks_pack && c->ks_colgroups != 0) ? 1 : 0;
    const int pack_col = pack | MHE_INTER_F64; // the column pass in front of the fused MAC (ntt.h)
    std::vector<int> order(count);
    for (int i = 0; i < count; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return keys[a] < keys[b]; });
    for (int i0 = 0; i0 < count; i0 += MHE_MAXB)
    {
        const int B = std::min(MHE_MAXB, count - i0);
        GalPtrs gp{};
        KsJob jobs[MHE_MAXB];
        u64 *accs[MHE_MAXB];
        const u64 *c1[MHE_MAXB];      // the permuted c1: what the classic path of a flagged input switches
        const int *flagged[MHE_MAXB]; // that path's kernels return unless the input's flag is set
        for (int e = 0; e < B; e++)
        {
            const int i = order[i0 + e], h = ent_in[i];
            gp.in[e] = in[h];
            gp.out[e] = out[i];
            gp.elt[e] = elts[i];
            jobs[e] = KsJob{ out[i], out[i] + ps, keys[i], key_limbs[i], nullptr };
            accs[e] = w->hacc[i];
            c1[e] = out[i] + ps;
            flagged[e] = w->flags + h;
        }
        int kpack = 1;
        for (int e = 0; e < B; e++)
            if ((r = ks_check_key(c, jobs[e], L, st, &kpack))) return r;
        if ((r = permute_batch(c, gp, B, L, st, true))) return r;
        count_op(c, MHE_OPK_KEYSWITCH, L, (unsigned long long)B);
        intt_targets(c, w, c1, B, L, flagged, st);
        const KsPtrs kp = ks_ptrs(w, jobs, B, accs, flagged);
        ks_modup_col(c, kp, B, L, pack_col, st);
        ks_row_mac_chunk(kp, B, c->primes, c->tw, L, c->K, log_n, c->nm_ks, 0, L + 1, pack, kpack, ks_shared_key(c, jobs, B),
                         ks_pair_of(c), c->itw, 0, st);
        HIP_LAUNCH_CHECK();
        run_moddown(c, jobs, B, L, w, 0, 1, st, accs);
    }
    c->hoist_rot += (unsigned long long)count;
    if (c->hoist_check) return hoist_check_pass(c, in, count, ent_in, out, elts, keys, key_limbs, L, st, w->flags);
    return MHE_OK;
}

MHE_EXPORT int mhe_apply_galois_batch(mhe_ctx *c, int count, const uint64_t *const *in, uint64_t *const *out,
                                      const uint32_t *elts, const uint64_t *const *keys, const int *key_limbs, int limbs,
                                      void *s)
{
    int r = check_limbs(c, limbs, 1);
    if (r) return r;
    if (count < 0 || (count && (!in || !out || !elts || !keys || !key_limbs))) return fail(MHE_ERR_ARG, "invalid argument");
    hipStream_t st = S(s);
    const size_t ps = (size_t)limbs << c->log_n;
    for (int i = 0; i < count; i++)
    {
        // every key is checked before the first launch, so a bad key leaves no output half-written
        if (!out[i]) return fail(MHE_ERR_ARG, "Galois key not present");
        if ((r = check_rotation(c, in[i], elts[i], keys[i], key_limbs[i], limbs))) return r;
        // outputs must be disjoint from every input and from each other (all are written before the
        // first key switch reads its input's permutation back from its own output)
        if (output_overlaps(out, i, count, 2 * ps, in, count, 2 * ps))
            return fail(MHE_ERR_ARG, "result cannot point to the same value as operand");
    }
    if (!c->galois_fused)
    {
        for (int i = 0; i < count; i++)
            if ((r = mhe_apply_galois_to(c, in[i], out[i], elts[i], keys[i], key_limbs[i], limbs, s))) return r;
        return MHE_OK;
    }
    // inputs rotated more than once share their ModUp (hoist.h), up to MHE_MAXB inputs per pass
    std::vector<int> rest;
    if (hoist_ok(c) && count > 1 && c->n >= 256)
    {
        std::vector<const u64 *> uin;
        std::vector<std::vector<int>> uent;
        for (int i = 0; i < count; i++)
        {
            size_t u = 0;
            while (u < uin.size() && uin[u] != in[i]) u++;
            if (u == uin.size())
            {
                uin.push_back(in[i]);
                uent.emplace_back();
            }
            uent[u].push_back(i);
        }
        // the pass being gathered: its inputs, and per rotation its input (index into in), output,
        // element and key
        struct
        {
            std::vector<const u64 *> in, key;
            std::vector<u64 *> out;
            std::vector<u32> elt;
            std::vector<int> ent_in, key_limbs;
        } p;
        auto flush = [&]() -> int {
            if (p.in.empty()) return MHE_OK;
            const int rr = run_galois_hoisted(c, p.in.data(), (int)p.in.size(), (int)p.ent_in.size(), p.ent_in.data(),
                                              p.out.data(), p.elt.data(), p.key.data(), p.key_limbs.data(), limbs, st);
            p = {};
            return rr;
        };
        for (size_t u = 0; u < uin.size(); u++)
        {
            if (uent[u].size() < 2)
            {
                rest.push_back(uent[u][0]);
                continue;
            }
            // at most MHE_MAXB inputs and MHE_MAXB * MHE_HOIST_R rotations per pass (w->hacc)
            if ((p.in.size() == MHE_MAXB || p.ent_in.size() + uent[u].size() > (size_t)MHE_MAXB * MHE_HOIST_R) &&
                (r = flush()))
                return r;
            if (uent[u].size() > (size_t)MHE_MAXB * MHE_HOIST_R)
            {
                // more rotations than one pass holds: the classic path (never in the callers' shapes)
                for (int i : uent[u]) rest.push_back(i);
                continue;
            }
            const int h = (int)p.in.size();
            p.in.push_back(uin[u]);
            for (int i : uent[u])
            {
                p.ent_in.push_back(h);
                p.out.push_back(out[i]);
                p.elt.push_back(elts[i]);
                p.key.push_back(keys[i]);
                p.key_limbs.push_back(key_limbs[i]);
            }
        }
        if ((r = flush())) return r;
    }
    else
        for (int i = 0; i < count; i++) rest.push_back(i);
    // entries of one key side by side: a launch of them shares the key stream (k_ks_row_mac share)
    std::stable_sort(rest.begin(), rest.end(), [&](int a, int b) { return keys[a] < keys[b]; });
    const int nrest = (int)rest.size();
    for (int i0 = 0; i0 < nrest; i0 += MHE_MAXB)
    {
        const int B = std::min(MHE_MAXB, nrest - i0);
        // out_e <- perm_e(in_e), then the key switch of out_e's c1 with c1 written (SEAL zeroes c1
        // and adds KS_1, the same words as writing it)
        GalPtrs gp{};
        KsJob jobs[MHE_MAXB];
        for (int e = 0; e < B; e++)
        {
            const int i = rest[i0 + e];
            gp.in[e] = in[i];
            gp.out[e] = out[i];
            gp.elt[e] = elts[i];
            jobs[e] = KsJob{ out[i], out[i] + ps, keys[i], key_limbs[i], nullptr };
        }
        if ((r = permute_batch(c, gp, B, limbs, st, true))) return r;
        if ((r = run_switch_key_batch(c, jobs, B, limbs, st, 1))) return r;
    }
    return MHE_OK;
}

MHE_EXPORT int mhe_ctx_set_hoist(mhe_ctx *c, int on, int check)
{
    if (!valid_ctx(c)) return fail(MHE_ERR_ARG, "context is not valid");
    c->ks_hoist = on ? 1 : 0;
    c->hoist_check = check ? 1 : 0;
    return MHE_OK;
}

MHE_EXPORT int mhe_ctx_get_hoist(mhe_ctx *c, int *on, int *check)
{
    if (!valid_ctx(c) || !on || !check) return fail(MHE_ERR_ARG, "invalid argument");
    *on = hoist_ok(c) ? 1 : 0;
    *check = c->hoist_check.load();
    return MHE_OK;
}

MHE_EXPORT int mhe_hoist_stats(mhe_ctx *c, uint64_t *rotations, uint64_t *mac_launches, uint64_t *check_mismatches,
                               int reset)
{
    if (!valid_ctx(c) || !rotations || !mac_launches || !check_mismatches) return fail(MHE_ERR_ARG, "invalid argument");
    *rotations = reset ? c->hoist_rot.exchange(0) : c->hoist_rot.load();
    *mac_launches = reset ? c->hoist_mac.exchange(0) : c->hoist_mac.load();
    *check_mismatches = reset ? c->hoist_bad.exchange(0) : c->hoist_bad.load();
    return MHE_OK;
}

MHE_EXPORT int mhe_ks_pair_stats(mhe_ctx *c, uint64_t *paired, uint64_t *single, int reset)
{
    if (!valid_ctx(c) || !paired || !single) return fail(MHE_ERR_ARG, "invalid argument");
    *paired = reset ? c->ks_paired.exchange(0) : c->ks_paired.load();
    *single = reset ? c->ks_single.exchange(0) : c->ks_single.load();
    return MHE_OK;
}

// The digit-major ModUp column pass (k_modup_col; keyswitch.h ks_modup_col): launches counts its
// launches since the last reset, whether by a key switch, an HMult or a rotation pipeline, and ig_sum
// adds up their output-prime groups per digit (the kernel's IG): ig_sum == n * launches says that every
// launch ran with n groups.  The generic column pass (MHE_KS_COLGROUPS=0) is not counted.
MHE_EXPORT int mhe_modup_stats(mhe_ctx *c, uint64_t *launches, uint64_t *ig_sum, int reset)
{
    if (!valid_ctx(c) || !launches || !ig_sum) return fail(MHE_ERR_ARG, "invalid argument");
    *launches = reset ? c->modup_launches.exchange(0) : c->modup_launches.load();
    *ig_sum = reset ? c->modup_ig_sum.exchange(0) : c->modup_ig_sum.load();
    return MHE_OK;
}

// ------------------------------------------------------------------------------ rotate and sum
// mhe_rotate_sum: a grouped sum (groupsum.h) whose entry e is in[e] rotated by elts[e].  The key switch
// of the permuted c1 leaves acc^e, the extra summand is the permuted c0, and its sum goes straight to
// out[g][0].  A chunk's entries come sorted by key (they share the key stream of the MAC), so a
// group's entries are anywhere in it.  One ModDown forward NTT per limb of each group follows.
MHE_EXPORT int mhe_rotsum_stats(mhe_ctx *c, uint64_t *sums, uint64_t *terms, int reset)
{
    return groupsum_stats(c, &mhe_ctx::rotsum_sums, &mhe_ctx::rotsum_terms, sums, terms, reset);
}

MHE_EXPORT int mhe_rotate_sum(mhe_ctx *c, int count, const uint64_t *const *in, const uint32_t *elts,
                              const uint64_t *const *keys, const int *key_limbs, const int *group, int groups,
                              uint64_t *const *out, int accumulate, int limbs, void *s)
{
    int r = check_limbs(c, limbs, 1);
    if (r) return r;
    if (count < 0 || groups < 0 || (count && (!in || !elts || !keys || !key_limbs || !group)) || (groups && !out))
        return fail(MHE_ERR_ARG, "invalid argument");
    hipStream_t st = S(s);
    const int L = limbs;
    const size_t n = c->n, ps = (size_t)L << c->log_n;
    if (!check_groups(group, count, groups)) return fail(MHE_ERR_ARG, "invalid argument");
    for (int g = 0; g < groups; g++)
        if (!out[g]) return fail(MHE_ERR_ARG, "Galois key not present");
    // every key is checked before the first launch, so a bad key leaves no output half-written
    for (int i = 0; i < count; i++)
        if ((r = check_rotation(c, in[i], elts[i], keys[i], key_limbs[i], limbs))) return r;
    // outputs must be disjoint from every input and from each other (a group's output is written
    // while later chunks still read their inputs)
    for (int g = 0; g < groups; g++)
        if (output_overlaps(out, g, groups, 2 * ps, in, count, 2 * ps))
            return fail(MHE_ERR_ARG, "result cannot point to the same value as operand");
    if (!count) return MHE_OK;
    if (!c->galois_fused || !c->ks_fused)
    {
        // the debugging paths: rotate one by one and add
        u64 *tmp = nullptr;
        if (injected_alloc_failure(c) || mhe_internal_alloc((void **)&tmp, 2 * ps * sizeof(u64), st) != hipSuccess)
            return fail(MHE_ERR_MEMORY, "device allocation failed");
        for (int i = 0; i < count && !r; i++)
        {
            const bool first = (i == 0 || group[i] != group[i - 1]) && !accumulate;
            u64 *o = out[group[i]];
            r = mhe_apply_galois_to(c, in[i], first ? o : tmp, elts[i], keys[i], key_limbs[i], limbs, s);
            if (!r && !first) r = launch_addsub(c, o, tmp, o, 2, limbs, 0, s);
        }
        (void)mhe_internal_free(tmp, st);
        if (r) return r;
        c->rotsum_sums += (unsigned long long)groups;
        c->rotsum_terms += (unsigned long long)count;
        return MHE_OK;
    }
    // all scratch before the first launch: a failed growth leaves every output as it was
    Workspace *w;
    if ((r = get_groupsum(c, st, std::min(count, MHE_MAXB), L, &Workspace::rotsum, &w))) return r;
    const SumPool &sp = w->rotsum;
    // rounds of at most MHE_MAXB groups: their entries, those of one key side by side (a launch of
    // them shares the key stream, k_ks_row_mac share), in chunks of at most MHE_MAXB that cut across
    // groups, then one ModDown forward NTT per limb for all of the round's groups
    for (const GroupSumRound &round : plan_group_sums(count, group, groups, MHE_MAXB, keys))
    {
        for (const GroupSumChunk &ch : round.chunks)
        {
            // permuted (c0, c1) of every entry into its scratch, then the key switch of the permuted c1
            // up to the key products (evaluator.cpp:2193-2214, 2281-2463)
            GalPtrs gp{};
            KsJob jobs[MHE_MAXB];
            GroupSumPtrs rp = groupsum_ptrs(ch, w, sp, 1, L, n);
            for (int e = 0; e < rp.B; e++)
            {
                const int i = ch.entries[e];
                gp.in[e] = in[i];
                gp.out[e] = w->e[e].ct3;
                gp.elt[e] = elts[i];
                jobs[e] = KsJob{ nullptr, w->e[e].ct3 + ps, keys[i], key_limbs[i], nullptr };
                rp.x[e] = w->e[e].ct3;
            }
            for (int z = 0; z < ch.Z(); z++)
            {
                rp.X[z] = out[round.g0 + ch.slot[z]];
                rp.firstx[z] = (ch.first[z] && !accumulate) ? 1 : 0; // out[0] written, not added to
            }
            if ((r = permute_batch(c, gp, rp.B, L, st, true))) return r;
            if ((r = groupsum_fold(c, w, jobs, rp, ch.Z(), L, st))) return r;
        }
        // the round's groups: T -> NTT(T) in place, then out += (A - NTT(T)) P^-1 (out[1] written
        // when not accumulating)
        JobB<JobFwdPlain> fc(2 * L);
        JobB<JobModDownRow> dr(2 * L);
        for (int z = 0; z < round.G; z++)
        {
            u64 *T = sp.at(z, 1, L, n);
            fc.j[z] = fwd_plain(c, T, T, L, 0);
            dr.j[z] = JobModDownRow{ T, sp.at(z, 0, L, n), out[round.g0 + z], c->primes, c->tw, c->invq, L, c->K, c->log_n };
            dr.j[z].fp = c->nm.fp ? 1 : 0;
            dr.j[z].c1_write = accumulate ? 0 : 1;
        }
        fwd_col(fc, c->log_n, 2 * L * round.G, c->nm, st);
        fwd_row(dr, c->log_n, 2 * L * round.G, c->nm, st);
        HIP_LAUNCH_CHECK();
        groupsum_count_adds(c, round, L, accumulate ? 1 : 0, nullptr);
    }
    c->rotsum_sums += (unsigned long long)groups;
    c->rotsum_terms += (unsigned long long)count;
    return MHE_OK;
}
