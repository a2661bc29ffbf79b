// The key-switch and rescale pipelines (host side): the steps the batched entry points and the
// rotation pipelines (rotate.h) share, then switch_key_inplace and rescale_to_next for up to MHE_MAXB
// entries per launch.  Included by mhe.hip once, after the context, the workspace and the job
// builders.
#pragma once

// Key-switching inner product (evaluator.cpp:2410-2463): for output prime I (I == L -> P),
// acc[k][I] = sum_J d_J[I] * key[J][k][I] mod q_I, where d_J[I] is the lifted NTT digit
// (modup[I][J]) or, for I == J, the input target limb itself.  128-bit accumulation with a
// single final Barrett reduction (digits are canonical so < 2^8 terms never overflow).
__global__ __launch_bounds__(256) void k_ks_mac(const u64 *modup, const u64 *target, const u64 *key, u64 *acc,
                                                const PrimeDev *primes, int L, int K, int key_limbs, int log_n, int I0)
{
    const u32 i = (blockIdx.x * 256 + threadIdx.x) * 2;
    const int I = I0 + blockIdx.y;
    const int pi = (I == L) ? K - 1 : I;
    const int ki = (I == L) ? key_limbs - 1 : I;
    const size_t n = (size_t)1 << log_n;
    const PrimeDev p = primes[pi];
    Acc128 a0x{ 0, 0 }, a0y{ 0, 0 }, a1x{ 0, 0 }, a1y{ 0, 0 };
    const size_t kstride = (size_t)key_limbs * n;
    for (int J = 0; J < L; J++)
    {
        const u64 *d = (I == J) ? target + (size_t)J * n : modup + ((size_t)(I - I0) * L + J) * n;
        ulonglong2 x = *(const ulonglong2 *)(d + i);
        const u64 *k0 = key + (size_t)(2 * J) * kstride + (size_t)ki * n;
        ulonglong2 y0 = *(const ulonglong2 *)(k0 + i);
        ulonglong2 y1 = *(const ulonglong2 *)(k0 + kstride + i);
        mac128(a0x, x.x, y0.x);
        mac128(a0y, x.y, y0.y);
        mac128(a1x, x.x, y1.x);
        mac128(a1y, x.y, y1.y);
    }
    ulonglong2 r0, r1;
    r0.x = barrett128(a0x.lo, a0x.hi, p);
    r0.y = barrett128(a0y.lo, a0y.hi, p);
    r1.x = barrett128(a1x.lo, a1x.hi, p);
    r1.y = barrett128(a1y.lo, a1y.hi, p);
    *(ulonglong2 *)(acc + (size_t)I * n + i) = r0;
    *(ulonglong2 *)(acc + (size_t)(L + 1 + I) * n + i) = r1;
}

// One entry of a (batched) key switch.
struct KsJob
{
    u64 *ct;               // [2][L][n]
    const u64 *target;     // [L][n], NTT form
    const u64 *key;        // [digits][2][key_limbs][n]
    int key_limbs;
    u64 *rescale_out;      // HMult: [2][L-1][n] (see run_switch_key_batch), else nullptr
};

// A key of key_limbs limbs serves a switch at `limbs` limbs: the level's primes and the special one.
static int check_key_limbs(mhe_ctx *c, int key_limbs, int limbs)
{
    if (key_limbs < limbs + 1 || key_limbs > c->K) return fail(MHE_ERR_ARG, "kswitch_keys is not valid for encryption parameters");
    return MHE_OK;
}

static int ks_check_key(mhe_ctx *c, const KsJob &j, int L, hipStream_t st, int *kpack)
{
    int r = check_key_limbs(c, j.key_limbs, L);
    if (r) return r;
    // a prepared key (mhe_key_prepare) is recognised by the fused MAC itself (key_word_prepared
    // on a word of each slot); the separate-MAC debugging path reads SEAL's layout only
    *kpack = 1;
    if (!c->ks_fused)
    {
        int tagged = 0;
        int r0 = key_tagged(c, j.key, j.key_limbs, st, &tagged);
        if (r0) return r0;
        if (tagged) return fail(MHE_ERR_ARG, "key switch: prepared keys need the fused key MAC");
        *kpack = 0;
    }
    // the key slice one switch streams: L digits x 2 polys x (L + 1) primes
    c->key_bytes += 2ull * (unsigned long long)L * (unsigned long long)(L + 1) * c->n * 8ull;
    // prepared: doubles stream the same 8 B per residue, the 48-bit planes 6 B for primes below 2^48
    // (the format of a prepared key is not known here without a host sync: counted as doubles)
    c->key_bytes_prep += 2ull * (unsigned long long)L * (unsigned long long)(L + 1) * c->n * 8ull;
    return MHE_OK;
}

// Step 1 of a key switch for B entries: t_e = INTT(src[e]), canonical, into w->e[e].coeff
// (evaluator.cpp:2351-2354): the row pass from src, the column pass in place.  run_if (or null): per
// entry the flag its jobs test, see JobStrided.
static void intt_targets(mhe_ctx *c, Workspace *w, const u64 *const *src, int B, int L, const int *const *run_if,
                         hipStream_t st)
{
    const size_t n = c->n;
    JobB<JobStrided> j(L);
    for (int e = 0; e < B; e++)
        j.j[e] = JobStrided{ src[e], w->e[e].coeff, n, n, 0, 1, c->primes, c->itw, c->log_n, 0, run_if ? run_if[e] : nullptr };
    inv_row(j, c->log_n, B * L, c->nm, st);
    for (int e = 0; e < B; e++)
    {
        j.j[e].src = w->e[e].coeff;
        j.j[e].mode = 1;
    }
    inv_col(j, c->log_n, B * L, c->nm, st);
}

// The pointers of the ModUp and key-MAC kernels for B entries: each entry's scratch, its job's target
// and key, its key products to accs[e] (null: the entry's scratch).  run_if as in intt_targets.
static KsPtrs ks_ptrs(Workspace *w, const KsJob *jobs, int B, u64 *const *accs, const int *const *run_if)
{
    KsPtrs kp{};
    for (int e = 0; e < B; e++)
    {
        kp.coeff[e] = w->e[e].coeff;
        kp.inter[e] = w->e[e].modup;
        kp.target[e] = jobs[e].target;
        kp.key[e] = jobs[e].key;
        kp.acc[e] = accs ? accs[e] : w->e[e].acc;
        kp.key_limbs[e] = jobs[e].key_limbs;
        kp.run_if[e] = run_if ? run_if[e] : nullptr;
    }
    return kp;
}

// The digit-major ModUp column pass (k_modup_col) of B entries at L limbs, every output prime, in the
// output-prime groups that modup_groups picks for the launch's size (MHE_KS_COLGROUPS=n forces n).
// Counted for mhe_modup_stats.
static void ks_modup_col(mhe_ctx *c, const KsPtrs &kp, int B, int L, int pack, hipStream_t st)
{
    const int IG = modup_groups(c->ks_colgroups, c->log_n, L, B, L + 1);
    modup_col(kp, B, c->primes, c->tw, L, c->K, c->log_n, c->nm_ks, 0, L + 1, IG, pack, st);
    c->modup_launches++;
    c->modup_ig_sum += (unsigned long long)IG;
}

// One key for every entry of a launch of several: XCD-grouped entries (k_ks_row_mac share).
static int ks_shared_key(const mhe_ctx *c, const KsJob *jobs, int B)
{
    if (B < 2 || !c->ks_share) return 0;
    for (int e = 1; e < B; e++)
        if (jobs[e].key != jobs[0].key || jobs[e].key_limbs != jobs[0].key_limbs) return 0;
    return 1;
}

// The pairing switch and counters of the fused MAC's launches (ntt.h KsPair).
static KsPair ks_pair_of(mhe_ctx *c)
{
    return KsPair{ c->ks_pair, &c->ks_paired, &c->ks_single };
}

// The fused HMult tail for B slots: with acc the key products (or their sum), ct the product's first
// two polys (or their sum) and S = ct + ModDown(acc), the rescale of S to out [2][L-1][n].  Limb L-1
// only: ct += (acc - NTT(t)) P^-1, t from col1's column pass into the slot's modup; last = INTT(S[L-1])
// into its coeff; then limbs 0 .. L-2 through one forward NTT each, col2's column pass (modup = the
// lifts of the special limbs and of last) and JobMDRRow.  ct limb L-1 is overwritten on the way.
struct TailSlot
{
    const u64 *acc; // [2][L+1][n]
    u64 *ct;        // [2][L][n]
    u64 *out;       // [2][L-1][n]
};

template <class Col1, class Col2>
static void run_hmult_tail(mhe_ctx *c, Workspace *w, const TailSlot *s, int B, int L, hipStream_t st, Col1 col1, Col2 col2)
{
    const int log_n = c->log_n, fp = c->nm.fp ? 1 : 0;
    const size_t n = c->n;
    JobB<JobModDownRow> dr(2);
    JobB<JobLastInv> li(2);
    JobB<JobStrided> j2(2);
    JobB<JobMDRRow> mr(2 * (L - 1));
    for (int e = 0; e < B; e++)
    {
        const WsEntry &we = w->e[e];
        dr.j[e] = JobModDownRow{ we.modup, s[e].acc, s[e].ct, c->primes, c->tw, c->invq, L, c->K, log_n, L - 1 };
        dr.j[e].fp = fp;
        li.j[e] = JobLastInv{ s[e].ct, we.coeff, c->primes, c->itw, L, log_n, 1 };
        j2.j[e] = JobStrided{ we.coeff, we.coeff, n, n, L - 1, 0, c->primes, c->itw, log_n, 1 };
        mr.j[e] = JobMDRRow{ we.modup, s[e].acc, s[e].ct, s[e].out, c->primes, c->tw, c->invq, L, c->K, log_n, fp };
    }
    col1();
    fwd_row(dr, log_n, 2 * B, c->nm, st);
    inv_row(li, log_n, 2 * B, c->nm, st);
    inv_col(j2, log_n, 2 * B, c->nm, st);
    col2();
    fwd_row(mr, log_n, 2 * (L - 1) * B, c->nm, st);
}

// Step 4 of a (batched) key switch, the ModDown (evaluator.cpp:2466-2524), over the key inner
// products in w->e[e].acc (or accs[e]): ct_e += ModDown(acc_e), or with rescale_out the fused HMult tail (see
// run_switch_key_batch).  special_inv_done: the key MAC already ran the special limbs' inverse
// row pass.
static void run_moddown(mhe_ctx *c, const KsJob *jobs, int B, int L, Workspace *w, int special_inv_done, int c1_write,
                        hipStream_t st, u64 *const *accs = nullptr)
{
    // key products of entry e: accs[e] when given (hoisted rotations), else the entry's scratch
    auto A = [&](int e) { return accs ? accs[e] : w->e[e].acc; };
    const bool hm = jobs[0].rescale_out != nullptr;
    const int log_n = c->log_n;
    const size_t n = c->n;
    // ModDown (evaluator.cpp:2466-2524): INTT_lazy of the special limbs, then fused
    //    lift + NTT + (c + 4q - t) * P^-1 + add.
    JobB<JobStrided> j(2);
    for (int e = 0; e < B; e++) j.j[e] = special_limbs(c, A(e), L);
    if (!special_inv_done) inv_row(j, log_n, 2 * B, c->nm, st);
    // the special limbs' inverse column pass runs inside the lift column pass (k_icol_lift)
    // (not in the HMult tail: JobMDRCol reads the fully inverse-transformed special limbs)
    ColSrc cs{};
    cs.stride = (size_t)(L + 1) * n;
    cs.per = 2;
    cs.primes = c->primes;
    cs.itw = c->itw;
    cs.pi = c->K - 1;
    for (int e = 0; e < B; e++) cs.src[e] = A(e) + (size_t)L * n;
    const bool fuse = c->icol_fused && (!hm || L < 2);
    if (!fuse) inv_col(j, log_n, 2 * B, c->nm, st);
    if (!hm || L < 2)
    {
        JobB<JobModDownCol> dc(2 * L);
        JobB<JobModDownRow> dr(2 * L);
        for (int e = 0; e < B; e++)
        {
            dc.j[e] = JobModDownCol{ A(e), w->e[e].modup, c->primes, c->tw, L, c->K, log_n };
            dr.j[e] = JobModDownRow{ w->e[e].modup, A(e), jobs[e].ct, c->primes, c->tw, c->invq, L, c->K, log_n };
            dr.j[e].fp = c->nm.fp ? 1 : 0;
            dr.j[e].c1_write = c1_write;
        }
        if (fuse)
            icol_lift(cs, dc, 2 * B, L, log_n, c->nm, st);
        else
            fwd_col(dc, log_n, 2 * L * B, c->nm, st);
        fwd_row(dr, log_n, 2 * L * B, c->nm, st);
    }
    else
    {
        TailSlot ts[MHE_MAXB];
        for (int e = 0; e < B; e++) ts[e] = TailSlot{ A(e), jobs[e].ct, jobs[e].rescale_out };
        run_hmult_tail(
            c, w, ts, B, L, st,
            [&] {
                JobB<JobModDownCol> dc(2);
                for (int e = 0; e < B; e++)
                    dc.j[e] = JobModDownCol{ A(e), w->e[e].modup, c->primes, c->tw, L, c->K, log_n, L - 1 };
                fwd_col(dc, log_n, 2 * B, c->nm, st);
            },
            [&] {
                JobB<JobMDRCol> mc(2 * (L - 1));
                for (int e = 0; e < B; e++)
                    mc.j[e] = JobMDRCol{ A(e), w->e[e].coeff, w->e[e].modup, c->primes, c->tw, c->invq, L, c->K, log_n,
                                         c->nm.fp ? 1 : 0 };
                if (c->nm.fp == 1)
                    col_lift2(mc, 2 * B, L - 1, log_n, c->nm, st);
                else
                    fwd_col(mc, log_n, 2 * (L - 1) * B, c->nm, st);
            });
    }
}

// switch_key_inplace (evaluator.cpp:2281-2525) for B <= MHE_MAXB independent entries of one
// level L, every kernel launched once for all of them: ct_e[2][L][n] += KS(target_e[L][n]).
// rescale_out != nullptr (HMult; all entries or none): ct_e is the first two polys of a product,
// and instead of ct += KS(target) the result of rescale_to_next(ct + KS(target)) goes to
// rescale_out [2][L-1][n] (JobMDRCol / JobMDRRow); ct limb L-1 is overwritten on the way.
// c1_write: ct[1] is taken as zero and written, not read (target may then alias ct[1]: it is last
// read by the key MAC, before the ModDown writes ct).
// front != nullptr (mhe_rotate_sum; fused key MAC only): stop before the ModDown, the key products
// left in the entries' scratch (w->e[e].acc), ct untouched; *front = the key MAC already ran the
// special limbs' inverse row pass.
// pair = 0: the key MAC runs one entry per workgroup whatever the context's switch says (the hoisting
// check recomputes by the kept one-entry kernel).
static int run_switch_key_batch(mhe_ctx *c, const KsJob *jobs, int B, int L, hipStream_t st, int c1_write = 0,
                                int *front = nullptr, int pair = 1)
{
    if (B < 1 || B > MHE_MAXB) return fail(MHE_ERR_ARG, "key switch: batch size out of range");
    // mhe_debug_fail_switch's countdown (tests): this launch sequence fails before its first launch
    for (int v = c->fail_switch.load(); v > 0;)
        if (c->fail_switch.compare_exchange_weak(v, v - 1))
        {
            if (v == 1) return fail(MHE_ERR_MEMORY, "device allocation failed (injected)");
            break;
        }
    const bool hm = jobs[0].rescale_out != nullptr;
    for (int e = 0; e < B; e++)
        if ((jobs[e].rescale_out != nullptr) != hm) return fail(MHE_ERR_ARG, "key switch: mixed fused-rescale batch");
    if (c1_write && hm) return fail(MHE_ERR_ARG, "key switch: c1_write with a fused rescale");
    if (!c->ks_fused && B > 1)
    {
        // the separate-MAC debugging path runs one entry at a time
        for (int e = 0; e < B; e++)
            if (int r = run_switch_key_batch(c, jobs + e, 1, L, st, c1_write, nullptr, pair)) return r;
        return MHE_OK;
    }
    int kpack = 1, r;
    for (int e = 0; e < B; e++)
        if ((r = ks_check_key(c, jobs[e], L, st, &kpack))) return r;
    count_op(c, MHE_OPK_KEYSWITCH, L, (unsigned long long)B);
    if (hm) count_op(c, MHE_OPK_RESCALE, L, 2ull * B); // the fused HMult tail rescales both polys
    Workspace *w;
    if ((r = get_ws(c, st, c->K - 1, &w, B))) return r;
    const int log_n = c->log_n;
    int special_inv_done = 0; // the fused MAC ran the special limbs' inverse row pass
    // 1. t_target = INTT(target), canonical
    const u64 *targets[MHE_MAXB];
    for (int e = 0; e < B; e++) targets[e] = jobs[e].target;
    intt_targets(c, w, targets, B, L, nullptr, st);
    if (c->ks_fused)
    {
        // 2+3. ModUp column pass, then its row pass fused with the key MAC so NTT'd digits
        //      never leave registers; every output prime in one launch (chunks of output primes
        //      sized for the Infinity Cache measured slower at every size).
        // 48-bit intermediate (ntt.h tile16): only k_modup_col writes it, so only with column groups
        // and it leaves the FP sweeps' other limbs as doubles (MHE_INTER_F64), as the fused MAC reads them
        const int pack = c->ks_colgroups != 0 ? ((c->ks_pack ? 1 : 0) | MHE_INTER_F64) : 0;
        const KsPtrs kp = ks_ptrs(w, jobs, B, nullptr, nullptr);
        hipEvent_t *tc = timing_slot(c, w, TK_MODUP_COL, st);
        if (c->ks_colgroups != 0)
            ks_modup_col(c, kp, B, L, pack, st);
        else
        {
            JobB<JobModUpCol> j((L + 1) * L);
            // f64 follows nm_ks, the MAC's arithmetic (its reader), not nm, this pass's own: the store
            // converts a word below 2^52 whichever butterflies made it
            for (int e = 0; e < B; e++) j.j[e] = JobModUpCol{ w->e[e].coeff, w->e[e].modup, c->primes, c->tw, L, c->K, log_n, 0, c->nm_ks.fp ? 1 : 0 };
            fwd_col(j, log_n, B * (L + 1) * L, c->nm, st);
        }
        timing_end(tc, st);
        hipEvent_t *tm = timing_slot(c, w, TK_KS_ROW_MAC, st);
        KsPair pr = ks_pair_of(c);
        if (!pair) pr.on = 0;
        special_inv_done = ks_row_mac_chunk(kp, B, c->primes, c->tw, L, c->K, log_n, c->nm_ks, 0, L + 1, pack, kpack,
                                            ks_shared_key(c, jobs, B), pr, c->itw, 1, st);
        timing_end(tm, st);
    }
    else
    {
        // 2+3. (MHE_KS_FUSED=0, the independent debugging path) ModUp + key inner products in
        //      three kernels: lift digit J to prime I and NTT it (evaluator.cpp:2386-2408; I == J
        //      skipped), then acc[k][I] = sum_J digit * key[J][k][I] (evaluator.cpp:2410-2463).
        //      (One entry: B == 1 here.)
        const WsEntry &s = w->e[0];
        JobModUpCol j{ s.coeff, s.modup, c->primes, c->tw, L, c->K, log_n, 0 };
        fwd_col(j, log_n, (L + 1) * L, c->nm, st);
        JobModUpRow r2{ s.modup, c->primes, c->tw, L, c->K, log_n, 0 };
        fwd_row(r2, log_n, (L + 1) * L, c->nm, st);
        dim3 grid((unsigned)(c->n / 512), L + 1);
        hipLaunchKernelGGL(k_ks_mac, grid, dim3(256), 0, st, s.modup, jobs[0].target, jobs[0].key, s.acc, c->primes, L,
                           c->K, jobs[0].key_limbs, log_n, 0);
    }
    if (front)
        *front = special_inv_done;
    else
        run_moddown(c, jobs, B, L, w, special_inv_done, c1_write, st);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

static int run_switch_key(mhe_ctx *c, u64 *ct, const u64 *target, const u64 *key, int key_limbs, int L,
                          hipStream_t st, u64 *rescale_out = nullptr, int c1_write = 0)
{
    const KsJob j{ ct, target, key, key_limbs, rescale_out };
    return run_switch_key_batch(c, &j, 1, L, st, c1_write);
}

// rescale_to_next (util/rns.cpp:737-808) of B <= MHE_MAXB independent ciphertexts of `size` polys
// at L limbs, in[e] -> out[e] ([size][L-1][n]), every kernel launched once for all of them.
static int run_rescale_batch(mhe_ctx *c, const u64 *const *in, u64 *const *out, int B, int size, int L, hipStream_t st)
{
    if (B < 1 || B > MHE_MAXB) return fail(MHE_ERR_ARG, "rescale: batch size out of range");
    Workspace *w;
    int r = get_ws(c, st, c->K - 1, &w, B);
    if (r) return r;
    count_op(c, MHE_OPK_RESCALE, L, (unsigned long long)B * size);
    const int log_n = c->log_n;
    // last[s] = INTT(in[s][L-1]) canonical -> the entry's coeff (size <= 3 polys)
    JobB<JobLastInv> li(size);
    JobB<JobRescaleCol> rc(size * (L - 1));
    JobB<JobRescaleRow> rr(size * (L - 1));
    ColSrc cs{};
    cs.stride = c->n;
    cs.per = size;
    cs.primes = c->primes;
    cs.itw = c->itw;
    cs.pi = L - 1;
    for (int e = 0; e < B; e++)
    {
        li.j[e] = JobLastInv{ in[e], w->e[e].coeff, c->primes, c->itw, L, log_n, 1 };
        rc.j[e] = JobRescaleCol{ w->e[e].coeff, w->e[e].modup, c->primes, c->tw, L, log_n };
        rr.j[e] = JobRescaleRow{ w->e[e].modup, in[e], out[e], c->primes, c->tw, c->invq, L, c->K, log_n };
        rr.j[e].fp = c->nm.fp ? 1 : 0;
        cs.src[e] = w->e[e].coeff;
    }
    inv_row(li, log_n, size * B, c->nm, st);
    if (c->icol_fused)
    {
        // the last limb's inverse column pass runs inside the lift column pass (k_icol_lift)
        icol_lift(cs, rc, size * B, L - 1, log_n, c->nm, st);
    }
    else
    {
        JobB<JobStrided> j2(size);
        for (int e = 0; e < B; e++) j2.j[e] = JobStrided{ w->e[e].coeff, w->e[e].coeff, c->n, c->n, L - 1, 0, c->primes, c->itw, log_n, 1 };
        inv_col(j2, log_n, size * B, c->nm, st);
        fwd_col(rc, log_n, size * (L - 1) * B, c->nm, st);
    }
    fwd_row(rr, log_n, size * (L - 1) * B, c->nm, st);
    HIP_LAUNCH_CHECK();
    return MHE_OK;
}

static int run_rescale(mhe_ctx *c, const u64 *in, u64 *out, int size, int L, hipStream_t st)
{
    return run_rescale_batch(c, &in, &out, 1, size, L, st);
}
