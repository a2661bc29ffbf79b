"""Per-operation timing at ResNet levels (N=2^16, the CNN chain 51 + 16x46 + 14x51 + special 51).

Times the evaluator's small-level building blocks through the C ABI with HIP events on the engine's
stream: rescale (1 and 4 ciphertexts per launch), key switch / relinearize (1 and 4), rotations with
4 distinct keys, forward NTT of one ciphertext, and an HMult.  Prints one JSON line per operation.
rotaddGxT / rotsumGxT (--rotsum GxT): the giant-step sums of G images, T rotations of distinct inputs
each with T keys shared over the images -- mhe_apply_galois_batch + T - 1 mhe_add per sum against one
mhe_rotate_sum.
prodseqGxT / prodsumGxT (--ops prodseq,prodsum --prodsum GxT[d],...): G sums of T products, doubled with
a trailing d -- mhe_ct_multiply, mhe_switch_key_batch, the mhe_adds and mhe_rescale_batch against
mhe_ct_multiply and one mhe_relin_sum_rescale; words compared first, interleaved rounds (prod_bench).
encseqB / encbatchB (--ops encrypt --encrypt B,...): B public-key encryptions with plaintexts -- per entry
the sequence of Encryptor::encrypt (3 mhe_prng_small, 2 mhe_ntt_forward, 2 x (mhe_multiply_plain, mhe_add),
mhe_rescale_to_next, mhe_add of the plaintext; buffers allocated once) against one mhe_encrypt_pk_batch;
words compared first, interleaved rounds (enc_bench).
keyseqD / keybatchD (--ops keygen --keygen D,...): one key-switching key of D digits (D = K - 1: a full
key; fewer: a level-truncated one) -- per digit the sequence seal's make_kswitch_key_seq issues
(mhe_prng_uniform_bulk with the download of its reject count and the host synchronisation, and for a
digit with rejected words the second download, the host's ordered walk of the stream tail, the upload
and mhe_prng_apply_fixes with its synchronisation; mhe_prng_small, mhe_ntt_forward, mhe_multiply_plain, mhe_add, mhe_negate, mhe_multiply_scalar, mhe_add,
and four device copies for a truncated key; buffers allocated once, which spares the sequence its three
stream-ordered allocations per digit) against one mhe_encrypt_sk_batch; words compared first, interleaved
rounds timed on the host clock, since the sequence synchronises (key_bench).
Used for A/B runs of library variants (MHE_LIB_PATH=build/var/NAME/libmhe.so).

    python scripts/ubench_ops.py [--limbs 31] [--reps 50]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-gpt-2_amd"))

import torch  # noqa: E402

import mhe  # noqa: E402


def prod_bench(eng, rnd, key, L, n, shape, reps, rounds, st):
    """prodseq against prodsum for G sums of T products (shape "GxT", a trailing d: every sum doubled).
    prodseq is the sequence the merged call replaces: mhe_ct_multiply per product, one
    mhe_switch_key_batch, the mhe_adds of every sum, one mhe_rescale_batch.  prodsum: the same
    products, then one mhe_relin_sum_rescale.  The legs' words are compared first; then `rounds`
    interleaved rounds of HIP events around `reps` calls after 3 warm-ups.  One JSON line per leg and
    round, then one with the medians and each leg's spread (max - min over its rounds)."""
    dbl = shape.endswith("d")
    G, T = (int(x) for x in shape.rstrip("d").split("x"))
    a = [rnd(2, L, n, limbs=L) for _ in range(G * T)]
    b = [rnd(2, L, n, limbs=L) for _ in range(G * T)]
    ct3 = [eng.empty(3, L, n) for _ in range(G * T)]
    groups = [g for g in range(G) for _ in range(T)]
    out_seq = [eng.empty(2, L - 1, n) for _ in range(G)]
    out_sum = [eng.empty(2, L - 1, n) for _ in range(G)]

    def products():
        for x, y, c in zip(a, b, ct3):
            eng.multiply(x, y, c)

    def prodseq():
        products()
        eng.switch_key_batch([c[:2] for c in ct3], [c[2] for c in ct3], [key] * len(ct3))
        sums = []
        for g in range(G):
            s = ct3[g * T][:2]
            for t in range(1, T):
                eng.add(s, ct3[g * T + t][:2], s)
            if dbl:
                eng.add(s, s, s)
            sums.append(s)
        eng.rescale_batch(sums, out_seq)

    def prodsum():
        products()
        eng.relin_sum_rescale(ct3, key, groups=groups, twice=[dbl] * G, outs=out_sum)

    legs = {"prodseq": prodseq, "prodsum": prodsum}
    prodseq()
    prodsum()
    torch.cuda.synchronize()
    if not all(torch.equal(x, y) for x, y in zip(out_seq, out_sum)):
        raise SystemExit(f"prodseq and prodsum differ at {shape}, {L} limbs")
    us = {k: [] for k in legs}
    for r in range(rounds):
        for name, f in legs.items():
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            for _ in range(reps):
                f()
            t1.record(st)
            torch.cuda.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1000 / reps)
            print(json.dumps({"op": name + shape, "limbs": L, "round": r, "us": round(us[name][-1], 2)}), flush=True)
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(json.dumps({"op": "prod" + shape, "limbs": L, "words_equal": True,
                      "prodseq_us": round(med["prodseq"], 2), "prodsum_us": round(med["prodsum"], 2),
                      "prodseq_spread_us": round(max(us["prodseq"]) - min(us["prodseq"]), 2),
                      "prodsum_spread_us": round(max(us["prodsum"]) - min(us["prodsum"]), 2),
                      "ratio": round(med["prodsum"] / med["prodseq"], 4)}), flush=True)


def enc_bench(eng, rnd, L, n, B, reps, rounds, st):
    """encseq against encbatch for B encryptions at L limbs (the dropped prime is prime L).  encseq is
    the sequence Encryptor::encrypt issues per ciphertext, on buffers allocated once; encbatch one
    mhe_encrypt_pk_batch.  The legs' words are compared first; then `rounds` interleaved rounds of HIP
    events around `reps` calls after 3 warm-ups.  One JSON line per leg and round, then one with the
    medians and each leg's spread (max - min over its rounds)."""
    m, K = L + 1, eng.K
    pk = rnd(2, K, n, limbs=K)
    seeds = [[100 + i, 2, 3, 4, 5, 6, 7, 8] for i in range(B)]
    plains = [rnd(L, n, limbs=L) for _ in range(B)]
    u, e, c = eng.empty(m, n), eng.empty(2, m, n), eng.empty(2, m, n)
    state = torch.zeros(2, dtype=torch.int32, device=eng.torch_device)
    out_seq = [eng.empty(2, L, n) for _ in range(B)]
    out_bat = [eng.empty(2, L, n) for _ in range(B)]

    def encseq():
        for i in range(B):
            eng.prng_small("ternary", m, seeds[i], out=u, state=state)
            eng.prng_small("cbd", m, seeds[i], 4 * n, out=e[0], state=state)
            eng.prng_small("cbd", m, seeds[i], 10 * n, out=e[1], state=state)
            eng.ntt_forward(u, lazy=True)
            eng.ntt_forward(e, lazy=True)
            for j in range(2):
                eng.multiply_plain(u, pk[j, :m], out=c[j])
                eng.add(e[j], c[j], out=c[j])
            eng.rescale_to_next(c, out_seq[i])
            eng.add(out_seq[i][0], plains[i], out=out_seq[i][0])

    def encbatch():
        eng.encrypt_pk_batch(seeds, pk, plains, L, outs=out_bat)

    legs = {"encseq": encseq, "encbatch": encbatch}
    encseq()
    encbatch()
    torch.cuda.synchronize()
    if not all(torch.equal(x, y) for x, y in zip(out_seq, out_bat)):
        raise SystemExit(f"encseq and encbatch differ at {B} entries, {L} limbs")
    us = {k: [] for k in legs}
    for r in range(rounds):
        for name, f in legs.items():
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            for _ in range(reps):
                f()
            t1.record(st)
            torch.cuda.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1000 / reps)
            print(json.dumps({"op": f"{name}{B}", "limbs": L, "round": r, "us": round(us[name][-1], 2)}), flush=True)
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(json.dumps({"op": f"encrypt{B}", "limbs": L, "words_equal": True,
                      "encseq_us": round(med["encseq"], 2), "encbatch_us": round(med["encbatch"], 2),
                      "encseq_spread_us": round(max(us["encseq"]) - min(us["encseq"]), 2),
                      "encbatch_spread_us": round(max(us["encbatch"]) - min(us["encbatch"]), 2),
                      "ratio": round(med["encbatch"] / med["encseq"], 4)}), flush=True)


def key_bench(eng, rnd, moduli, n, D, reps, rounds):
    """keyseq against keybatch for one key of D digits over the context's K primes.  The legs' words
    are compared first; then `rounds` interleaved rounds of `reps` keys after one warm-up, each round
    timed on the host clock from a drained device to a drained device.  One JSON line per leg and
    round, then one with the medians and each leg's spread (max - min over its rounds)."""
    import ctypes
    import time

    K, KL = eng.K, D + 1
    full = KL == K
    lib, h = mhe.lib(), eng._h
    sk, nk = rnd(K, n, limbs=K), rnd(K, n, limbs=K)
    seeds = [[200 + j, 2, 3, 4, 5, 6, 7, 8] for j in range(D)]
    # the public seed of a: the first 64 bytes of the bootstrap stream, as the host derives it
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    pub = [np.frombuffer(O.prng_bytes(sd, 64), dtype=np.uint64).copy() for sd in seeds]
    # the first words after the bulk of a's stream, for the host walk of a digit with rejected words
    # (seal's StreamReader computes them on the host as it walks; here once, outside the timed region)
    tails = [np.frombuffer(O.prng_bytes([int(w) for w in pb], (K * n + 1024) * 8), dtype=np.uint64)[K * n:].copy()
             for pb in pub]
    mmul = [(1 << 64) - 1 - (((1 << 64) - 1) % int(qi)) - 1 for qi in moduli]
    idx = np.arange(K, dtype=np.int32)
    idx_p = idx.ctypes.data_as(ctypes.c_void_p)
    cap = 1 << 16
    rej = torch.zeros(cap, dtype=torch.int64, device=eng.torch_device)
    cnt = torch.zeros(1, dtype=torch.int32, device=eng.torch_device)
    key_seq, key_bat = eng.empty(D, 2, KL, n), eng.empty(D, 2, KL, n)
    tmp, t = eng.empty(2, K, n), eng.empty(K, n)
    def keyseq():
        for j in range(D):
            c = key_seq[j] if full else tmp
            cnt.zero_()
            rc = lib.mhe_prng_uniform_bulk(h, pub[j].ctypes.data_as(ctypes.c_void_p), K, idx_p, idx_p, c[1].data_ptr(),
                                           rej.data_ptr(), cnt.data_ptr(), cap, eng.stream())
            if rc:
                raise SystemExit(mhe.lib().mhe_last_error().decode())
            count = int(cnt.item())  # the download and the host synchronisation
            if count:
                # rnd::sample_uniform_host_walk: the indices come back, are ordered and redrawn in turn
                tail, ti, fixes = tails[j], 0, []
                for g in sorted(rej[:count].cpu().tolist()):
                    l = g // n
                    while int(tail[ti]) >= mmul[l]:
                        ti += 1
                    fixes += [l * n + g % n, int(tail[ti]) % int(moduli[l])]
                    ti += 1
                fx = torch.from_numpy(np.array(fixes, np.uint64).view(np.int64)).to(eng.torch_device)
                if lib.mhe_prng_apply_fixes(h, fx.data_ptr(), count, c[1].data_ptr(), eng.stream()):
                    raise SystemExit(mhe.lib().mhe_last_error().decode())
                torch.cuda.synchronize()  # the host fix list is temporary
            eng.prng_small("cbd", K, seeds[j], 64, out=c[0])
            eng.ntt_forward(c[0], lazy=True)
            eng.multiply_plain(sk, c[1], out=t)
            eng.add(t, c[0], out=c[0])
            eng.negate(c[0], out=c[0])
            f = [0] * K
            f[j] = P % q[j]
            eng.multiply_scalar(nk, f, out=t)
            eng.add(c[0], t, out=c[0])
            if not full:
                for p in range(2):
                    key_seq[j, p, :D].copy_(tmp[p, :D])
                    key_seq[j, p, D].copy_(tmp[p, K - 1])

    def keybatch():
        eng.encrypt_sk_batch(seeds, sk, K, D, 1, [nk] * D, list(range(D)), outs=[key_bat[j] for j in range(D)])

    q, P = moduli, moduli[-1]
    legs = {"keyseq": keyseq, "keybatch": keybatch}
    keyseq()
    keybatch()
    torch.cuda.synchronize()
    if not torch.equal(key_seq, key_bat):
        raise SystemExit(f"keyseq and keybatch differ at {D} digits")
    us = {k: [] for k in legs}
    for r in range(rounds):
        for name, f in legs.items():
            f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6 / reps)
            print(json.dumps({"op": f"{name}{D}", "limbs": K, "round": r, "us": round(us[name][-1], 2)}), flush=True)
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(json.dumps({"op": f"keygen{D}", "limbs": K, "words_equal": True, "key_bytes": D * 2 * KL * n * 8,
                      "keyseq_us": round(med["keyseq"], 2), "keybatch_us": round(med["keybatch"], 2),
                      "keyseq_spread_us": round(max(us["keyseq"]) - min(us["keyseq"]), 2),
                      "keybatch_spread_us": round(max(us["keybatch"]) - min(us["keybatch"]), 2),
                      "ratio": round(med["keybatch"] / med["keyseq"], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limbs", type=int, default=31)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ops", default="rescale,rescale4,ks,ks4,ks4s,rot4,ntt,hmult")
    ap.add_argument("--bsgs", default="8x7", help="inputs x rotations of the bsgs op (keys shared over inputs)")
    ap.add_argument("--rotsum", default="1x8", help="sums x rotations per sum of the rotadd / rotsum ops")
    ap.add_argument("--hoist", type=int, default=None, help="hoisted rotations on (1) / off (0); default: the context's")
    ap.add_argument("--prodsum", default="8x1,8x1d,1x8,4x2",
                    help="sums x products per sum of the prodseq / prodsum ops, comma-separated; a trailing d: doubled")
    ap.add_argument("--prod-reps", type=int, default=20, help="calls per timed round of prodseq / prodsum")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds of prodseq / prodsum / encrypt")
    ap.add_argument("--encrypt", default="8,1", help="entries per call of the encrypt op, comma-separated")
    ap.add_argument("--keygen", default="31,12", help="digits per key of the keygen op, comma-separated")
    ap.add_argument("--key-reps", type=int, default=5, help="keys per timed round of keyseq / keybatch")
    a = ap.parse_args()
    log_n, n = 16, 1 << 16
    bits = [51] + [46] * 16 + [51] * 14 + [51]
    moduli = mhe.coeff_modulus_create(n, bits)
    eng = mhe.Engine(log_n, moduli, device=0)
    if a.hoist is not None:
        eng.set_hoist(bool(a.hoist))
    K, L = len(moduli), a.limbs
    qs = torch.tensor(np.array(moduli, np.uint64).view(np.int64), device=eng.torch_device)

    def rnd(*shape, limbs):
        # residues below each limb's prime (shape [..., limbs, n])
        g = torch.randint(0, 2**62, shape, dtype=torch.int64, device=eng.torch_device)
        q = qs[:limbs].view(*([1] * (len(shape) - 2)), limbs, 1)
        return torch.remainder(g, q)

    st = torch.cuda.current_stream(eng.torch_device)
    if a.ops == "keygen":
        # on its own: the keys it makes are the large buffers
        for D in a.keygen.split(","):
            key_bench(eng, rnd, moduli, n, int(D), a.key_reps, a.rounds)
        return
    if a.ops == "encrypt":
        # on its own: none of the key-switching keys the other ops need
        for B in a.encrypt.split(","):
            enc_bench(eng, rnd, L, n, int(B), a.prod_reps, a.rounds, st)
        return
    eng.reserve(K - 1)
    keys = [rnd(L, 2, K, n, limbs=K) for _ in range(4)]
    for k in keys:
        eng.key_prepare(k)
    cts = [rnd(2, L, n, limbs=L) for _ in range(8)]
    ct3 = [rnd(3, L, n, limbs=L) for _ in range(4)]
    outs = [eng.empty(2, L - 1, n) for _ in range(8)]
    rot_out = [eng.empty(2, L, n) for _ in range(4)]
    elts = [pow(5, s, 2 * n) for s in (1, 2, 4, 8)]
    # bsgs: the BSGS baby steps of several images (FiberBatch): each input rotated R ways, the R keys
    # shared by the inputs -- the hoisted path (csrc/hoist.h) when hoisting is on (--hoist 1)
    if "bsgs" in a.ops:
        H, R = (int(x) for x in a.bsgs.split("x"))
        bkeys = [rnd(L, 2, K, n, limbs=K) for _ in range(R)]
        for k in bkeys:
            eng.key_prepare(k)
        bin_ = [rnd(2, L, n, limbs=L) for _ in range(H)]
        b_in = [c for c in bin_ for _ in range(R)]
        b_el = [pow(5, s + 1, 2 * n) for _ in range(H) for s in range(R)]
        b_k = [bkeys[s] for _ in range(H) for s in range(R)]
        b_out = [eng.empty(2, L, n) for _ in b_in]

    if "rotsum" in a.ops or "rotadd" in a.ops:
        G, T = (int(x) for x in a.rotsum.split("x"))
        rkeys = [rnd(L, 2, K, n, limbs=K) for _ in range(T)]
        for k in rkeys:
            eng.key_prepare(k)
        r_in = [rnd(2, L, n, limbs=L) for _ in range(G * T)]
        r_el = [pow(5, 8 * (t + 1), 2 * n) for _ in range(G) for t in range(T)]
        r_k = [rkeys[t] for _ in range(G) for t in range(T)]
        r_grp = [g for g in range(G) for _ in range(T)]
        r_rot = [eng.empty(2, L, n) for _ in r_in]
        r_sum = [eng.empty(2, L, n) for _ in range(G)]

    def rotadd():
        eng.apply_galois_batch(r_in, r_el, r_k, r_rot)
        for g in range(G):
            for t in range(1, T):
                eng.add(r_rot[g * T], r_rot[g * T + t], r_rot[g * T])

    ops = {
        "rotadd": rotadd,
        "rotsum": lambda: eng.rotate_sum(r_in, r_el, r_k, groups=r_grp, outs=r_sum),
        "rescale": lambda: eng.rescale_to_next(cts[0], outs[0]),
        "rescale4": lambda: eng.rescale_batch(cts[:4], outs[:4]),
        "rescale8": lambda: eng.rescale_batch(cts, outs),
        "ks": lambda: eng.relinearize(ct3[0], keys[0]),
        "ks4": lambda: eng.switch_key_batch([c[:2] for c in ct3], [c[2] for c in ct3], keys),
        "ks4s": lambda: eng.switch_key_batch([c[:2] for c in ct3], [c[2] for c in ct3], [keys[0]] * 4),
        "rot4": lambda: eng.apply_galois_batch(cts[:4], elts, keys, rot_out),
        "bsgs": lambda: eng.apply_galois_batch(b_in, b_el, b_k, b_out),
        "ntt": lambda: eng.ntt_forward(cts[1]),
        "hmult": lambda: eng.hmult(cts[2], cts[3], keys[0], outs[1]),
        # elementwise, one ciphertext (2 x L limbs): HBM-bound, so us -> GB/s directly
        "add": lambda: eng.add(cts[0], cts[1], rot_out[0]),
        "mulplain": lambda: eng.multiply_plain(cts[0], cts[2][0], rot_out[0]),
    }
    names = a.ops.split(",")
    if "encrypt" in names:
        for B in a.encrypt.split(","):
            enc_bench(eng, rnd, L, n, int(B), a.prod_reps, a.rounds, st)
        names = [x for x in names if x != "encrypt"]
    if "prodseq" in names or "prodsum" in names:
        # both legs always run: their words are compared first, and the rounds interleave them
        for shape in a.prodsum.split(","):
            prod_bench(eng, rnd, keys[0], L, n, shape, a.prod_reps, a.rounds, st)
        names = [x for x in names if x not in ("prodseq", "prodsum")]
    for name in names:
        f = ops[name]
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(st)
        for _ in range(a.reps):
            f()
        t1.record(st)
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1000 / a.reps
        label = name + a.bsgs if name == "bsgs" else name + a.rotsum if name in ("rotadd", "rotsum") else name
        print(json.dumps({"op": label, "limbs": L, "us": round(us, 2),
                          "hoist": int(eng.hoist()[0]), "lib": os.environ.get("MHE_LIB_PATH", "libmhe.so")}),
              flush=True)


if __name__ == "__main__":
    main()
