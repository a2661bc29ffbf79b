"""GPU parity at the ring degrees and launch sizes between the suite's N = 2^12 and N = 2^16 cases.

The kernels are templates and the dispatch (csrc/ntt.h launch_col / launch_row / modup_col /
icol_lift / col_lift2 / ks_row_mac_chunk) picks the instantiation by ring degree:

    log_n   column LOGR      row LOGR
    13      7                6
    14      7                7
    15      8 (logC = 7)     7

so N = 2^13 .. 2^15 run the 7-bit row and column kernels and the 8-bit column kernels at logC = 7,
none of which N = 2^12 (LOGR 6) or N = 2^16 (LOGR 8) reach.  Part A runs every operation at these
sizes in three arithmetic modes, part B the forward row passes of more than row_pre_max_wg
workgroups (the grouped epilogue loads of k_fwd_row<..., PRE_ON = false>).  Every comparison is
np.array_equal against the CPU oracle on seeded uniform residues; the encoder's decode compares
double for double."""
import os
import re

import numpy as np
import pytest

import mhe
import oracle as O
from test_gpu_batch import truncated
from test_gpu_parity import C2_BITS, GPT2_BITS, MIXED_BITS, SMALL_BITS, Chain

pytestmark = pytest.mark.gpu

LOG_NS = [13, 14, 15]
# fp64: every prime below 2^51 (NttMode fp = 1 everywhere, hoisting available); integer: the same
# chain with the Harvey / Shoup kernels; mixed: data primes below 2^51 and a 60-bit special prime
# (key switch fp = 2, every row / column pass outside it integer)
MODES = {"fp64": (SMALL_BITS, {}), "integer": (SMALL_BITS, {"MHE_FP": "0"}), "mixed": (MIXED_BITS, {})}
BATCH_MODES = ["fp64", "mixed"]


def make_chain(log_n, bits, env, seed):
    """A Chain whose engine is created under `env` (read at mhe_ctx_create only)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Chain(log_n, bits, seed=seed)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def chains():
    """One chain per (log_n, mode) with one random key, made on first use and shared."""
    made = {}

    def get(log_n, mode):
        if (log_n, mode) not in made:
            bits, env = MODES[mode]
            ch = make_chain(log_n, bits, env, 100 * log_n + list(MODES).index(mode))
            ch.key = ch.rand_key()
            ch.dkey = ch.up(ch.key)
            ch.key.setflags(write=False)
            made[(log_n, mode)] = ch
        return made[(log_n, mode)]

    return get


def row_logr(log_n):
    return log_n // 2


both = pytest.mark.parametrize("mode", list(MODES))
sizes = pytest.mark.parametrize("log_n", LOG_NS)
batch_modes = pytest.mark.parametrize("mode", BATCH_MODES)


# =============================================================================== A. ring degrees
@sizes
@both
def test_ntt(chains, log_n, mode):
    """k_fwd_col / k_fwd_row / k_inv_row / k_inv_col with the plain NTT jobs over all K limbs (the
    60-bit special prime of the mixed chain included) and 2 polys; lazy outputs stay below 4q
    (forward) and 2q (inverse)."""
    ch = chains(log_n, mode)
    q = np.array(ch.moduli, np.uint64)[None, :, None]
    x = ch.rand(2, ch.K, ch.n)
    for lazy in (False, True):
        got = ch.down(ch.eng.ntt_forward(ch.up(x), lazy=lazy))
        if lazy:
            assert (got < 4 * q).all()
            got = got % q
        assert np.array_equal(got, ch.oc.ntt(x, O.NTT_FWD)), ("forward", lazy)
        got = ch.down(ch.eng.ntt_inverse(ch.up(x), lazy=lazy))
        if lazy:
            assert (got < 2 * q).all()
            got = got % q
        assert np.array_equal(got, ch.oc.ntt(x, O.NTT_INV)), ("inverse", lazy)


@sizes
@both
def test_switch_key(chains, log_n, mode):
    """k_modup_col, k_ks_row_mac (fp64 / integer / MIX) and the ModDown (k_icol_lift or k_col_lift2,
    k_fwd_row<JobModDownRow>) at L = 1, 2 and K - 1 with the full key, a level-truncated key slice
    at a middle level, and relinearize."""
    ch = chains(log_n, mode)
    for L in (1, 2, ch.K - 1):
        ct, target = ch.rand(2, L, ch.n), ch.rand(L, ch.n)
        got = ch.down(ch.eng.switch_key(ch.up(ct), ch.up(target), ch.dkey))
        assert np.array_equal(got, ch.oc.switch_key(ct, target, ch.key)), L
    L = ch.K // 2
    ct, target = ch.rand(2, L, ch.n), ch.rand(L, ch.n)
    got = ch.down(ch.eng.switch_key(ch.up(ct), ch.up(target), ch.up(truncated(ch.key, L))))
    assert np.array_equal(got, ch.oc.switch_key(ct, target, ch.key)), "truncated"
    ct3 = ch.rand(3, ch.K - 1, ch.n)
    t = ch.up(ct3)
    ch.eng.relinearize(t, ch.dkey)
    assert np.array_equal(ch.down(t)[:2], ch.oc.relinearize(ct3, ch.key))


@sizes
@both
def test_hmult(chains, log_n, mode):
    """The fused ModDown + rescale tail (k_fwd_row<JobMDRRow>): L = 2 is its smallest level (one
    output limb), L = K - 1 the full chain."""
    ch = chains(log_n, mode)
    for L in (2, ch.K - 1):
        a, b = ch.rand(2, L, ch.n), ch.rand(2, L, ch.n)
        got = ch.down(ch.eng.hmult(ch.up(a), ch.up(b), ch.dkey))
        assert np.array_equal(got, ch.oc.hmult(a, b, ch.key)), L


@sizes
@both
def test_galois(chains, log_n, mode):
    """Rotation by 3 and conjugation, out of place (source untouched) and in place, and the NTT-domain
    permutation on its own."""
    ch = chains(log_n, mode)
    L = ch.K - 1
    for step in (3, 0):
        elt = mhe.galois_elt_from_step(log_n, step)
        assert elt == O.galois_elt_from_step(ch.n, step)
        ct = ch.rand(2, L, ch.n)
        want = ch.oc.apply_galois(ct, elt, ch.key)
        src = ch.up(ct)
        assert np.array_equal(ch.down(ch.eng.apply_galois_to(src, elt, ch.dkey)), want), step
        assert np.array_equal(ch.down(src), ct), step
        assert np.array_equal(ch.down(ch.eng.apply_galois(src, elt, ch.dkey)), want), step
    a = ch.rand(2, 3, ch.n)
    for elt in (3, 5, 2 * ch.n - 1):
        got = ch.down(ch.eng.permute_galois(ch.up(a), elt))
        assert np.array_equal(got, O.apply_galois_ntt(a.reshape(-1, ch.n), log_n, elt).reshape(a.shape)), elt


@sizes
@both
def test_rescale(chains, log_n, mode):
    """k_inv_row<JobLastInv>, k_icol_lift<JobRescaleCol>, k_fwd_row<JobRescaleRow> for 1, 2 and 3
    polys at L = 2 and K - 1, and one rescale at L = K, which drops the special prime (the
    Encryptor's path; 60-bit in the mixed chain)."""
    ch = chains(log_n, mode)
    for L in (2, ch.K - 1):
        for size in (1, 2, 3):
            ct = ch.rand(size, L, ch.n)
            assert np.array_equal(ch.down(ch.eng.rescale_to_next(ch.up(ct))), ch.oc.rescale(ct)), (L, size)
    ct = ch.rand(2, ch.K, ch.n)
    assert np.array_equal(ch.down(ch.eng.rescale_to_next(ch.up(ct))), ch.oc.rescale(ct)), "L = K"


@sizes
@both
def test_elementwise(chains, log_n, mode):
    ch = chains(log_n, mode)
    oc, L = ch.oc, ch.K - 1
    a, b, pt = ch.rand(2, L, ch.n), ch.rand(2, L, ch.n), ch.rand(L, ch.n)
    da, db = ch.up(a), ch.up(b)
    assert np.array_equal(ch.down(ch.eng.add(da, db)), oc.add(a, b))
    assert np.array_equal(ch.down(ch.eng.sub(da, db)), oc.sub(a, b))
    assert np.array_equal(ch.down(ch.eng.negate(da)), oc.negate(a))
    assert np.array_equal(ch.down(ch.eng.multiply_plain(da, ch.up(pt))), oc.multiply_plain(a, pt))
    assert np.array_equal(ch.down(ch.eng.multiply(da, db)), oc.multiply(a, b))
    assert np.array_equal(ch.down(ch.eng.square(da)), oc.square(a))
    # per-limb scalars: a * s is the plaintext product with a constant plaintext; a + s in integers
    s = [int(ch.rng.integers(0, q)) for q in ch.moduli[:L]]
    const = np.broadcast_to(np.array(s, np.uint64)[:, None], (L, ch.n))
    assert np.array_equal(ch.down(ch.eng.multiply_scalar(da, s)), oc.multiply_plain(a, const))
    assert np.array_equal(ch.down(ch.eng.add_scalar(da, s)), oc.add(a, np.broadcast_to(const, a.shape)))
    x = ch.rand(2, 1, ch.n)
    q0 = ch.moduli[0]
    x[0, 0, :4] = [0, q0 >> 1, (q0 >> 1) + 1, q0 - 1]
    assert np.array_equal(ch.down(ch.eng.modraise(ch.up(x), ch.K)), oc.modraise(x, ch.K))


@sizes
@both
def test_extreme_residues(chains, log_n, mode):
    """Every residue of the ciphertexts, the target and the key equal to q - 1: the bound of the
    exact-FP64 butterflies, key MAC, lifts and epilogues in these instantiations."""
    ch = chains(log_n, mode)
    L, K, n = ch.K - 1, ch.K, ch.n
    qm1 = np.array(ch.moduli, np.uint64) - np.uint64(1)
    a = np.broadcast_to(qm1[None, :L, None], (2, L, n)).copy()
    tgt = np.broadcast_to(qm1[:L, None], (L, n)).copy()
    key = np.broadcast_to(qm1[None, None, :, None], (L, 2, K, n)).copy()
    dkey = ch.up(key)
    assert np.array_equal(ch.down(ch.eng.hmult(ch.up(a), ch.up(a), dkey)), ch.oc.hmult(a, a, key))
    assert np.array_equal(ch.down(ch.eng.switch_key(ch.up(a), ch.up(tgt), dkey)), ch.oc.switch_key(a, tgt, key))
    assert np.array_equal(ch.down(ch.eng.rescale_to_next(ch.up(a))), ch.oc.rescale(a))


# ------------------------------------------------------------------------------ batched paths
@sizes
@batch_modes
def test_hmult_batch(chains, log_n, mode):
    """9 HMults sharing the key: launches of 8 + 1 entries, the first on k_ks_row_mac's shared-key
    path (checked below: 4 output primes at L = 3); every 4th entry a square.  The low level keeps
    the oracle's nine HMults short; test_hmult has the full level."""
    ch = chains(log_n, mode)
    L = 3
    assert ks_share_taken(log_n, L)
    a = [ch.rand(2, L, ch.n) for _ in range(9)]
    b = [ch.rand(2, L, ch.n) for _ in range(9)]
    da = [ch.up(x) for x in a]
    db = [da[i] if i % 4 == 3 else ch.up(b[i]) for i in range(9)]
    outs = ch.eng.hmult_batch(da, db, ch.dkey)
    for i in range(9):
        want = ch.oc.hmult(a[i], a[i] if i % 4 == 3 else b[i], ch.key)
        assert np.array_equal(ch.down(outs[i]), want), i


def ks_share_taken(log_n, L):
    """k_ks_row_mac groups the entries of a shared key by XCD when grid.x * grid.y % 8 == 0, with
    grid.x = 2^(log_n - LOGR) / S blocks groups (S = 32, 16, 8 for LOGR 6, 7, 8) and grid.y = L + 1
    output primes (ntt.h ks_row_mac_a)."""
    logr = row_logr(log_n)
    gx = (1 << (log_n - logr)) // {6: 32, 7: 16, 8: 8}[logr]
    return gx * (L + 1) % 8 == 0


@sizes
@batch_modes
def test_switch_key_batch_shared_key(chains, log_n, mode):
    """4 key switches of one key at two levels.  At log_n = 13 grid.x is 4: L = 3 (4 output primes)
    takes the XCD-grouped `share` branch and L = 4 (5 output primes) does not.  At log_n = 14 and 15
    grid.x is 8 and 16, so every level takes the `share` branch."""
    ch = chains(log_n, mode)
    assert ks_share_taken(log_n, 3)
    assert ks_share_taken(log_n, 4) == (log_n != 13)
    for L in (3, 4):
        cts = [ch.rand(2, L, ch.n) for _ in range(4)]
        tgs = [ch.rand(L, ch.n) for _ in range(4)]
        dct = [ch.up(c) for c in cts]
        ch.eng.switch_key_batch(dct, [ch.up(t) for t in tgs], [ch.dkey] * 4)
        for i in range(4):
            assert np.array_equal(ch.down(dct[i]), ch.oc.switch_key(cts[i], tgs[i], ch.key)), (L, i)


ROT_STEPS = [1, -1, 3, 100, 0, 7, -5, 64, 2]
ROT_L = 4  # the batched rotations run at a middle level: nine oracle rotations per test stay short


def rot_keys(ch):
    """Entry i rotates by key i % 2: the chain's key in full, and its level-truncated slice."""
    return [ch.dkey, ch.up(truncated(ch.key, ROT_L))]


@sizes
@batch_modes
def test_rotate_batch_one_input(chains, log_n, mode):
    """One input rotated by 9 steps (8 + 1): hoisted in fp64 mode (mhe_hoist_stats must count the
    rotations), by the classic path with hoisting off and in mixed mode, where the 60-bit special
    prime rules hoisting out (hoist_ok)."""
    ch = chains(log_n, mode)
    eng, L = ch.eng, ROT_L
    elts = [mhe.galois_elt_from_step(log_n, s) for s in ROT_STEPS]
    dkeys = rot_keys(ch)
    ct = ch.rand(2, L, ch.n)
    want = [ch.oc.apply_galois(ct, e, ch.key) for e in elts]
    src = ch.up(ct)
    saved = eng.hoist()
    try:
        eng.set_hoist(True, check=False)
        assert eng.hoist()[0] == (mode == "fp64")
        eng.hoist_stats(reset=True)
        outs = eng.apply_galois_batch([src] * 9, elts, [dkeys[i % 2] for i in range(9)])
        eng.synchronize()
        rot, mac, _ = eng.hoist_stats(reset=True)
        if mode == "fp64":
            assert rot == 9 and mac >= 1, (rot, mac)
        else:
            assert rot == 0 and mac == 0, (rot, mac)
        for i in range(9):
            assert np.array_equal(ch.down(outs[i]), want[i]), f"step {ROT_STEPS[i]}"
        eng.set_hoist(False)
        outs = eng.apply_galois_batch([src] * 9, elts, [dkeys[i % 2] for i in range(9)])
        eng.synchronize()
        assert eng.hoist_stats(reset=True)[:2] == (0, 0)
        for i in range(9):
            assert np.array_equal(ch.down(outs[i]), want[i]), f"step {ROT_STEPS[i]}, hoisting off"
    finally:
        eng.set_hoist(*saved)
    assert np.array_equal(ch.down(src), ct)


@sizes
@batch_modes
def test_rotate_batch_many_inputs(chains, log_n, mode):
    """9 distinct inputs in one call: launches of 8 + 1 entries on the classic path."""
    ch = chains(log_n, mode)
    L = ROT_L
    elts = [mhe.galois_elt_from_step(log_n, s) for s in ROT_STEPS]
    dkeys = rot_keys(ch)
    cts = [ch.rand(2, L, ch.n) for _ in range(9)]
    outs = ch.eng.apply_galois_batch([ch.up(c) for c in cts], elts, [dkeys[i % 2] for i in range(9)])
    for i in range(9):
        assert np.array_equal(ch.down(outs[i]), ch.oc.apply_galois(cts[i], elts[i], ch.key)), f"input {i}"


@sizes
@batch_modes
def test_rotate_sum(chains, log_n, mode):
    """mhe_rotate_sum over groups of 3, 1 and 5 entries, stored and accumulated."""
    ch = chains(log_n, mode)
    L = ROT_L
    groups = [0] * 3 + [1] + [2] * 5
    steps = [1, -1, 3, 100, 7, -5, 64, 2, 9]
    elts = [mhe.galois_elt_from_step(log_n, s) for s in steps]
    cts = [ch.rand(2, L, ch.n) for _ in steps]
    dcts = [ch.up(c) for c in cts]
    rot = [ch.oc.apply_galois(c, e, ch.key) for c, e in zip(cts, elts)]
    want = []
    for g in range(3):
        acc = None
        for i, r in enumerate(rot):
            if groups[i] == g:
                acc = r if acc is None else ch.oc.add(acc, r)
        want.append(acc)
    outs = ch.eng.rotate_sum(dcts, elts, [ch.dkey] * 9, groups=groups)
    for g in range(3):
        assert np.array_equal(ch.down(outs[g]), want[g]), g
    prior = [ch.rand(2, L, ch.n) for _ in range(3)]
    outs = ch.eng.rotate_sum(dcts, elts, [ch.dkey] * 9, groups=groups, outs=[ch.up(p) for p in prior], accumulate=True)
    for g in range(3):
        assert np.array_equal(ch.down(outs[g]), ch.oc.add(prior[g], want[g])), (g, "accumulate")
    for d, c in zip(dcts, cts):
        assert np.array_equal(ch.down(d), c)


def icol_primes_per_wg(polys, cnt):
    """Output primes per workgroup of k_icol_lift (ntt.h icol_lift_a): 1, 2 or MHE_ICOL_G = 5."""
    jobs = polys * cnt
    return 5 if jobs >= 128 else 2 if jobs >= 56 else 1


@sizes
@batch_modes
def test_rescale_batch(chains, log_n, mode):
    """icol_lift_a shares the inverse column stages over 1, 2 or MHE_ICOL_G output primes, split at
    polys * cnt = 56 and 128 (cnt = L - 1 output primes).  7+1-limb chain at L = 7: 5 entries of 2
    polys give 60 (2 primes per workgroup), 8 entries of 3 polys 144 (MHE_ICOL_G).  The 5+1-limb
    mixed chain cannot reach 128 with the 8 entries of one launch; at L = K = 6 the same two
    batches give 50 (1 prime) and 120 (2 primes), the two sides of its reachable split."""
    ch = chains(log_n, mode)
    L, per = (7, (2, 5)) if mode == "fp64" else (6, (1, 2))
    for (count, size), p in zip(((5, 2), (8, 3)), per):
        assert icol_primes_per_wg(count * size, L - 1) == p
        cts = [ch.rand(size, L, ch.n) for _ in range(count)]
        outs = ch.eng.rescale_batch([ch.up(c) for c in cts])
        for i, (c, o) in enumerate(zip(cts, outs)):
            assert np.array_equal(ch.down(o), ch.oc.rescale(c)), (count, size, i)


@sizes
@pytest.mark.parametrize("fmt", [1, 2], ids=["doubles", "pack48"])
def test_prepared_key(chains, log_n, fmt):
    """Both prepared key formats in the 7-bit key MAC: switch_key at two levels and HMult stay
    bit-identical, and unprepare restores the key word for word."""
    ch = chains(log_n, "fp64")
    dkey = ch.up(ch.key.copy())
    ch.eng.key_prepare(dkey, fmt)
    assert ch.eng.key_format(dkey) == fmt
    for L in (2, ch.K - 1):
        ct, target = ch.rand(2, L, ch.n), ch.rand(L, ch.n)
        got = ch.down(ch.eng.switch_key(ch.up(ct), ch.up(target), dkey))
        assert np.array_equal(got, ch.oc.switch_key(ct, target, ch.key)), L
    L = ch.K - 1
    a, b = ch.rand(2, L, ch.n), ch.rand(2, L, ch.n)
    assert np.array_equal(ch.down(ch.eng.hmult(ch.up(a), ch.up(b), dkey)), ch.oc.hmult(a, b, ch.key))
    ch.eng.key_unprepare(dkey)
    assert np.array_equal(ch.down(dkey), ch.key)


# ------------------------------------------------------------------------------ engine variants
RING_VARIANTS = [
    {"MHE_KS_FUSED": "0"},                              # k_fwd_row<JobModUpRow> + k_ks_mac
    {"MHE_KS_COLGROUPS": "0"},                          # k_fwd_col<JobModUpCol>, one job per (I, J)
    {"MHE_KS_COLGROUPS": "3", "MHE_KS_SHARE": "0"},     # three output-prime groups
    {"MHE_ICOL_FUSED": "0", "MHE_GALOIS_FUSED": "0"},   # separate inverse column pass, SEAL's galois order
    {"MHE_HMULT_FUSED": "0"},                           # HMult: separate ModDown and rescale
]


@pytest.mark.parametrize("log_n", [14, 15])
@pytest.mark.parametrize("variant", range(len(RING_VARIANTS)))
def test_engine_variants(log_n, variant):
    """Each fusion switched off on the fp64 chain at log_n = 14 (LOGR 7 as row and as column) and
    15 (LOGR 8 columns at logC = 7)."""
    env = RING_VARIANTS[variant]
    ch = make_chain(log_n, SMALL_BITS, env, 300 + 10 * log_n + variant)
    key = ch.rand_key()
    dkey = ch.up(key)
    for L in (1, ch.K - 1):
        ct, target = ch.rand(2, L, ch.n), ch.rand(L, ch.n)
        got = ch.down(ch.eng.switch_key(ch.up(ct), ch.up(target), dkey))
        assert np.array_equal(got, ch.oc.switch_key(ct, target, key)), (env, L)
    L = ch.K - 1
    a, b = ch.rand(2, L, ch.n), ch.rand(2, L, ch.n)
    assert np.array_equal(ch.down(ch.eng.hmult(ch.up(a), ch.up(b), dkey)), ch.oc.hmult(a, b, key)), env
    assert np.array_equal(ch.down(ch.eng.rescale_to_next(ch.up(a))), ch.oc.rescale(a)), env
    elt = mhe.galois_elt_from_step(log_n, 3)
    assert np.array_equal(ch.down(ch.eng.apply_galois_to(ch.up(a), elt, dkey)), ch.oc.apply_galois(a, elt, key)), env


# ------------------------------------------------------------------------------------- encoder
@sizes
def test_encode(chains, log_n):
    """k_enc_fft_tail<log_n - 12>: a real, a complex and a partial vector at scale 2^46, and the
    128-bit coefficient path at 2^70, word for word."""
    ch = chains(log_n, "fp64")
    rng = np.random.default_rng(40 + log_n)
    L, half = ch.K - 1, ch.n // 2
    real = rng.uniform(-1, 1, half)
    for name, v, scale in (("real", real, 2.0 ** 46),
                           ("complex", rng.uniform(-1, 1, half) + 1j * rng.uniform(-1, 1, half), 2.0 ** 46),
                           ("partial", rng.uniform(-4, 4, 37), 2.0 ** 46),
                           ("wide", real, 2.0 ** 70)):
        assert np.array_equal(ch.down(ch.eng.encode(v, scale, L)), ch.oc.encode(v, scale, L)), name


@sizes
def test_decode(chains, log_n):
    """Decode of an oracle-encoded complex vector, and of an arbitrary plaintext at 1, 16 and n / 2
    sparse slots, double for double."""
    ch = chains(log_n, "fp64")
    rng = np.random.default_rng(50 + log_n)
    z = rng.uniform(-1, 1, ch.n // 2) + 1j * rng.uniform(-1, 1, ch.n // 2)
    pt = ch.oc.encode(z, 2.0 ** 46, 3)
    got = ch.eng.decode(ch.up(pt), 2.0 ** 46)
    assert np.array_equal(got, ch.oc.decode(pt, 2.0 ** 46))
    assert np.abs(got - z).max() < 1e-5
    pt = ch.rand(3, ch.n)
    for sparse in (1, 16, ch.n // 2):
        got = ch.eng.decode(ch.up(pt), 2.0 ** 40, sparse_slots=sparse)
        assert np.array_equal(got, ch.oc.decode(pt, 2.0 ** 40, sparse_slots=sparse)), sparse


# =============================================================================== B. large launches
def row_pre_max_wg():
    """The threshold above which launch_pass_a starts k_fwd_row without the epilogue prefetch."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fhe-gpt-2_amd", "csrc", "ntt.h")
    with open(path) as f:
        m = re.search(r"row_pre_max_wg\s*=\s*(\d+)", f.read())
    assert m, "csrc/ntt.h no longer defines row_pre_max_wg: these tests do not know what they cover"
    return int(m.group(1))


def row_workgroups(jobs, log_n):
    """Workgroups of a forward row pass of `jobs` (poly, limb) jobs: launch_pass_a's grid,
    2^(log_n - LOGR) / S sub-transform groups per job, S = 32 for LOGR <= 7 and 16 for LOGR 8."""
    logr = row_logr(log_n)
    return jobs * ((1 << (log_n - logr)) // (32 if logr <= 7 else 16))


@pytest.mark.slow
def test_large_rescale_fp64_n15():
    """k_fwd_row<7, 3, JobRescaleRow, FP, PRE_ON = false>: 8 ciphertexts of 3 polys on the C2 chain
    at N = 2^15, L = 45 (the special prime dropped): 8 * 3 * 44 jobs * 8 = 8448 workgroups."""
    log_n, count, size = 15, 8, 3
    ch = Chain(log_n, C2_BITS, seed=215)
    L = ch.K
    wg = row_workgroups(count * size * (L - 1), log_n)
    print("workgroups", wg)
    assert wg > row_pre_max_wg(), wg
    assert all(q < (1 << 51) for q in ch.moduli)  # FP64 row passes (k_fwd_row3 is N = 2^16 only)
    cts = [ch.rand(size, L, ch.n) for _ in range(count)]
    outs = ch.eng.rescale_batch([ch.up(c) for c in cts])
    for i, (c, o) in enumerate(zip(cts, outs)):
        assert np.array_equal(ch.down(o), ch.oc.rescale(c)), i


@pytest.fixture(scope="module")
def gpt2():
    """The GPT-2 chain at N = 2^16 (60-bit special prime: integer row passes outside the key
    switch) with a 34-digit key, shared by the large-launch cases."""
    ch = Chain(16, GPT2_BITS, seed=216)
    ch.L = 34
    ch.key = ch.rand_key(digits=ch.L)
    ch.dkey = ch.up(ch.key)
    return ch


@pytest.mark.slow
def test_large_rescale_integer_n16(gpt2):
    """k_fwd_row<8, 4, JobRescaleRow, integer, PRE_ON = false>: 8 ciphertexts of 3 polys at L = 24:
    8 * 3 * 23 jobs * 16 = 8832 workgroups."""
    ch, count, size, L = gpt2, 8, 3, 24
    wg = row_workgroups(count * size * (L - 1), ch.log_n)
    print("workgroups", wg)
    assert wg > row_pre_max_wg(), wg
    cts = [ch.rand(size, L, ch.n) for _ in range(count)]
    outs = ch.eng.rescale_batch([ch.up(c) for c in cts])
    for i, (c, o) in enumerate(zip(cts, outs)):
        assert np.array_equal(ch.down(o), ch.oc.rescale(c)), i


@pytest.mark.slow
def test_large_moddown_integer_n16(gpt2):
    """k_fwd_row<8, 4, JobModDownRow, integer, PRE_ON = false>: 8 key switches, then 8 rotations,
    sharing the key at L = 34: 2 * 34 * 8 jobs * 16 = 8704 workgroups.  Two distinct inputs: entry
    e works on its own device copy of input e % 2."""
    ch, count = gpt2, 8
    L = ch.L
    wg = row_workgroups(2 * L * count, ch.log_n)
    print("workgroups", wg)
    assert wg > row_pre_max_wg(), wg
    cts = [ch.rand(2, L, ch.n) for _ in range(2)]
    tgs = [ch.rand(L, ch.n) for _ in range(2)]
    want = [ch.oc.switch_key(c, t, ch.key) for c, t in zip(cts, tgs)]
    dct = [ch.up(cts[e % 2]) for e in range(count)]
    ch.eng.switch_key_batch(dct, [ch.up(tgs[e % 2]) for e in range(count)], [ch.dkey] * count)
    for e in range(count):
        assert np.array_equal(ch.down(dct[e]), want[e % 2]), ("switch_key", e)
    elt = mhe.galois_elt_from_step(ch.log_n, 5)
    want = [ch.oc.apply_galois(c, elt, ch.key) for c in cts]
    outs = ch.eng.apply_galois_batch([ch.up(cts[e % 2]) for e in range(count)], [elt] * count, [ch.dkey] * count)
    for e in range(count):
        assert np.array_equal(ch.down(outs[e]), want[e % 2]), ("rotation", e)


@pytest.mark.slow
def test_large_hmult_tail_integer_n16(gpt2):
    """k_fwd_row<8, 4, JobMDRRow, integer, PRE_ON = false>: 8 HMults at L = 34, whose fused ModDown +
    rescale tail has 2 * 33 * 8 jobs * 16 = 8448 workgroups.  Two distinct input pairs, as above."""
    ch, count = gpt2, 8
    L = ch.L
    wg = row_workgroups(2 * (L - 1) * count, ch.log_n)
    print("workgroups", wg)
    assert wg > row_pre_max_wg(), wg
    a = [ch.rand(2, L, ch.n) for _ in range(2)]
    b = [ch.rand(2, L, ch.n) for _ in range(2)]
    want = [ch.oc.hmult(x, y, ch.key) for x, y in zip(a, b)]
    outs = ch.eng.hmult_batch([ch.up(a[e % 2]) for e in range(count)], [ch.up(b[e % 2]) for e in range(count)], ch.dkey)
    for e in range(count):
        assert np.array_equal(ch.down(outs[e]), want[e % 2]), e
