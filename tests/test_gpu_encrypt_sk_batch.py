"""GPU parity of mhe_encrypt_sk_batch (csrc/keygen.h): symmetric encryption of a batch -- the digits
of a key-switching key, a public key, a ciphertext-level encryption of zero.  Every case is compared
word for word with the oracle's encrypt_zero_symmetric(seed, sk, sample_limbs) restricted to the kept
limbs, the gadget term (q_{K-1} mod q_j) new_key_j added with Python integers.  The chains of primes
just above 1.5 * 2^60 (keygen_ref.chain) run the uniform sampler's redraw path; their redrawn-word
totals are recomputed from the PRNG's bytes and asserted against mhe_keygen_stats."""
import ctypes
import os

import numpy as np
import pytest

import mhe
import oracle as O
from keygen_ref import FP_BITS, MIXED_BITS, chain, public_seed, redraw_counts, seed_of

pytestmark = pytest.mark.gpu

SEED = [11, 22, 33, 44, 55, 66, 77, 88]
MHE_ERR_ARG = -1
OPK_MULPLAIN, OPK_ADDSUB, OPK_SCALAR, OPK_NTT = 3, 4, 5, 6


class Setup:
    """One chain: oracle context, engine (created under `env`), a secret key, a new key, cached references."""

    def __init__(self, log_n, moduli, env=None):
        self.log_n, self.n, self.moduli, self.K = log_n, 1 << log_n, moduli, len(moduli)
        self.oc = O.Context(log_n, moduli)
        env = env or {}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            self.eng = mhe.Engine(log_n, moduli)  # MHE_FP is read at mhe_ctx_create only
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        self.sk = self.oc.keygen_secret(SEED, 32)
        rng = np.random.default_rng(log_n)
        self.nk = np.stack([rng.integers(0, q, size=self.n, dtype=np.uint64) for q in moduli])
        self.dsk, self.dnk = self.eng.to_device(self.sk), self.eng.to_device(self.nk)
        self.refs = {}

    def ref(self, seed, sample_limbs, sk=None):
        if sk is not None:
            return self.oc.encrypt_zero_symmetric(seed, sk, sample_limbs)
        key = (tuple(seed), sample_limbs)
        if key not in self.refs:
            r = self.oc.encrypt_zero_symmetric(seed, self.sk, sample_limbs)
            r.setflags(write=False)
            self.refs[key] = r
        return self.refs[key]

    def want(self, seed, sample_limbs, keep, keep_last, nk=None, digit=None, sk=None):
        idx = list(range(keep)) + ([sample_limbs - 1] if keep_last else [])
        w = np.array(self.ref(seed, sample_limbs, sk)[:, idx])
        if nk is not None:
            q = int(self.moduli[digit])
            f = int(self.moduli[-1]) % q
            w[0, digit] = ((w[0, digit].astype(object) + f * nk[digit].astype(object)) % q).astype(np.uint64)
        return w

    def check(self, seeds, sample_limbs, keep, keep_last, digits=None):
        """digits[i] None: no new key for entry i."""
        digits = [None] * len(seeds) if digits is None else digits
        nks = None if all(d is None for d in digits) else [None if d is None else self.dnk for d in digits]
        dg = None if nks is None else [0 if d is None else d for d in digits]
        outs = self.eng.encrypt_sk_batch(seeds, self.dsk, sample_limbs, keep, keep_last, nks, dg)
        self.eng.synchronize()
        for i, (seed, d) in enumerate(zip(seeds, digits)):
            want = self.want(seed, sample_limbs, keep, keep_last, None if d is None else self.nk, d)
            got = mhe.Engine.to_host(outs[i])
            assert np.array_equal(got, want), (
                f"entry {i} of {len(seeds)} (sample_limbs {sample_limbs}, keep {keep}+{keep_last}, digit {d}): "
                f"{(got != want).sum()} words differ")


CHAINS = {"fp64": (FP_BITS, None), "mixed": (MIXED_BITS, None), "integer": (FP_BITS, {"MHE_FP": "0"})}


@pytest.fixture(scope="module")
def setups():
    made = {}

    def get(log_n, which):
        if (log_n, which) not in made:
            if which in CHAINS:
                bits, env = CHAINS[which]
                made[(log_n, which)] = Setup(log_n, O.coeff_modulus_create(1 << log_n, bits), env)
            else:
                made[(log_n, which)] = Setup(log_n, chain(which, log_n))
        return made[(log_n, which)]

    yield get
    for s in made.values():
        s.eng.close()


@pytest.fixture(scope="module")
def fp(setups):
    return setups(12, "fp64")


@pytest.mark.parametrize("which", ["fp64", "mixed", "integer", "H4", "MIX"])
def test_key_digits(setups, which):
    """Digits 0, middle and last of a full key, and an entry without a new key among them.  H4 and MIX
    redraw hundreds of words per entry; the total is the count recomputed from a's stream."""
    s = setups(12, which)
    seeds = [seed_of(i) for i in range(4)]
    s.eng.keygen_stats(reset=True)
    s.check(seeds, s.K, s.K - 1, 1, [0, 1, None, s.K - 2])
    redrawn = sum(sum(redraw_counts(public_seed(sd), s.moduli, s.n)[0]) for sd in seeds)
    assert s.eng.keygen_stats() == (4, 1, redrawn, 0)
    assert (redrawn > 400) == (which in ("H4", "MIX"))


@pytest.mark.parametrize("which", ["fp64", "H4"])
@pytest.mark.parametrize("keep", [1, 2, 3])
def test_truncated_keys(setups, which, keep):
    """keep = digits of a level-truncated key with the special limb behind them: the dropped limbs
    are drawn (their rejects consume tail words on H4) and not written."""
    s = setups(12, which)
    s.check([seed_of(i) for i in range(keep)], s.K, keep, 1, list(range(keep)))


@pytest.mark.parametrize("which", ["fp64", "integer"])
def test_ciphertext_level(setups, which):
    """keep_last = 0: the encryption of zero at 3 limbs and at 1 limb, and the first two of three."""
    s = setups(12, which)
    seeds = [seed_of(0), seed_of(1)]
    s.check(seeds, 3, 3, 0)
    s.check(seeds, 1, 1, 0)
    s.check(seeds, 3, 2, 0)
    s.check(seeds, s.K, s.K, 0)  # every limb kept by `keep` alone: the public key's form


@pytest.mark.parametrize("count", [1, 3, 8, 9, 17])
def test_entry_counts(fp, count):
    fp.eng.keygen_stats(reset=True)
    fp.check([seed_of(i) for i in range(count)], fp.K, fp.K - 1, 1, [i % (fp.K - 1) for i in range(count)])
    assert fp.eng.keygen_stats() == (count, (count + 7) // 8, 0, 0)


@pytest.mark.parametrize("mode", ["fp64", "integer"])
@pytest.mark.parametrize("log_n", [13, 14, 15, 16])
def test_ring_degrees(setups, log_n, mode):
    s = setups(log_n, mode)
    s.check([seed_of(0), seed_of(1)], 3, 3, 0)
    s.check([seed_of(0)], s.K, 2, 1, [1])


@pytest.mark.parametrize("which", ["fp64", "mixed", "integer"])
def test_extreme_residues(setups, which):
    """sk and new_key all q - 1 and all 0: the lazy ranges of the epilogue."""
    s = setups(12, which)
    q = np.array(s.moduli, np.uint64)
    top = np.broadcast_to((q - 1)[:, None], (s.K, s.n)).copy()
    seeds = [seed_of(0), seed_of(1)]
    for val in (top, np.zeros_like(top)):
        d = s.eng.to_device(val)
        outs = s.eng.encrypt_sk_batch(seeds, d, s.K, s.K - 1, 1, [d, d], [0, s.K - 2])
        s.eng.synchronize()
        for i, (seed, dg) in enumerate(zip(seeds, [0, s.K - 2])):
            assert np.array_equal(mhe.Engine.to_host(outs[i]), s.want(seed, s.K, s.K - 1, 1, val, dg, sk=val))


def test_whole_key(fp):
    """count = K - 1, one seed per digit: tests/ckks_helpers.kswitch_key's construction digit by digit,
    key[J] = (c0 + [J] (P mod q_J) s', a) with (c0, a) the oracle's encryption of zero."""
    K, n, oc = fp.K, fp.n, fp.oc
    seeds = [seed_of(10 + j) for j in range(K - 1)]
    outs = fp.eng.encrypt_sk_batch(seeds, fp.dsk, K, K - 1, 1, [fp.dnk] * (K - 1), list(range(K - 1)))
    fp.eng.synchronize()
    for J in range(K - 1):
        z = fp.ref(seeds[J], K)
        fac = np.zeros((K, n), np.uint64)
        fac[J] = fp.moduli[-1] % fp.moduli[J]
        c0 = oc.add(np.array(z[0]), oc.dyadic(fac, fp.nk))
        assert np.array_equal(mhe.Engine.to_host(outs[J]), np.stack([c0, z[1]]))


def sequence(s, seed, dnk, digit):
    """Today's entry points, call by call, at the key level (seal/keys.cpp make_kswitch_key_seq)."""
    eng, K = s.eng, s.K
    a, _, rejects = eng.prng_uniform_bulk(K, public_seed(seed))
    assert rejects == 0  # SEAL's own primes: the bulk is the whole sample, no fix-up to apply
    c0, _ = eng.prng_small("cbd", K, seed, 64)
    eng.ntt_forward(c0, lazy=True)
    t = eng.multiply_plain(s.dsk, a)
    eng.add(t, c0, out=c0)
    eng.negate(c0, out=c0)
    if dnk is not None:
        f = [0] * K
        f[digit] = s.moduli[-1] % s.moduli[digit]
        eng.multiply_scalar(dnk, f, out=t)
        eng.add(c0, t, out=c0)
    return c0, a


def test_sequence_words_and_op_counts(fp):
    kinds = (OPK_MULPLAIN, OPK_ADDSUB, OPK_SCALAR, OPK_NTT)
    counts = lambda: [fp.eng.op_counts(k, reset=True) for k in kinds]
    seeds, digits = [seed_of(0), seed_of(1), seed_of(2)], [2, None, 0]
    counts()
    seq = [sequence(fp, sd, None if d is None else fp.dnk, d) for sd, d in zip(seeds, digits)]
    by_sequence = counts()
    outs = fp.eng.encrypt_sk_batch(seeds, fp.dsk, fp.K, fp.K, 0, [None if d is None else fp.dnk for d in digits],
                                   [0 if d is None else d for d in digits])
    by_batch = counts()
    assert any(any(row) for row in by_sequence) and by_batch == by_sequence
    for o, (c0, a) in zip(outs, seq):
        assert np.array_equal(mhe.Engine.to_host(o), np.stack([mhe.Engine.to_host(c0), mhe.Engine.to_host(a)]))


def test_rejected_before_launch(fp):
    eng, K, n = fp.eng, fp.K, fp.n
    seeds = [seed_of(0), seed_of(1)]
    a, b = eng.empty(2, K, n), eng.empty(2, K, n)
    skc, nkc = eng.to_device(fp.sk), eng.to_device(fp.nk)
    a.fill_(7)
    b.fill_(7)
    eng.synchronize()
    eng.keygen_stats(reset=True)

    def rejected(**kw):
        args = dict(seeds=seeds, sk=fp.dsk, sample_limbs=K, keep=K - 1, keep_last=1, new_keys=[fp.dnk, fp.dnk],
                    digits=[0, 1], outs=[a, b])
        args.update(kw)
        with pytest.raises(mhe.MheError) as ei:
            eng.encrypt_sk_batch(**args)
        assert ei.value.code == MHE_ERR_ARG

    rejected(sample_limbs=0)
    rejected(sample_limbs=K + 1)
    rejected(keep=-1)
    rejected(keep=0, keep_last=0, new_keys=None, digits=None)
    rejected(keep=K)                                                # keep > sample_limbs - keep_last
    rejected(sample_limbs=3, keep=2, keep_last=1, new_keys=None, digits=None)  # keep_last below the key level
    rejected(sample_limbs=3, keep=3, keep_last=0)                   # a new key below the key level
    rejected(digits=[0, K - 1])                                     # digit = keep
    rejected(digits=[-1, 0])
    rejected(outs=[a, a])                                           # overlapping outputs
    rejected(outs=[a, a[1:]])                                       # ... by one poly
    rejected(sk=skc, outs=[a, skc])                                 # an output on the secret key
    rejected(new_keys=[nkc, None], outs=[a, nkc])                   # an output on a new key
    sd = np.ascontiguousarray(np.array(seeds, np.uint64))
    rc = mhe.lib().mhe_encrypt_sk_batch(eng._h, 0, sd.ctypes.data_as(ctypes.c_void_p), fp.dsk.data_ptr(), K, K - 1, 1,
                                        None, None, eng._ptrs([a, b]), eng.stream())
    assert rc == MHE_ERR_ARG                                        # count = 0
    eng.synchronize()
    assert bool((a == 7).all()) and bool((b == 7).all())
    assert np.array_equal(mhe.Engine.to_host(skc), fp.sk) and np.array_equal(mhe.Engine.to_host(nkc), fp.nk)
    assert eng.keygen_stats()[:2] == (0, 0)
    # a fresh context grows its scratch before the first launch: a failed allocation leaves the output
    fresh = mhe.Engine(fp.log_n, fp.moduli)
    try:
        o = fresh.empty(2, K, n)
        o.fill_(7)
        dsk = fresh.to_device(fp.sk)
        fresh.synchronize()
        for nth in (1, 2):  # the key-switch workspace, then the sampling scratch
            assert mhe.lib().mhe_debug_fail_alloc(fresh._h, nth) == 0
            try:
                with pytest.raises(mhe.MheError, match="allocation failed"):
                    fresh.encrypt_sk_batch([seed_of(0)], dsk, K, K - 1, 1, outs=[o])
            finally:
                assert mhe.lib().mhe_debug_fail_alloc(fresh._h, 0) == 0
            fresh.synchronize()
            assert bool((o == 7).all())
        fresh.encrypt_sk_batch([seed_of(0)], dsk, K, K - 1, 1, outs=[o])
        fresh.synchronize()
        assert np.array_equal(mhe.Engine.to_host(o), fp.want(seed_of(0), K, K - 1, 1))
    finally:
        fresh.close()
