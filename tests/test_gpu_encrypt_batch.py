"""GPU parity of mhe_encrypt_pk_batch (csrc/encrypt.h): public-key encryption of a batch, the
samples kept as bytes and one forward NTT per output limb.  Every case is compared word for word
with the oracle's encrypt_zero_asymmetric(seed, pk, L + 1, L) plus the plaintext mod q."""
import ctypes
import json
import os

import numpy as np
import pytest

import mhe
import oracle as O

pytestmark = pytest.mark.gpu

SEED = [11, 22, 33, 44, 55, 66, 77, 88]
FP_BITS = [50, 40, 40, 50]      # every prime below 2^51: the FP64 passes and epilogue
MIXED_BITS = [50, 40, 40, 60]   # a 60-bit special prime: every plain pass integer
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ternary_redraw_seed.json")
MHE_ERR_ARG = -1


def seed_of(i):
    return [1000 + i, 2, 3, 4, 5, 6, 7, 8]


class Setup:
    """One chain: oracle context, engine (created under `env`), a real key pair, cached references."""

    def __init__(self, log_n, bits, env=None):
        self.log_n, self.n = log_n, 1 << log_n
        self.moduli = O.coeff_modulus_create(self.n, bits)
        self.K = len(self.moduli)
        self.oc = O.Context(log_n, self.moduli)
        env = env or {}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            self.eng = mhe.Engine(log_n, self.moduli)  # MHE_FP is read at mhe_ctx_create only
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        self.sk = self.oc.keygen_secret(SEED, 32)
        self.pk = self.oc.encrypt_zero_symmetric(SEED, self.sk, self.K)
        self.dpk = self.eng.to_device(self.pk)
        self.pk.setflags(write=False)
        self.refs = {}
        self.rng = np.random.default_rng(log_n)

    def ref(self, seed, L, pk=None):
        """The oracle's encryption of zero, computed once per (seed, L) for the chain's own key."""
        if pk is not None:
            return self.oc.encrypt_zero_asymmetric(seed, pk, L + 1, L)
        key = (tuple(seed), L)
        if key not in self.refs:
            r = self.oc.encrypt_zero_asymmetric(seed, self.pk, L + 1, L)
            r.setflags(write=False)
            self.refs[key] = r
        return self.refs[key]

    def plain(self, L):
        return np.stack([self.rng.integers(0, q, size=self.n, dtype=np.uint64) for q in self.moduli[:L]])

    def want(self, seed, L, plain=None, pk=None):
        w = np.array(self.ref(seed, L, pk))
        if plain is not None:
            q = np.array(self.moduli[:L], np.uint64)[:, None]
            w[0] = (w[0] + plain) % q  # both below 2^60: no wrap
        return w

    def run(self, seeds, L, plains=None, dpk=None):
        dpl = None if plains is None else [None if p is None else self.eng.to_device(p) for p in plains]
        outs = self.eng.encrypt_pk_batch(seeds, self.dpk if dpk is None else dpk, dpl, L)
        self.eng.synchronize()
        return [mhe.Engine.to_host(o) for o in outs]


@pytest.fixture(scope="module")
def setups():
    made = {}

    def get(log_n, bits, integer=False):
        key = (log_n, tuple(bits), integer)
        if key not in made:
            made[key] = Setup(log_n, bits, {"MHE_FP": "0"} if integer else None)
        return made[key]

    yield get
    for s in made.values():
        s.eng.close()


@pytest.fixture(scope="module")
def fp(setups):
    return setups(12, FP_BITS)


def check(s, seeds, L, plains=None):
    got = s.run(seeds, L, plains)
    for i, seed in enumerate(seeds):
        want = s.want(seed, L, None if plains is None else plains[i])
        assert np.array_equal(got[i], want), f"entry {i} of {len(seeds)} at L = {L}: {(got[i] != want).sum()} words differ"


@pytest.mark.parametrize("L", [3, 2, 1])
@pytest.mark.parametrize("count", [1, 3, 8, 9, 17])
def test_entry_counts(fp, count, L):
    """L = 3 drops the special prime, L = 2 a data prime, L = 1 leaves one output limb; 9 and 17
    entries run in more than one launch group."""
    fp.eng.encrypt_stats(reset=True)
    check(fp, [seed_of(i) for i in range(count)], L)
    assert fp.eng.encrypt_stats() == (count, (count + 7) // 8)


def test_plain_mix(fp):
    L = 3
    seeds = [seed_of(i) for i in range(3)]
    check(fp, seeds, L, [fp.plain(L), None, fp.plain(L)])
    check(fp, seeds, L, None)
    check(fp, seeds[:2], 2, [None, fp.plain(2)])


def test_ternary_redraw(fp):
    """The golden seed draws a zero 32-bit word among its first 4096: the fix-up kernel redoes u and
    moves the entry's CBD offsets; the neighbours keep theirs."""
    g = json.load(open(GOLDEN))
    assert g["log_n"] == fp.log_n
    redraw = [g["seed0"], 2, 3, 4, 5, 6, 7, 8]
    for L in (3, 2):
        check(fp, [seed_of(0), redraw, seed_of(1)], L, [None, fp.plain(L), None])


@pytest.mark.parametrize("L", [3, 2])
@pytest.mark.parametrize("which", ["mixed", "forced_integer"])
def test_60_bit_special_prime(setups, which, L):
    """The chain with a 60-bit special prime (every plain pass integer; L = 3 drops the 60-bit prime,
    L = 2 a data prime), and the FP64 chain on an engine created with MHE_FP=0."""
    s = setups(12, MIXED_BITS) if which == "mixed" else setups(12, FP_BITS, integer=True)
    check(s, [seed_of(i) for i in range(3)], L, [s.plain(L), None, s.plain(L)])


@pytest.mark.parametrize("mode", ["fp64", "integer"])
@pytest.mark.parametrize("log_n", [13, 14, 15, 16])
def test_ring_degrees(setups, log_n, mode):
    """k_fwd_col<7> / <8>, the 7-bit rows, k_fwd_row3 at 2^16 and the samplers' workgroup counts."""
    s = setups(log_n, FP_BITS, integer=mode == "integer")
    check(s, [seed_of(0), seed_of(1)], 2, [s.plain(2), None])


@pytest.mark.parametrize("which", ["fp64", "mixed", "integer"])
def test_extreme_residues(setups, which):
    """pk words all q - 1 and all 0, the plaintext all q - 1: the lazy ranges of the epilogue."""
    s = setups(12, MIXED_BITS if which == "mixed" else FP_BITS, integer=which == "integer")
    q = np.array(s.moduli, np.uint64)
    top = np.broadcast_to((q - 1)[None, :, None], (2, s.K, s.n)).copy()
    seeds = [seed_of(0), seed_of(1)]
    for L in (3, 2):
        plain = np.broadcast_to((q[:L] - 1)[:, None], (L, s.n)).copy()
        for pk in (top, np.zeros_like(top)):
            got = s.run(seeds, L, [plain, None], dpk=s.eng.to_device(pk))
            for i, seed in enumerate(seeds):
                assert np.array_equal(got[i], s.want(seed, L, plain if i == 0 else None, pk=pk))


def test_roundtrip(fp):
    """decode(decrypt(encrypt(encode(x)))) = x within the 1e-6 of test_gpu_parity's encrypt round trips."""
    L, scale = 3, 2.0 ** 40
    xs = [np.random.default_rng(i).uniform(-1, 1, size=fp.n // 2) for i in range(2)]
    pts = [fp.eng.encode(x, scale, L) for x in xs]
    cts = fp.eng.encrypt_pk_batch([seed_of(5), seed_of(6)], fp.dpk, pts, L)
    dsk = fp.eng.to_device(fp.sk)
    for x, ct in zip(xs, cts):
        dec = fp.eng.decode(fp.eng.decrypt(ct, dsk), scale)
        assert np.abs(dec - x).max() < 1e-6


def sequence(s, seed, L, dplain):
    """Today's entry points, call by call (Encryptor::encrypt_zero_at + encrypt_plain)."""
    eng, n, m = s.eng, s.n, L + 1
    u, state = eng.prng_small("ternary", m, seed)
    e = eng.empty(2, m, n)
    eng.prng_small("cbd", m, seed, 4 * n, out=e[0], state=state)
    eng.prng_small("cbd", m, seed, 10 * n, out=e[1], state=state)
    eng.ntt_forward(u, lazy=True)
    eng.ntt_forward(e, lazy=True)
    c = eng.empty(2, m, n)
    for j in range(2):
        eng.multiply_plain(u, s.dpk[j, :m], out=c[j])
        eng.add(e[j], c[j], out=c[j])
    d = eng.rescale_to_next(c)
    if dplain is not None:
        eng.add(d[0], dplain, out=d[0])
    return d


def op_counts(eng, reset=False):
    return [eng.op_counts(kind, reset=reset) for kind in range(8)]


def test_stats_and_op_counts(fp):
    L = 2
    seeds = [seed_of(i) for i in range(3)]
    plains = [fp.eng.to_device(fp.plain(L)), None, fp.eng.to_device(fp.plain(L))]
    op_counts(fp.eng, reset=True)
    seq = [sequence(fp, sd, L, p) for sd, p in zip(seeds, plains)]
    by_sequence = op_counts(fp.eng, reset=True)
    fp.eng.encrypt_stats(reset=True)
    outs = fp.eng.encrypt_pk_batch(seeds, fp.dpk, plains, L)
    by_batch = op_counts(fp.eng, reset=True)
    fp.eng.synchronize()
    assert fp.eng.encrypt_stats() == (3, 1)
    assert any(any(row) for row in by_sequence)
    assert by_batch == by_sequence
    for a, b in zip(outs, seq):
        assert np.array_equal(mhe.Engine.to_host(a), mhe.Engine.to_host(b))


def test_rejected_before_launch(fp):
    eng, L, n = fp.eng, 2, fp.n
    seeds = [seed_of(0), seed_of(1)]
    a, b = eng.empty(2, L, n), eng.empty(2, L, n)
    pkc = eng.to_device(np.array(fp.pk))
    pat = mhe.Engine.to_host(pkc).copy()
    a.fill_(7)
    b.fill_(7)
    eng.synchronize()
    eng.encrypt_stats(reset=True)

    def rejected(**kw):
        args = dict(seeds=seeds, pk=fp.dpk, plains=None, L=L, outs=[a, b])
        args.update(kw)
        with pytest.raises(mhe.MheError) as ei:
            eng.encrypt_pk_batch(**args)
        assert ei.value.code == MHE_ERR_ARG

    rejected(outs=[a, a])                       # overlapping outputs
    rejected(outs=[a, a[1:]])                   # ... by one poly
    rejected(pk=pkc, outs=[a, pkc])             # an output on the key
    rejected(plains=[b[0], None], outs=[a, b])  # an output on a plaintext
    rejected(L=0)
    rejected(L=fp.K)                            # limbs = key_limbs
    sd = np.ascontiguousarray(np.array(seeds, np.uint64))
    rc = mhe.lib().mhe_encrypt_pk_batch(eng._h, 0, sd.ctypes.data_as(ctypes.c_void_p), fp.dpk.data_ptr(), fp.K, None,
                                        eng._ptrs([a, b]), L, eng.stream())
    assert rc == MHE_ERR_ARG                    # count = 0
    eng.synchronize()
    assert bool((a == 7).all()) and bool((b == 7).all())
    assert np.array_equal(mhe.Engine.to_host(pkc), pat)
    assert eng.encrypt_stats() == (0, 0)
    injected_allocation_failure(fp)


def injected_allocation_failure(fp):
    """A fresh context grows its workspace before the first launch: failing that allocation leaves
    the outputs as they were, and the next call works."""
    eng = mhe.Engine(fp.log_n, fp.moduli)
    try:
        L = 3
        dpk = eng.to_device(np.array(fp.pk))
        o = eng.empty(2, L, fp.n)
        o.fill_(7)
        eng.synchronize()
        assert mhe.lib().mhe_debug_fail_alloc(eng._h, 1) == 0
        try:
            with pytest.raises(mhe.MheError, match="allocation failed"):
                eng.encrypt_pk_batch([seed_of(0)], dpk, None, L, outs=[o])
        finally:
            assert mhe.lib().mhe_debug_fail_alloc(eng._h, 0) == 0
        eng.synchronize()
        assert bool((o == 7).all())
        assert eng.encrypt_stats() == (0, 0)
        eng.encrypt_pk_batch([seed_of(0)], dpk, None, L, outs=[o])
        eng.synchronize()
        assert np.array_equal(mhe.Engine.to_host(o), fp.want(seed_of(0), L))
    finally:
        eng.close()
