"""GPU parity of mhe_rotate_sum (include/mhe.h): the sum of several rotations, with each rotation's
own special-limb inverse NTT and lift but one ModDown forward NTT per limb for the whole sum, must
give the words of rotating one by one (the oracle's apply_galois_inplace restatement,
SEAL/evaluator.cpp:2120-2222, 2281-2525) and folding with add_inplace (evaluator.cpp:78-120).
Every comparison is np.array_equal on every word; every input is compared unchanged afterwards.

One launch holds 8 entries and one finishing launch 8 groups, so 8 / 9 / 17 terms and 9 groups cover
a full chunk, the splits and more than two chunks."""
import ctypes

import numpy as np
import pytest

import mhe
from test_gpu_batch import truncated
from test_gpu_parity import RESNET_BITS, SMALL_BITS, Chain

pytestmark = pytest.mark.gpu

# a 60-bit special prime above 49-bit data primes: the integer epilogue, the lift's reduction
# mod q_i, and 17 P > 2^64 (an unreduced 64-bit sum of 17 special limbs would wrap)
BIGP_BITS = [49] + [46] * 3 + [49] * 2 + [60]
STEPS = [1, -1, 3, 100, 7, -5, 64, 2, 9, 31, 12, -17, 5, 256, 33, -64, 11]


class Pool:
    """17 random ciphertexts at L limbs with a step and a key each, and the oracle's rotation of
    each: computed once per (chain, L) and shared by the tests, never written."""

    def __init__(self, ch, L, special=()):
        self.ch, self.L = ch, L
        self.cts = [ch.rand(2, L, ch.n) for _ in STEPS]
        for i, kind in special:
            self.cts[i][1] = 0  # c1 all zeros / a single nonzero coefficient
            if kind == "one":
                self.cts[i][1, :, 5] = 1
        self.elts = [mhe.galois_elt_from_step(ch.log_n, s) for s in STEPS]
        self.keys = [ch.rand_key() for _ in range(4)]  # entry i uses key i % 4
        self.rot = [ch.oc.apply_galois(c, e, self.keys[i % 4]) for i, (c, e) in enumerate(zip(self.cts, self.elts))]
        self.dcts = [ch.up(c) for c in self.cts]
        # full keys and level-truncated slices, alternating
        self.dkeys = [ch.up(k if j % 2 else truncated(k, L)) for j, k in enumerate(self.keys)]
        for r in self.rot:
            r.setflags(write=False)

    def want(self, idx, prior=None):
        acc = None if prior is None else prior
        for i in idx:
            acc = self.rot[i] if acc is None else self.ch.oc.add(acc, self.rot[i])
        return acc

    def args(self, idx, shared_key=False):
        return ([self.dcts[i] for i in idx], [self.elts[i] for i in idx],
                [self.dkeys[0 if shared_key else i % 4] for i in idx])

    def inputs_unchanged(self):
        for d, c in zip(self.dcts, self.cts):
            assert np.array_equal(self.ch.down(d), c)


@pytest.fixture(scope="module")
def small():
    return Chain(12, SMALL_BITS, seed=21)


@pytest.fixture(scope="module")
def pools(small):
    made = {}

    def get(L):
        if L not in made:
            # entry 2: c1 all zeros; entry 4: one nonzero coefficient -- terms among random ones
            made[L] = Pool(small, L, special=((2, "zero"), (4, "one")))
        return made[L]

    return get


@pytest.fixture(scope="module")
def bigp():
    ch = Chain(12, BIGP_BITS, seed=22)
    return Pool(ch, ch.K - 1)


@pytest.mark.parametrize("L", [1, 3, 7])
@pytest.mark.parametrize("terms", [1, 2, 8, 9, 17])
def test_rotate_sum_one_group(small, pools, L, terms):
    """SMALL_BITS (every prime below 2^51): the FP64 epilogue."""
    p = pools(L)
    idx = list(range(terms))
    (out,) = small.eng.rotate_sum(*p.args(idx))
    assert np.array_equal(small.down(out), p.want(idx))
    p.inputs_unchanged()


@pytest.mark.parametrize("terms", [2, 9])
def test_rotate_sum_shared_key(small, pools, terms):
    p = pools(3)
    idx = list(range(terms))
    cts, elts, keys = p.args(idx, shared_key=True)
    (out,) = small.eng.rotate_sum(cts, elts, keys)
    want = None
    for i in idx:
        r = small.oc.apply_galois(p.cts[i], p.elts[i], p.keys[0])
        want = r if want is None else small.oc.add(want, r)
    assert np.array_equal(small.down(out), want)
    p.inputs_unchanged()


@pytest.mark.parametrize("L", [1, 7])
@pytest.mark.parametrize("terms", [1, 9])
def test_rotate_sum_accumulate(small, pools, L, terms):
    """accumulate: the prior contents of out (a random ciphertext) appear in the sum."""
    p = pools(L)
    idx = list(range(3, 3 + terms))
    prior = small.rand(2, L, small.n)
    out = small.up(prior)
    small.eng.rotate_sum(*p.args(idx), outs=[out], accumulate=True)
    assert np.array_equal(small.down(out), p.want(idx, prior=prior))
    p.inputs_unchanged()


@pytest.mark.parametrize("sizes", [(3, 1, 5), (2,) * 8, (1,) * 9, (9, 8)], ids=["3-1-5", "8x2", "9x1", "9-8"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_rotate_sum_groups(small, pools, sizes, accumulate):
    """Several sums in one call: a chunk boundary inside a group (3, 1, 5 and 9, 8), a full
    finishing launch (8 groups) and more groups than one finishing launch holds (9)."""
    L = 3
    p = pools(L)
    idx = list(range(sum(sizes)))
    groups = [g for g, s in enumerate(sizes) for _ in range(s)]
    priors = [small.rand(2, L, small.n) for _ in sizes]
    outs = [small.up(x) for x in priors]
    got = small.eng.rotate_sum(*p.args(idx), groups=groups, outs=outs, accumulate=accumulate)
    at = 0
    for g, s in enumerate(sizes):
        want = p.want(idx[at:at + s], prior=priors[g] if accumulate else None)
        assert np.array_equal(small.down(got[g]), want), f"group {g}"
        at += s
    p.inputs_unchanged()


@pytest.mark.parametrize("accumulate", [False, True])
def test_rotate_sum_60_bit_special_prime(bigp, accumulate):
    """The GPT-2 chain's shape of primes: integer epilogue, lift with a reduction mod q_i, and 17
    terms, more than floor((2^64 - 1) / P) = 15."""
    p, ch = bigp, bigp.ch
    assert 17 * ch.moduli[-1] > 2**64 and all(q < ch.moduli[-1] for q in ch.moduli[:-1])
    idx = list(range(17))
    prior = ch.rand(2, p.L, ch.n)
    out = ch.up(prior)
    ch.eng.rotate_sum(*p.args(idx), outs=[out], accumulate=accumulate)
    assert np.array_equal(ch.down(out), p.want(idx, prior=prior if accumulate else None))
    p.inputs_unchanged()


def test_rotate_sum_prepared_keys_n16():
    """N = 2^16 on the ResNet chain, L = 6, 4 terms, prepared keys alternating doubles / 48-bit planes."""
    ch = Chain(16, RESNET_BITS, seed=23)
    L = 6
    steps = [1, 2, 4, 8]
    cts = [ch.rand(2, L, ch.n) for _ in steps]
    elts = [mhe.galois_elt_from_step(ch.log_n, s) for s in steps]
    keys = [truncated(ch.rand_key(digits=L), L) for _ in steps]
    dkeys = [ch.eng.key_prepare(ch.up(k), 1 + i % 2) for i, k in enumerate(keys)]
    dcts = [ch.up(c) for c in cts]
    (out,) = ch.eng.rotate_sum(dcts, elts, dkeys)
    want = None
    for c, e, k in zip(cts, elts, keys):
        full = np.zeros((L, 2, ch.K, ch.n), np.uint64)  # the truncated slice inside a full-shape key
        full[:, :, :L] = k[:, :, :L]
        full[:, :, -1] = k[:, :, -1]
        r = ch.oc.apply_galois(c, e, full)
        want = r if want is None else ch.oc.add(want, r)
    assert np.array_equal(ch.down(out), want)
    for d, c in zip(dcts, cts):
        assert np.array_equal(ch.down(d), c)


def test_rotate_sum_errors(small, pools):
    """Every argument is checked before the first launch: out keeps its words."""
    L = 3
    p = pools(L)
    eng, n = small.eng, small.n
    cts, elts, keys = p.args([0, 1, 2])
    o = eng.empty(2, L, n)
    o.fill_(7)
    o2 = eng.empty(2, L, n)
    o2.fill_(7)
    with pytest.raises(mhe.MheError, match="Galois element"):
        eng.rotate_sum(cts, [elts[0], 4, elts[2]], keys, outs=[o], accumulate=True)
    short = p.dkeys[1][:, :, :L]  # a full key cut to L limbs: fewer than L + 1
    with pytest.raises(mhe.MheError, match="kswitch_keys"):
        eng.rotate_sum(cts, elts, [keys[0], keys[1], short], outs=[o])
    with pytest.raises(mhe.MheError, match="invalid argument"):
        eng.rotate_sum(cts, elts, keys, groups=[0, 1, 0], outs=[o, o2])  # decreasing
    with pytest.raises(mhe.MheError, match="invalid argument"):
        eng.rotate_sum(cts, elts, keys, groups=[0, 0, 2], outs=[o, o2, eng.empty(2, L, n)])  # a gap
    with pytest.raises(mhe.MheError, match="invalid argument"):
        eng.rotate_sum(cts, elts, keys, groups=[1, 1, 1], outs=[o, o2])  # group 0 empty
    with pytest.raises(mhe.MheError, match="same value"):
        eng.rotate_sum(cts, elts, keys, outs=[cts[1]])  # the output is an input
    big = eng.empty(3, L, n)
    big.fill_(7)
    with pytest.raises(mhe.MheError, match="same value"):  # two outputs overlapping by one poly
        eng.rotate_sum(cts, elts, keys, groups=[0, 0, 1], outs=[big[0:2], big[1:3]])
    small.eng.synchronize()
    assert bool((o == 7).all()) and bool((o2 == 7).all()) and bool((big == 7).all())
    p.inputs_unchanged()
    assert eng.rotate_sum([], [], [], outs=[]) == []  # count == 0 with groups == 0


def op_counts(eng):
    out = {}
    for kind in range(8):
        buf = (ctypes.c_uint64 * 64)()
        assert mhe.lib().mhe_op_counts(eng._h, kind, buf, 64, 1) == 0
        out[kind] = list(buf)
    return out


@pytest.mark.parametrize("accumulate", [False, True])
def test_rotate_sum_stats_and_op_counts(small, pools, accumulate):
    """mhe_rotsum_stats counts the sums and terms of the calls made; the op mix (mhe_op_counts) is
    that of rotating one by one and adding, run on a second context."""
    L = 3
    p = pools(L)
    sizes = (3, 1, 5)
    idx = list(range(sum(sizes)))
    groups = [g for g, s in enumerate(sizes) for _ in range(s)]
    eng = small.eng
    eng.synchronize()
    op_counts(eng)
    eng.rotsum_stats(reset=True)
    outs = [small.up(small.rand(2, L, small.n)) for _ in sizes]
    eng.rotate_sum(*p.args(idx), groups=groups, outs=outs, accumulate=accumulate)
    eng.rotate_sum(*p.args([0, 1]))
    assert eng.rotsum_stats() == (4, 11)
    assert eng.rotsum_stats(reset=True) == (4, 11)
    assert eng.rotsum_stats() == (0, 0)
    got = op_counts(eng)

    other = mhe.Engine(small.log_n, small.moduli)
    try:
        cts = [other.to_device(c) for c in p.cts]
        keys = [other.to_device(k) for k in p.keys]
        for gl, acc in ((groups, accumulate), ([0, 0], False)):
            sums = [other.to_device(small.rand(2, L, small.n)) for _ in range(max(gl) + 1)]
            seen = set()
            for i, g in enumerate(gl):
                r = other.apply_galois_to(cts[i], p.elts[i], keys[i % 4])
                if g in seen or acc:
                    other.add(sums[g], r, out=sums[g])
                seen.add(g)
        other.synchronize()
        assert other.rotsum_stats() == (0, 0)
        assert got == op_counts(other)
    finally:
        other.close()
