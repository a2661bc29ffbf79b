"""GPU parity of mhe_relin_sum_rescale (include/mhe.h): a sum of relinearized products, optionally
doubled, then rescaled -- every product with its own key switch, special-limb inverse NTT and lift,
but one forward NTT per limb per sum behind them -- must give the words of the oracle's
rescale(add(relinearize(multiply(a, b)), ...)) (SEAL/evaluator.cpp:2281-2525, 78-120,
util/rns.cpp:737-808).  Every comparison is np.array_equal on every word; every input is compared
unchanged afterwards; mhe_prodsum_stats is asserted, so a silent fall-back fails.

One launch holds 8 entries and one finishing launch 8 groups, so 8 / 9 / 17 terms and 9 groups cover
a full chunk, the splits and more than two chunks."""
import numpy as np
import pytest

import mhe
from test_gpu_batch import truncated
from test_gpu_parity import SMALL_BITS, Chain
from test_gpu_ring_degrees import MODES, make_chain
from test_rotate_sum import BIGP_BITS, op_counts

pytestmark = pytest.mark.gpu

TERMS = 17


class Pool:
    """17 products at L limbs (the oracle's multiply of random ciphertexts; entry 16 a square), one
    relinearization key and the oracle's relinearization of each: computed once per (chain, L) and
    shared by the tests, never written."""

    def __init__(self, ch, L, terms=TERMS):
        self.ch, self.L = ch, L
        self.key = ch.rand_key()
        self.a = [ch.rand(2, L, ch.n) for _ in range(terms)]
        self.b = [ch.rand(2, L, ch.n) for _ in range(terms)]
        self.ct3 = [ch.oc.multiply(x, y) for x, y in zip(self.a, self.b)]
        self.ct3[-1] = ch.oc.square(self.a[-1])
        self.rel = [ch.oc.relinearize(c, self.key) for c in self.ct3]
        self.dct3 = [ch.up(c) for c in self.ct3]
        self.dkey = ch.up(self.key)
        for r in self.rel + self.ct3:
            r.setflags(write=False)

    def want(self, idx, twice=False):
        acc = None
        for i in idx:
            acc = self.rel[i] if acc is None else self.ch.oc.add(acc, self.rel[i])
        if twice:
            acc = self.ch.oc.add(acc, acc)
        return self.ch.oc.rescale(acc)

    def inputs_unchanged(self):
        for d, c in zip(self.dct3, self.ct3):
            assert np.array_equal(self.ch.down(d), c)
        assert np.array_equal(self.ch.down(self.dkey), self.key)


def run(ch, p, sizes, twice, key=None, outs=None, first=0):
    """One call over consecutive groups of `sizes` terms from entry `first`; compares every group and
    the counters of the merged path."""
    idx = list(range(first, first + sum(sizes)))
    groups = [g for g, s in enumerate(sizes) for _ in range(s)]
    ch.eng.synchronize()
    ch.eng.prodsum_stats(reset=True)
    got = ch.eng.relin_sum_rescale([p.dct3[i] for i in idx], p.dkey if key is None else key, groups=groups,
                                   twice=twice, outs=outs)
    assert ch.eng.prodsum_stats() == (len(sizes), len(idx))
    at = 0
    for g, s in enumerate(sizes):
        assert got[g].shape == (2, p.L - 1, ch.n)
        assert np.array_equal(ch.down(got[g]), p.want(idx[at:at + s], twice[g] if twice else False)), f"group {g}"
        at += s
    p.inputs_unchanged()
    return got


@pytest.fixture(scope="module")
def small():
    return Chain(12, SMALL_BITS, seed=31)


@pytest.fixture(scope="module")
def pools(small):
    made = {}

    def get(L):
        if L not in made:
            made[L] = Pool(small, L)
        return made[L]

    return get


@pytest.fixture(scope="module")
def bigp():
    ch = Chain(12, BIGP_BITS, seed=32)
    return Pool(ch, ch.K - 1)


@pytest.mark.parametrize("L", [2, 3, 7])
@pytest.mark.parametrize("terms", [1, 2, 8, 9, 17])
@pytest.mark.parametrize("twice", [False, True])
def test_one_group(small, pools, L, terms, twice):
    """SMALL_BITS (every prime below 2^51): the FP64 lift and epilogues.  L = 2: a one-limb output."""
    run(small, pools(L), (terms,), [twice])


@pytest.mark.parametrize("sizes", [(3, 1, 5), (2,) * 8, (1,) * 9, (9, 8)], ids=["3-1-5", "8x2", "9x1", "9-8"])
def test_groups(small, pools, sizes):
    """Several sums in one call, doubled or not per group: a chunk boundary inside a group (3, 1, 5
    and 9, 8), a full finishing launch (8 groups) and more groups than one finishing launch holds (9)."""
    run(small, pools(3), sizes, [g % 2 == 0 for g in range(len(sizes))])
    run(small, pools(3), sizes, None)


def test_squares(small):
    """ct3 as mhe_ct_square and mhe_ct_multiply write it on the device."""
    ch, L = small, 3
    key = ch.rand_key()
    a, b = [ch.rand(2, L, ch.n) for _ in range(3)], ch.rand(2, L, ch.n)
    d3 = [ch.eng.square(ch.up(x)) for x in a] + [ch.eng.multiply(ch.up(a[0]), ch.up(b))]
    rel = [ch.oc.relinearize(ch.oc.square(x), key) for x in a] + [ch.oc.relinearize(ch.oc.multiply(a[0], b), key)]
    ch.eng.prodsum_stats(reset=True)
    o0, o1 = ch.eng.relin_sum_rescale(d3, ch.up(key), groups=[0, 0, 1, 1], twice=[1, 0])
    assert ch.eng.prodsum_stats() == (2, 4)
    s0 = ch.oc.add(rel[0], rel[1])
    assert np.array_equal(ch.down(o0), ch.oc.rescale(ch.oc.add(s0, s0)))
    assert np.array_equal(ch.down(o1), ch.oc.rescale(ch.oc.add(rel[2], rel[3])))


@pytest.mark.parametrize("twice", [False, True])
def test_60_bit_special_prime(bigp, twice):
    """The GPT-2 chain's shape of primes: the integer lift and epilogues, the ModDown lift with a
    reduction mod q_i, and 17 terms: 17 P > 2^64, so special limbs summed unreduced would wrap."""
    ch = bigp.ch
    assert 17 * ch.moduli[-1] > 2**64 and all(q < ch.moduli[-1] for q in ch.moduli[:-1])
    run(ch, bigp, (17,), [twice])


@pytest.mark.parametrize("fmt", ["seal", "doubles", "pack48", "truncated"])
def test_key_formats(small, pools, fmt):
    """SEAL's layout, the two prepared formats and a level-truncated key give the same words."""
    p = pools(3)
    if fmt == "truncated":
        key = small.up(truncated(p.key, p.L))
    else:
        key = small.up(p.key)
        if fmt != "seal":
            small.eng.key_prepare(key, 1 if fmt == "doubles" else 2)
    run(small, p, (2, 1), [True, False], key=key)


@pytest.mark.parametrize("fill", ["zero", "max"])
def test_extreme_residues(small, fill):
    """Every residue 0, and every residue q - 1 in the products and the key: each modular sum of the
    nine terms and the doubling wrap."""
    ch, L, terms = small, 7, 9
    q = np.array(ch.moduli, np.uint64)
    p = Pool.__new__(Pool)
    p.ch, p.L = ch, L
    p.key = np.zeros((ch.K - 1, 2, ch.K, ch.n), np.uint64)
    one = np.zeros((3, L, ch.n), np.uint64)
    if fill == "max":
        p.key[:] = (q - np.uint64(1))[None, None, :, None]
        one[:] = (q[:L] - np.uint64(1))[None, :, None]
    p.ct3 = [one] * terms
    p.rel = [ch.oc.relinearize(one, p.key)] * terms
    p.dct3 = [ch.up(one) for _ in range(terms)]
    p.dkey = ch.up(p.key)
    run(ch, p, (terms,), [True])
    run(ch, p, (4, 5), [False, True])


@pytest.fixture(scope="module")
def ring_chains():
    made = {}

    def get(log_n, mode):
        if (log_n, mode) not in made:
            bits, env = MODES[mode]
            made[(log_n, mode)] = make_chain(log_n, bits, env, 200 * log_n + list(MODES).index(mode))
        return made[(log_n, mode)]

    return get


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("log_n", [13, 14, 15, 16])
def test_ring_degrees(ring_chains, log_n, mode):
    """Every instantiation of the new column job: row / column shapes of 2^13 .. 2^16 in FP64, integer
    and mixed (FP64 key switch, integer tail) arithmetic; L = 3, groups of 2 (doubled) and 1."""
    ch = ring_chains(log_n, mode)
    run(ch, Pool(ch, 3, terms=3), (2, 1), [True, False])


def test_ks_fused_off_same_words(small, pools):
    """The separate-MAC debugging path runs the sequence entry by entry: the same words, and nothing
    counted as merged."""
    p = pools(3)
    ch = make_chain(12, SMALL_BITS, {"MHE_KS_FUSED": "0"}, 33)
    try:
        d3 = [ch.up(np.array(c)) for c in p.ct3[:9]]
        outs = ch.eng.relin_sum_rescale(d3, ch.up(p.key), groups=[0] * 3 + [1] + [2] * 5, twice=[1, 0, 1])
        assert ch.eng.prodsum_stats() == (0, 0)
        for g, idx in enumerate(([0, 1, 2], [3], [4, 5, 6, 7, 8])):
            assert np.array_equal(ch.down(outs[g]), p.want(idx, g != 1)), g
        for d, c in zip(d3, p.ct3):
            assert np.array_equal(ch.down(d), c)
    finally:
        ch.eng.close()


def test_op_counts(small, pools):
    """mhe_op_counts sees the op mix of the sequence the call replaces, run on a second context."""
    L = 3
    p = pools(L)
    sizes, twice = (3, 1, 5), [True, False, True]
    eng = small.eng
    eng.synchronize()
    op_counts(eng)
    run(small, p, sizes, twice)
    got = op_counts(eng)
    other = mhe.Engine(small.log_n, small.moduli)
    try:
        key = other.to_device(p.key)
        at = 0
        for s, tw in zip(sizes, twice):
            acc = None
            for i in range(at, at + s):
                t = other.to_device(np.array(p.ct3[i]))
                other.relinearize(t, key)
                acc = t[:2].contiguous() if acc is None else other.add(acc, t[:2].contiguous(), out=acc)
            if tw:
                other.add(acc, acc, out=acc)
            other.rescale_to_next(acc)
            at += s
        other.synchronize()
        assert other.prodsum_stats() == (0, 0)
        assert got == op_counts(other)
    finally:
        other.close()


def test_errors(small, pools):
    """Every argument is checked before the first launch: the outputs keep their words."""
    L = 3
    p = pools(L)
    eng, n = small.eng, small.n
    d3 = p.dct3[:3]
    o, o2 = eng.empty(2, L - 1, n), eng.empty(2, L - 1, n)
    o.fill_(7)
    o2.fill_(7)
    eng.prodsum_stats(reset=True)
    with pytest.raises(mhe.MheError, match="same value"):
        eng.relin_sum_rescale(d3, p.dkey, outs=[d3[1][1:3]])  # the output inside an input
    big = eng.empty(3, L - 1, n)
    big.fill_(7)
    with pytest.raises(mhe.MheError, match="same value"):  # two outputs overlapping by one poly
        eng.relin_sum_rescale(d3, p.dkey, groups=[0, 0, 1], outs=[big[0:2], big[1:3]])
    one = [eng.empty(3, 1, n) for _ in range(2)]
    with pytest.raises(mhe.MheError, match="end of modulus switching chain"):
        eng.relin_sum_rescale(one, p.dkey, outs=[o])  # limbs = 1
    short = p.dkey[:, :, :L]  # a full key cut to L limbs: fewer than L + 1
    with pytest.raises(mhe.MheError, match="kswitch_keys"):
        eng.relin_sum_rescale(d3, short, outs=[o])
    with pytest.raises(mhe.MheError, match="invalid argument"):
        eng.relin_sum_rescale(d3, p.dkey, groups=[0, 1, 0], outs=[o, o2])  # decreasing
    with pytest.raises(mhe.MheError, match="invalid argument"):
        eng.relin_sum_rescale(d3, p.dkey, groups=[0, 0, 2], outs=[o, o2, eng.empty(2, L - 1, n)])  # a gap
    with pytest.raises(mhe.MheError, match="invalid argument"):
        eng.relin_sum_rescale(d3, p.dkey, groups=[1, 1, 1], outs=[o, o2])  # group 0 empty
    # an injected key-switch failure, in the first chunk and in the second (the tail runs after both)
    for nth in (1, 2):
        assert mhe.lib().mhe_debug_fail_switch(eng._h, nth) == 0
        try:
            with pytest.raises(mhe.MheError, match="injected"):
                eng.relin_sum_rescale(p.dct3[:9], p.dkey, outs=[o])
        finally:
            assert mhe.lib().mhe_debug_fail_switch(eng._h, 0) == 0
    eng.synchronize()
    assert bool((o == 7).all()) and bool((o2 == 7).all()) and bool((big == 7).all())
    assert eng.prodsum_stats() == (0, 0)
    p.inputs_unchanged()
    assert eng.relin_sum_rescale([], p.dkey, outs=[]) == []  # count == 0 with groups == 0


@pytest.mark.parametrize("nth", [1, 2])
def test_injected_allocation_failure(small, pools, nth):
    """A fresh context grows the workspace (allocation 1) and the group accumulators (allocation 2)
    before the first launch: failing either leaves the output as it was, and the next call works."""
    p = pools(3)
    eng = mhe.Engine(small.log_n, small.moduli)
    try:
        d3 = [eng.to_device(np.array(c)) for c in p.ct3[:3]]
        key = eng.to_device(p.key)
        o = eng.empty(2, p.L - 1, small.n)
        o.fill_(7)
        eng.synchronize()
        assert mhe.lib().mhe_debug_fail_alloc(eng._h, nth) == 0
        try:
            with pytest.raises(mhe.MheError, match="allocation failed"):
                eng.relin_sum_rescale(d3, key, outs=[o])
        finally:
            assert mhe.lib().mhe_debug_fail_alloc(eng._h, 0) == 0
        eng.synchronize()
        assert bool((o == 7).all())
        assert eng.prodsum_stats() == (0, 0)
        eng.relin_sum_rescale(d3, key, outs=[o])
        eng.synchronize()
        assert np.array_equal(mhe.Engine.to_host(o), p.want([0, 1, 2]))
    finally:
        eng.close()
