"""GPU parity of the streaming ModUp column pass (csrc/ntt.h k_modup_col), bit for bit against the oracle.

A workgroup of the pass takes any number of output primes: their column twiddles go through a ring of
five one-prime LDS slots in the order the workgroup processes them (the lazy sweep, the non-lazy sweep,
the integer sweep of the mixed kernels; the digit's own prime left out), the prime five places on
refilling a slot behind the next prime's transpose barrier.  The chain has 16 data primes at N = 2^16,
twelve below 2^47 (46- and 47-bit: both exits of the lazy sweep) and four above (48, 50, 51, 51 bits),
its first seven limbs those of test_modup_trim's chain, so both lift rules are met on both sides.  With
one group per digit (MHE_KS_COLGROUPS=1) the levels 2, 5, 6, 11 and 16 give a workgroup 3, 6, 7, 12 and
17 output primes: fewer than the ring holds, one more, and past two wraps; at L = 16 the lazy sweep alone
walks the ring more than twice and the non-lazy sweep starts at a slot that is not 0.  Every digit is
switched, so the skipped prime I == J falls on every place of the order, the first, the sixth and the
last among them.  Each shape also runs with two groups and with the grouping the library picks from the
launch's size; the launch counter (mhe_modup_stats) shows which grouping ran."""
import gc

import numpy as np
import pytest
import torch

import mhe
from test_gpu_batch import hoisting, truncated
from test_gpu_ring_degrees import make_chain

pytestmark = pytest.mark.gpu

STREAM_BITS = [51, 46, 46, 47, 48, 50, 51, 46, 47, 46, 47, 46, 47, 46, 47, 46] + [51]  # 16 data limbs + special
SMALL_N_BITS = [51, 46, 46, 46, 46, 46, 47] + [51]
MIX_BITS = [49, 46, 46, 47, 48, 50] + [60]  # 60-bit special prime: the mixed kernels, integer sweep last
LEVELS = [2, 5, 6, 11, 16]
GROUPS = [1, 2, None]  # MHE_KS_COLGROUPS; None: unset, the library's rule
IG_MAX = 9             # the most groups the rule picks (ntt.h MHE_MODUP_IGMAX)


def groups_env(groups):
    return {} if groups is None else {"MHE_KS_COLGROUPS": str(groups)}


def check_grouping(stats, groups, launches, L):
    """mhe_modup_stats after `launches` column-pass launches at L limbs under MHE_KS_COLGROUPS=groups."""
    n, ig = stats
    assert n == launches, stats
    if groups is None:
        assert n <= ig <= n * min(IG_MAX, L + 1), stats
    else:
        assert ig == n * min(groups, L + 1), stats


class Data:
    """Per level L, made once and left unchanged: a key (limbs 0..L-1 and the special limb random), operand
    pairs, switch inputs; the oracle's results on first use.  Shared by the engines of every grouping."""

    def __init__(self, ch, L):
        self.ch, self.L = ch, L
        self.key = np.zeros((L, 2, ch.K, ch.n), np.uint64)
        for l in list(range(L)) + [ch.K - 1]:
            self.key[:, :, l, :] = ch.rng.integers(0, ch.moduli[l], size=(L, 2, ch.n), dtype=np.uint64)
        self.tkey = truncated(self.key, L)
        self.a = [ch.rand(2, L, ch.n) for _ in range(2)]
        self.b = [ch.rand(2, L, ch.n) for _ in range(2)]
        self.ct = [ch.rand(2, L, ch.n) for _ in range(3)]
        self.target = [ch.rand(L, ch.n) for _ in range(3)]
        self._hm, self._sk = {}, {}

    def hmult(self, i):
        if i not in self._hm:
            self._hm[i] = self.ch.oc.hmult(self.a[i], self.b[i], self.key)
        return self._hm[i]

    def switch_key(self, i):
        if i not in self._sk:
            self._sk[i] = self.ch.oc.switch_key(self.ct[i], self.target[i], self.key)
        return self._sk[i]


class Env:
    """A chain's data and oracle (the first engine's Chain) and one engine per grouping, made on first use."""

    def __init__(self, log_n, bits, seed):
        self.log_n, self.bits, self.seed = log_n, bits, seed
        self.chains, self.levels = {}, {}

    def chain(self, groups):
        if groups not in self.chains:
            self.chains[groups] = make_chain(self.log_n, self.bits, groups_env(groups), self.seed)
        return self.chains[groups]

    @property
    def ch(self):
        """The chain whose rng and oracle make the data: one, whichever grouping asks first."""
        if not self.chains:
            self.chain(1)
        return next(iter(self.chains.values()))

    def level(self, L):
        if L not in self.levels:
            self.levels[L] = Data(self.ch, L)
        return self.levels[L]

    def close(self):
        self.levels.clear()
        for ch in self.chains.values():
            ch.eng.close()
        self.chains.clear()
        gc.collect()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def env():
    e = Env(16, STREAM_BITS, seed=71)
    yield e
    e.close()


def dkey(ch, d, fmt):
    """The level-truncated key on ch's device: fmt 0 SEAL's layout, 1 prepared (doubles)."""
    k = ch.up(d.tkey)
    return ch.eng.key_prepare(k, fmt) if fmt else k


def run_switch(ch, d, count, fmt):
    cts = [ch.up(c) for c in d.ct[:count]]
    dk = dkey(ch, d, fmt)
    ch.eng.modup_stats(reset=True)
    ch.eng.switch_key_batch(cts, [ch.up(t) for t in d.target[:count]], [dk] * count)
    got = [ch.down(c) for c in cts]
    return got, ch.eng.modup_stats(reset=True)


def test_chain_has_every_class(env):
    """The chain's primes are what the cases below rely on (a generator change would hollow them out)."""
    q = env.ch.moduli
    assert [int(x).bit_length() for x in q] == STREAM_BITS
    assert len(set(q)) == len(q)
    assert sum(1 for x in q[:16] if x < 2**47) == 12 and sum(1 for x in q[:16] if x < 2**46) >= 6
    assert sorted(int(x).bit_length() for x in q[:16] if x >= 2**47) == [48, 50, 51, 51]
    # both sides of the lazy rule (q_J <= 4 q_I) and of the non-lazy one (q_J <= 2 q_I)
    assert any(qj <= 4 * q[1] for qj in q[:16]) and any(qj > 4 * q[1] for qj in q[:16])
    assert any(qj <= 2 * q[4] for qj in q[:16]) and any(qj > 2 * q[4] for qj in q[:16])
    # the lazy sweep of one group at L = 16 walks the five-slot ring more than twice
    assert sum(1 for x in q[:16] if x < 2**47) - 1 > 10


@pytest.mark.parametrize("groups", GROUPS, ids=lambda g: f"groups{g}")
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("L", LEVELS)
def test_switch_key_batch(env, L, count, groups):
    """One entry and three; SEAL's key layout at L = 5 and 11, the prepared key at the other levels."""
    ch, d = env.chain(groups), env.level(L)
    got, stats = run_switch(ch, d, count, 0 if L in (5, 11) else 1)
    check_grouping(stats, groups, 1, L)
    for i in range(count):
        assert np.array_equal(got[i], d.switch_key(i)), f"entry {i}"


@pytest.mark.parametrize("groups", GROUPS, ids=lambda g: f"groups{g}")
@pytest.mark.parametrize("L", LEVELS)
def test_hmult_batch(env, L, groups):
    """Two HMults behind the same column pass; the prepared key at L = 5 and 11, SEAL's layout elsewhere."""
    ch, d = env.chain(groups), env.level(L)
    dk = dkey(ch, d, 1 if L in (5, 11) else 0)
    ch.eng.modup_stats(reset=True)
    outs = ch.eng.hmult_batch([ch.up(x) for x in d.a], [ch.up(x) for x in d.b], dk)
    got = [ch.down(o) for o in outs]
    check_grouping(ch.eng.modup_stats(reset=True), groups, 1, L)
    for i in range(2):
        assert np.array_equal(got[i], d.hmult(i)), f"entry {i}"


@pytest.mark.parametrize("fill", ["zero", "max"])
def test_extreme_limbs(env, fill):
    """Every residue 0, and every residue q - 1 (ciphertext, target and key), at L = 11 with one group."""
    ch, L = env.chain(1), 11
    q = np.array(ch.moduli, np.uint64)

    def filled(shape, limbs):
        out = np.zeros(shape, np.uint64)
        if fill == "max":
            for k, l in enumerate(limbs):
                out[..., k, :] = q[l] - np.uint64(1)
        return out

    ct, target = filled((2, L, ch.n), range(L)), filled((L, ch.n), range(L))
    key = filled((L, 2, ch.K, ch.n), range(ch.K))
    dk = ch.eng.key_prepare(ch.up(truncated(key, L)), 1)
    cts = [ch.up(ct), ch.up(ct)]
    ch.eng.modup_stats(reset=True)
    ch.eng.switch_key_batch(cts, [ch.up(target)] * 2, [dk] * 2)
    got = [ch.down(c) for c in cts]
    check_grouping(ch.eng.modup_stats(reset=True), 1, 1, L)
    want = env.ch.oc.switch_key(ct, target, key)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)


@pytest.mark.parametrize("groups", [1, None], ids=lambda g: f"groups{g}")
def test_hoisted_rotation_batch(env, groups):
    """One input rotated three ways at L = 6: the hoisted path's shared ModUp runs the column pass with
    canonical, unpacked output; the engine's own check recomputes every rotation by the classic path."""
    ch, L = env.chain(groups), 6
    d = env.level(L)
    ct = d.ct[0]
    elts = [mhe.galois_elt_from_step(ch.log_n, s) for s in (1, -3, 64)]
    src = ch.up(ct)
    dk = dkey(ch, d, 1)
    ch.eng.modup_stats(reset=True)
    with hoisting(ch.eng, len(elts)):
        outs = ch.eng.apply_galois_batch([src] * len(elts), elts, [dk] * len(elts))
    n, ig = ch.eng.modup_stats(reset=True)
    assert n >= 2, (n, ig)  # the hoisted ModUp, and the classic path's (of the check, and of flagged inputs)
    if groups is not None:
        assert ig == n * groups
    for j, elt in enumerate(elts):
        assert np.array_equal(ch.down(outs[j]), env.ch.oc.apply_galois(ct, elt, d.key)), f"rotation {j}"


@pytest.mark.parametrize("log_n", [13, 12])
def test_switch_key_small_n(log_n):
    """N = 2^13 and 2^12 with one group: the other two kernel shapes, whose ring slots hold 128 and 64
    twiddles; 2, 7 and 8 output primes per workgroup."""
    e = Env(log_n, SMALL_N_BITS, seed=70 + log_n)
    try:
        ch = e.chain(1)
        for L in (1, 6, 7):
            d = e.level(L)
            for count, fmt in ((1, 0), (3, 1)):
                got, stats = run_switch(ch, d, count, fmt)
                check_grouping(stats, 1, 1, L)
                for i in range(count):
                    assert np.array_equal(got[i], d.switch_key(i)), (L, count, i)
    finally:
        e.close()


def test_switch_key_integer_kernel():
    """The integer kernel (MHE_FP=0) at N = 2^12 with one group: one sweep, 7 and 8 primes through the ring."""
    e = Env(12, SMALL_N_BITS, seed=77)
    try:
        ch = make_chain(12, SMALL_N_BITS, {"MHE_FP": "0", "MHE_KS_COLGROUPS": "1"}, 77)
        e.chains[1] = ch
        for L in (6, 7):
            d = e.level(L)
            got, stats = run_switch(ch, d, 2, 0)
            check_grouping(stats, 1, 1, L)
            for i in range(2):
                assert np.array_equal(got[i], d.switch_key(i)), (L, i)
    finally:
        e.close()


def test_switch_key_mixed_60bit_special():
    """A 60-bit special prime at N = 2^16, L = 6, one group: the FP64 sweeps for the data primes, then
    the integer sweep for the special prime, the last of the ring's order."""
    e = Env(16, MIX_BITS, seed=76)
    try:
        ch, L = e.chain(1), 6
        d = e.level(L)
        got, stats = run_switch(ch, d, 2, 1)
        check_grouping(stats, 1, 1, L)
        for i in range(2):
            assert np.array_equal(got[i], d.switch_key(i)), f"entry {i}"
    finally:
        e.close()
