"""GPU parity of the trimmed ModUp column pass (csrc/ntt.h k_modup_col) and of what it hands to the
fused key MAC (k_ks_row_mac), bit for bit against the oracle.

The column pass lifts a digit without reducing it where the first butterfly allows (lazy output prime:
q_J <= 4 q_I; non-lazy: q_J <= 2 q_I), folds a lazy prime's exit reduction into its last stage when
q < 2^46, and leaves non-packed FP limbs as doubles for the fused MAC.  The main chain puts a prime in
every class at N = 2^16 -- 46-bit (lazy, packed, folded exit), 47-bit (lazy, packed, reduced exit),
48-bit (non-lazy, packed), 50- and 51-bit (non-lazy, doubles) -- and digit / output pairs on both sides
of both lift rules (46 against 48 and 50 against 51 bits sit next to the boundaries).  N = 2^13 and
2^12 cover the non-packed lazy slots of the other two kernel shapes, a 60-bit special prime the mixed
kernels, whose integer sweep is untouched.  The launch counters (mhe_ks_pair_stats) show that the
expected fused-MAC kernel ran, so nothing passes through a fallback."""
import gc

import numpy as np
import pytest
import torch

import mhe
from test_gpu_batch import hoisting, truncated
from test_gpu_parity import Chain
from test_ks_pair import expected_launches

pytestmark = pytest.mark.gpu

TRIM_BITS = [51, 46, 46, 47, 48, 50, 51] + [51]  # 7 data limbs + special
SMALL_N_BITS = [51, 46, 46] + [51]
MIX_BITS = [49, 46, 46, 47, 48, 50] + [60]        # 60-bit special prime: the mixed FP / integer kernels
LEVELS = [2, 4, 7]


class Data:
    """Per level L, made once and left unchanged: a key (limbs 0..L-1 and the special limb random), three
    operand pairs, three switch inputs; the oracle's results on first use."""

    def __init__(self, ch, L):
        self.ch, self.L = ch, L
        self.key = np.zeros((L, 2, ch.K, ch.n), np.uint64)
        for l in list(range(L)) + [ch.K - 1]:
            self.key[:, :, l, :] = ch.rng.integers(0, ch.moduli[l], size=(L, 2, ch.n), dtype=np.uint64)
        self.a = [ch.rand(2, L, ch.n) for _ in range(3)]
        self.b = [ch.rand(2, L, ch.n) for _ in range(3)]
        self.ct = [ch.rand(2, L, ch.n) for _ in range(3)]
        self.target = [ch.rand(L, ch.n) for _ in range(3)]
        self._hm, self._sk, self._dkey = {}, {}, {}

    def hmult(self, i):
        if i not in self._hm:
            self._hm[i] = self.ch.oc.hmult(self.a[i], self.b[i], self.key)
        return self._hm[i]

    def switch_key(self, i):
        if i not in self._sk:
            self._sk[i] = self.ch.oc.switch_key(self.ct[i], self.target[i], self.key)
        return self._sk[i]

    def dkey(self, fmt):
        """The level-truncated key on the device: fmt 0 SEAL's layout, 1 prepared (doubles)."""
        if fmt not in self._dkey:
            k = self.ch.up(truncated(self.key, self.L))
            self._dkey[fmt] = self.ch.eng.key_prepare(k, fmt) if fmt else k
        return self._dkey[fmt]


class Env:
    def __init__(self, log_n, bits, seed):
        self.ch = Chain(log_n, bits, seed=seed)
        self.levels = {}

    def level(self, L):
        if L not in self.levels:
            self.levels[L] = Data(self.ch, L)
        return self.levels[L]

    def close(self):
        self.levels.clear()
        self.ch.eng.close()
        gc.collect()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def env():
    e = Env(16, TRIM_BITS, seed=46)
    yield e
    e.close()


def test_chain_has_every_class(env):
    """The chain's primes are what the cases below rely on (a generator change would hollow them out)."""
    q = env.ch.moduli
    assert [int(x).bit_length() for x in q] == TRIM_BITS
    assert q[1] < 2**46 and q[2] < 2**46 and 2**46 < q[3] < 2**47 <= q[4] < 2**48 <= q[5] < 2**51
    # both sides of the lazy rule (q_J <= 4 q_I) and of the non-lazy one (q_J <= 2 q_I)
    assert any(qj <= 4 * q[1] for qj in q[:7]) and any(qj > 4 * q[1] for qj in q[:7])
    assert any(qj <= 2 * q[4] for qj in q[:7]) and any(qj > 2 * q[4] for qj in q[:7])
    # next to the boundaries: 48 against 46 bits just above 4 q_I, 51 against 50 bits just above 2 q_I
    assert 0 < q[4] - 4 * q[1] < 2**25 and 0 < q[0] - 2 * q[5] < 2**32


def run_switch(ch, d, count, fmt):
    cts = [ch.up(c) for c in d.ct[:count]]
    ch.eng.ks_pair_stats(reset=True)
    ch.eng.switch_key_batch(cts, [ch.up(t) for t in d.target[:count]], [d.dkey(fmt)] * count)
    got = [ch.down(c) for c in cts]
    stats = ch.eng.ks_pair_stats(reset=True)
    return got, stats


@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("L", LEVELS)
def test_switch_key_batch(env, L, count):
    """One entry (the one-entry MAC), two (paired) and three (paired and an odd one); the prepared key
    at L = 2 and 7, SEAL's layout at L = 4."""
    ch, d = env.ch, env.level(L)
    got, stats = run_switch(ch, d, count, 0 if L == 4 else 1)
    assert stats == expected_launches(count)
    for i in range(count):
        assert np.array_equal(got[i], d.switch_key(i)), f"entry {i}"


@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("L", LEVELS)
def test_hmult_batch(env, L, count):
    """The fused HMult tail behind the same two kernels; SEAL's key layout at L = 2 and 7, prepared at 4."""
    ch, d = env.ch, env.level(L)
    dk = d.dkey(1 if L == 4 else 0)
    ch.eng.ks_pair_stats(reset=True)
    outs = ch.eng.hmult_batch([ch.up(x) for x in d.a[:count]], [ch.up(x) for x in d.b[:count]], dk)
    got = [ch.down(o) for o in outs]
    assert ch.eng.ks_pair_stats(reset=True) == expected_launches(count)
    for i in range(count):
        assert np.array_equal(got[i], d.hmult(i)), f"entry {i}"


@pytest.mark.parametrize("L", LEVELS)
def test_hoisted_rotation_batch(env, L):
    """One input rotated three ways: the hoisted path's shared ModUp runs the same column pass with
    canonical output (its row pass reads u64 words), so the unreduced lifts alone; the engine's own check
    recomputes every rotation by the classic path, whose column pass hands doubles to the fused MAC."""
    ch, d = env.ch, env.level(L)
    ct = d.ct[0]
    elts = [mhe.galois_elt_from_step(ch.log_n, s) for s in (1, -3, 64)]
    src = ch.up(ct)
    with hoisting(ch.eng, len(elts)):
        outs = ch.eng.apply_galois_batch([src] * len(elts), elts, [d.dkey(1)] * len(elts))
    for j, elt in enumerate(elts):
        assert np.array_equal(ch.down(outs[j]), ch.oc.apply_galois(ct, elt, d.key)), f"rotation {j}"


@pytest.mark.parametrize("fill", ["zero", "max"])
def test_extreme_limbs(env, fill):
    """Every residue 0, and every residue q - 1 (ciphertext, target and key): the largest unreduced lifts."""
    ch, L = env.ch, 7
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
    ch.eng.ks_pair_stats(reset=True)
    ch.eng.switch_key_batch(cts, [ch.up(target)] * 2, [dk] * 2)
    got = [ch.down(c) for c in cts]
    assert ch.eng.ks_pair_stats(reset=True) == (1, 0)
    want = ch.oc.switch_key(ct, target, key)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)


@pytest.mark.parametrize("log_n", [13, 12])
def test_switch_key_small_n(log_n):
    """N = 2^13 and 2^12: the other two shapes of both kernels, where a lazy prime's limb is not packed
    and leaves as the double of its centred residue.  One entry per workgroup below N = 2^16."""
    e = Env(log_n, SMALL_N_BITS, seed=50 + log_n)
    try:
        ch = e.ch
        for L in (1, 2, 3):
            d = e.level(L)
            for count, fmt in ((1, 0), (3, 1)):
                got, stats = run_switch(ch, d, count, fmt)
                assert stats == (0, 1)
                for i in range(count):
                    assert np.array_equal(got[i], d.switch_key(i)), (L, count, i)
    finally:
        e.close()


def test_switch_key_mixed_60bit_special():
    """A 60-bit special prime at N = 2^16: FP64 sweeps for the data primes (doubles and packed limbs as
    above), the integer sweep and the integer MAC for the special prime, canonical words as before."""
    e = Env(16, MIX_BITS, seed=60)
    try:
        ch, L = e.ch, 6
        d = e.level(L)
        got, stats = run_switch(ch, d, 2, 1)
        assert stats == (0, 1)  # the mixed kernel runs one entry per workgroup
        for i in range(2):
            assert np.array_equal(got[i], d.switch_key(i)), f"entry {i}"
    finally:
        e.close()
