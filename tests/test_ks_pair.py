"""GPU parity of the paired fused key MAC (csrc/ntt.h k_ks_row_mac NE = 2): at N = 2^16 a batched
key switch whose entries share one key runs two entries per workgroup.  Every word must equal the
oracle's (and the one-entry kernel's), and the engine's launch counters (mhe_ks_pair_stats) must
show which kernel ran -- without them a parity test passes vacuously when the host code falls back.

The ResNet chain's low limbs are one 51-bit prime, then 46-bit primes, and a 51-bit special prime,
so lazy (q < 2^47) and non-lazy workgroups both run at small L."""
import gc
import os

import numpy as np
import pytest
import torch

import mhe
from test_gpu_batch import hoisting, truncated, with_zero_coeffs
from test_gpu_parity import RESNET_BITS, Chain

pytestmark = pytest.mark.gpu

MAXB = 8  # entries of one launch (MHE_MAXB): larger batches run in chunks of 8


@pytest.fixture(scope="module")
def ch():
    """The chain and its engine; at module teardown the per-level data (device keys among them) is
    dropped and the engine closed, so its workspaces (several GB at the key level) do not stay
    allocated under the tests that follow in the same process."""
    c = Chain(16, RESNET_BITS, seed=31)
    yield c
    _levels.clear()
    c.eng.close()
    gc.collect()
    torch.cuda.empty_cache()


def expected_launches(count):
    """(paired, single) fused-MAC launches of `count` shared-key entries: chunks of 8; a chunk of B >= 2
    runs its leading B - (B % 2) entries paired and an odd last entry through the one-entry kernel."""
    chunks = [min(MAXB, count - i) for i in range(0, count, MAXB)]
    return sum(1 for b in chunks if b >= 2), sum(1 for b in chunks if b % 2)


class LevelData:
    """Per level L, made once and left unchanged: a key with random limbs 0..L-1 and special limb (the
    only ones level L reads) in full shape for the oracle, 9 operand pairs, 9 switch inputs, and the
    oracle's results, computed on first use."""

    def __init__(self, ch, L):
        self.ch, self.L = ch, L
        self.key = np.zeros((L, 2, ch.K, ch.n), np.uint64)
        self.key[:, :, :L] = self._limbs(ch, L, range(L))
        self.key[:, :, -1:] = self._limbs(ch, L, [ch.K - 1])
        self.a = [ch.rand(2, L, ch.n) for _ in range(9)]
        self.b = [ch.rand(2, L, ch.n) for _ in range(9)]
        self.ct = [ch.rand(2, L, ch.n) for _ in range(8)]
        self.target = [ch.rand(L, ch.n) for _ in range(8)]
        self._hm, self._sk, self._dkey = {}, {}, {}

    @staticmethod
    def _limbs(ch, digits, limbs):
        out = np.empty((digits, 2, len(limbs), ch.n), np.uint64)
        for k, l in enumerate(limbs):
            out[:, :, k, :] = ch.rng.integers(0, ch.moduli[l], size=(digits, 2, ch.n), dtype=np.uint64)
        return out

    def b_of(self, i):
        return self.a[i] if i % 4 == 3 else self.b[i]  # every fourth entry a square

    def hmult(self, i):
        if i not in self._hm:
            self._hm[i] = self.ch.oc.hmult(self.a[i], self.b_of(i), self.key)
        return self._hm[i]

    def switch_key(self, i):
        if i not in self._sk:
            self._sk[i] = self.ch.oc.switch_key(self.ct[i], self.target[i], self.key)
        return self._sk[i]

    def dkey(self, fmt):
        """The level-truncated key on the device in format fmt (0: SEAL's layout, 1: doubles, 2: 48-bit planes)."""
        if fmt not in self._dkey:
            k = self.ch.up(truncated(self.key, self.L))
            self._dkey[fmt] = self.ch.eng.key_prepare(k, fmt) if fmt else k
        return self._dkey[fmt]


_levels = {}


def level(ch, L):
    if L not in _levels:
        _levels[L] = LevelData(ch, L)
    return _levels[L]


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["seal", "doubles", "planes48"])
@pytest.mark.parametrize("count", [2, 3, 8, 9])
@pytest.mark.parametrize("L", [2, 3, 6])
def test_hmult_batch_paired(ch, L, count, fmt):
    """hmult_batch with the shared relinearization key in each key format: L = 2 gives every data-prime
    workgroup one digit besides its own limb (the special prime two), L = 3 odd and even digit counts;
    counts 3 and 9 leave an odd entry to the one-entry kernel."""
    d = level(ch, L)
    dk = d.dkey(fmt)
    ups = [ch.up(x) for x in d.a[:count]]
    a = ups
    b = [ups[i] if i % 4 == 3 else ch.up(d.b[i]) for i in range(count)]
    ch.eng.ks_pair_stats(reset=True)
    outs = ch.eng.hmult_batch(a, b, dk)
    got = [ch.down(o) for o in outs]
    assert ch.eng.ks_pair_stats(reset=True) == expected_launches(count)
    for i in range(count):
        assert np.array_equal(got[i], d.hmult(i)), f"entry {i} vs oracle"
        assert np.array_equal(got[i], ch.down(ch.eng.hmult(a[i], b[i], dk))), f"entry {i} vs one-by-one hmult"
    assert ch.eng.ks_pair_stats(reset=True) == (0, count)  # one-by-one never pairs


@pytest.mark.parametrize("count", [2, 3, 8])
@pytest.mark.parametrize("L", [1, 2, 5])
def test_switch_key_batch_paired(ch, L, count):
    """switch_key_batch with one key: the epilogue without the fused rescale, and the special limbs'
    inverse rows inside the kernel; L = 1 is the nd == 0 edge of output prime 0."""
    d = level(ch, L)
    dk = d.dkey(1)
    cts = [ch.up(c) for c in d.ct[:count]]
    ch.eng.ks_pair_stats(reset=True)
    ch.eng.switch_key_batch(cts, [ch.up(t) for t in d.target[:count]], [dk] * count)
    got = [ch.down(c) for c in cts]
    paired, single = ch.eng.ks_pair_stats(reset=True)
    assert (paired, single) == expected_launches(count) and paired > 0
    for i in range(count):
        assert np.array_equal(got[i], d.switch_key(i)), f"entry {i}"


def test_switch_key_batch_unshared_key_stays_single(ch):
    """8 entries, one with a different key: no pairing, and still the oracle's words."""
    L = 3
    d = level(ch, L)
    other = d.key.copy()
    other[:, :, :L] = LevelData._limbs(ch, L, range(L))
    dks = [ch.up(truncated(other, L)) if i == 5 else d.dkey(1) for i in range(8)]
    cts = [ch.up(c) for c in d.ct]
    ch.eng.ks_pair_stats(reset=True)
    ch.eng.switch_key_batch(cts, [ch.up(t) for t in d.target], dks)
    got = [ch.down(c) for c in cts]
    assert ch.eng.ks_pair_stats(reset=True) == (0, 1)
    for i in range(8):
        want = ch.oc.switch_key(d.ct[i], d.target[i], other) if i == 5 else d.switch_key(i)
        assert np.array_equal(got[i], want), f"entry {i}"


def test_hmult_batch_paired_equals_single_entry_path(ch):
    """The same 8-entry call on an engine created under MHE_KS_PAIR=0 (the kept one-entry path)."""
    L = 6
    d = level(ch, L)
    saved = os.environ.get("MHE_KS_PAIR")
    os.environ["MHE_KS_PAIR"] = "0"  # read at context creation only
    try:
        single_eng = mhe.Engine(ch.log_n, ch.moduli)
    finally:
        if saved is None:
            del os.environ["MHE_KS_PAIR"]
        else:
            os.environ["MHE_KS_PAIR"] = saved
    try:
        outs = []
        for eng in (ch.eng, single_eng):
            a = [eng.to_device(x) for x in d.a[:8]]
            b = [a[i] if i % 4 == 3 else eng.to_device(d.b[i]) for i in range(8)]
            dk = eng.key_prepare(eng.to_device(truncated(d.key, L)), 1)
            eng.ks_pair_stats(reset=True)
            o = eng.hmult_batch(a, b, dk)
            eng.synchronize()
            outs.append([mhe.Engine.to_host(x) for x in o])
        assert ch.eng.ks_pair_stats(reset=True) == (1, 0)
        assert single_eng.ks_pair_stats(reset=True) == (0, 1)
    finally:
        single_eng.close()
    for i in range(8):
        assert np.array_equal(outs[0][i], outs[1][i]), f"entry {i}"


def test_hoisted_rotations_with_flags_stay_single(ch):
    """Hoisted rotations (two inputs, two steps each) whose entries all share one key: the classic fallback's launches carry
    run_if flags (one input has zero coefficients, so its flag is set and the fallback computes) and
    must keep the one-entry kernel; the engine's check finds no differing word."""
    L = 3
    d = level(ch, L)
    cts = [ch.rand(2, L, ch.n), with_zero_coeffs(ch, L, 2)]
    elts = [mhe.galois_elt_from_step(ch.log_n, s) for s in (1, 5)] * 2
    dk = d.dkey(1)
    ins = [ch.up(cts[0])] * 2 + [ch.up(cts[1])] * 2  # each input twice: the hoisted path
    ch.eng.ks_pair_stats(reset=True)
    with hoisting(ch.eng, 4):
        outs = ch.eng.apply_galois_batch(ins, elts, [dk] * 4)
    paired, single = ch.eng.ks_pair_stats(reset=True)
    assert paired == 0 and single >= 1, (paired, single)
    for j in range(4):
        assert np.array_equal(ch.down(outs[j]), ch.oc.apply_galois(cts[j // 2], elts[j], d.key)), f"entry {j}"
