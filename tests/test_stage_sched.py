"""GPU parity of the scheduled reduction of x in the non-lazy FP64 forward stages (csrc/fparith.h,
"Scheduled reduction of x"), bit for bit against the oracle.

The non-lazy sweep of the ModUp column pass (csrc/ntt.h k_modup_col) and the non-lazy row stages of the
fused key MAC (k_ks_row_mac) reduce x in every second stage only, and the doubles the first hands to the
second are within 2.46q instead of 2q + 1.  The chain's data primes are 51, 46, 51, 48, 50 and 51 bits
with a 51-bit special prime: a non-lazy prime is entered by a reduced lift (the 46-bit digit, and 51
bits into 48 or 50) and by an unreduced one (51 into 51, 50 into 51, 48 into 50), the 48-bit prime is
non-lazy and packed at N = 2^16, and the 46-bit prime keeps the lazy sweep beside them.  N = 2^16, 2^13
and 2^12 are the three shapes of both kernels (column passes of 8, 7 and 6 stages, row passes of 8, 6
and 6).  A chain with a 60-bit special prime runs the mixed kernels, whose integer sweep is untouched.
The launch counters (mhe_ks_pair_stats) show which fused-MAC kernel ran."""
import numpy as np
import pytest

from test_gpu_batch import truncated
from test_ks_pair import expected_launches
from test_modup_stream import Env, dkey

pytestmark = pytest.mark.gpu

SCHED_BITS = [51, 46, 51, 48, 50, 51] + [51]
MIX_BITS = [49, 46, 48, 50] + [60]
LEVELS = [2, 3, 6]
GROUPS = [1, None]  # MHE_KS_COLGROUPS; None: unset, the library's rule
FILLS = ["max", "zero", "alternating"]


@pytest.fixture(scope="module")
def env():
    e = Env(16, SCHED_BITS, seed=91)
    yield e
    e.close()


def launches(ch, count):
    """(paired, single) fused-MAC launches of `count` shared-key entries: pairs at N = 2^16 only."""
    return expected_launches(count) if ch.log_n == 16 else (0, 1)


def run_switch(ch, d, count, fmt):
    cts = [ch.up(c) for c in d.ct[:count]]
    dk = dkey(ch, d, fmt)
    ch.eng.ks_pair_stats(reset=True)
    ch.eng.switch_key_batch(cts, [ch.up(t) for t in d.target[:count]], [dk] * count)
    got = [ch.down(c) for c in cts]
    return got, ch.eng.ks_pair_stats(reset=True)


def run_hmult(ch, d, fmt):
    dk = dkey(ch, d, fmt)
    ch.eng.ks_pair_stats(reset=True)
    outs = ch.eng.hmult_batch([ch.up(x) for x in d.a], [ch.up(x) for x in d.b], dk)
    got = [ch.down(o) for o in outs]
    return got, ch.eng.ks_pair_stats(reset=True)


def filled(ch, fill, shape, limbs):
    """Limbs that are all q - 1, all 0, or 0 and q - 1 in turn along the coefficients."""
    q = np.array(ch.moduli, np.uint64)
    out = np.zeros(shape, np.uint64)
    for k, l in enumerate(limbs):
        if fill == "max":
            out[..., k, :] = q[l] - np.uint64(1)
        elif fill == "alternating":
            out[..., k, 1::2] = q[l] - np.uint64(1)
    return out


def check_extremes(ch, oc, L, fill, paired):
    """Two entries of extreme limbs in the ciphertext, the target and the key."""
    ct, target = filled(ch, fill, (2, L, ch.n), range(L)), filled(ch, fill, (L, ch.n), range(L))
    key = filled(ch, fill, (L, 2, ch.K, ch.n), range(ch.K))
    dk = ch.eng.key_prepare(ch.up(truncated(key, L)), 1)
    cts = [ch.up(ct), ch.up(ct)]
    ch.eng.ks_pair_stats(reset=True)
    ch.eng.switch_key_batch(cts, [ch.up(target)] * 2, [dk] * 2)
    got = [ch.down(c) for c in cts]
    assert ch.eng.ks_pair_stats(reset=True) == paired
    want = oc.switch_key(ct, target, key)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want), fill


def test_chain_has_every_class(env):
    """The chain's primes are what the cases below rely on (a generator change would hollow them out)."""
    q = [int(x) for x in env.ch.moduli]
    assert [x.bit_length() for x in q] == SCHED_BITS
    assert len(set(q)) == len(q)
    full = [x for x in q[:6] if x >= 2**47]
    assert len(full) == 5 and q[1] < 2**46 and 2**47 <= q[3] < 2**48
    # both lift rules into a non-lazy prime: q_J <= 2 q_I enters as it stands, q_J > 2 q_I reduced
    for qi in full:
        others = [x for x in q[:6] if x != qi]
        assert any(qj <= 2 * qi for qj in others)
    assert any(qj > 2 * q[3] for qj in q[:6]) and any(qj > 2 * q[4] for qj in q[:6])
    assert any(q[4] < qj <= 2 * q[4] for qj in q[:6])  # an unreduced lift above the output prime itself


@pytest.mark.parametrize("groups", GROUPS, ids=lambda g: f"groups{g}")
@pytest.mark.parametrize("count", [1, 2, 3])
@pytest.mark.parametrize("L", LEVELS)
def test_switch_key_batch(env, L, count, groups):
    """One entry (the one-entry MAC), two (paired) and three (a pair and the one-entry kernel); SEAL's key
    layout at L = 3, the prepared key at the other levels."""
    ch, d = env.chain(groups), env.level(L)
    got, stats = run_switch(ch, d, count, 0 if L == 3 else 1)
    assert stats == expected_launches(count)
    for i in range(count):
        assert np.array_equal(got[i], d.switch_key(i)), f"entry {i}"


@pytest.mark.parametrize("groups", GROUPS, ids=lambda g: f"groups{g}")
@pytest.mark.parametrize("L", LEVELS)
def test_hmult_batch(env, L, groups):
    """Two HMults behind the same two kernels; the prepared key at L = 3, SEAL's layout elsewhere."""
    ch, d = env.chain(groups), env.level(L)
    got, stats = run_hmult(ch, d, 1 if L == 3 else 0)
    assert stats == expected_launches(2)
    for i in range(2):
        assert np.array_equal(got[i], d.hmult(i)), f"entry {i}"


@pytest.mark.parametrize("groups", GROUPS, ids=lambda g: f"groups{g}")
@pytest.mark.parametrize("fill", FILLS)
def test_extreme_limbs(env, fill, groups):
    """Every residue q - 1 (the largest lifts and the largest products), every residue 0, and the two in
    turn, at L = 6."""
    check_extremes(env.chain(groups), env.ch.oc, 6, fill, (1, 0))


@pytest.mark.parametrize("groups", GROUPS, ids=lambda g: f"groups{g}")
@pytest.mark.parametrize("log_n", [13, 12])
def test_small_n(log_n, groups):
    """N = 2^13 and 2^12: column passes of 7 stages (the first one reduces) and of 6, row passes of 6; no
    limb is packed, so every non-lazy limb crosses as a double.  One entry per workgroup."""
    e = Env(log_n, SCHED_BITS, seed=90 + log_n)
    try:
        ch = e.chain(groups)
        for L in LEVELS:
            d = e.level(L)
            for count in (1, 2, 3):
                got, stats = run_switch(ch, d, count, 0 if L == 3 else 1)
                assert stats == launches(ch, count)
                for i in range(count):
                    assert np.array_equal(got[i], d.switch_key(i)), (L, count, i)
            got, stats = run_hmult(ch, d, 1 if L == 3 else 0)
            assert stats == launches(ch, 2)
            for i in range(2):
                assert np.array_equal(got[i], d.hmult(i)), (L, i)
        for fill in FILLS:
            check_extremes(ch, ch.oc, 6, fill, (0, 1))
    finally:
        e.close()


@pytest.mark.parametrize("groups", GROUPS, ids=lambda g: f"groups{g}")
def test_mixed_60bit_special(groups):
    """A 60-bit special prime at N = 2^16: the mixed kernels.  Their FP64 sweeps follow the same schedule;
    the integer sweep and the integer MAC of the special prime are as they were."""
    e = Env(16, MIX_BITS, seed=96)
    try:
        ch = e.chain(groups)
        for L in (2, 3, 4):
            d = e.level(L)
            for count in (1, 2, 3):
                got, stats = run_switch(ch, d, count, 0 if L == 3 else 1)
                assert stats == (0, 1)  # the mixed kernel runs one entry per workgroup
                for i in range(count):
                    assert np.array_equal(got[i], d.switch_key(i)), (L, count, i)
            got, stats = run_hmult(ch, d, 1 if L == 3 else 0)
            assert stats == (0, 1)
            for i in range(2):
                assert np.array_equal(got[i], d.hmult(i)), (L, i)
        for fill in FILLS:
            check_extremes(ch, ch.oc, 4, fill, (0, 1))
    finally:
        e.close()
