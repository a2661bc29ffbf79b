"""GPU parity of mhe_prng_uniform_batch (csrc/sample.hip k_uni_bulk, k_uni_redraw): sample_poly_uniform
with its rejected words ordered and redrawn on the device, word for word against the oracle's
sample_poly_uniform(Blake2xbPRNG(seed)).  SEAL's own primes never reject, so the redraw path runs on
chains of primes just above 1.5 * 2^60 (keygen_ref.chain), and every test recomputes the reject counts
from the PRNG's bytes and asserts them against mhe_keygen_stats: a silent skip of the path fails."""
import numpy as np
import pytest

import mhe
import oracle as O
from keygen_ref import chain, heavy_primes, public_seed, redraw_counts, seed_of

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


def useed(i):
    """The uniform stream of bootstrap seed i, as a key digit draws it."""
    return public_seed(seed_of(i))


class Setup:
    def __init__(self, log_n, moduli):
        self.log_n, self.n, self.moduli = log_n, 1 << log_n, moduli
        self.oc = O.Context(log_n, moduli)
        self.eng = mhe.Engine(log_n, moduli)
        self.refs, self.counts = {}, {}

    def ref(self, seed, limbs):
        key = (tuple(seed), limbs)
        if key not in self.refs:
            r = self.oc.sample(seed, "uniform", limbs)
            r.setflags(write=False)
            self.refs[key] = r
            self.counts[key] = redraw_counts(seed, self.moduli[:limbs], self.n)
        return self.refs[key]

    def check(self, seeds, limbs, slots=None):
        """Runs the batch; compares the kept limbs with the oracle's and the redrawn-word total with
        the count recomputed from the stream.  Returns (rejects per limb, tail re-rejections) per seed."""
        self.eng.keygen_stats(reset=True)
        outs = self.eng.prng_uniform_batch(seeds, limbs, slot_of_limb=slots)
        stats = self.eng.keygen_stats()
        kept = [l for l in range(limbs) if slots is None or slots[l] >= 0]
        for i, seed in enumerate(seeds):
            want = self.ref(seed, limbs)[kept]
            got = mhe.Engine.to_host(outs[i])
            assert np.array_equal(got, want), f"entry {i} of {len(seeds)}: {(got != want).sum()} words differ"
        counts = [self.counts[(tuple(s), limbs)] for s in seeds]
        # entries and launch groups count mhe_encrypt_sk_batch only
        assert stats == (0, 0, sum(sum(c[0]) for c in counts), 0)
        return counts


@pytest.fixture(scope="module")
def setups():
    made = {}

    def get(log_n, name):
        if (log_n, name) not in made:
            moduli = heavy_primes(log_n, 18) if name == "H18" else chain(name, log_n)
            made[(log_n, name)] = Setup(log_n, moduli)
        return made[(log_n, name)]

    yield get
    for s in made.values():
        s.eng.close()


@pytest.mark.parametrize("count", [1, 3, 8, 9])
@pytest.mark.parametrize("name", ["H4", "MIX"])
def test_heavy_chains(setups, name, count):
    """Bootstrap seeds 0..3: H4 rejects 205-277 words per limb and 56-72 tail words again; MIX rejects
    on limbs 1 and 3 only (236-277, 216-256) and 26-42 tail words.  9 entries run in two groups."""
    s = setups(12, name)
    counts = s.check([useed(i) for i in range(count)], 4)
    for per_limb, again in counts[:4]:
        if name == "H4":
            assert all(205 <= c <= 277 for c in per_limb) and 56 <= again <= 72
        else:
            assert per_limb[0] == per_limb[2] == 0
            assert 236 <= per_limb[1] <= 277 and 216 <= per_limb[3] <= 256 and 26 <= again <= 42


def test_seal_primes(setups):
    """No reject: the redraw workgroups return at once."""
    s = setups(12, "SEAL")
    counts = s.check([useed(i) for i in range(3)], 4)
    assert all(sum(c[0]) == 0 for c in counts)
    s.check([useed(0)], 2)


def test_unkept_limb_consumes_tail(setups):
    """Limb 2 is dropped (slot -1): its rejects still consume tail words, so limb 3 matches."""
    s = setups(12, "H4")
    s.check([useed(0), useed(1)], 4, slots=[0, 1, -1, 2])
    s.check([useed(2)], 4, slots=[-1, -1, -1, 0])


def test_past_the_old_cap(setups):
    """N = 2^16 over 18 heavy limbs: about 74 k rejects, more than the 65536 of the host-walk path."""
    s = setups(16, "H18")
    (per_limb, again), = s.check([useed(0)], 18)
    assert sum(per_limb) > 65536 and again > 0


@pytest.mark.parametrize("log_n", [13, 14, 15])
def test_ring_degrees(setups, log_n):
    s = setups(log_n, "H4")
    counts = s.check([useed(0), useed(1)], 4)
    assert all(min(c[0]) > 0 and c[1] > 0 for c in counts)


def test_overflow_writes_nothing_beyond_the_buffer(setups):
    """The redraw buffer limited to 100 words (mhe_debug_keygen_cap) against about 1000 rejects per
    entry: the accepted bulk words and the first 100 redraws, in stream order, are the oracle's, every
    later rejected slot keeps what it held, both entries are counted as overflowed, and the next call
    without the limit is whole again."""
    s = setups(12, "H4")
    cap, seeds = 100, [useed(0), useed(1)]
    outs = [s.eng.empty(4, s.n) for _ in seeds]
    for o in outs:
        o.fill_(7)
    s.eng.keygen_stats(reset=True)
    s.eng.debug_keygen_cap(cap)
    try:
        s.eng.prng_uniform_batch(seeds, 4, outs=outs)
        stats = s.eng.keygen_stats()
    finally:
        s.eng.debug_keygen_cap(0)
    total = 0
    for seed, o in zip(seeds, outs):
        want = np.array(s.ref(seed, 4))
        bulk = np.frombuffer(O.prng_bytes(seed, 4 * s.n * 8), dtype=np.uint64).reshape(4, s.n)
        mm = np.array([M64 - (M64 % int(q)) - 1 for q in s.moduli], dtype=np.uint64)[:, None]
        rejected = np.argwhere(bulk >= mm)  # row-major: stream order
        total += len(rejected)
        assert len(rejected) > 8 * cap
        for l, i in rejected[cap:]:
            want[l, i] = 7
        assert np.array_equal(mhe.Engine.to_host(o), want)
    assert stats == (0, 0, total, 2)
    s.check(seeds, 4)


def test_rejected_arguments(setups):
    s = setups(12, "H4")
    o = s.eng.empty(4, s.n)
    o.fill_(7)
    s.eng.synchronize()
    for kw in (dict(limbs=0), dict(limbs=65), dict(limbs=4, prime_of_limb=[0, 1, 2, 4]),
               dict(limbs=4, slot_of_limb=[0, 1, 2, -2])):
        with pytest.raises(mhe.MheError):
            s.eng.prng_uniform_batch([useed(0)], outs=[o], **kw)
    s.eng.synchronize()
    assert bool((o == 7).all())
