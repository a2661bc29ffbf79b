"""Shared by the key-generation tests: the prime chains whose uniform samples reject often, and the
reject counts of sample_poly_uniform (util/rlwe.cpp:136-162) recomputed from the PRNG's bytes."""
import numpy as np

import oracle as O

M64 = (1 << 64) - 1
FP_BITS = [50, 40, 40, 50]     # every prime below 2^51: the FP64 passes and epilogue
MIXED_BITS = [50, 40, 40, 60]  # a 60-bit special prime: every plain pass integer


def seed_of(i):
    return [1000 + i, 2, 3, 4, 5, 6, 7, 8]


def public_seed(seed):
    """The seed of a's PRNG in encrypt_zero_symmetric: the first 64 bytes of the bootstrap stream
    (rlwe.cpp:317-318)."""
    return [int(w) for w in np.frombuffer(O.prng_bytes(seed, 64), dtype=np.uint64)]


def heavy_primes(log_n, count):
    """NTT primes just above 1.5 * 2^60 (tests/test_sample.py): 2^64 mod q ~ 0.67 q, so about one
    word in 16 is redrawn.  SEAL's own primes never reject in practice."""
    out, q = [], (3 << 59) + 1
    while len(out) < count:
        if O.is_prime(q):
            out.append(q)
        q += 2 << log_n
    return out


def chain(name, log_n=12):
    """H4: the first four heavy primes.  MIX: [S0, H0, S1, H1] with S SEAL's [50, 40, 40, 50] chain."""
    h = heavy_primes(log_n, 4)
    if name == "H4":
        return h
    s = O.coeff_modulus_create(1 << log_n, FP_BITS)
    return {"MIX": [s[0], h[0], s[1], h[1]], "SEAL": s}[name]


def max_multiple(q):
    return M64 - (M64 % int(q)) - 1


def redraw_counts(seed, moduli, n):
    """(rejected bulk words per limb, tail words rejected again) of sample_poly_uniform(Blake2xbPRNG(seed))
    over `moduli`: a rejected word is redrawn, in index order, from the words after the bulk, and a tail
    word at or above the consuming limb's max_multiple is skipped."""
    limbs = len(moduli)
    mm = [max_multiple(q) for q in moduli]
    bulk = np.frombuffer(O.prng_bytes(seed, limbs * n * 8), dtype=np.uint64).reshape(limbs, n)
    per_limb = [int((bulk[l] >= np.uint64(mm[l])).sum()) for l in range(limbs)]
    total = sum(per_limb)
    if not total:
        return per_limb, 0
    # four times the expected need is far beyond what the walk below consumes
    tail = np.frombuffer(O.prng_bytes(seed, (limbs * n + 4 * total + 64) * 8), dtype=np.uint64)[limbs * n:]
    t = again = 0
    for l in range(limbs):
        for _ in range(per_limb[l]):
            while int(tail[t]) >= mm[l]:
                t += 1
                again += 1
            t += 1
    return per_limb, again
