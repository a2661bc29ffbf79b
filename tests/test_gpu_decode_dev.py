"""Device decode (mhe_ckks_decode_dev) and decrypt (mhe_decrypt) against the CPU oracle.

Decode compares double for double (np.array_equal) with oracle.Context.decode on every word-count
class of the composition kernel (limbs 1, 2, 3, 7, 12, 20, 33 -> 1, 2, 4, 8, 16, 32, 64 words), with no
register head (N = 2^12), the shortest (N = 2^13) and the longest one plus several LDS blocks
(N = 2^16), at sparse_slots 1, 16 and n/2.  Random residues are not a valid encoding: their CRT value
is uniform in [0, Q), so both sign branches and both sides of every per-word comparison occur.  The
crafted coefficients sit where the threshold, the zero-word skip and the negative branch's per-word
comparison can go wrong.  Decrypt compares word for word with tests/ckks_helpers.decrypt."""
import numpy as np
import pytest
import torch

import ckks_helpers as H
import mhe
import oracle as O
from test_gpu_parity import MIXED_BITS, SMALL_BITS, Chain

pytestmark = pytest.mark.gpu

NARROW20_BITS = [30 + i % 11 for i in range(20)] + [40]  # 20 data limbs of 30..40 bits: Q has 11 words of 20
NARROW33_BITS = [30] * 33 + [40]  # 33 data limbs, the 64-word class, with Q < 2^990 still a finite double
CHAINS = {
    "small12": (12, SMALL_BITS),
    "narrow20": (12, NARROW20_BITS),
    "narrow33": (12, NARROW33_BITS),
    "small13": (13, SMALL_BITS),
    "two16": (16, [51, 46, 51]),
    "mixed14": (14, MIXED_BITS),
}


@pytest.fixture(scope="module")
def chains():
    """One chain per name, made on first use and shared."""
    made = {}

    def get(name):
        if name not in made:
            log_n, bits = CHAINS[name]
            made[name] = Chain(log_n, bits, seed=500 + list(CHAINS).index(name))
        return made[name]

    return get


SHAPES = [("small12", 1), ("small12", 2), ("small12", 3), ("small12", 7), ("narrow20", 20), ("narrow33", 12),
          ("narrow33", 33), ("small13", 3), ("two16", 2)]


@pytest.mark.parametrize("name,limbs", SHAPES, ids=[f"{n}-L{l}" for n, l in SHAPES])
def test_decode_dev_random_residues(chains, name, limbs):
    ch = chains(name)
    rng = np.random.default_rng(limbs + 17 * ch.log_n)
    pt = np.stack([rng.integers(0, ch.moduli[l], size=ch.n, dtype=np.uint64) for l in range(limbs)])
    dpt = ch.up(pt)
    scale = 2.0 ** 30
    for sparse in (1, 16, ch.n // 2):
        got = ch.eng.decode_dev(dpt, scale, sparse_slots=sparse)
        assert got.is_cuda and got.dtype == torch.complex128 and got.shape == (sparse,)
        ref = ch.oc.decode(pt, scale, sparse_slots=sparse)
        assert np.array_equal(got.cpu().numpy(), ref), (name, limbs, sparse)
    assert np.array_equal(mhe.Engine.to_host(dpt), pt)  # the plaintext itself is left alone


def crafted_values(moduli):
    """Python integers in [0, Q) at the conversion's edges (Q = product of `moduli`, 3 words)."""
    Q = 1
    for q in moduli:
        Q *= q
    assert 2 ** 128 < Q < 2 ** 192
    w = 2 ** 64
    q0, q1, q2 = Q % w, (Q >> 64) % w, Q >> 128
    vals = [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2, (Q + 1) // 2 + 1, (Q - 1) // 2 - 1,
            w - 1, w, w + 1, Q - w, Q - w + 1, Q - w - 1, 2 ** 128, 2 ** 128 - 1, Q - 2 ** 128]
    # low word equal to Q's low word, in the positive and in the negative half
    vals += [q0, (1 << 64) + q0, (5 << 128) + (7 << 64) + q0, Q - (1 << 64), Q - (3 << 128), Q - (9 << 128) - (2 << 64)]
    # middle word equal to Q's middle word; top word equal to Q's top word
    vals += [(q1 << 64) + 5, ((q2 - 1) << 128) + (q1 << 64) + 12345, (q2 << 128) + 1, (q2 << 128) + (q1 << 64)]
    # zero middle word, zero low word, zero top word, in both halves
    vals += [(3 << 128) + 9, ((q2 - 1) << 128) + 9, (q2 << 128) + 9, 4 << 128, (q2 - 2) << 128, (q2 >> 1) << 128,
             (1 << 64) * 77, (q2 << 128) + (1 << 64)]
    # words on either side of Q's words in the negative half
    vals += [(q2 << 128) + ((q1 - 1) << 64) + (w - 1), ((q2 - 1) << 128) + ((w - 1) << 64) + (q0 + 1) % w,
             ((q2 - 1) << 128) + ((q1 + 1) % w << 64) + (q0 - 1)]
    assert all(0 <= v < Q for v in vals)
    return Q, vals


@pytest.mark.parametrize("sparse", [0, 256])
def test_decode_dev_crafted_coefficients(chains, sparse):
    ch = chains("small12")
    limbs = 3
    Q, vals = crafted_values(ch.moduli[:limbs])
    rng = np.random.default_rng(77)
    # every crafted value at several positions, the rest uniform in [0, Q); a sparse decode keeps
    # the coefficients at multiples of the sparsity, so each value also goes to one of those
    coeffs = [int.from_bytes(rng.bytes(24), "little") % Q for _ in range(ch.n)]
    for k in range(ch.n // 2):
        coeffs[(k * 37 + 11) % ch.n] = vals[k % len(vals)]
    sparsity = (ch.n // 2) // (sparse or ch.n // 2)
    assert len(vals) * sparsity <= ch.n
    for k, v in enumerate(vals):
        coeffs[k * sparsity] = v
    res = np.array([[c % q for c in coeffs] for q in ch.moduli[:limbs]], np.uint64)
    pt = ch.oc.ntt(res, O.NTT_FWD)
    scale = 2.0 ** 40
    # the construction does what it says: the oracle's FFT input is the centred value over the scale
    # (a few roundings of terms below Q / scale: absolute error below 2^-50 Q / scale)
    fft_in = ch.oc.decode_coeffs(pt, scale, sparse_slots=sparse)
    for k, v in enumerate(vals):
        want = v if v < (Q + 1) // 2 else v - Q
        assert abs(int(fft_in[k * sparsity] * scale) - want) <= Q >> 50, (k, v)
    got = ch.eng.decode_dev(ch.up(pt), scale, sparse_slots=sparse).cpu().numpy()
    assert np.array_equal(got, ch.oc.decode(pt, scale, sparse_slots=sparse))


def test_decode_equals_decode_dev(chains):
    ch = chains("small12")
    pt = ch.rand(3, ch.n)
    dpt = ch.up(pt)
    for sparse in (0, 16):
        dev = ch.eng.decode_dev(dpt, 2.0 ** 40, sparse_slots=sparse)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.complex128
        host = ch.eng.decode(dpt, 2.0 ** 40, sparse_slots=sparse)
        assert isinstance(host, np.ndarray)
        assert np.array_equal(host, dev.cpu().numpy())
        out = torch.empty(sparse or ch.n // 2, dtype=torch.complex128, device=dev.device)
        assert ch.eng.decode_dev(dpt, 2.0 ** 40, sparse_slots=sparse, out=out) is out
        assert torch.equal(out, dev)


def test_decode_scale_errors(chains):
    ch = chains("small12")
    limbs = 2
    dpt = ch.up(ch.rand(limbs, ch.n))
    tb = ch.oc.total_bits(limbs)
    for fn in (ch.eng.decode, ch.eng.decode_dev):
        for scale in (0.0, -1.0, 2.0 ** tb, 2.0 ** (tb + 3)):
            with pytest.raises(mhe.MheError, match="scale out of bounds") as ei:
                fn(dpt, scale)
            assert ei.value.code == -1
        fn(dpt, 2.0 ** (tb - 1))  # the largest scale SEAL accepts


@pytest.mark.parametrize("name", ["small12", "mixed14"])
@pytest.mark.parametrize("size", [2, 3])
def test_decrypt(chains, name, size):
    ch = chains(name)
    keys = H.Keys()
    keys.s = ch.rand(ch.K, ch.n)
    keys.s2 = ch.oc.dyadic(keys.s, keys.s)
    dsk = ch.up(keys.s)
    for L in (1, ch.K - 1):
        ct = ch.rand(size, L, ch.n)
        want = H.decrypt(ch.oc, keys, ct)
        dct = ch.up(ct)
        assert np.array_equal(ch.down(ch.eng.decrypt(dct, dsk)), want), L
        assert np.array_equal(ch.down(dct), ct)
        # out aliasing ct[0]
        out = ch.eng.decrypt(dct, dsk, out=dct[0])
        assert out.data_ptr() == dct.data_ptr()
        got = ch.down(dct)
        assert np.array_equal(got[0], want), L
        assert np.array_equal(got[1:], ct[1:])


def test_decrypt_argument_errors(chains):
    ch = chains("small12")
    dsk = ch.up(ch.rand(ch.K, ch.n))
    with pytest.raises(mhe.MheError) as ei:
        ch.eng.decrypt(ch.up(ch.rand(1, 2, ch.n)), dsk)  # size 1
    assert ei.value.code == -1


def test_decrypt_op_counts(chains):
    """mhe_decrypt reports the op mix of the multiply_plain / add sequence it replaces."""
    import ctypes

    ch = chains("small12")
    L = 3
    dsk = ch.up(ch.rand(ch.K, ch.n))

    def counts(kind, reset):
        c = (ctypes.c_uint64 * 64)()
        assert mhe.lib().mhe_op_counts(ch.eng._h, kind, c, 64, reset) == 0
        return list(c)

    for size in (2, 3, 4):
        counts(mhe.OPK_MULPLAIN, 1), counts(mhe.OPK_ADDSUB, 1)
        ch.eng.decrypt(ch.up(ch.rand(size, L, ch.n)), dsk)
        mp, ad = counts(mhe.OPK_MULPLAIN, 0), counts(mhe.OPK_ADDSUB, 0)
        assert mp[L] == 2 * size - 3 and sum(mp) == mp[L]
        assert ad[L] == size - 1 and sum(ad) == ad[L]
