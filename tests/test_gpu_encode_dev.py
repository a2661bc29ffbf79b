"""Batched device encode (mhe_ckks_encode_dev / Engine.encode_dev) against the CPU oracle, word for
word (np.array_equal, no tolerance), and against the host entry Engine.encode on the same values.

Shapes: N = 2^12 (no FFT tail: the last stage and the maximum in the block kernel), 2^13 (tail<1>,
two blocks), 2^14 (tail<2>), 2^15 (tail<3>), 2^16 (tail<4>, 16 blocks).  Entry counts on both sides
of a round of 8.  The size check is driven to both sides of its threshold with constant vectors
whose coefficient 0 is 2^(tb-2) (1 -+ 2^-20): max_bits = tb - 1 (accepted) and tb (rejected)."""
import ctypes

import numpy as np
import pytest
import torch

import mhe
from test_gpu_parity import MIXED_BITS, SMALL_BITS, Chain

pytestmark = pytest.mark.gpu

CHAINS = {
    "small12": (12, SMALL_BITS),
    "small13": (13, SMALL_BITS),
    "small14": (14, SMALL_BITS),
    "small15": (15, SMALL_BITS),
    "two16": (16, [51, 46, 51]),
    "mixed14": (14, MIXED_BITS),
}
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def chains():
    """One chain per name, made on first use and shared."""
    made = {}

    def get(name):
        if name not in made:
            log_n, bits = CHAINS[name]
            made[name] = Chain(log_n, bits, seed=700 + list(CHAINS).index(name))
        return made[name]

    return get


def vectors(rng, B, count, cplx, amp=1.0):
    """B distinct vectors of `count` values."""
    vs = [rng.uniform(-amp, amp, count) for _ in range(B)]
    if cplx:
        vs = [v + 1j * rng.uniform(-amp, amp, count) for v in vs]
    return vs


def dev(ch, v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(ch.eng.torch_device)


def sentinel_out(ch, B, limbs):
    return torch.full((B, limbs, ch.n), SENTINEL, dtype=torch.int64, device=ch.eng.torch_device)


def reference(ch, vs, scale, limbs, bound_limbs=None):
    return np.stack([ch.oc.encode(v, scale, bound_limbs or limbs)[:limbs] for v in vs])


def run(ch, vs, scale, limbs, **kw):
    """encode_dev of host vectors -> (words [B, limbs, n], status [B] or None); the device copies of
    the values must come back unchanged."""
    dvs = [dev(ch, v) for v in vs]
    out, status = ch.eng.encode_dev(dvs, scale, limbs, **kw)
    assert out.shape == (len(vs), limbs, ch.n) or kw.get("out") is not None
    got = ch.down(out)
    for d, v in zip(dvs, vs):
        assert np.array_equal(d.cpu().numpy(), v, equal_nan=True)  # inputs untouched
    return got, None if status is None else status.cpu().numpy()


SHAPES = [("small12", 2, 2), ("small13", 3, 2), ("small14", 3, 2), ("small15", 2, 2), ("two16", 2, 3)]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("name,limbs,B", SHAPES, ids=[s[0] for s in SHAPES])
def test_every_fft_shape(chains, name, limbs, B, cplx):
    ch = chains(name)
    vs = vectors(np.random.default_rng(ch.log_n + 100 * cplx), B, ch.n // 2, cplx)
    scale = 2.0 ** 40
    got, status = run(ch, vs, scale, limbs)
    assert status.dtype == np.int32 and np.array_equal(status, np.zeros(B, np.int32))
    assert np.array_equal(got, reference(ch, vs, scale, limbs))
    for b, v in enumerate(vs):
        assert np.array_equal(got[b], ch.down(ch.eng.encode(v, scale, limbs))), b


@pytest.mark.parametrize("B", [1, 3, 8, 9, 17])
def test_entry_counts(chains, B):
    """One round, a full round, rounds with a remainder; every entry has its own data."""
    ch = chains("small12")
    vs = vectors(np.random.default_rng(B), B, ch.n // 2, B % 2 == 1)
    got, status = run(ch, vs, 2.0 ** 46, 3)
    assert np.array_equal(status, np.zeros(B, np.int32))
    assert np.array_equal(got, reference(ch, vs, 2.0 ** 46, 3))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("count", ["half", 37, 1, 0])
def test_input_kinds(chains, count, cplx):
    ch = chains("small13")
    count = ch.n // 2 if count == "half" else count
    vs = vectors(np.random.default_rng(count + 5), 3, count, cplx, amp=4.0)
    got, status = run(ch, vs, 2.0 ** 46, 2)
    assert np.array_equal(status, np.zeros(3, np.int32))
    assert np.array_equal(got, reference(ch, vs, 2.0 ** 46, 2))
    # one 2-D tensor instead of a list
    if count:
        out, _ = ch.eng.encode_dev(dev(ch, np.stack(vs)), 2.0 ** 46, 2)
        assert np.array_equal(ch.down(out), got)


def test_zero_count_with_null_pointers(chains):
    ch = chains("small12")
    B, limbs = 2, 2
    out = sentinel_out(ch, B, limbs)
    status = torch.full((B,), 7, dtype=torch.int32, device=out.device)
    rc = raw_call(ch, [None, None], 0, False, 2.0 ** 30, limbs, [out[b].data_ptr() for b in range(B)], status)
    assert rc == 0
    zero = ch.oc.encode(np.zeros(0), 2.0 ** 30, limbs)
    assert np.array_equal(ch.down(out), np.stack([zero, zero]))
    assert np.array_equal(status.cpu().numpy(), [0, 0])


def test_round_trip_from_decode_dev(chains):
    """decode_dev's complex128 tensor goes straight back into encode_dev: no host copy in between."""
    ch = chains("small12")
    rng = np.random.default_rng(9)
    z = rng.uniform(-1, 1, ch.n // 2) + 1j * rng.uniform(-1, 1, ch.n // 2)
    scale, limbs = 2.0 ** 40, 3
    slots = ch.eng.decode_dev(ch.up(ch.oc.encode(z, scale, limbs)), scale)
    assert slots.is_cuda and slots.dtype == torch.complex128
    out, status = ch.eng.encode_dev(slots, scale, limbs)
    assert out.shape == (1, limbs, ch.n)
    assert np.array_equal(ch.down(out)[0], ch.oc.encode(slots.cpu().numpy(), scale, limbs))
    assert np.array_equal(status.cpu().numpy(), [0])


@pytest.mark.parametrize("scale", [2.0 ** 20, 2.0 ** 70, 2.0 ** 140])
def test_coefficient_widths(chains, scale):
    """<= 64-bit, 128-bit and multi-word branches of the reduction, 7 limbs."""
    ch = chains("small12")
    vs = vectors(np.random.default_rng(41), 2, ch.n // 2, False)
    got, status = run(ch, vs, scale, ch.K - 1)
    assert np.array_equal(status, [0, 0])
    assert np.array_equal(got, reference(ch, vs, scale, ch.K - 1))


def test_bound_limbs_above_limbs(chains):
    """2^110 is too wide for 2 limbs (97 bits) but fits the first level's bound."""
    ch = chains("small12")
    vs = vectors(np.random.default_rng(43), 2, ch.n // 2, False)
    got, status = run(ch, vs, 2.0 ** 110, 2, bound_limbs=ch.K - 1)
    assert np.array_equal(status, [0, 0])
    assert np.array_equal(got, reference(ch, vs, 2.0 ** 110, 2, bound_limbs=ch.K - 1))
    with pytest.raises(mhe.MheError, match="scale out of bounds"):
        ch.eng.encode_dev([dev(ch, v) for v in vs], 2.0 ** 110, 2)


def test_integer_ntt_chain(chains):
    """The mixed chain (a 60-bit prime) runs the integer NTT."""
    ch = chains("mixed14")
    vs = vectors(np.random.default_rng(44), 3, ch.n // 2, True)
    got, status = run(ch, vs, 2.0 ** 40, ch.K - 1)
    assert np.array_equal(status, [0, 0, 0])
    assert np.array_equal(got, reference(ch, vs, 2.0 ** 40, ch.K - 1))


def edge_vectors(ch, limbs, scale):
    """(tb, accepted, rejected): full-slot constants on either side of the size check."""
    tb = ch.oc.total_bits(limbs)
    c = 2.0 ** (tb - 2) / scale
    lo = np.full(ch.n // 2, c * (1 - 2.0 ** -20))
    hi = np.full(ch.n // 2, c * (1 + 2.0 ** -20))
    ch.oc.encode(lo, scale, limbs)  # the oracle accepts
    with pytest.raises(ValueError, match="too large"):
        ch.oc.encode(hi, scale, limbs)
    return tb, lo, hi


# the third level has tb >= 258, where log2 rounds to tb - 2 on more than 64 ulps above 2^(tb-2)
@pytest.mark.parametrize("name,limbs,tb_want", [("small12", 2, 97), ("small13", 1, 51), ("small12", 7, 337)])
def test_size_check_both_sides(chains, name, limbs, tb_want):
    ch = chains(name)
    scale = 2.0 ** 30
    tb, lo, hi = edge_vectors(ch, limbs, scale)
    assert tb == tb_want
    other = np.random.default_rng(3).uniform(-1, 1, ch.n // 2)
    vs = [lo, hi, other]
    out = sentinel_out(ch, 3, limbs)
    status = torch.full((3,), 7, dtype=torch.int32, device=out.device)
    got, st = run(ch, vs, scale, limbs, out=out, status=status)
    assert np.array_equal(st, [0, 1, 0])
    assert np.array_equal(got[0], ch.oc.encode(lo, scale, limbs))
    assert np.array_equal(got[2], ch.oc.encode(other, scale, limbs))
    assert (got[1] == np.uint64(SENTINEL)).all()  # a rejected entry's output is not written
    # the same buffers again with acceptable values: no flag is left over
    vs2 = [other, lo, other * 0.5]
    got, st = run(ch, vs2, scale, limbs, out=out, status=status)
    assert np.array_equal(st, [0, 0, 0])
    assert np.array_equal(got, reference(ch, vs2, scale, limbs))


def test_l1_bounds(chains):
    ch = chains("small12")
    scale, limbs = 2.0 ** 40, 2
    vs = vectors(np.random.default_rng(12), 3, ch.n // 2, True)
    l1 = [float(np.abs(v.real).sum() + np.abs(v.imag).sum()) * (1 + 1e-9) for v in vs]
    want = reference(ch, vs, scale, limbs)
    for b in l1:
        assert mhe.lib().mhe_ckks_encode_l1_proves(ch.eng._h, scale, limbs, b) == 1
    # every bound sufficient: no status array is needed
    got, st = run(ch, vs, scale, limbs, l1_bounds=l1, status=False)
    assert st is None and np.array_equal(got, want)
    # one entry unknown and no status array: an argument error before any launch
    out = sentinel_out(ch, 3, limbs)
    for unknown in (None, -1.0, float("nan")):
        with pytest.raises(mhe.MheError, match="status_dev") as ei:
            ch.eng.encode_dev([dev(ch, v) for v in vs], scale, limbs, out=out, l1_bounds=[l1[0], unknown, l1[2]],
                              status=False)
        assert ei.value.code == -1
    assert (ch.down(out) == np.uint64(SENTINEL)).all()
    # a true bound that proves nothing: the device check accepts the entry
    assert mhe.lib().mhe_ckks_encode_l1_proves(ch.eng._h, scale, limbs, 1e30) == 0
    got, st = run(ch, vs, scale, limbs, l1_bounds=[l1[0], 1e30, None])
    assert np.array_equal(st, [0, 0, 0]) and np.array_equal(got, want)


def test_non_finite_values_are_rejected(chains):
    ch = chains("small13")
    scale, limbs = 2.0 ** 30, 2
    vs = vectors(np.random.default_rng(13), 3, ch.n // 2, False)
    vs[1][5] = np.inf
    out = sentinel_out(ch, 3, limbs)
    got, st = run(ch, vs, scale, limbs, out=out)
    assert np.array_equal(st, [0, 1, 0])
    assert np.array_equal(got[0], ch.oc.encode(vs[0], scale, limbs))
    assert np.array_equal(got[2], ch.oc.encode(vs[2], scale, limbs))
    assert (got[1] == np.uint64(SENTINEL)).all()


def raw_call(ch, dvs, count, cplx, scale, limbs, out_ptrs, status):
    B = len(out_ptrs)
    vals = (ctypes.c_void_p * B)(*[None if d is None else d.data_ptr() for d in dvs])
    outs = (ctypes.c_void_p * B)(*out_ptrs)
    return mhe.lib().mhe_ckks_encode_dev(ch.eng._h, ch.eng._encoder(), B, vals, count, 1 if cplx else 0, scale, limbs,
                                         limbs, outs, None, ctypes.c_void_p(status.data_ptr()), ch.eng.stream())


def test_argument_errors_come_before_any_launch(chains):
    ch = chains("small12")
    limbs = 2
    out = sentinel_out(ch, 2, limbs)
    status = torch.full((2,), 7, dtype=torch.int32, device=out.device)
    ok = [dev(ch, v) for v in vectors(np.random.default_rng(14), 2, ch.n // 2, False)]
    long = [dev(ch, np.zeros(ch.n // 2 + 1)) for _ in range(2)]
    with pytest.raises(mhe.MheError, match="values_size is too large"):
        ch.eng.encode_dev(long, 2.0 ** 20, limbs, out=out, status=status)
    with pytest.raises(mhe.MheError, match="scale out of bounds"):
        ch.eng.encode_dev(ok, 2.0 ** 400, limbs, out=out, status=status)
    # two equal output pointers; an output on top of an input
    for ptrs in ([out[0].data_ptr(), out[0].data_ptr()], [out[0].data_ptr(), ok[0].data_ptr()]):
        assert raw_call(ch, ok, ch.n // 2, False, 2.0 ** 20, limbs, ptrs, status) == -1
        assert b"alias" in mhe.lib().mhe_last_error()
    assert (ch.down(out) == np.uint64(SENTINEL)).all()
    assert np.array_equal(status.cpu().numpy(), [7, 7])
