"""GPU parity of the merged elementwise launches (include/mhe.h mhe_launch_run): same-shaped
descriptors run as one k_elem_b / k_copy16_b launch of up to 8 entries, whose scalar table is built
on the host.  Every kind and op, merged and one by one, must give the words of the oracle's
single-operation restatement (oracle/oracle.py); so must the single launches that had no bit-exact
test: mhe_multiply_plain_add (k_mulplain_add) and mhe_set_scalar (k_scalar op 2).  Every comparison
is np.array_equal.  No hook is set: the tests build the descriptors themselves."""
import numpy as np
import pytest

import mhe
from test_gpu_parity import SMALL_BITS, Chain, _variant_chain

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 8, 11]  # one by one; merged; one full merged launch; 8 + 3
MHE_ERR_ARG = -1        # include/mhe.h


@pytest.fixture(scope="module")
def small():
    return Chain(12, SMALL_BITS, seed=31)


def edged(ch, x):
    """Residues 0 and q - 1 in every limb (slots 0 and 1), as test_elementwise_products_both_paths."""
    qs = np.array(ch.moduli[:x.shape[-2]], np.uint64)
    x[..., 0] = 0
    x[..., 1] = qs - np.uint64(1)
    return x


def scalar_ref(ch, a, s, op):
    """Per-limb scalar multiply (0) / add (1) / set (2) in Python integers."""
    out = np.empty_like(a)
    for l in range(a.shape[-2]):
        q = ch.moduli[l]
        if op == 2:
            out[..., l, :] = np.uint64(s[l])
        else:
            x = a[..., l, :].astype(object)
            out[..., l, :] = ((x * s[l] if op == 0 else x + s[l]) % q).astype(np.uint64)
    return out


def rand_scalars(ch, L):
    """One scalar per limb; the edge values 0 and q - 1 in the first two limbs."""
    s = [int(ch.rng.integers(0, q)) for q in ch.moduli[:L]]
    s[0] = 0
    if L > 1:
        s[1] = ch.moduli[1] - 1
    return s


def desc(ch, kind, op=0, a=None, b=None, out=None, polys=0, limbs=0, nbytes=0, scalars=()):
    d = mhe.Launch(kind=kind, op=op, polys=polys, limbs=limbs, bytes=nbytes, rc=-1)
    d.a = a.data_ptr() if a is not None else None
    d.b = b.data_ptr() if b is not None else None
    d.out = out.data_ptr() if out is not None else None
    for i, s in enumerate(scalars):
        d.scalars[i] = s
    d.stream = ch.eng.stream()
    return d


class Case:
    """One descriptor with its operands kept alive, its output tensor and the oracle's words."""

    def __init__(self, ch, name, L, scalars=None):
        oc, n = ch.oc, ch.n
        self.ch, self.name = ch, name
        a, b = edged(ch, ch.rand(2, L, n)), edged(ch, ch.rand(2, L, n))
        pt = edged(ch, ch.rand(L, n))
        self.keep = [ch.up(a), ch.up(b), ch.up(pt)]
        da, db, dpt = self.keep
        self.out = ch.eng.empty(2, L, n)
        k = dict(polys=2, limbs=L)
        if name in ("add", "sub", "negate"):
            op = ("add", "sub", "negate").index(name)
            self.want = (oc.add(a, b), oc.sub(a, b), oc.negate(a))[op]
            self.d = desc(ch, mhe.LK_ADDSUB, op, da, None if op == 2 else db, self.out, **k)
        elif name == "multiply_plain":
            self.want = oc.multiply_plain(a, pt)
            self.d = desc(ch, mhe.LK_MULPLAIN, 0, da, dpt, self.out, **k)
        elif name == "multiply_plain_add":
            self.out = ch.up(b)  # out is the accumulator
            self.want = oc.add(b, oc.multiply_plain(a, pt))
            self.d = desc(ch, mhe.LK_MULPLAIN_ADD, 0, da, dpt, self.out, **k)
        elif name in ("scalar_multiply", "scalar_add", "scalar_set"):
            op = ("scalar_multiply", "scalar_add", "scalar_set").index(name)
            s = rand_scalars(ch, L) if scalars is None else scalars
            self.want = scalar_ref(ch, a, s, op)
            self.out.fill_(-1)
            self.d = desc(ch, mhe.LK_SCALAR, op, None if op == 2 else da, None, self.out, scalars=s, **k)
        elif name in ("tensor_multiply", "tensor_square"):
            sq = name == "tensor_square"
            self.out = ch.eng.empty(3, L, n)
            self.want = oc.square(a) if sq else oc.multiply(a, b)
            self.d = desc(ch, mhe.LK_TENSOR, int(sq), da, None if sq else db, self.out, **k)
        else:
            raise ValueError(name)

    def check(self, tag=""):
        assert self.d.rc == 0, (self.name, tag, self.d.rc)
        assert np.array_equal(self.ch.down(self.out), self.want), (self.name, tag)


KINDS = ["add", "sub", "negate", "multiply_plain", "multiply_plain_add", "scalar_multiply", "scalar_add",
         "scalar_set", "tensor_multiply", "tensor_square"]


# ----------------------------------------------------------------------------- single launches
@pytest.mark.parametrize("env", [{}, {"MHE_FP": "0"}], ids=["fp64", "integer"])
def test_multiply_plain_add_and_set_scalar(env):
    """k_mulplain_add as a single launch == add(acc, multiply_plain(ct, pt)); k_scalar op 2 == a
    broadcast of the residues; FP64 and integer products, residues 0 and q - 1 included."""
    ch = _variant_chain(env, 33)
    for L in (1, ch.K - 1):
        ct, acc = edged(ch, ch.rand(2, L, ch.n)), edged(ch, ch.rand(2, L, ch.n))
        pt = edged(ch, ch.rand(L, ch.n))
        got = ch.down(ch.eng.multiply_plain_add(ch.up(ct), ch.up(pt), ch.up(acc)))
        assert np.array_equal(got, ch.oc.add(acc, ch.oc.multiply_plain(ct, pt))), L
        s = rand_scalars(ch, L)
        for polys in (1, 2, 3):
            out = ch.eng.empty(polys, L, ch.n)
            out.fill_(-1)
            got = ch.down(ch.eng.set_scalar(s, polys, L, out=out))
            want = np.broadcast_to(np.array(s, np.uint64)[None, :, None], (polys, L, ch.n))
            assert np.array_equal(got, want), (L, polys)


# ----------------------------------------------------------------- every kind and op, merged
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", KINDS)
def test_launch_run_every_kind(small, name, count):
    """`count` same-shaped descriptors with distinct operands: 1 runs one by one, 3 and 8 as one
    merged launch, 11 as 8 + 3.  Scalar descriptors merge only with equal scalar tables, so they
    share one."""
    ch = small
    L = ch.K - 1
    s = rand_scalars(ch, L)
    cases = [Case(ch, name, L, scalars=s) for _ in range(count)]
    assert ch.eng.launch_run([c.d for c in cases]) == 0
    for i, c in enumerate(cases):
        c.check(i)


@pytest.mark.parametrize("env", [{"MHE_FP": "0"}], ids=["integer"])
def test_launch_run_products_integer(env):
    """k_elem_b's integer products (fp = 0): the three product kinds merged, 3 descriptors each."""
    ch = _variant_chain(env, 34)
    L = ch.K - 1
    cases = [Case(ch, name, L) for name in ("multiply_plain", "multiply_plain_add", "tensor_multiply", "tensor_square")
             for _ in range(3)]
    assert ch.eng.launch_run([c.d for c in cases]) == 0
    for i, c in enumerate(cases):
        c.check(i)


@pytest.mark.parametrize("count", COUNTS)
def test_launch_run_copy(small, count):
    """k_copy16_b: `count` copies of a byte count that is a multiple of 16 (and not of 4096: the
    grid-stride tail), nothing written past the end."""
    ch = small
    words = 3 * ch.n + 6
    srcs = [ch.rand(1, 4, ch.n).reshape(-1) for _ in range(count)]
    dsrc = [ch.up(x) for x in srcs]
    outs = [ch.eng.empty(4 * ch.n) for _ in range(count)]
    for o in outs:
        o.fill_(-1)
    ds = [desc(ch, mhe.LK_COPY, a=a, out=o, nbytes=8 * words) for a, o in zip(dsrc, outs)]
    assert ch.eng.launch_run(ds) == 0
    for d, x, o in zip(ds, srcs, outs):
        got = ch.down(o)
        assert d.rc == 0
        assert np.array_equal(got[:words], x[:words])
        assert (got[words:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


def test_launch_run_copy_unaligned_size(small):
    """A byte count that is no multiple of 16 cannot use 16-byte copies: the descriptors run one by
    one and copy exactly their bytes."""
    ch = small
    words = ch.n + 3  # 8 * words % 16 == 8
    srcs = [ch.rand(1, 2, ch.n).reshape(-1) for _ in range(3)]
    dsrc = [ch.up(x) for x in srcs]
    outs = [ch.eng.empty(2 * ch.n) for _ in range(3)]
    for o in outs:
        o.fill_(-1)
    ds = [desc(ch, mhe.LK_COPY, a=a, out=o, nbytes=8 * words) for a, o in zip(dsrc, outs)]
    assert (8 * words) % 16 != 0
    assert ch.eng.launch_run(ds) == 0
    for d, x, o in zip(ds, srcs, outs):
        got = ch.down(o)
        assert d.rc == 0
        assert np.array_equal(got[:words], x[:words])
        assert (got[words:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


# ------------------------------------------------------------------------------- mixed list
def test_launch_run_mixed_shapes(small):
    """Interleaved descriptors that same_shape must keep apart: scalar multiplies at two levels,
    with two scalar tables that differ in one limb only, and adds in between.  Each group of equal
    shape merges on its own; every output is right."""
    ch = small
    La, Lb = ch.K - 1, 3
    s1 = rand_scalars(ch, La)
    s2 = list(s1)
    s2[La - 1] = (s2[La - 1] + 1) % ch.moduli[La - 1]  # differs from s1 in the last limb only
    assert sum(x != y for x, y in zip(s1, s2)) == 1
    cases = []
    for _ in range(3):
        cases.append(Case(ch, "scalar_multiply", La, scalars=s1))
        cases.append(Case(ch, "add", La))
        cases.append(Case(ch, "scalar_multiply", La, scalars=s2))
        cases.append(Case(ch, "scalar_multiply", Lb, scalars=s1[:Lb]))
    assert ch.eng.launch_run([c.d for c in cases]) == 0
    for i, c in enumerate(cases):
        c.check(i)


# ------------------------------------------------------------------------- invalid descriptor
def test_launch_run_rejects_out_of_range_scalar_table(small):
    """Three scalar multiplies that would merge share a table whose first scalar is q_0: each gets the
    rc of mhe_multiply_scalar (MHE_ERR_ARG) and takes part in no launch, so its output keeps the
    sentinel; the valid add of the same call runs."""
    ch = small
    L = ch.K - 1
    s = rand_scalars(ch, L)
    bad = [Case(ch, "scalar_multiply", L, scalars=s) for _ in range(3)]
    for c in bad:
        c.d.scalars[0] = ch.moduli[0]  # the shared table, now out of range in limb 0
        c.out.fill_(-1)
    good = Case(ch, "add", L)
    assert ch.eng.launch_run([bad[0].d, good.d, bad[1].d, bad[2].d]) == MHE_ERR_ARG
    for c in bad:
        assert c.d.rc == MHE_ERR_ARG
        assert (ch.down(c.out) == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    good.check()


# ------------------------------------------------------------------------------- op counts
@pytest.mark.parametrize("B", [3, 8])
def test_launch_run_op_counts(small, B):
    """A merged run of B multiply_plain_add descriptors counts B * polys products and B * polys adds
    at its level, as B single calls would."""
    ch = small
    L = 5
    cases = [Case(ch, "multiply_plain_add", L) for _ in range(B)]
    ch.eng.op_counts(mhe.OPK_MULPLAIN, reset=True)
    ch.eng.op_counts(mhe.OPK_ADDSUB, reset=True)
    assert ch.eng.launch_run([c.d for c in cases]) == 0
    mul, add = ch.eng.op_counts(mhe.OPK_MULPLAIN, reset=True), ch.eng.op_counts(mhe.OPK_ADDSUB, reset=True)
    want = [0] * (ch.K + 1)
    want[L] = 2 * B
    assert mul == want and add == want
    for c in cases:
        c.check()
