"""Argument errors of the batched entry points (include/mhe.h): a table of (entry point, bad
argument) against (return code, mhe_last_error text).  Every check runs before the first launch, so
after a rejected call every operand and output holds the bytes it held before.  Where two checks fail
at once the table pins which one is reported.

N = 2^12 on the small chain at L = 3 limbs.  All ciphertext operands are slots of one device arena
(a slot is one 2-poly ciphertext, 2 * L * n words), so "overlapping by one word" is a pointer one
word before the end of a slot, and "unchanged" is one comparison of the arena with its snapshot.
The calls go through ctypes (mhe.lib()): the Engine methods cannot pass a null entry or a
key_limbs that differs from the key's shape."""
import ctypes

import pytest
import torch

import mhe
from test_gpu_parity import SMALL_BITS, Chain

pytestmark = pytest.mark.gpu

ARG, RANGE = -1, -3  # MHE_ERR_ARG, MHE_ERR_RANGE
L = 3

M_ELT = "Galois element is not valid"
M_KEY = "kswitch_keys is not valid for encryption parameters"
M_GKEY = "Galois key not present"
M_SAME = "result cannot point to the same value as operand"
M_INV = "invalid argument"
M_TARGET = "target_iter"
M_ENC = "encrypted is not valid for encryption parameters"
M_ALIAS = "rescale output must not alias its input"
M_DISTINCT = "outputs must be distinct"
M_OTHER = "result cannot point to the same value as another entry's operand"
M_CHAIN = "end of modulus switching chain reached"


class Setup:
    def __init__(self):
        self.ch = ch = Chain(12, SMALL_BITS, seed=31)
        self.eng, self.n, self.K = ch.eng, ch.n, ch.K
        self.ps = L * ch.n  # words of one poly
        # residues below 2^40: valid under every prime of the chain, so an accepted call computes
        self.arena = ch.up(ch.rng.integers(0, 1 << 40, size=12 * 2 * self.ps, dtype="uint64"))
        self.key = ch.up(ch.rand_key())
        self.snap = self.arena.clone()
        self.key_snap = self.key.clone()
        self.elts = [mhe.galois_elt_from_step(ch.log_n, s) for s in (1, 2, 3)]

    def slot(self, k, words=0):
        """Address of word `words` of slot k."""
        return self.arena.data_ptr() + 8 * (k * 2 * self.ps + words)

    def slots(self, *ks):
        return [self.slot(k) for k in ks]

    def unchanged(self):
        self.eng.synchronize()
        return torch.equal(self.arena, self.snap) and torch.equal(self.key, self.key_snap)

    def defaults(self, entry):
        """A valid argument set of 3 entries: operands in slots 0 .. 5, outputs from slot 6."""
        kp, K = self.key.data_ptr(), self.K
        if entry == "apply_galois_batch":
            return dict(inp=self.slots(0, 1, 2), out=self.slots(6, 7, 8), elts=list(self.elts), keys=[kp] * 3,
                        kl=[K] * 3, limbs=L)
        if entry == "rotate_sum":
            return dict(inp=self.slots(0, 1, 2), elts=list(self.elts), keys=[kp] * 3, kl=[K] * 3, group=[0, 0, 1],
                        groups=2, out=self.slots(6, 7), accumulate=0, limbs=L)
        if entry == "switch_key_batch":
            return dict(ct=self.slots(0, 1, 2), target=self.slots(3, 4, 5), keys=[kp] * 3, kl=[K] * 3, limbs=L)
        if entry == "rescale_batch":
            return dict(inp=self.slots(0, 1, 2), out=self.slots(6, 7, 8), size=2, limbs=L)
        if entry == "hmult_batch":
            return dict(a=self.slots(0, 1, 2), b=self.slots(3, 4, 5), key=kp, kl=K, out=self.slots(6, 7, 8), limbs=L)
        raise KeyError(entry)

    def call(self, entry, a):
        """The entry point on argument set a: (return code, mhe_last_error text)."""
        lib, h, st = mhe.lib(), self.eng._h, self.eng.stream()
        # a list as a C array (None in a pointer list: a null entry; None for the list: a null list)
        arr = lambda t, v: None if v is None else (t * len(v))(*v)  # noqa: E731
        ptrs = lambda v: arr(ctypes.c_void_p, v)  # noqa: E731
        ints = lambda v: arr(ctypes.c_int, v)  # noqa: E731
        u32s = lambda v: arr(ctypes.c_uint32, v)  # noqa: E731
        if entry == "apply_galois_batch":
            rc = lib.mhe_apply_galois_batch(h, len(a["inp"]), ptrs(a["inp"]), ptrs(a["out"]), u32s(a["elts"]),
                                            ptrs(a["keys"]), ints(a["kl"]), a["limbs"], st)
        elif entry == "rotate_sum":
            rc = lib.mhe_rotate_sum(h, len(a["inp"]), ptrs(a["inp"]), u32s(a["elts"]), ptrs(a["keys"]), ints(a["kl"]),
                                    ints(a["group"]), a["groups"], ptrs(a["out"]), a["accumulate"], a["limbs"], st)
        elif entry == "switch_key_batch":
            rc = lib.mhe_switch_key_batch(h, len(a["ct"]), ptrs(a["ct"]), ptrs(a["target"]), ptrs(a["keys"]),
                                          ints(a["kl"]), a["limbs"], st)
        elif entry == "rescale_batch":
            rc = lib.mhe_rescale_batch(h, len(a["inp"]), ptrs(a["inp"]), ptrs(a["out"]), a["size"], a["limbs"], st)
        else:
            rc = lib.mhe_hmult_batch(h, len(a["a"]), ptrs(a["a"]), ptrs(a["b"]), a["key"], a["kl"], ptrs(a["out"]),
                                     a["limbs"], st)
        return rc, lib.mhe_last_error().decode()


@pytest.fixture(scope="module")
def setup():
    return Setup()


def put(field, i, value):
    """A change of one argument: a[field][i] = value (value may be a function of the Setup)."""

    def apply(s, a):
        a[field][i] = value(s) if callable(value) else value

    return apply


def whole(field, value):
    def apply(s, a):
        a[field] = value(s) if callable(value) else value

    return apply


# the last word of slot k: a 2-poly range from there covers that word and most of slot k + 1
def tail(k):
    return lambda s: s.slot(k, 2 * s.ps - 1)


# the last word of the [2][L-1][n] output that starts at slot k (rescale / hmult outputs)
def tail_low(k):
    return lambda s: s.slot(k, 2 * (L - 1) * s.n - 1)


# (entry point, what is wrong, changes to a valid argument set, return code, message)
TABLE = [
    # ---------------------------------------------------------------- mhe_apply_galois_batch
    ("apply_galois_batch", "even element", [put("elts", 1, 4)], ARG, M_ELT),
    ("apply_galois_batch", "element = 2N + 1", [put("elts", 2, lambda s: 2 * s.n + 1)], ARG, M_ELT),
    ("apply_galois_batch", "key_limbs = limbs", [put("kl", 1, L)], ARG, M_KEY),
    ("apply_galois_batch", "key_limbs = K + 1", [put("kl", 2, lambda s: s.K + 1)], ARG, M_KEY),
    ("apply_galois_batch", "null input", [put("inp", 1, None)], ARG, M_GKEY),
    ("apply_galois_batch", "null output", [put("out", 2, None)], ARG, M_GKEY),
    ("apply_galois_batch", "null key", [put("keys", 0, None)], ARG, M_GKEY),
    ("apply_galois_batch", "null list", [whole("elts", lambda s: None)], ARG, M_INV),
    # out[1] starts at the last word of input 2
    ("apply_galois_batch", "output overlaps an input by one word", [put("out", 1, tail(2))], ARG, M_SAME),
    ("apply_galois_batch", "output is its own input", [put("out", 0, lambda s: s.slot(0))], ARG, M_SAME),
    # out[2] starts at the last word of out[0] (slot 6) and ends before out[1]'s successor
    ("apply_galois_batch", "two outputs overlap by one word", [put("out", 1, lambda s: s.slot(9)),
                                                               put("out", 2, tail(6))], ARG, M_SAME),
    # entries are checked one after the other, each one's element, key and output together: entry 0's
    # overlap is reported, not entry 1's element
    ("apply_galois_batch", "entry 0 overlaps and entry 1 has an even element",
     [put("out", 0, tail(1)), put("elts", 1, 6)], ARG, M_SAME),
    # within one entry: null, then element, then key_limbs, then overlap
    ("apply_galois_batch", "one entry: even element and key_limbs = limbs and overlap",
     [put("elts", 1, 6), put("kl", 1, L), put("out", 1, tail(0))], ARG, M_ELT),
    ("apply_galois_batch", "one entry: key_limbs = K + 1 and overlap",
     [put("kl", 0, lambda s: s.K + 1), put("out", 0, tail(1))], ARG, M_KEY),
    ("apply_galois_batch", "limbs = K", [whole("limbs", lambda s: s.K)], ARG, M_ENC),
    # ------------------------------------------------------------------------ mhe_rotate_sum
    ("rotate_sum", "even element", [put("elts", 0, 2)], ARG, M_ELT),
    ("rotate_sum", "element = 2N + 1", [put("elts", 2, lambda s: 2 * s.n + 1)], ARG, M_ELT),
    ("rotate_sum", "key_limbs = limbs", [put("kl", 2, L)], ARG, M_KEY),
    ("rotate_sum", "key_limbs = K + 1", [put("kl", 0, lambda s: s.K + 1)], ARG, M_KEY),
    ("rotate_sum", "null input", [put("inp", 2, None)], ARG, M_GKEY),
    ("rotate_sum", "null key", [put("keys", 1, None)], ARG, M_GKEY),
    ("rotate_sum", "null output", [put("out", 1, None)], ARG, M_GKEY),
    ("rotate_sum", "output overlaps an input by one word", [put("out", 1, tail(0))], ARG, M_SAME),
    ("rotate_sum", "two outputs overlap by one word", [put("out", 1, tail(6))], ARG, M_SAME),
    ("rotate_sum", "a gap in group[]", [whole("group", [0, 0, 2]), whole("groups", 3),
                                        whole("out", lambda s: s.slots(6, 7, 8))], ARG, M_INV),
    ("rotate_sum", "group[] decreasing", [whole("group", [0, 1, 0])], ARG, M_INV),
    ("rotate_sum", "group[] not starting at 0", [whole("group", [1, 1, 1])], ARG, M_INV),
    ("rotate_sum", "groups != last group + 1", [whole("groups", 3), whole("out", lambda s: s.slots(6, 7, 8))], ARG,
     M_INV),
    # the groups are checked before the outputs, every rotation before any overlap
    ("rotate_sum", "a gap in group[] and a null output", [whole("group", [0, 2, 2]), put("out", 0, None)], ARG, M_INV),
    ("rotate_sum", "null output and even element", [put("out", 0, None), put("elts", 0, 2)], ARG, M_GKEY),
    ("rotate_sum", "output 0 overlaps an input and entry 2 has an even element",
     [put("out", 0, tail(1)), put("elts", 2, 8)], ARG, M_ELT),
    ("rotate_sum", "output 0 overlaps an input and entry 2 has key_limbs = limbs",
     [put("out", 0, tail(1)), put("kl", 2, L)], ARG, M_KEY),
    # ------------------------------------------------------------------ mhe_switch_key_batch
    ("switch_key_batch", "key_limbs = limbs", [put("kl", 0, L)], ARG, M_KEY),
    ("switch_key_batch", "key_limbs = K + 1", [put("kl", 2, lambda s: s.K + 1)], ARG, M_KEY),
    ("switch_key_batch", "null ciphertext", [put("ct", 1, None)], ARG, M_TARGET),
    ("switch_key_batch", "null target", [put("target", 2, None)], ARG, M_TARGET),
    ("switch_key_batch", "null key", [put("keys", 0, None)], ARG, M_TARGET),
    ("switch_key_batch", "null list", [whole("kl", lambda s: None)], ARG, M_INV),
    ("switch_key_batch", "entry 0 has key_limbs = limbs and entry 1 is null", [put("kl", 0, L), put("ct", 1, None)],
     ARG, M_KEY),
    ("switch_key_batch", "entry 0 is null and has key_limbs = limbs", [put("kl", 0, L), put("keys", 0, None)], ARG,
     M_TARGET),
    # --------------------------------------------------------------------- mhe_rescale_batch
    ("rescale_batch", "null input", [put("inp", 1, None)], ARG, M_ENC),
    ("rescale_batch", "null output", [put("out", 0, None)], ARG, M_ENC),
    ("rescale_batch", "output overlaps an input by one word", [put("out", 2, tail(1))], ARG, M_ALIAS),
    ("rescale_batch", "output is its own input", [put("out", 1, lambda s: s.slot(1))], ARG, M_ALIAS),
    ("rescale_batch", "two outputs overlap by one word", [put("out", 1, tail_low(6))], ARG, M_ALIAS),
    ("rescale_batch", "limbs = 1", [whole("limbs", 1)], RANGE, M_CHAIN),
    ("rescale_batch", "size = 4", [whole("size", 4)], ARG, M_ENC),
    ("rescale_batch", "entry 0 overlaps and entry 1 is null", [put("out", 0, tail(1)), put("inp", 1, None)], ARG,
     M_ALIAS),
    # ----------------------------------------------------------------------- mhe_hmult_batch
    ("hmult_batch", "key_limbs = limbs", [whole("kl", L)], ARG, M_KEY),
    ("hmult_batch", "key_limbs = K + 1", [whole("kl", lambda s: s.K + 1)], ARG, M_KEY),
    ("hmult_batch", "null operand", [put("b", 1, None)], ARG, M_INV),
    ("hmult_batch", "null output", [put("out", 2, None)], ARG, M_INV),
    ("hmult_batch", "null key", [whole("key", None)], ARG, M_INV),
    ("hmult_batch", "output overlaps another entry's operand by one word", [put("out", 0, tail(1))], ARG, M_OTHER),
    ("hmult_batch", "output is another entry's operand", [put("out", 1, lambda s: s.slot(5))], ARG, M_OTHER),
    ("hmult_batch", "two outputs overlap by one word", [put("out", 1, tail_low(6))], ARG, M_DISTINCT),
    ("hmult_batch", "limbs = 1", [whole("limbs", 1)], ARG, M_ENC),
    # the key before the entries; for one output, the other entries in order, each one's output
    # before its operands
    ("hmult_batch", "key_limbs = limbs and a null operand", [whole("kl", L), put("a", 0, None)], ARG, M_KEY),
    ("hmult_batch", "output 1 overlaps entry 0's operand and entry 2's output",
     [put("out", 1, tail(0)), put("out", 2, lambda s: s.slot(1, 8))], ARG, M_OTHER),
    ("hmult_batch", "output 0 overlaps entry 1's output and entry 2's operand",
     [put("out", 0, tail(1)), put("out", 1, lambda s: s.slot(2, 8))], ARG, M_DISTINCT),
]


@pytest.mark.parametrize("entry,what,changes,rc,msg", TABLE, ids=[f"{t[0]}-{t[1]}".replace(" ", "_") for t in TABLE])
def test_batch_argument_errors(setup, entry, what, changes, rc, msg):
    a = setup.defaults(entry)
    for change in changes:
        change(setup, a)
    got = setup.call(entry, a)
    print(f"{entry}: {what}: {got}")
    assert got == (rc, msg)
    assert setup.unchanged(), "a rejected call wrote to an operand or an output"


def test_valid_argument_sets_are_accepted(setup):
    """The table's starting points are valid: each entry point accepts its defaults (so every row
    fails for the one reason it names)."""
    s = setup
    for entry in ("apply_galois_batch", "rotate_sum", "switch_key_batch", "rescale_batch", "hmult_batch"):
        assert s.call(entry, s.defaults(entry))[0] == 0, entry
    s.eng.synchronize()
    s.arena.copy_(s.snap)


def test_hmult_batch_output_may_overlap_its_own_operands(setup):
    """out[i] on a[i] or on b[i] is accepted and gives the words of separate outputs: the tensor
    product has consumed an entry's operands before its tail writes."""
    s = setup
    ow = 2 * (L - 1) * s.n

    def run(out_slots):
        a = s.defaults("hmult_batch")
        a["out"] = s.slots(*out_slots)
        assert s.call("hmult_batch", a)[0] == 0
        s.eng.synchronize()
        got = [s.arena[k * 2 * s.ps:k * 2 * s.ps + ow].clone() for k in out_slots]
        s.arena.copy_(s.snap)
        return got

    want = run((6, 7, 8))
    got = run((0, 4, 8))  # on a[0], on b[1], apart
    for g, w in zip(got, want):
        assert torch.equal(g, w)
