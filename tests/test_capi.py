"""CPU-side checks of the C ABI boundary (no GPU compute): libmhe.so loads, exports every
entry point include/mhe.h declares, and its host-only helpers agree with the oracle/KATs."""
import ctypes
import json
import os
import re

import pytest

import mhe
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mhe.h")).read()
    return sorted(set(re.findall(r"\b(mhe_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(mhe.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    # and the Python binding binds exactly the declared surface
    assert set(mhe.SIGNATURES) == set(names)


def test_coeff_modulus_create_matches_oracle():
    for n, bits in [(1 << 16, [51] + [46] * 30 + [51] * 13 + [51]),
                    (1 << 16, [49] + [46] * 21 + [49] * 14 + [60]),
                    (1 << 12, [30, 40, 50, 60])]:
        assert mhe.coeff_modulus_create(n, bits) == O.coeff_modulus_create(n, bits)


def test_coeff_modulus_create_kats():
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "seal_kats.json")))["coeff_modulus_create"]
    for n, bits, want in kats["cases"]:
        assert mhe.coeff_modulus_create(n, bits) == want
    with pytest.raises(mhe.MheError):
        mhe.coeff_modulus_create(1 << 16, [61])


def test_galois_elt_from_step():
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "seal_kats.json")))["galois_elt_from_step"]
    for step, elt in kats["cases"]:
        assert mhe.galois_elt_from_step(kats["log_n"], step) == elt
    for step in (1, -1, 5, 1000, -32767, 0):
        assert mhe.galois_elt_from_step(16, step) == O.galois_elt_from_step(1 << 16, step)
    assert mhe.galois_elt_from_step(16, 1 << 15) == 0  # step count too large


NULL_CTX_ENTRY_POINTS = [
    "mhe_ntt_forward", "mhe_ntt_inverse", "mhe_add", "mhe_sub", "mhe_negate", "mhe_multiply_plain",
    "mhe_multiply_scalar", "mhe_add_scalar", "mhe_ct_multiply", "mhe_ct_square", "mhe_switch_key",
    "mhe_relinearize", "mhe_permute_galois", "mhe_apply_galois", "mhe_apply_galois_to", "mhe_rescale_to_next",
    "mhe_modraise", "mhe_mod_switch_drop"]

_NULL_CTX_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
kinds = {"p": ctypes.c_void_p, "i": ctypes.c_int, "u": ctypes.c_uint32}
for name, sig in json.loads(sys.argv[2]):
    f = getattr(lib, name)
    f.restype = ctypes.c_int
    f.argtypes = [kinds[k] for k in sig]
    rc = f(*[kinds[k](0) for k in sig])
    print(name, rc, flush=True)
"""


def test_null_context_is_an_argument_error():
    """Every entry point that traces its operands returns MHE_ERR_ARG for a null context (all other
    arguments zero / null) instead of reading through it.  A fresh child process that only loads the
    library: it never creates a context, so it opens no GPU, and a crash cannot take the suite down."""
    import subprocess
    import sys

    def code(t):
        return "i" if t is ctypes.c_int else "u" if t is ctypes.c_uint32 else "p"

    assert len(NULL_CTX_ENTRY_POINTS) == 18
    sigs = []
    for name in NULL_CTX_ENTRY_POINTS:
        res, args = mhe.SIGNATURES[name]
        assert res is ctypes.c_int
        sigs.append((name, "".join(code(t) for t in args)))
    p = subprocess.run([sys.executable, "-c", _NULL_CTX_CHILD, mhe.LIB_PATH, json.dumps(sigs)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    got = [line.split() for line in p.stdout.splitlines()]
    assert got == [[name, "-1"] for name in NULL_CTX_ENTRY_POINTS], (got, p.stderr)


def test_ctx_create_rejects_bad_chain_without_gpu_work():
    lib = mhe.lib()
    h = ctypes.c_void_p()
    bad = (ctypes.c_uint64 * 2)(12289, 15)  # 15 is not prime / not NTT friendly
    assert lib.mhe_ctx_create(ctypes.byref(h), 12, bad, 2, 0) == -1
    assert b"NTT-friendly" in lib.mhe_last_error()
    assert lib.mhe_ctx_create(ctypes.byref(h), 20, bad, 2, 0) == -1
