"""CPU-side checks of the batched device encode entry points (no GPU compute): libmhe.so exports
mhe_ckks_encode_dev and mhe_ckks_encode_l1_proves, the Python binding declares them, and both
answer a null context with MHE_ERR_ARG."""
import ctypes
import json
import subprocess
import sys

import mhe

NEW_ENTRY_POINTS = ["mhe_ckks_encode_dev", "mhe_ckks_encode_l1_proves"]

_NULL_CTX_CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
kinds = {"p": ctypes.c_void_p, "i": ctypes.c_int, "d": ctypes.c_double, "z": ctypes.c_size_t}
for name, sig in json.loads(sys.argv[2]):
    f = getattr(lib, name)
    f.restype = ctypes.c_int
    f.argtypes = [kinds[k] for k in sig]
    rc = f(*[kinds[k](0) for k in sig])
    print(name, rc, flush=True)
"""


def test_library_exports_encode_dev():
    lib = ctypes.CDLL(mhe.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in mhe.SIGNATURES, name
    assert hasattr(mhe.Engine, "encode_dev")
    res, args = mhe.SIGNATURES["mhe_ckks_encode_dev"]
    assert res is ctypes.c_int and len(args) == 13


def test_null_context_is_an_argument_error():
    """A fresh child process that only loads the library calls each new entry point with a null
    context and every other argument zero: MHE_ERR_ARG, nothing read through the context, no GPU
    opened."""
    codes = {ctypes.c_int: "i", ctypes.c_double: "d", ctypes.c_size_t: "z", ctypes.c_void_p: "p"}
    sigs = []
    for name in NEW_ENTRY_POINTS:
        res, args = mhe.SIGNATURES[name]
        assert res is ctypes.c_int
        sigs.append((name, "".join(codes[t] for t in args)))
    p = subprocess.run([sys.executable, "-c", _NULL_CTX_CHILD, mhe.LIB_PATH, json.dumps(sigs)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    got = [line.split() for line in p.stdout.splitlines()]
    assert got == [[name, "-1"] for name in NEW_ENTRY_POINTS], (got, p.stderr)
