"""CPU-side checks of the key-generation entry points: libmhe.so exports them, include/mhe.h declares
them with the arguments the Python binding passes, and the capacity formula of the uniform sampler's
redraw buffer (csrc/sample_cap.h, tests/cpp/sample_cap_test.cpp) holds on the host."""
import ctypes
import os
import re
import subprocess

import mhe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"mhe_prng_uniform_batch": 8, "mhe_encrypt_sk_batch": 11, "mhe_keygen_stats": 6, "mhe_keygen_overflows": 4,
        "mhe_debug_keygen_cap": 2}


def test_exported_declared_and_bound():
    lib = ctypes.CDLL(mhe.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "mhe.h")).read()
    for name, count in ARGS.items():
        assert hasattr(lib, name), name
        decl = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, text).group(1)
        assert len(decl.split(",")) == count, name
        assert len(mhe.SIGNATURES[name][1]) == count, name
    for method in ("prng_uniform_batch", "encrypt_sk_batch", "keygen_stats"):
        assert callable(getattr(mhe.Engine, method))


def test_null_context_is_an_error():
    lib = mhe.lib()
    v = ctypes.c_uint64()
    assert lib.mhe_prng_uniform_batch(None, 1, None, 1, None, None, None, None) != 0
    assert lib.mhe_encrypt_sk_batch(None, 1, None, None, 1, 1, 0, None, None, None, None) != 0
    assert lib.mhe_keygen_stats(None, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v), ctypes.byref(v), 0) != 0
    assert lib.mhe_keygen_overflows(None, None, ctypes.byref(v), ctypes.byref(v)) != 0
    assert lib.mhe_debug_keygen_cap(None, 1) != 0


def test_redraw_capacity_formula():
    exe = os.path.join(ROOT, "build", "sample_cap_test")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "fhe-gpt-2_amd", "seal"), "../../build/sample_cap_test"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
