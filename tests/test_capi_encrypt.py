"""CPU-side checks of the batched encryption's C ABI (no GPU compute): libmhe.so exports
mhe_encrypt_pk_batch and mhe_encrypt_stats, include/mhe.h declares them, and the Python binding
exposes them."""
import ctypes
import os
import re

import mhe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mhe_encrypt_pk_batch", "mhe_encrypt_stats"]


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(mhe.LIB_PATH)
    missing = [n for n in NAMES if not hasattr(lib, n)]
    assert not missing, missing


def test_header_declares_them():
    text = open(os.path.join(ROOT, "include", "mhe.h")).read()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(\s*mhe_ctx\s*\*", text), n
    # the batch entry's argument list, as the issue states it
    decl = re.search(r"int\s+mhe_encrypt_pk_batch\s*\(([^;]*)\)\s*;", text).group(1)
    kinds = [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]
    assert len(kinds) == 9
    assert kinds[2] == "const uint64_t (*seeds)[8]" and kinds[5].startswith("const uint64_t *const *")


def test_binding_exposes_them():
    for n in NAMES:
        assert n in mhe.SIGNATURES
    assert len(mhe.SIGNATURES["mhe_encrypt_pk_batch"][1]) == 9
    assert len(mhe.SIGNATURES["mhe_encrypt_stats"][1]) == 4
    assert callable(mhe.Engine.encrypt_pk_batch) and callable(mhe.Engine.encrypt_stats)
