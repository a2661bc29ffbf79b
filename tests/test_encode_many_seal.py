"""seal::CKKSEncoder::encode_many on the GPU (tests/cpp/encode_many_test.cpp): the words, scale and
parms_id of one encode call per vector."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fhe-gpt-2_amd")
EXE = os.path.join(ROOT, "build", "encode_many_test")

pytestmark = pytest.mark.gpu


def test_encode_many_equals_encode():
    """N = 2^13, three limbs: 11 real and 11 complex vectors, batched launches on and off, three
    FiberBatch fibers; an oversized vector throws and leaves every destination's words; unequal
    sizes throw."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "seal"), "all", "test"])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
