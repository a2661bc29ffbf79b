"""seal::Encryptor::encrypt_many / encrypt_zero_many on the GPU (tests/cpp/encrypt_many_test.cpp): the
words, scales and parms_ids of the same sequence of encrypt / encrypt_zero calls."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fhe-gpt-2_amd")
EXE = os.path.join(ROOT, "build", "encrypt_many_test")

pytestmark = pytest.mark.gpu


def test_encrypt_many_equals_encrypt():
    """N = 2^13: two encryptors on identically seeded contexts (a fixed seed, and a seed sequence that
    shows the order of the draws), batches of 1, 3 and 9 at two levels, batched launches on and off;
    SEAL's exceptions, each leaving every destination's words."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "seal"), "all", "test"])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
