"""seal::KeyGenerator through mhe_encrypt_sk_batch on the GPU (tests/cpp/keygen_batch_test.cpp): the
words of the per-digit sequence for every kind of key, the seeded serializations, the counters."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fhe-gpt-2_amd")
EXE = os.path.join(ROOT, "build", "keygen_batch_test")

pytestmark = pytest.mark.gpu


def test_batched_keys_equal_the_sequence():
    """N = 2^13, two contexts on the same seed sequence, batched launches on against off: public key,
    relinearization key, Galois keys, truncated keys of 1, 2 and K-1 digits, a deferred key grown
    from level 2 to 4, seeded save -> load, mhe_keygen_stats, and decryption after a rotation and a
    relinearization with the batched keys."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "seal"), "all", "test"])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
