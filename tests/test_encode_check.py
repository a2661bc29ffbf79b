"""The threshold of the device size check of mhe_ckks_encode_dev (fhe-gpt-2_amd/csrc/encode_check.h) on
the CPU: tests/cpp/encode_check_test.cpp checks for every total bit count from 2 to 1100 that
largest_fitting gives a double the host's check accepts whose successor it rejects, and that comparing
bit patterns with it gives the host's verdict on 4096 ulps either side of 2^(tb-2)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "encode_check_test")


def test_encode_check():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "fhe-gpt-2_amd", "seal"), "../../build/encode_check_test"])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1100 checked, 0 failed" in r.stdout
