"""seal::Evaluator::rotate_sum and the Bootstrapper's merged giant-step sums on the GPU
(tests/cpp/rotate_sum_test.cpp): the words and scale of rotate_vectors + add_inplace_reduced_error."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fhe-gpt-2_amd")
EXE = os.path.join(ROOT, "build", "rotate_sum_test")

pytestmark = pytest.mark.gpu


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "seal"), "all", "test"])


def _run(*args):
    _build()
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


def test_rotate_sum_equals_rotate_then_add():
    """N = 2^13, seeded keys: term lists with a zero step, a step without a key and mixed levels (the
    last two on the one-by-one path); three FiberBatch fibers merged into one mhe_rotate_sum with no
    merged-call fallback; a failing scratch allocation leaves the destination's words alone."""
    _run()


def test_bootstrap_merged_giant_sums_words_equal():
    """One sparse bootstrap (N = 2^12, logn 10) with Bootstrapper::set_merged_giant_sums off and on:
    equal output words and scale; mhe_rotsum_stats nonzero only with the switch on."""
    _run("boot")
