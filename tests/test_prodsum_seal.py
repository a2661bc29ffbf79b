"""seal::Evaluator::multiply_sum_rescale and the callers' merged product sums on the GPU
(tests/cpp/prodsum_test.cpp): the words, scale and parms_id of multiply_reduced_error, the adds and
rescale_to_next_inplace in order."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fhe-gpt-2_amd")
EXE = os.path.join(ROOT, "build", "prodsum_test")

pytestmark = pytest.mark.gpu


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "seal"), "all", "test"])


def _run(*args, env=None):
    _build()
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr


def test_multiply_sum_rescale_equals_the_sequence():
    """N = 2^13, seeded keys: sums of one to nine products, doubled or not, factors at unequal levels and
    sums at two levels on the merged path; a mixed-level sum, batched launches off and a level of one
    limb on the sequence's; three FiberBatch fibers merged into one mhe_relin_sum_rescale with no
    merged-call fallback; a failing allocation leaves the destinations' words alone."""
    _run()


def test_relu_merged_product_sums_words_equal():
    """One composite ReLU (alpha 13, degrees 15 / 15 / 27) with seal::set_merged_product_sums off and
    on: equal output words and scale; mhe_prodsum_stats nonzero only with the switch on."""
    _run("relu", env=dict(os.environ, MHE_COMP_DIR=os.path.join(ROOT, "tests", "golden", "comp")))
