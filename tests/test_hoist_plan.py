"""The launch plan of a hoisted pass's key MACs (fhe-gpt-2_amd/csrc/hoist_plan.h) on the CPU:
tests/cpp/hoist_plan_test.cpp checks every plan's invariants (each rotation in exactly one item of
one launch, an item's rotations of one input and sorted by key, one rotation count per launch, the
limits of MHE_MAXB items and MHE_HOIST_R rotations, shared launches of at least two items with equal
key lists) and the exact plans of passes derived by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "hoist_plan_test")


def test_hoist_plan():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "fhe-gpt-2_amd", "seal"), "../../build/hoist_plan_test"])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ", 0 failed" in r.stdout
