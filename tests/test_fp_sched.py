"""Host-side check of the scheduled reduction of x in the non-lazy FP64 forward stages (csrc/fparith.h,
"Scheduled reduction of x"): tests/fp_sched.cpp is built with the host compiler, contraction off, against
fparith.h's own functions, and run.  No GPU."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fp_sched_host_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fp_sched")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "fp_sched.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count(": ok") == 3  # the largest primes below 2^51, 2^50 and 2^48
