"""Host-side check of the FP64 butterfly bounds behind the ModUp column pass's unreduced lifts and
folded exit (csrc/fparith.h, "Unreduced lifts"): tests/fp_bounds.cpp is built with the host compiler,
contraction off, against fparith.h's own functions, and run.  No GPU."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fp_bounds_host_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fp_bounds")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "fp_bounds.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count(": ok") == 4  # primes below 2^46, 2^47, 2^48 and 2^51
