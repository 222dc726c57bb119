"""CPU: the tap index function of the correlation lookup (eogs2_amd/csrc/raft_taps.h) compiled for the host
(tests/raft_taps_host.cpp): an in-range floor, a finite weight and an "inside" or "outside" verdict per tap for NaN, +-Inf,
+-1e30, denormals and +-0 — what is not a tame coordinate has every tap outside and weight 0 — and exact agreement with the
float64 statement for finite coordinates. The bit-pattern cases live here, on the CPU, not in a GPU test."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tap_function_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "raft_taps_host")
    build = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "eogs2_amd", "csrc"),
                            os.path.join(ROOT, "tests", "raft_taps_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "ALL CHECKS PASSED" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert "FAILED" not in run.stdout
