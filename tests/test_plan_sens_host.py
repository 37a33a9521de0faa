"""The step bodies of the plan-sensitivity kernels (cddp-cpp_amd/csrc/plan_sens.hpp) on the host: tests/cpp/test_plan_sens.cpp, a
stand-alone program, walks the forward and the adjoint recursion with them on random stacks (nx = 3, nu = 2, N = 5; one vector per call
and three at once; every combination of present and absent cotangents) and compares bit for bit with the sums of include/cddp_hip.h
written out in their stated order.  Built twice with g++ -ffp-contract=off: plainly, and with -fsanitize=address,undefined; each runs as
its own process.  No GPU, no library: the header is all the program includes."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "cddp-cpp_amd", "build")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def build_exe(kind):
    exe = os.path.join(BUILD, "test_plan_sens_" + kind)
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_plan_sens.cpp")
    hdr = os.path.join(REPO, "cddp-cpp_amd", "csrc", "plan_sens.hpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in (src, hdr, __file__)):   # (this file holds the compile line)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + FLAGS[kind] + [src, "-o", exe])
    return exe


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_step_bodies_match_the_sums_written_out(kind):
    out = subprocess.run([build_exe(kind)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan sens: ok" in out.stdout
