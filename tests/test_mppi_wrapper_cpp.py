"""Builds and runs the C++ test of the sampling front end of the host-side mirror (cddp-cpp_amd/host/cddp_hip.hpp: sampleControls, mppiBlend,
mppiRefine): refusals as exceptions on the CPU; on the GPU a solved 2 x 1 LTI batch whose candidates are csrc/mppi.hpp evaluated by the test
program itself, whose two-round refinement is the loop written out over sampleControls -> scoreRollouts -> mppiBlend, host and device pointers
alike, a re-solve from the refined seed, and the pointer refusals (a host pointer, a device allocation one element short)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "cddp-cpp_amd", "build", "test_mppi_wrapper")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def build_exe():
    lib = os.path.join(REPO, "cddp-cpp_amd", "lib", "libcddp_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_mppi_wrapper.cpp")
    hdr = os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")
    arith = os.path.join(REPO, "cddp-cpp_amd", "csrc", "mppi.hpp")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in (src, hdr, arith, lib, __file__)):   # (this file holds the link line)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), src, "-o", EXE,
                               "-L" + os.path.dirname(lib), "-lcddp_hip", "-Wl,-rpath,$ORIGIN/../lib", "-L" + os.path.join(ROCM, "lib"),
                               "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-lamdhip64"])
    return EXE


def test_mppi_wrapper_cpu():
    out = subprocess.run([build_exe(), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_mppi_wrapper_gpu():
    out = subprocess.run([build_exe(), "gpu"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
