"""Builds and runs the C++ test of the RAII Plant wrapper of the host-side mirror (cddp-cpp_amd/host/cddp_hip.hpp): refusals as
exceptions on the CPU, a stepped batch on the GPU."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "cddp-cpp_amd", "build", "test_plant_wrapper")


def build_exe():
    lib = os.path.join(REPO, "cddp-cpp_amd", "lib", "libcddp_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_plant_wrapper.cpp")
    hdr = os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in (src, hdr, lib, __file__)):   # (this file holds the link line)
        subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-o", EXE, "-L" + os.path.dirname(lib), "-lcddp_hip",
                               "-Wl,-rpath,$ORIGIN/../lib", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    return EXE


def test_plant_wrapper_cpu():
    out = subprocess.run([build_exe(), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_plant_wrapper_gpu():
    out = subprocess.run([build_exe(), "gpu"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
