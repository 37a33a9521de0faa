"""The index maps of the device I/O kernels (cddp-cpp_amd/csrc/io_layout.hpp) on the host: tests/cpp/test_io_layout.cpp, a stand-alone
program, is built with g++ -fsanitize=address,undefined and tiles / un-tiles through the maps for every (b, t, e) of four shapes (one
trajectory; one full tile; a partial second tile; three tiles), the sub-tile-minor stack and a slotted field with a scrambled slot table.
No GPU, no library: the header is all it includes."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "cddp-cpp_amd", "build", "test_io_layout")


def build_exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_io_layout.cpp")
    hdr = os.path.join(REPO, "cddp-cpp_amd", "csrc", "io_layout.hpp")
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in (src, hdr, __file__)):   # (this file holds the compile line)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", EXE])
    return EXE


def test_index_maps_match_the_layout_formulas():
    out = subprocess.run([build_exe()], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "io layout: ok" in out.stdout
