"""Builds tests/cpp/test_score_select.cpp -- the selection rule of cddp_hip_seed_best (cddp-cpp_amd/csrc/score_select.hpp) on hand-built
records and a sweep against its two-pass statement -- as a stand-alone executable with the address and undefined-behaviour sanitizers and
runs it.  Host code only: nothing of it is loaded into Python and nothing needs a GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_select_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_score_select")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(REPO, "tests", "cpp", "test_score_select.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "score select: ok" in out.stdout
