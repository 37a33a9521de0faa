"""The reference window of a path-following MPC step (cddp-cpp_amd/csrc/ref_window.hpp, the function the window kernel of inst_ref.hip runs
per element) on the host, and the numpy restatement the GPU tests use (tests/ref_window_ref.py).

tests/cpp/test_ref_window.cpp, a stand-alone program, evaluates windows for rows_per_step 1.0, 2.0, 0.5 and 0.3, paths of one row and of
nine, nx = 1, 3 and 14 and cursors that run past the end of the path (up to 2^62), over a heap array of exactly rows * nx doubles, and
checks the copy and hold-last-row properties itself.  Built twice with g++ -ffp-contract=off: plainly, and with
-fsanitize=address,undefined; each runs as its own process.  It writes every case's path and window to a file, and ref_window_ref.window
must reproduce the windows from the paths bit for bit.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

import ref_window_ref as RW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "cddp-cpp_amd", "build")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
RATES, DIMS, LENS = [1.0, 2.0, 0.5, 0.3], [1, 3, 14], [1, 9]


def build_exe(kind):
    exe = os.path.join(BUILD, "test_ref_window_" + kind)
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_ref_window.cpp")
    hdr = os.path.join(REPO, "cddp-cpp_amd", "csrc", "ref_window.hpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in (src, hdr, __file__)):   # (this file holds the compile line)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + FLAGS[kind] + [src, "-o", exe])
    return exe


def parse(path):
    cases = []
    with open(path) as fh:
        for line in fh:
            w = line.split()
            if w[0] == "case":
                cases.append({"nx": int(w[1]), "L": int(w[2]), "N": int(w[3]), "k": int(w[4]), "rps": float.fromhex(w[5])})
            else:
                assert int(w[1]) == len(w) - 2, w[0]
                cases[-1][w[0]] = np.array([float.fromhex(x) for x in w[2:]])
    return cases


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_header_function_matches_the_restatement(kind, tmp_path):
    out_file = str(tmp_path / ("ref_window_%s.txt" % kind))
    out = subprocess.run([build_exe(kind), out_file], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ref window: ok" in out.stdout
    cases = parse(out_file)
    assert sorted({c["rps"] for c in cases}) == sorted(RATES) and sorted({c["nx"] for c in cases}) == DIMS and sorted({c["L"] for c in cases}) == LENS
    held = blended = 0
    for c in cases:
        nx, L, N, k, rps = c["nx"], c["L"], c["N"], c["k"], c["rps"]
        path = c["path"].reshape(L, nx)
        got = c["window"].reshape(N + 1, nx)
        want = RW.window(path, k, N, rps)
        assert np.array_equal(got, want), (nx, L, k, rps, int(np.sum(got != want)))
        assert np.array_equal(RW.goal(path, k, N, rps), got[N])
        held += int(np.array_equal(got[N], path[L - 1]) and float(k + N) * rps >= L - 1)
        blended += int(L > 1 and any(0.0 < (float(k + t) * rps) % 1.0 and float(k + t) * rps < L - 1 for t in range(N + 1)))
    # the cases reach both branches: windows held at the last row (cursors past the end, L = 1) and rows blended between two path rows
    assert held > 0 and blended > 0, (held, blended)
    assert any(c["L"] == 1 for c in cases) and any(c["k"] >= 2 ** 62 for c in cases)
