"""The arithmetic of the Monte-Carlo plan evaluation (cddp-cpp_amd/csrc/plan_mc.hpp) on the host, and the C++ mirror.

1. tests/cpp/test_plan_mc.cpp, a stand-alone program over that header alone: the element-index map (a pair that straddles a step where
   nx + nu is odd, a source switched off, keep_nominal), the triangular product, the tree sum against a tree written out for S in 1, 2, 63,
   64, 65, 130, the moment and stats formulas on hand-built records, and the LTI (2, 1) closed loop of tests/test_plan_mc.py's statistical
   test (B = 64, S = 1024, N = 20, all three noises, seed 20261018) against the closed-form covariance recursion inside the bounds of 6
   standard errors stated there -- the fixed seed is shown to pass before any GPU run.  Built twice with g++ -ffp-contract=off: plainly,
   and with -fsanitize=address,undefined; each runs as its own process.  With arguments the same program writes the noise files the GPU
   test compares with; here that mode is held against a numpy restatement.
2. tests/cpp/test_plan_mc_wrapper.cpp: mcSampleNoise / planMonteCarlo of cddp-cpp_amd/host/cddp_hip.hpp, refusals as exceptions on the
   CPU, and the ABI of the descriptor.
3. The Python binding's own refusals, which need no library.
No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "cddp-cpp_amd", "build")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def build_exe(kind):
    exe = os.path.join(BUILD, "test_plan_mc_" + kind)
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_plan_mc.cpp")
    hdrs = [os.path.join(REPO, "cddp-cpp_amd", "csrc", n) for n in ("plan_mc.hpp", "mppi.hpp", "dev_trig.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src, __file__] + hdrs):   # (this file holds the compile line)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + FLAGS[kind] + [src, "-o", exe])
    return exe


def noise_files(exe, tmp, L0, Lw, Lu, seed, stream, B, S, N, keep):
    """Z0 (B, S, nx), E (B, S, N, nu), Wn (B, S, N, nx) as the host program writes them"""
    nx, nu = L0.shape[0], Lu.shape[0]
    fin, fout = os.path.join(str(tmp), "mc_in.bin"), os.path.join(str(tmp), "mc_out.bin")
    np.concatenate([L0.ravel(), Lw.ravel(), Lu.ravel()]).tofile(fin)
    subprocess.check_call([exe, "noise", fin, fout, hex(seed), str(stream), str(B), str(S), str(N), str(nx), str(nu), "1" if keep else "0"])
    got = np.fromfile(fout)
    n0, nE = B * S * nx, B * S * N * nu
    return got[:n0].reshape(B, S, nx), got[n0:n0 + nE].reshape(B, S, N, nu), got[n0 + nE:].reshape(B, S, N, nx)


def factors(nx, nu, seed):
    rng = np.random.default_rng(seed)
    tri = lambda n, s: np.tril(s * rng.uniform(-1.0, 1.0, (n, n))) + s * np.eye(n)
    return tri(nx, 0.05), tri(nx, 0.01), tri(nu, 0.1)


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_header_checks(kind):
    out = subprocess.run([build_exe(kind)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan mc: ok" in out.stdout and "lti statistics: seed 20261018" in out.stdout


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_noise_files(kind, tmp_path):
    """the file mode on (3, 2): nx + nu odd.  Whitened by the factors, the noise is one stream of normals per sample in the element order
    of the header: standard moments, sample 0 zero under keep_nominal, and L z restated in numpy"""
    exe = build_exe(kind)
    B, S, N, nx, nu = 3, 65, 3, 3, 2
    L0, Lw, Lu = factors(nx, nu, 5)
    Z0, E, Wn = noise_files(exe, tmp_path, L0, Lw, Lu, 0x1234567890, 2, B, S, N, True)
    assert (Z0[:, 0] == 0).all() and (E[:, 0] == 0).all() and (Wn[:, 0] == 0).all()
    z0 = np.linalg.solve(L0, Z0.reshape(-1, nx).T).T.reshape(B, S, nx)
    ze = np.linalg.solve(Lu, E.reshape(-1, nu).T).T.reshape(B, S, N, nu)
    zw = np.linalg.solve(Lw, Wn.reshape(-1, nx).T).T.reshape(B, S, N, nx)
    z = np.concatenate([z0[:, 1:].reshape(B, S - 1, -1), np.concatenate([ze, zw], axis=-1)[:, 1:].reshape(B, S - 1, -1)], axis=-1)
    n = z.size                                             # 3 * 64 * 18 = 3456 normals: 5 standard errors
    assert abs(z.mean()) < 5.0 / np.sqrt(n) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
    assert len(np.unique(z)) == n
    # the product restated: s = 0; s += L[i][j] * z[j], j ascending -- on the whitened z it reproduces the file to rounding
    back = np.zeros_like(Z0)
    for i in range(nx):
        s = np.zeros((B, S))
        for j in range(i + 1):
            s = s + L0[i, j] * z0[:, :, j]
        back[:, :, i] = s
    assert np.allclose(back, Z0, rtol=0, atol=1e-15)
    # a second run gives the same bits; another stream does not
    again = noise_files(exe, tmp_path, L0, Lw, Lu, 0x1234567890, 2, B, S, N, True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (Z0, E, Wn)))
    other = noise_files(exe, tmp_path, L0, Lw, Lu, 0x1234567890, 3, B, S, N, True)
    assert not np.array_equal(other[1], E)


def wrapper_exe():
    lib = os.path.join(REPO, "cddp-cpp_amd", "lib", "libcddp_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    exe = os.path.join(BUILD, "test_plan_mc_wrapper")
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_plan_mc_wrapper.cpp")
    deps = [src, os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp"), os.path.join(REPO, "cddp-cpp_amd", "csrc", "plan_mc.hpp"), lib, __file__]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):   # (this file holds the link line)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), src, "-o", exe,
                               "-L" + os.path.dirname(lib), "-lcddp_hip", "-Wl,-rpath,$ORIGIN/../lib", "-L" + os.path.join(ROCM, "lib"),
                               "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-lamdhip64"])
    return exe


def test_wrapper_cpu():
    out = subprocess.run([wrapper_exe(), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan mc wrapper (cpu): ok" in out.stdout


def test_binding_and_abi(api):
    """the descriptor's layout, the exported entries, and the refusals the binding makes before the library is called"""
    assert C.sizeof(api.McDesc) == 56 and api.McDesc.viol_tol.offset == 24 and api.McDesc.L0.offset == 32 and api.McDesc.Lu.offset == 48
    assert (api.MC_DEVICE, api.MC_DIAG) == (1, 2)
    assert "cddp_hip_mc_sample_noise" in api.EXPORTED_SYMBOLS and "cddp_hip_plan_montecarlo" in api.EXPORTED_SYMBOLS
    if not os.path.exists(api.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = api.load_hip()
    assert hasattr(lib, "cddp_hip_mc_sample_noise") and hasattr(lib, "cddp_hip_plan_montecarlo")
    with open(os.path.join(REPO, "include", "cddp_hip.h")) as fh:
        text = fh.read()
    assert "int cddp_hip_plan_montecarlo(" in text and "int cddp_hip_mc_sample_noise(" in text and "CDDP_HIP_MC_DIAG = 2" in text

    class Stub(api.HipBatchSolver):
        def __init__(self):
            self.p = type("P", (), {"nx": 2, "nu": 1, "N": 4})()
            self.B = 3

        def __del__(self):
            pass
    s = Stub()
    ok = np.diag([0.1, 0.2])
    for kw, what in ((dict(nsamp=0), "nsamp"), (dict(nsamp=1025), "nsamp"), (dict(nsamp=4, viol_tol=float("nan")), "viol_tol is NaN"),
                     (dict(nsamp=4, seed=-1), "seed"), (dict(nsamp=4, want=()), "want"), (dict(nsamp=4, want=("cost", "nope")), "want")):
        with pytest.raises(ValueError, match=what):
            s.plan_montecarlo(ok, **kw)
    with pytest.raises(ValueError, match="Sigma0"):
        s.plan_montecarlo(np.eye(3), nsamp=4)
    with pytest.raises(ValueError, match="not positive definite"):
        s.plan_montecarlo(np.array([[1.0, 2.0], [2.0, 1.0]]), nsamp=4)
    with pytest.raises(ValueError, match="Wu"):
        s.plan_montecarlo(ok, Wu=np.array([[np.inf]]), nsamp=4)
    d, keep = s._mc_desc("t", np.array([[4.0, 2.0], [2.0, 5.0]]), None, np.array([[0.25]]), 7)
    assert np.array_equal(keep[0], [[2.0, 0.0], [1.0, 2.0]]) and np.array_equal(keep[1], [[0.5]]) and not d.Lw and d.nsamp == 7
    d, keep = s._mc_desc("t", np.array([[1.0, 9.0], [3.0, 0.0]]), None, None, 7, factors=True)
    assert np.array_equal(keep[0], [[1.0, 0.0], [3.0, 0.0]])          # a semidefinite factor as given, its upper triangle dropped


@pytest.mark.gpu
def test_wrapper_gpu():
    """a solved LTI batch through the C++ mirror: the noise is plan_mc.hpp's, the per-sample costs are scoreRollouts' on that noise, stats
    is cddp_mc::stats of the records"""
    out = subprocess.run([wrapper_exe(), "gpu"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan mc wrapper (gpu): ok" in out.stdout
