"""The arithmetic of the output-feedback Monte-Carlo evaluation (cddp-cpp_amd/csrc/plan_mcof.hpp) on the host.

1. tests/cpp/test_plan_mcof.cpp, a stand-alone program over that header, plan_mc.hpp and mppi.hpp: the index map of the measurement
   normals, steps 2 to 6 on written-out sums (strides 1, 4 and 64).  Built twice with g++ -ffp-contract=off: plainly, and with
   -fsanitize=address,undefined; each runs as its own process.
2. Its `noise` mode (the file the GPU test compares with) against the raw normals of tests/cpp/test_plan_mc.cpp's program, bit for bit.
3. Its `estimate` mode against the numpy restatement tests/plan_mcof_ref.py, bit for bit.
4. The index space: no measurement element is an initial-state, actuator or process element.
5. Statistics on the CPU first: the LTI (2, 1) case of the GPU suite (N = 12, ny = 1, B = 64, S = 1024), the numpy restatement of the whole
   loop on the noise files of the two host programs, against tests/plan_kf_ref.kalman inside 6 standard errors.  This fixes the seed the GPU
   test uses.
No GPU."""
import os
import subprocess

import numpy as np
import pytest

import plan_kf_ref as KF
import plan_mc_ref as MR
import plan_mcof_ref as R
import test_plan_mc_cpu as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "cddp-cpp_amd", "build")
FLAGS = H.FLAGS
SHAPES = [(2, 1, 5, 1), (3, 2, 4, 16), (14, 7, 3, 15)]          # nx, nu, N, ny


def build_exe(kind):
    exe = os.path.join(BUILD, "test_plan_mcof_" + kind)
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(REPO, "tests", "cpp", "test_plan_mcof.cpp")
    hdrs = [os.path.join(REPO, "cddp-cpp_amd", "csrc", n) for n in ("plan_mcof.hpp", "plan_mc.hpp", "mppi.hpp", "dev_trig.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src, __file__] + hdrs):   # (this file holds the compile line)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + FLAGS[kind] + [src, "-o", exe])
    return exe


def meas_noise_file(exe, tmp, v, seed, stream, B, S, N, nx, nu, keep):
    """Yn (B, S, N + 1, ny) as the host program writes it"""
    v = np.asarray(v, dtype=np.float64)
    fin, fout = os.path.join(str(tmp), "mcof_v.bin"), os.path.join(str(tmp), "mcof_yn.bin")
    v.tofile(fin)
    subprocess.check_call([exe, "noise", fin, fout, hex(seed), str(stream), str(B), str(S), str(N), str(nx), str(nu), str(v.shape[0]), "1" if keep else "0"])
    return np.fromfile(fout).reshape(B, S, N + 1, v.shape[0])


def raw_normals(tmp, seed, stream, B, S, n):
    """z(e) for e < n of every (b, c): the initial-state block of the plan_mc program at nx = n with the identity as its factor"""
    eye = np.eye(n)
    Z0, _, _ = H.noise_files(H.build_exe("plain"), tmp, eye, eye, np.eye(1), seed, stream, B, S, 0, False)
    return Z0


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_header_checks(kind):
    out = subprocess.run([build_exe(kind)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan mcof: ok" in out.stdout


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_noise_file_is_the_generators_elements(kind, tmp_path):
    exe = build_exe(kind)
    B, S, seed, stream = 3, 5, 0x1234567890, 2
    for nx, nu, N, ny in SHAPES:
        v = 0.01 * (1.0 + np.arange(ny))
        Yn = meas_noise_file(exe, tmp_path, v, seed, stream, B, S, N, nx, nu, True)
        assert (Yn[:, 0] == 0).all() and (Yn[:, 1:] != 0).all()
        free = meas_noise_file(exe, tmp_path, v, seed, stream, B, S, N, nx, nu, False)
        assert np.array_equal(free[:, 1:], Yn[:, 1:]) and (free[:, 0] != 0).all()
        last = R.elem_y(nx, nu, N, ny, N, ny - 1)
        z = raw_normals(tmp_path, seed, stream, B, S, last + 1)
        sd = np.sqrt(v)
        for t in range(N + 1):
            for r in range(ny):
                assert np.array_equal(free[:, :, t, r], sd[r] * z[:, :, R.elem_y(nx, nu, N, ny, t, r)]), (nx, t, r)
    other = meas_noise_file(exe, tmp_path, v, seed, stream + 1, B, S, N, nx, nu, False)
    assert not np.array_equal(other, free)


@pytest.mark.parametrize("shape", SHAPES)
def test_index_space(shape):
    nx, nu, N, ny = shape
    mc = R.mc_elems(nx, nu, N)
    ys = [R.elem_y(nx, nu, N, ny, t, r) for t in range(N + 1) for r in range(ny)]
    assert len(set(mc)) == len(mc) == nx + N * (nu + nx) and not set(mc) & set(ys)
    assert ys == list(range(max(mc) + 1, max(mc) + 1 + (N + 1) * ny))      # behind the last of them, without a gap, t then r ascending


@pytest.mark.parametrize("kind", sorted(FLAGS))
@pytest.mark.parametrize("shape", [(2, 1, 6, 1), (3, 2, 4, 4), (14, 7, 3, 15)])
def test_restatement_is_the_host_programs(kind, shape, tmp_path):
    nx, nu, T, ny = shape
    n = 7
    rng = np.random.default_rng(nx * 100 + ny)
    C = rng.uniform(-1, 1, (ny, nx)); L = 0.3 * rng.uniform(-1, 1, (T + 1, nx, ny)); K = rng.uniform(-1, 1, (T, nu, nx))
    A = rng.uniform(-1, 1, (T, nx, nx)); Bm = rng.uniform(-1, 1, (T, nx, nu))
    DX = rng.uniform(-1, 1, (n, T + 1, nx)); Yn = 0.1 * rng.uniform(-1, 1, (n, T + 1, ny))
    fin, fout = os.path.join(str(tmp_path), "est_in.bin"), os.path.join(str(tmp_path), "est_out.bin")
    np.concatenate([a.ravel() for a in (C, L, K, A, Bm, DX, Yn)]).tofile(fin)
    subprocess.check_call([build_exe(kind), "estimate", fin, fout, str(n), str(T), str(nx), str(nu), str(ny)])
    got = np.fromfile(fout)
    nH, nF = n * (T + 1) * nx, n * T * nu
    Xh, FB, XP = R.estimator(C, L, K, A, Bm, DX, Yn)
    assert np.array_equal(got[:nH].reshape(Xh.shape), Xh)
    assert np.array_equal(got[nH:nH + nF].reshape(FB.shape), FB)
    assert np.array_equal(got[nH + nF:].reshape(XP.shape), XP)
    assert np.isfinite(got).all() and len(np.unique(got)) == got.size
    # the order of update, control and prediction matters: predicting before the update, or from another feedback, gives other numbers
    assert not np.array_equal(R.predict(A[0], Bm[0], Xh[:, 0], FB[:, 0]), R.predict(A[0], Bm[0], np.zeros((n, nx)), FB[:, 0]))


def lti_case():
    c = R.LTI
    N, B = c["N"], c["B"]
    K = R.lqr_gains(c["A"], c["Bm"], c["Q"] * c["dt"], c["R"] * c["dt"], c["Qf"], N)
    rep = lambda M: np.ascontiguousarray(np.broadcast_to(M, (B,) + M.shape))
    return c, rep(np.broadcast_to(c["A"], (N, 2, 2))), rep(np.broadcast_to(c["Bm"], (N, 2, 1))), rep(K)


def test_statistics_on_the_cpu(tmp_path):
    """The whole loop in numpy at the seed of the GPU test, pooled over the batch, against the filter of plan_kf_ref: the mean of the
    estimation error against 0, SE against SF, SX and SU against the filter's, each inside 6 standard errors (the bounds of
    tests/test_plan_mc.py::test_statistics_against_plan_covariance).  Seed 20261018, the first one tried: the largest ratios are
    printed, and recorded in the GPU test's docstring."""
    c, A, Bm, K = lti_case()
    N, B, S, nx, nu = c["N"], c["B"], c["S"], 2, 1
    kf = KF.kalman(A[:1], Bm[:1], K[:1], c["C"], c["v"], c["L0"] @ c["L0"].T, c["Lw"] @ c["Lw"].T, c["Lu"] @ c["Lu"].T)
    assert (kf["info"] == 0).all()
    L = np.ascontiguousarray(np.broadcast_to(kf["L"], (B,) + kf["L"].shape[1:]))
    Z0, E, Wn = H.noise_files(H.build_exe("plain"), tmp_path, c["L0"], c["Lw"], c["Lu"], R.SEED, 0, B, S, N, False)
    Yn = meas_noise_file(build_exe("plain"), tmp_path, c["v"], R.SEED, 0, B, S, N, nx, nu, False)
    Xp = np.zeros((B, N + 1, nx)); Up = np.zeros((B, N, nu))     # (an LTI loop's deviation from its plan does not depend on the plan)
    X, U, Xh = R.closed_loop(R.lti_step(c["A"], c["Bm"]), Xp, Up, K, A, Bm, c["C"], L, np.zeros((B, nx)), Z0, E, Wn, Yn)
    dEm, SE = MR.moments(X - Xh)
    _, SX = MR.moments(X)
    _, SU = MR.moments(U)
    ratios = R.statistics_ratios(SX, SU, SE, dEm, {k: kf[k][0] for k in ("SX", "SU", "SF")}, B, S)
    print("statistics on the CPU, seed %d: largest |pooled - filter| / (6 standard errors): %s" % (R.SEED, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    for k, r in ratios.items():
        assert r <= 1.0, (k, r)
    # the estimator earns its keep: the error is smaller than the state's spread, and feeding back the estimate costs spread against SX of state feedback
    assert (np.diagonal(kf["SF"][0], axis1=1, axis2=2) < np.diagonal(kf["SX"][0], axis1=1, axis2=2)).all()
