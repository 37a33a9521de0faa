"""Test data of the stack-fed sweeps (helper module, not a test file): what a host plug-in hands to HipStackSolver.

* make_case(): the one generator of the random stack data sets that tests/test_stack_fed_shapes.py runs on the GPU and that
  tests/test_stack_twin.py checks for conditioning -- fixed seeds, so both files see the same numbers.
* twin_stacks(): the stacks of a numpy-twin iterate (oracle/twin/cddp_twin.py), as a host-plugin adapter builds them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "twin"))

SEED = 20261016
STACK_KEYS = ("fx", "fu", "lx", "lu", "lxx", "luu", "lux", "VxN", "VxxN")
PATH_KEYS = ("y", "s", "g", "Gx", "Gu")
HESS_KEYS = ("Fxx", "Fuu", "Fux")


def _spd(rng, lead, n):
    """Symmetric positive definite blocks with every eigenvalue >= 0.5."""
    W = rng.standard_normal(lead + (n, n)) / np.sqrt(n)
    return 0.5 * np.eye(n) + 0.5 * (W @ np.swapaxes(W, -1, -2))


def make_case(nx, nu, m, B, N, seed=0, bad=()):
    """One random data set of B trajectories over N steps, batch-major ([B][N][...]), every optional part included:
    * fx = I + 0.05 noise, fu = 0.3 noise, SPD l_xx / l_uu (eigenvalues >= 0.5), non-zero l_ux, a NON-symmetric V_xxN (the IPDDP /
      LogDDP / MSIPDDP sweeps symmetrise it, CLDDP does not);
    * path rows (m > 0): y in [0.5, 0.9]; even rows nearly active (s in [0.01, 0.03], so that the step caps fall below 1), odd rows
      inactive (s in [0.2, 0.6]); g = -s + 0.01 noise; mu per trajectory 0.1 / 1e-3;
    * dynamics Hessian stacks (0.005 noise: larger ones make Q_uu nearly singular somewhere over 40 steps at nx = 12), multiple-shooting
      defects (0.05 noise);
    * a control box [-1, 1] with the controls at +-0.98 (steps towards the near bound are clamped);
    * reg per trajectory 1e-6 / 1e-2;
    * trajectories in `bad` get l_uu = -5 I at step max(N - 3, 0): the CLDDP eigenvalue test fails there until the retry loop has raised
      the regularisation past 5."""
    rng = np.random.default_rng([SEED, seed, nx, nu, m, B, N])
    c = {}
    c["fx"] = np.eye(nx) + 0.05 * rng.standard_normal((B, N, nx, nx))
    c["fu"] = 0.3 * rng.standard_normal((B, N, nx, nu))
    c["lx"] = rng.standard_normal((B, N, nx)); c["lu"] = rng.standard_normal((B, N, nu))
    c["lxx"] = _spd(rng, (B, N), nx); c["luu"] = _spd(rng, (B, N), nu)
    c["lux"] = 0.1 * rng.standard_normal((B, N, nu, nx))
    c["VxN"] = rng.standard_normal((B, nx))
    W = rng.standard_normal((B, nx, nx)) / np.sqrt(nx)
    c["VxxN"] = _spd(rng, (B,), nx) + 0.2 * (W - np.swapaxes(W, 1, 2)) + 0.1 * np.eye(nx)   # a skew part: NOT symmetric
    for b in bad:
        c["luu"][b, max(N - 3, 0)] = -5.0 * np.eye(nu)
    c["reg"] = np.where(np.arange(B) % 2 == 0, 1e-6, 1e-2)
    if m:
        c["y"] = 0.5 + 0.4 * rng.random((B, N, m))
        near = (np.arange(m) % 2 == 0)[None, None, :]
        c["s"] = np.where(near, 0.01 + 0.02 * rng.random((B, N, m)), 0.2 + 0.4 * rng.random((B, N, m)))
        c["g"] = -c["s"] + 0.01 * rng.standard_normal((B, N, m))
        c["Gx"] = 0.3 * rng.standard_normal((B, N, m, nx)); c["Gu"] = 0.5 * rng.standard_normal((B, N, m, nu))
        c["mu"] = np.where(np.arange(B) % 3 == 0, 0.1, 1e-3)
    c["Fxx"] = 0.005 * rng.standard_normal((B, N, nx, nx, nx))
    c["Fuu"] = 0.005 * rng.standard_normal((B, N, nx, nu, nu))
    c["Fux"] = 0.005 * rng.standard_normal((B, N, nx, nu, nx))
    c["d"] = 0.05 * rng.standard_normal((B, N, nx))
    c["lo"], c["up"] = -np.ones(nu), np.ones(nu)
    c["U"] = 0.98 * np.sign(rng.standard_normal((B, N, nu)))
    return c


def trajectory(c, b):
    """Trajectory b of a data set, in the per-trajectory form oracle/twin/stack_twin.py takes."""
    return {k: v[b] for k, v in c.items() if k not in ("lo", "up") and isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == c["fx"].shape[0]}


def twin_stacks(tw):
    """What a host-plugin adapter hands to cddp_hip_set_stacks / cddp_hip_set_constraint_stacks for the twin's iterate."""
    N, nx, nu, m = tw.N, tw.nx, tw.nu, tw.m
    fx = np.zeros((N, nx, nx)); fu = np.zeros((N, nx, nu)); lx = np.zeros((N, nx)); lu = np.zeros((N, nu))
    Gx = np.zeros((N, m, nx)); Gu = np.zeros((N, m, nu))
    for t in range(N):
        fx[t], fu[t] = tw.lin(t)
        lx[t], lu[t], lxx, luu, lux = tw.cost_derivs(t)
        off = 0
        for _, c in tw.cons:
            gx, gu = c.jac(tw.X[t], tw.U[t]); Gx[t, off:off + c.dim] = gx; Gu[t, off:off + c.dim] = gu; off += c.dim
    H = 2.0 * tw.Qf
    return dict(fx=fx, fu=fu, lx=lx, lu=lu, lxx=np.tile(lxx, (N, 1, 1)), luu=np.tile(luu, (N, 1, 1)), lux=np.tile(lux, (N, 1, 1)),
                VxN=2.0 * tw.Qf @ (tw.X[N] - tw.xref), VxxN=H, y=getattr(tw, "Y", np.zeros((N, m))).copy(), s=getattr(tw, "S", np.zeros((N, m))).copy(),
                g=getattr(tw, "G", np.zeros((N, m))).copy(), Gx=Gx, Gu=Gu)
