"""The stack-level reference of the stack-fed sweeps (oracle/twin/stack_twin.py) and the data tests/test_stack_fed_shapes.py runs on the GPU.

* Pin: fed the stacks of a numpy-twin iterate, the stack-level functions reproduce Twin.backward() (and MSIPDDP.backward_pass) to 1e-13.
* Conditioning: every data set of the GPU file, re-run under a relative perturbation of 1e-15, moves no output by more than 1e-11 and
  flips no discrete decision (ok, the retry count, BoxQP's clamped rows) -- the GPU tolerance of 1e-9 is spent on the kernel.
* Shape list: the GPU file's shapes are the PICK(...) lists of stacks.hip / stacks_te.hpp, parsed from the source."""
import os
import re
import sys

import numpy as np
import pytest

import stack_data as D
import test_stack_fed_shapes as G

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
PIN = 1e-13


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def _twin(name, b, use_ilqr=True):
    import make_twin_golden as GT
    spec = GT.CASES[name](); spec["options"]["use_ilqr"] = use_ilqr
    tw = GT.T.Twin(spec)
    pert = np.random.default_rng(20261016 + b).uniform(-0.05, 0.05, size=len(spec["x0"])) * (0.0 if b == 0 else 1.0)
    tw.set_initial(np.array(spec["x0"], float) + pert, spec.get("U0")); tw.initialize(); tw.X_lin, tw.U_lin = tw.X, tw.U
    return tw


def _advance(tw):
    best = tw.line_search()
    if best["success"]:
        tw.apply(best); tw.reg_down()
    else:
        tw.forward_failure()


@pytest.mark.parametrize("name,use_ilqr", [("pendulum_ipddp_unc", True), ("cartpole_ipddp_unc", True), ("cartpole_ipddp_unc", False),
                                           ("pendulum_ipddp_box", True), ("pendulum_ipddp_box", False), ("cartpole_ipddp_box", True),
                                           ("cartpole_ipddp_box", False), ("unicycle_ipddp_box_ball", True), ("unicycle_ipddp_box_ball", False),
                                           ("cartpole_clddp_unc", True), ("pendulum_clddp_unc", True), ("pendulum_clddp_box", True),
                                           ("cartpole_clddp_box", True), ("unicycle_clddp_box", True)])
def test_stack_functions_reproduce_the_twin_backward_pass(name, use_ilqr):
    """The plant cases test_stack_fed.py feeds through _twin_stacks: over the first iterates of the twin's own solve, every output of the
    stack-level function equals the twin's backward pass (gains, value function, dV, residuals, constraint gains, rollout, step caps; the
    control-limited CLDDP step through BoxQP with the previous sweep's warm start; the regularisation of the retry loop)."""
    import stack_twin as S
    for b in range(2):
        tw = _twin(name, b, use_ilqr)
        opt = tw.o
        box = tw.clddp_box() if tw.solver == "CLDDP" else None
        k_warm = tw.k_u.copy()
        for outer in range(3):
            st = D.twin_stacks(tw)
            hess = None
            if not use_ilqr:
                H = [tw.hess_stack(t) for t in range(tw.N)]
                hess = tuple(np.array([h[i] for h in H]) for i in range(3))
            reg = tw.reg
            if tw.solver == "CLDDP":
                U = tw.U.copy()
                ref = S.retry(lambda r: S.clddp(st, r, opt, None if box is None else (box.lo, box.up), U, k_warm), reg, opt)
            elif tw.m:
                ref = S.retry(lambda r: S.ipddp_path(st, r, tw.mu, opt, hess), reg, opt)
            else:
                ref = S.retry(lambda r: S.ipddp(st, r, hess), reg, opt)
            okt = False
            while not okt:          # the twin's retry loop (cddp_solver_base.cpp:93-111)
                okt = tw.backward()
                if not okt:
                    tw.reg_up()
                    if tw.reg_limit():
                        break
            assert ref["ok"] == okt and ref["reg"] == tw.reg, (name, b, outer)
            assert okt
            pairs = [("K", tw.K_u), ("k", tw.k_u), ("Vx", tw.Vx), ("Vxx", tw.Vxx), ("dV", tw.dV), ("inf_du", tw.inf_du)]
            if tw.solver != "CLDDP":
                pairs += [("step_norm", tw.step_norm), ("inf_pr", tw.inf_pr), ("inf_comp", tw.inf_comp)]
            if tw.m and tw.solver != "CLDDP":
                apm, adm = tw.max_step_sizes()
                pairs += [("ky", tw.k_y), ("Ky", tw.K_y), ("ks", tw.k_s), ("Ks", tw.K_s), ("dX", tw.dX), ("alpha_pr_max", apm), ("alpha_du_max", adm)]
            for key, want in pairs:
                assert rel(ref[key], want) <= PIN, (name, b, outer, key, rel(ref[key], want))
            if box is not None:
                assert np.array_equal(np.all(ref["K"] == 0.0, axis=2), np.all(tw.K_u == 0.0, axis=2))
            _advance(tw)
            k_warm = tw.k_u.copy()


@pytest.mark.parametrize("name", ["pendulum_box", "cartpole_box"])
def test_msipddp_path_function_reproduces_the_solver_class(name):
    """The constrained MSIPDDP branch restated on stacks against MSIPDDP.backward_pass (msipddp_solver.cpp:1222-1420) on the iterates of a
    multiple-shooting start (defects non-zero), as tests/test_msipddp.py runs them."""
    import make_twin_golden as GT
    import msipddp_twin as M
    import stack_twin as S
    spec = GT._pendulum("IPDDP", True) if name.startswith("pendulum") else GT._cartpole("IPDDP", True)
    spec.setdefault("options", {}).update(ms_rollout_type="nonlinear", ms_segment_length=5, warm_start=True)
    x0 = np.array(spec["x0"], float); xr = np.array(spec["xref"], float); N = spec["N"]
    X0 = np.array([x0 + (xr - x0) * t / N for t in range(N + 1)])
    tw = M.MSIPDDP(spec); tw.set_initial(x0, spec.get("U0"), X0); tw.initialize()
    for sweep in range(2):
        st = dict(fx=np.zeros((N, tw.nx, tw.nx)), fu=np.zeros((N, tw.nx, tw.nu)), Gx=np.zeros((N, tw.m, tw.nx)), Gu=np.zeros((N, tw.m, tw.nu)))
        for t in range(N):
            Fx, Fu = tw.model.jac(tw.X[t], tw.U[t], t * tw.dt)
            st["fx"][t] = tw.dt * Fx + np.eye(tw.nx); st["fu"][t] = tw.dt * Fu
            st["Gx"][t], st["Gu"][t] = tw.jac_all(tw.X[t], tw.U[t])
        st.update(lx=np.array([2.0 * tw.Qdt @ (tw.X[t] - tw.xref) for t in range(N)]), lu=np.array([2.0 * tw.Rdt @ tw.U[t] for t in range(N)]),
                  lxx=np.tile(2.0 * tw.Qdt, (N, 1, 1)), luu=np.tile(2.0 * tw.Rdt, (N, 1, 1)), lux=np.zeros((N, tw.nu, tw.nx)),
                  VxN=2.0 * tw.Qf @ (tw.X[-1] - tw.xref), VxxN=2.0 * tw.Qf, y=tw.Y.copy(), s=tw.S.copy(), g=tw.G.copy())
        d = tw.F - tw.X[1:]
        ref = S.msipddp_path(st, tw.reg, tw.mu, d)
        assert tw.backward_pass() and ref["ok"]
        for key, want in (("K", tw.K), ("k", tw.k), ("ky", tw.k_y), ("Ky", tw.K_y), ("ks", tw.k_s), ("Ks", tw.K_s), ("dV", tw.dV),
                          ("inf_du", tw.inf_du), ("step_norm", tw.step_norm), ("inf_comp", tw.inf_comp)):
            assert rel(ref[key], want) <= PIN, (name, sweep, key, rel(ref[key], want))
        assert rel(max(ref["inf_pr"], float(np.max(np.abs(d)))), tw.inf_pr) <= PIN
        r = None
        for a in tw.alphas:
            r = tw.forward_pass(a)
            if r is not None:
                break
        if r is None:
            break
        tw.X, tw.U, tw.F, tw.Lam, tw.S, tw.Y, tw.G, tw.cost = r["X"], r["U"], r["F"], r["Lam"], r["S"], r["Y"], r["G"], r["cost"]


def test_retry_follows_the_regularisation_rule():
    """reg *= update_factor, a zero regularisation restarts at reg_min_value (reg_max_value when that is 0), capped at reg_max_value; the
    loop gives up once the cap is reached -- and agrees with the twin's reg_up / reg_limit for a positive start."""
    import stack_twin as S
    import cddp_twin as T
    opt = T.default_options()
    seen = []
    out = S.retry(lambda r: (seen.append(r), dict(ok=r > 5.0))[1], 1e-6, opt)
    assert out["ok"] and out["reg"] == seen[-1] and out["retries"] == len(seen) - 1 and seen[0] == 1e-6
    r = 1e-6; want = [r]
    while r <= 5.0:
        r = min(r * opt["reg_update_factor"], opt["reg_max_value"]); want.append(r)
    assert seen == want
    seen.clear()
    out = S.retry(lambda r: (seen.append(r), dict(ok=False))[1], 0.0, opt)
    assert seen[:2] == [0.0, opt["reg_min_value"]] and not out["ok"] and out["reg"] == opt["reg_max_value"]
    assert seen[-1] < opt["reg_max_value"]   # the cap itself is not tried
    seen.clear()
    out = S.retry(lambda r: (seen.append(r), dict(ok=False))[1], 0.0, dict(opt, reg_min_value=0.0))
    assert seen == [0.0] and out["reg"] == opt["reg_max_value"]
    seen.clear()
    out = S.retry(lambda r: (seen.append(r), dict(ok=False))[1], 1e-6, dict(opt, reg_update_factor=0.0))
    assert seen == [1e-6] and out["reg"] == 1e-6 and out["retries"] == 0


# ---- conditioning of the GPU data sets --------------------------------------------------------------------------------------------------
def _perturbed(c, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in c.items():
        if isinstance(v, np.ndarray) and v.dtype == np.float64 and k not in ("reg", "mu", "lo", "up", "U"):
            v = v * (1.0 + 1e-15 * rng.standard_normal(v.shape))
        out[k] = v
    return out


OUTPUTS = G.ARRAYS + G.PATH_ARRAYS + ("dX",) + G.SCALARS


def _check_conditioning(shape, branch, c, refs, idx):
    opt = G.twin_options()
    cp = _perturbed(c, 7)
    worst = 0.0
    for b in idx:
        for r0, r1 in zip(refs[b], G.reference(branch, cp, b, opt)):
            assert r0["ok"] == r1["ok"] and r0["reg"] == r1["reg"] and r0["retries"] == r1["retries"], (shape, branch, b)
            if "free" in r0:
                assert np.array_equal(r0["free"], r1["free"]), (shape, branch, b)
            if not r0["ok"]:
                continue
            for key in OUTPUTS:
                if key in r0:
                    e = rel(r1[key], r0[key]); worst = max(worst, e)
                    assert e <= 1e-11, (shape, branch, b, key, e)
    return worst


@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "nx%d_nu%d_m%d" % s)
def test_gpu_data_sets_are_well_conditioned(shape):
    for branch in G.branches(shape):
        for B, N in G.datasets(shape):
            c, refs = G.cached_reference(shape, branch, B, N)
            _check_conditioning(shape, branch, c, refs, range(B))


def test_gpu_flip_and_grid_data_sets_are_well_conditioned():
    for shape, B in ((4, 1, 2), 8192), ((4, 1, 2), 8256), ((3, 2, 5), 16384), ((3, 2, 5), 16448):
        idx = G.flip_sample(B)
        c, refs = G.cached_reference(shape, "path", B, G.FLIP_N, idx)
        _check_conditioning(shape, "path", c, refs, idx)
    for shape, N in G.GRID_CASES:
        c, refs = G.cached_reference(shape, "ipddp_hess", G.GRID_B, N)
        _check_conditioning(shape, "ipddp_hess", c, refs, range(G.GRID_B))


# ---- the shape list ---------------------------------------------------------------------------------------------------------------------
def _picks(text):
    return [tuple(int(v) for v in m_.groups() if v is not None) for m_ in re.finditer(r"PICK\((\d+),\s*(\d+)(?:,\s*(\d+))?\)", text)]


def _function_body(src, name):
    i = src.index(name + "(")
    j = src.index("{", i)
    depth = 0
    for k in range(j, len(src)):
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[j:k + 1]
    raise ValueError(name)


def test_gpu_shape_list_is_every_instantiation():
    """A new instantiation in pick() / pick_coop() / pick_te() cannot arrive without a reference test."""
    csrc = os.path.join(REPO, "cddp-cpp_amd", "csrc")
    src = open(os.path.join(csrc, "stacks.hip")).read()
    body = _function_body(src, "LaunchFn pick")
    lane = body[body.index("#ifndef CDDP_STACKS_DEV_SHAPE"):body.index("#endif")]
    coop = _function_body(src, "LaunchFn pick_coop")
    coop = coop[coop.index("#else"):coop.index("#endif")]
    te = _function_body(open(os.path.join(csrc, "stacks_te.hpp")).read(), "LaunchTeFn pick_te")
    assert _picks(lane) == G.LANE_SHAPES
    assert _picks(coop) == G.COOP_SHAPES
    assert _picks(te) == G.TE_SHAPES
    assert set(G.SHAPES) == set(G.LANE_SHAPES) | set(G.COOP_SHAPES) and len(G.SHAPES) == 24
    # every shape runs every branch it admits in the GPU file
    for shape in G.SHAPES:
        want = {"clddp", "clddp_box", "clddp_retry", "ipddp", "ipddp_hess", "logddp", "logddp_hess", "msipddp"} if shape[2] == 0 else \
            {"path", "path_hess"} | ({"mspath"} if shape[1] == 1 else set())
        assert set(G.branches(shape)) == want
