"""The straight-line step of the two-role IPDDP rollout's producer (kernels_lean.hpp::k_forward_ipddp_pc, round 10): integrator chosen
once per launch, ONE range test of the fast sin / cos per step with the checked step behind it, running row pointers.

The comparison route is CDDP_HIP_K4_NA=2 (kernels_pcm.hpp, untouched: Stepper::step with its per-call range tests and the row
addresses derived from t).  Everything compared is compared bitwise (NaN == NaN).

What is compared: the C-ABI hands out a trial's record (cddp_hip_forward: step sizes, cost, merit, theta, the two infeasibilities,
the success flag -- every one a function of the trial's X / U / slack / dual rows) and, once a trial is accepted, its rows themselves
(trajectory, duals) with the work counters (rollout_steps credits each trial's first failing step).  So each case takes the trial
records of a step-level forward pass AND the iterate after a few iterations of the solve."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INTEGRATORS = ["EULER", "HEUN", "RK3", "RK4"]


def cartpole(api, integrator, iters=None):
    p = api.cartpole_problem(api.SOLVER_IPDDP, True)
    p.c.integrator = getattr(api, integrator)
    if iters is not None:
        p.options.max_iterations = iters
    return p


def same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=(a.dtype.kind == "f"))


def snapshot(api, mk, B, x0, n_alpha=None, iters=3):
    """[(name, array with the batch on axis 0), ...]: the trial records of one forward pass over the first n_alpha step sizes (all of
    them by default) and the iterate after `iters` iterations, plus the work counters (no batch axis) under the name "work"."""
    p = mk(None)
    U0 = api.batch_U0(p, B)
    hs = api.HipBatchSolver(p, B); hs.set_initial(x0, U0); hs.initialize(); hs.backward()
    al = api.Oracle(p).alphas()
    tr = hs.forward(al if n_alpha is None else al[:n_alpha]); hs.close()
    out = [("trial." + f, tr[f].copy()) for f in tr.dtype.names if not f.startswith("_")]
    p = mk(iters)
    hs = api.HipBatchSolver(p, B); hs.set_initial(x0, U0); st = hs.solve()
    r = hs.results(); X, U = hs.trajectory(); S, Y, G = hs.duals(); K, k = hs.gains(); hs.close()
    out += [("result." + f, r[f].copy()) for f in r.dtype.names if not f.startswith("_")]
    out += [("X", X), ("U", U), ("S", S), ("Y", Y), ("G", G), ("K", K), ("k", k)]
    out += [("work", np.array([st.sweeps, st.rollouts, st.rollout_steps]))]
    return out


def both_routes(api, monkeypatch, **kw):
    monkeypatch.delenv("CDDP_HIP_K4_NA", raising=False)
    new = snapshot(api, **kw)
    monkeypatch.setenv("CDDP_HIP_K4_NA", "2")
    ref = snapshot(api, **kw)
    monkeypatch.delenv("CDDP_HIP_K4_NA", raising=False)
    return new, ref


def assert_same(new, ref, tag, rows=None):
    for (name, a), (name_r, b) in zip(new, ref):
        assert name == name_r
        if rows is not None:
            if name == "work":
                continue
            a, b = a[rows], b[rows]
        assert same(a, b), (tag, name)


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("ladder", ["whole", "first4"])
def test_default_route_equals_per_call_checked_route(api, monkeypatch, integrator, ladder):
    """Tests 1 and 2 of the round: an in-range batch (three tiles, the last one ragged), cart-pole with its control box, each of the four
    integrators; the whole ladder in one launch, and a first stage of four step sizes (the forward pass over four step sizes; the solve
    with the two-stage ladder pinned to a first stage of four)."""
    B = 150
    p = cartpole(api, integrator)
    x0 = api.batch_x0(p, B, 20271001, [0.1, 0.3, 0.1, 0.1])
    if ladder == "whole":
        monkeypatch.setenv("CDDP_HIP_LS_STAGES", "1")
        n_alpha = None
    else:
        monkeypatch.setenv("CDDP_HIP_LS_STAGES", "2"); monkeypatch.setenv("CDDP_HIP_LS_FIRST", "4")
        n_alpha = 4
    new, ref = both_routes(api, monkeypatch, mk=lambda it: cartpole(api, integrator, it), B=B, x0=x0, n_alpha=n_alpha)
    assert_same(new, ref, (integrator, ladder))


# lanes of the SECOND tile (trajectories 64..127) that leave the fast sin / cos range, as (trajectory, pole angle, pole rate)
OUT_OF_RANGE = {
    # two of a tile's 64 lanes start at a finite pole angle outside the fast range: every step of theirs is served by the libm
    "start_outside": [(64 + 5, 2.0e9, None), (64 + 40, -2.0e9, None)],
    # lanes that start inside and cross 1e9 within the horizon, i.e. at some later stage of some step.  (The C-ABI has no way to plant a
    # gain; the pole rate carries the angle across instead: from 0.9e9 at 2.5e7 rad/s, and gently -- all values stay finite -- from
    # 150 rad below the limit at 100 rad/s.)
    "crosses_inside_horizon": [(64 + 17, 0.9e9, 2.5e7), (64 + 33, 1.0e9 - 150.0, 100.0)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(OUT_OF_RANGE))
def test_out_of_range_lanes_take_the_checked_step(api, monkeypatch, case):
    """Test 3: nothing faults; the in-range lanes keep the rows they have in the in-range batch; the out-of-range lanes (and everything
    else) equal the comparison route."""
    B = 150
    integrator = "RK4"
    p = cartpole(api, integrator)
    x0_in = api.batch_x0(p, B, 20271002, [0.1, 0.3, 0.1, 0.1])
    x0 = x0_in.copy()
    lanes = []
    for b, angle, rate in OUT_OF_RANGE[case]:
        x0[b, 1] = angle
        if rate is not None:
            x0[b, 3] = rate
        lanes.append(b)
    mk = lambda it: cartpole(api, integrator, it)
    monkeypatch.delenv("CDDP_HIP_K4_NA", raising=False)
    base = snapshot(api, mk=mk, B=B, x0=x0_in, iters=1)
    new, ref = both_routes(api, monkeypatch, mk=mk, B=B, x0=x0, iters=1)
    assert_same(new, ref, case)                                   # every lane, the out-of-range ones included, and the counters
    inside = np.array([b for b in range(B) if b not in lanes])
    assert_same(new, base, case + ": in-range lanes", rows=inside)


@pytest.mark.gpu
@pytest.mark.parametrize("plant", ["cartpole", "unicycle"])
def test_whole_solves_are_bitwise_equal(api, monkeypatch, plant):
    """Test 4: whole solves at B = 256 with the default settings against the comparison route: result records and trajectories."""
    B = 256
    mk = (lambda: api.cartpole_problem(api.SOLVER_IPDDP, True)) if plant == "cartpole" else (lambda: api.unicycle_problem(api.SOLVER_IPDDP, 100, True))
    p = mk()
    x0 = api.batch_x0(p, B, 20271003, [0.1, 0.3, 0.1, 0.1] if plant == "cartpole" else [0.05, 0.05, 0.05])
    U0 = api.batch_U0(p, B)

    def run():
        hs = api.HipBatchSolver(mk(), B); hs.set_initial(x0, U0); st = hs.solve()
        r = hs.results(); X, U = hs.trajectory(); hs.close()
        return [r[f].copy() for f in r.dtype.names] + [X, U, np.array([st.sweeps, st.rollouts, st.rollout_steps])]

    monkeypatch.delenv("CDDP_HIP_K4_NA", raising=False)
    new = run()
    monkeypatch.setenv("CDDP_HIP_K4_NA", "2")
    ref = run()
    for i, (a, b) in enumerate(zip(new, ref)):
        assert same(a, b), (plant, i)


def test_flagged_trig_entry_on_the_host(tmp_path):
    """Test 5 (no GPU): dev_trig.hpp::sincos_fast_flag compiled for the host returns the bits of sincos_fast on 1e6 seeded arguments up
    to 1e9 (and at every quadrant boundary) and sets its flag exactly for |a| >= 1e9, NaN and inf."""
    exe = str(tmp_path / "test_dev_trig_flag")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(REPO, "tests", "cpp", "test_dev_trig_flag.cpp")])
    out = subprocess.run([exe, "1000000"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    mismatches, flag_errors, n = (int(v) for v in out.stdout.split()[:3])
    assert mismatches == 0 and flag_errors == 0 and n == 1000000
