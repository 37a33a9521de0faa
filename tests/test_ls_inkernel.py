"""Second line-search stage inside the first stage's rollout launch (kernels_lean.hpp::k_forward_ipddp_pc with a split argument;
capi.hip::SolveRun::enqueue_iteration).  Where the deferred costate is active, a two-stage iteration is ONE rollout launch: the
workgroups of the step sizes >= k1 wait for the success masks their tile's first-stage workgroups publish and run the trial only for the
lanes none of the first k1 step sizes worked for.  The selected trials cannot depend on that, so everything a caller can read must be
the SAME BITS as with CDDP_HIP_LS_INKERNEL=0 (two launches, update and costate flush between them): result records, trajectories,
slack / dual / constraint rows, gains, value rows, costates, and the work counters (iterations, sweeps, rollouts, rollout steps).
The stage counters (cddp_hip_ls_stage_counts) say what the second-stage workgroups did; give-ups must be 0 on a healthy device."""
import numpy as np
import pytest

from test_costate_shadow import _same, _snapshot
from test_gpu_parity import make, spread_for

pytestmark = pytest.mark.gpu


def _run(api, monkeypatch, p, B, x0, U0, env):
    for k in ("CDDP_HIP_LS_STAGES", "CDDP_HIP_LS_FIRST", "CDDP_HIP_LS_INKERNEL", "CDDP_HIP_COSTATE", "CDDP_HIP_TEST_LS_POLL_US", "CDDP_HIP_TEST_FAIL_SHADOW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    hs = api.HipBatchSolver(p, B); hs.set_initial(x0, U0)
    st = hs.solve()
    snap = _snapshot(hs, st)
    info = {"counts": hs.ls_stage_counts(), "mode": hs.costate_mode(), "redos": hs.costate_redos(), "groups": hs.num_groups()}
    hs.close()
    return snap, info


def _ab(api, monkeypatch, p, B, x0, U0, env, tag, want_form=True):
    """The in-kernel form against the two-launch form under the same switches; returns the in-kernel side's counters."""
    ref, ri = _run(api, monkeypatch, p, B, x0, U0, dict(env, CDDP_HIP_LS_INKERNEL="0"))
    assert ri["counts"] == (0, 0, 0) and ri["mode"] == 1 and ri["redos"] == 0, (tag, ri)
    got, gi = _run(api, monkeypatch, p, B, x0, U0, env)
    assert gi["mode"] == 1 and gi["redos"] == 0, (tag, gi)
    ran, ret, gave = gi["counts"]
    print(tag, "stage-2 tiles: ran %d, returned %d, gave up %d" % (ran, ret, gave))
    _same(ref, got, tag)
    if "CDDP_HIP_TEST_LS_POLL_US" not in env:
        assert gave == 0, (tag, gi)
    if want_form:
        assert ran + ret > 0, (tag, "no launch took the in-kernel form", gi)
    return gi["counts"]


def _cartpole(api, iters):
    p = make(api, "cartpole_ipddp_box")   # rk4, N = 100
    p.options.max_iterations = iters
    return p


@pytest.mark.parametrize("first", ["1", "4", "10"])
def test_pinned_two_stage_ladder_is_bitwise_the_two_launch_form(api, first, monkeypatch):
    """Cart-pole + box, B = 150: three tiles, the last one ragged (22 lanes); a first stage of 1, 4 and 10 of the 11 step sizes."""
    p = _cartpole(api, 6)
    B = 150
    x0 = api.batch_x0(p, B, 20270111, [3.0 * v for v in spread_for(p)])
    _ab(api, monkeypatch, p, B, x0, None, {"CDDP_HIP_COSTATE": "shadow", "CDDP_HIP_LS_STAGES": "2", "CDDP_HIP_LS_FIRST": first}, ("pinned", first))


def test_adaptive_ladder_is_bitwise_the_two_launch_form(api, monkeypatch):
    """No pin: the host picks the shape (one stage, or k1 from the accepted-step histogram) from poll to poll, 12 iterations."""
    p = _cartpole(api, 12)
    B = 150
    x0 = api.batch_x0(p, B, 20270112, [3.0 * v for v in spread_for(p)])
    _ab(api, monkeypatch, p, B, x0, None, {"CDDP_HIP_COSTATE": "shadow"}, "adaptive", want_form=False)


def test_unicycle_box_ball_is_bitwise_the_two_launch_form(api, monkeypatch):
    """The nu = 2 instantiation (control box + ball rows, Euler), four full tiles."""
    p = make(api, "unicycle_ipddp_box_ball")
    p.options.max_iterations = 10
    B = 256
    x0 = api.batch_x0(p, B, 20270113, spread_for(p))
    _ab(api, monkeypatch, p, B, x0, api.batch_U0(p, B), {"CDDP_HIP_COSTATE": "shadow", "CDDP_HIP_LS_STAGES": "2"}, "unicycle")


def test_tiles_that_need_nothing_and_tiles_that_need_everything(api, monkeypatch):
    """Tile 0 is 64 copies of a start whose first iteration accepts one of the first three step sizes (every second-stage workgroup of
    the tile returns with lanes in phase), tile 1 is 64 copies of one that needs a later step size (every lane runs the second stage),
    tile 2 alternates the two.  The starts are chosen with the CPU oracle; with one iteration the counters are known exactly."""
    p = _cartpole(api, 1)
    cand = api.batch_x0(p, 48, 20270114, [3.0 * v for v in spread_for(p)])
    nf = api.oracle_solve_batch(p, cand, n_threads=4, want_traj=False)[0]["n_forward"]
    early, late = np.flatnonzero(nf <= 3), np.flatnonzero(nf > 3)
    assert len(early) > 0 and len(late) > 0, nf
    xa, xb = cand[early[0]], cand[late[0]]
    x0 = np.ascontiguousarray(np.concatenate([np.tile(xa, (64, 1)), np.tile(xb, (64, 1)), np.tile(np.stack([xa, xb]), (32, 1))]))
    B = 192
    env = {"CDDP_HIP_COSTATE": "shadow", "CDDP_HIP_LS_STAGES": "2", "CDDP_HIP_LS_FIRST": "3"}
    ran, ret, gave = _ab(api, monkeypatch, p, B, x0, None, env, "tiles-1")
    n2 = p.options.ls_max_iterations - 3   # second-stage step sizes
    assert (ran, ret, gave) == (2 * n2, n2, 0)
    p.options.max_iterations = 5
    ran, ret, gave = _ab(api, monkeypatch, p, B, x0, None, env, "tiles-5")
    assert ran > 0 and ret > 0 and gave == 0


def test_give_up_path_is_a_one_stage_launch(api, monkeypatch):
    """Test knob CDDP_HIP_TEST_LS_POLL_US=0: every second-stage workgroup with a lane in phase stops waiting at once and runs the trial for
    all of them -- what a one-stage launch does.  Same bits; give-ups = the second-stage tiles that were in phase."""
    p = _cartpole(api, 6)
    B = 150
    x0 = api.batch_x0(p, B, 20270111, [3.0 * v for v in spread_for(p)])
    env = {"CDDP_HIP_COSTATE": "shadow", "CDDP_HIP_LS_STAGES": "2", "CDDP_HIP_LS_FIRST": "4"}
    ran_n, ret_n, gave_n = _ab(api, monkeypatch, p, B, x0, None, env, "give-up/normal")
    ran, ret, gave = _ab(api, monkeypatch, p, B, x0, None, dict(env, CDDP_HIP_TEST_LS_POLL_US="0"), "give-up/zero")
    assert gave_n == 0 and ret == 0 and gave == ran and gave == ran_n + ret_n, ((ran_n, ret_n, gave_n), (ran, ret, gave))


def test_redo_takes_the_two_launch_form(api, monkeypatch):
    """CDDP_HIP_TEST_FAIL_SHADOW: the deferred costate of outer iteration 2 reports "not finite"; the solve is discarded and run again
    with the costate on the chain, where a two-stage iteration is two launches.  The bits of a CDDP_HIP_COSTATE=sync solve."""
    p = _cartpole(api, 6)
    B = 150
    x0 = api.batch_x0(p, B, 20270111, [3.0 * v for v in spread_for(p)])
    env = {"CDDP_HIP_LS_STAGES": "2", "CDDP_HIP_LS_FIRST": "4"}
    ref, ri = _run(api, monkeypatch, p, B, x0, None, dict(env, CDDP_HIP_COSTATE="sync"))
    assert ri["mode"] == 0 and ri["redos"] == 0 and ri["counts"] == (0, 0, 0), ri
    got, gi = _run(api, monkeypatch, p, B, x0, None, dict(env, CDDP_HIP_COSTATE="shadow", CDDP_HIP_TEST_FAIL_SHADOW="2"))
    assert gi["mode"] == 0 and gi["redos"] == gi["groups"] and gi["counts"] == (0, 0, 0), gi
    _same(ref, got, "redo")
