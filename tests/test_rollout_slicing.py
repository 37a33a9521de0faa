"""Time-sliced wave priority in the two-role IPDDP rollout (kernels_lean.hpp::k_forward_ipddp_pc_sl, arguments slice_ticks / late_from;
launch.hpp::PcSlice: the cart-pole and unicycle layouts; capi.hip::roll_slice_for).  Where a launch puts more waves on the stream's share
of the chip than it has SIMDs, the early- and the late-placed workgroups take wave priority 3 in alternating windows of the wall clock.
Priority decides WHEN an instruction issues, never what it computes, so everything a caller can read must be the same bits as with the
switch off (CDDP_HIP_K4_SLICE_US=0).

CDDP_HIP_K4_SLICE_US=2 forces a short window on every rollout launch, those of cddp_hip_forward included (at these batches no launch
oversubscribes, so the default rule alone would leave the window off); CDDP_HIP_K4_LATE_PRIO=1, the fixed-priority comparison mode,
goes through the same arguments and is held to the same bits.  With the switch off the launch is k_forward_ipddp_pc, the kernel every
other layout runs."""
import numpy as np
import pytest

from test_costate_shadow import _same, _snapshot
from test_gpu_parity import make, spread_for
from test_rollout_straightline import assert_same, cartpole, snapshot

pytestmark = pytest.mark.gpu

SWITCHES = ("CDDP_HIP_K4_SLICE_US", "CDDP_HIP_K4_LATE_PRIO", "CDDP_HIP_LS_STAGES", "CDDP_HIP_LS_FIRST", "CDDP_HIP_K4_NA", "CDDP_HIP_K4_CONSUMERS")
OFF = {"CDDP_HIP_K4_SLICE_US": "0"}
MODES = {"window": {"CDDP_HIP_K4_SLICE_US": "2"}, "fixed_late": {"CDDP_HIP_K4_SLICE_US": "2", "CDDP_HIP_K4_LATE_PRIO": "1"}}


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def cartpole_off(api):
    """The switch-off side of the cart-pole shape, computed once per ladder shape and left unchanged."""
    cache = {}

    def get(monkeypatch, ladder):
        if ladder not in cache:
            _env(monkeypatch, dict(OFF, **LADDERS[ladder][0]))
            cache[ladder] = snapshot(api, **_cartpole_case(api, ladder))
        return cache[ladder]
    return get


LADDERS = {"whole": ({"CDDP_HIP_LS_STAGES": "1"}, None), "first4": ({"CDDP_HIP_LS_STAGES": "2", "CDDP_HIP_LS_FIRST": "4"}, 4)}


def _cartpole_case(api, ladder):
    B = 150   # three tiles, the last one ragged (22 lanes); N = 100, RK4
    p = cartpole(api, "RK4")
    return dict(mk=lambda it: cartpole(api, "RK4", it), B=B, x0=api.batch_x0(p, B, 20271701, [0.1, 0.3, 0.1, 0.1]), n_alpha=LADDERS[ladder][1], iters=3)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("ladder", sorted(LADDERS))
def test_cartpole_box_is_bitwise_the_switch_off(api, monkeypatch, cartpole_off, ladder, mode):
    """Cart-pole + box, B = 150, N = 100: the trial records of one forward pass, then the iterate, duals, gains, result records and work
    counters after three iterations -- the whole ladder in one launch, and a split with a first stage of four step sizes."""
    ref = cartpole_off(monkeypatch, ladder)
    _env(monkeypatch, dict(MODES[mode], **LADDERS[ladder][0]))
    got = snapshot(api, **_cartpole_case(api, ladder))
    assert_same(got, ref, (ladder, mode))


def test_unicycle_box_ball_whole_solve_is_bitwise_the_switch_off(api, monkeypatch):
    """The nu = 2 instantiation (control box + ball rows, Euler), four full tiles, a whole solve with the default ladder rules."""
    p = make(api, "unicycle_ipddp_box_ball")
    B = 256
    x0 = api.batch_x0(p, B, 20271702, spread_for(p))
    U0 = api.batch_U0(p, B)

    def run(env):
        _env(monkeypatch, env)
        hs = api.HipBatchSolver(p, B); hs.set_initial(x0, U0); st = hs.solve()
        snap = _snapshot(hs, st); hs.close()
        return snap

    ref = run(OFF)
    for mode in sorted(MODES):
        _same(ref, run(MODES[mode]), ("unicycle", mode))
