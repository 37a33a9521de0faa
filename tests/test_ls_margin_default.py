"""Default of CDDP_HIP_LS_MARGIN (capi.hip::SolveRun::adapt_ladder): the first stage of a two-stage ladder is the histogram's count kq
plus a margin.  Unset, the margin is 0 where both stages run in one rollout launch (SolveRun::inkernel: a miss costs one tile's chain
inside the launch) and 1 for every two-launch shape; an explicit value holds everywhere.  The switches are read when a handle is
created and the ladder decisions go to stderr (CDDP_HIP_DEBUG_LADDER), so each side runs in a child process of its own."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(%(repo)r, "tests"))
import conftest
api = conftest.load_api()
p = api.cartpole_problem(api.SOLVER_IPDDP, True)
B = 256
x0 = api.batch_x0(p, B, 20271721, [0.1, 0.3, 0.1, 0.1])
hs = api.HipBatchSolver(p, B); hs.set_initial(x0, api.batch_U0(p, B)); st = hs.solve()
r = hs.results(); X, U = hs.trajectory(); K, k = hs.gains()
ran, ret, gave = hs.ls_stage_counts()
print("MODE", hs.costate_mode(), "STAGE2", ran + ret, "NA", p.options.ls_max_iterations)
np.savez(%(out)r, X=X, U=U, K=K, k=k, iterations=r["iterations"], status=r["status"], final_objective=r["final_objective"])
hs.close()
'''

LADDER = re.compile(r"\[ladder\] it=(\d+) total=\d+ kq=(\d+) -> (one|two) k1=(\d+)")


def _child(tmp_path, tag, env):
    out = str(tmp_path / (tag + ".npz"))
    e = dict(os.environ, CDDP_HIP_DEBUG_LADDER="1")
    for k in ("CDDP_HIP_LS_MARGIN", "CDDP_HIP_LS_INKERNEL", "CDDP_HIP_LS_STAGES", "CDDP_HIP_LS_FIRST", "CDDP_HIP_COSTATE", "CDDP_HIP_GROUPS"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD % {"repo": REPO, "out": out}], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (tag, r.stdout[-1000:], r.stderr[-3000:])
    head = [l for l in r.stdout.splitlines() if l.startswith("MODE")][-1].split()
    lines = [(int(m.group(1)), int(m.group(2)), m.group(3), int(m.group(4))) for m in LADDER.finditer(r.stderr)]
    return {"mode": int(head[1]), "stage2": int(head[3]), "na": int(head[5]), "ladder": lines, "data": dict(np.load(out))}


def _margins(run, m):
    """k1 - kq of every decision that sets k1 from the histogram (kq < na - 1) and that a margin of m does not push into the cap of na - 1
    step sizes (at B = 256 the one-wave-per-SIMD cap is far above the ladder's length)."""
    na = run["na"]
    return [k1 - kq for _, kq, _, k1 in run["ladder"] if kq < na - 1 and kq + m <= na - 1]


@pytest.mark.gpu
def test_margin_is_zero_in_kernel_and_one_with_two_launches(tmp_path):
    ink = _child(tmp_path, "inkernel", {})
    two = _child(tmp_path, "two_launch", {"CDDP_HIP_LS_INKERNEL": "0"})
    pin = _child(tmp_path, "explicit", {"CDDP_HIP_LS_MARGIN": "2"})
    print("in-kernel:", ink["ladder"]); print("two-launch:", two["ladder"]); print("explicit 2:", pin["ladder"])
    assert ink["mode"] == 1 and two["mode"] == 1 and pin["mode"] == 1            # all three on the deferred costate
    assert two["stage2"] == 0                                                     # ... and only the first with stages inside a launch
    m_ink, m_two, m_pin = _margins(ink, 0), _margins(two, 1), _margins(pin, 2)
    assert len(m_ink) > 0 and len(m_two) > 0 and len(m_pin) > 0, "no decision took k1 from the histogram"
    assert set(m_ink) == {0}, m_ink
    assert set(m_two) == {1}, m_two
    assert set(m_pin) == {2}, m_pin                                               # an explicit value wins on the in-kernel form too
    # the selected trials do not depend on the ladder's shape (the work counters do: a shorter first stage evaluates fewer trials)
    for other in (two, pin):
        for name in ("iterations", "status", "final_objective", "X", "U", "K", "k"):
            assert np.array_equal(ink["data"][name], other["data"][name], equal_nan=True), name
