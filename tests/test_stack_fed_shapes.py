"""Every stack-fed shape against the stack-level numpy reference (oracle/twin/stack_twin.py), not against another GPU result.

For every (nx, nu, m) that pick() or pick_coop() instantiates (stacks.hip) and every branch the shape admits, the sweep of the one data set
generator (tests/stack_data.py) is compared with the float64 reference: ok and reg exactly, every other output within 1e-9 relative -- on
the handle's default form and layout and on every other combination the handle admits (CDDP_HIP_STACKS_SWEEP = lane | coop,
CDDP_HIP_STACKS_LAYOUT = plain | t4), at the main batch / horizon and at the edges (a lone trajectory, a ragged 4-tile, a ragged wavefront,
a one-step horizon).  Also: the batch where the default form flips, and stacks with more than 65535 rows (the transposition's grid).
tests/test_stack_twin.py pins the reference to the solver twins and checks that these data sets are far from every knife-edge."""
import numpy as np
import pytest

import stack_data as D

pytestmark = pytest.mark.gpu
TOL = 1e-9

# the (nx, nu, m) lists of pick() (the non-development block) and pick_coop() in cddp-cpp_amd/csrc/stacks.hip -- tests/test_stack_twin.py
# parses the source and holds these lists equal to it
LANE_SHAPES = [(1, 1, 0), (1, 1, 1), (1, 1, 2), (2, 1, 0), (2, 1, 2), (3, 1, 0), (3, 1, 2), (4, 1, 0), (4, 1, 2),
               (3, 2, 0), (3, 2, 4), (3, 2, 5), (4, 2, 0), (4, 2, 4), (6, 3, 0), (6, 3, 6), (8, 3, 0), (8, 3, 6),
               (12, 4, 0), (12, 4, 8), (13, 4, 0), (13, 4, 8), (14, 7, 0)]
COOP_SHAPES = [(4, 1, 0), (4, 1, 2), (3, 2, 0), (3, 2, 5), (6, 3, 0), (6, 3, 6),
               (12, 4, 0), (12, 4, 8), (13, 4, 0), (13, 4, 8), (14, 7, 0), (14, 7, 14)]
SHAPES = sorted(set(LANE_SHAPES) | set(COOP_SHAPES))
# pick_te() in cddp-cpp_amd/csrc/stacks_te.hpp: (nx, nu) of the terminal-equality sweep (tests/test_stack_fed.py runs them)
TE_SHAPES = [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2), (6, 3)]


def branches(shape):
    nx, nu, m = shape
    if m == 0:
        return ["clddp", "clddp_box", "clddp_retry", "ipddp", "ipddp_hess", "logddp", "logddp_hess", "msipddp"]
    return ["path", "path_hess"] + (["mspath"] if nu == 1 else [])


def datasets(shape):
    """(B, N): the main case, then a lone trajectory over one step, a ragged 4-tile, a ragged wavefront over one step."""
    return [(9, 9) if shape[0] >= 12 else (67, 17), (1, 1), (5, 2), (67, 1)]


def bad_trajectories(B):
    return tuple(b for b in range(B) if b % 7 == 3) or (0,)


def twin_options():
    import cddp_twin as T
    return T.default_options()


def reference(branch, c, b, opt):
    """The reference outputs of trajectory b, one dict per sweep the GPU side runs (two for clddp_box and clddp_retry)."""
    import stack_twin as S
    st = D.trajectory(c, b); reg = float(c["reg"][b])
    once = dict(opt, reg_update_factor=0.0)
    hess = (st["Fxx"], st["Fuu"], st["Fux"])
    if branch in ("clddp", "clddp_retry"):
        outs = [S.retry(lambda r: S.clddp(st, r, opt), reg, once)]
        if branch == "clddp_retry":
            outs.append(S.retry(lambda r: S.clddp(st, r, opt), reg, opt))
        return outs
    if branch == "clddp_box":
        kw = np.zeros_like(st["lu"])   # the handle's k stack starts zeroed: the first sweep's warm start
        return [S.retry(lambda r: S.clddp(st, r, opt, (c["lo"], c["up"]), st["U"], kw), reg, once) for _ in range(2)]
    if branch in ("ipddp", "ipddp_hess"):
        return [S.retry(lambda r: S.ipddp(st, r, hess if branch == "ipddp_hess" else None), reg, once)]
    if branch in ("logddp", "logddp_hess"):
        return [S.retry(lambda r: S.logddp(st, r, hess if branch == "logddp_hess" else None), reg, once)]
    if branch == "msipddp":
        return [S.retry(lambda r: S.msipddp(st, r, st["d"]), reg, once)]
    if branch in ("path", "path_hess"):
        return [S.retry(lambda r: S.ipddp_path(st, r, float(c["mu"][b]), opt, hess if branch == "path_hess" else None), reg, once)]
    if branch == "mspath":
        return [S.retry(lambda r: S.msipddp_path(st, r, float(c["mu"][b]), st["d"]), reg, once)]
    raise KeyError(branch)


def make_data(shape, branch, B, N):
    nx, nu, m = shape
    c = D.make_case(nx, nu, m, B, N, bad=bad_trajectories(B) if branch == "clddp_retry" else ())
    if branch == "clddp_box":   # CLDDP keeps V_xxN as it is, and BoxQP's LDLT reads one triangle: a skew part would end most sweeps in NO_DESCENT
        c["VxxN"] = 0.5 * (c["VxxN"] + np.swapaxes(c["VxxN"], 1, 2))
    return c


_REF = {}


def cached_reference(shape, branch, B, N, idx=None):
    key = (shape, branch, B, N)
    if key not in _REF:
        c = make_data(shape, branch, B, N)
        opt = twin_options()
        idx = range(B) if idx is None else idx
        _REF[key] = (c, {b: reference(branch, c, b, opt) for b in idx})
    return _REF[key]


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


ARRAYS = ("K", "k", "Vx", "Vxx", "dV")
PATH_ARRAYS = ("ky", "Ky", "ks", "Ks")
SCALARS = ("inf_du", "inf_pr", "inf_comp", "step_norm", "alpha_pr_max", "alpha_du_max")


def run_gpu(api, shape, branch, c, env, monkeypatch):
    """Upload the data set, run the branch's sweeps, download every output.  env: {variable: value or None}."""
    nx, nu, m = shape
    B, N = c["fx"].shape[:2]
    for var in ("CDDP_HIP_STACKS_LAYOUT", "CDDP_HIP_STACKS_SWEEP"):
        monkeypatch.delenv(var, raising=False)
    if env.get("CDDP_HIP_STACKS_LAYOUT"):
        monkeypatch.setenv("CDDP_HIP_STACKS_LAYOUT", env["CDDP_HIP_STACKS_LAYOUT"])
    hs = api.HipStackSolver(B, nx, nu, m, N)
    monkeypatch.delenv("CDDP_HIP_STACKS_LAYOUT", raising=False)
    if env.get("CDDP_HIP_STACKS_SWEEP"):
        monkeypatch.setenv("CDDP_HIP_STACKS_SWEEP", env["CDDP_HIP_STACKS_SWEEP"])
    try:
        hs.set_stacks(*[c[k] for k in D.STACK_KEYS])
        if m:
            hs.set_constraint_stacks(*[c[k] for k in D.PATH_KEYS])
        if branch.endswith("_hess"):
            hs.set_hessian_stacks(*[c[k] for k in D.HESS_KEYS])
        if branch in ("msipddp", "mspath"):
            hs.set_defect_stack(c["d"])
        if branch == "clddp_box":
            hs.set_control_box(c["lo"], c["up"], c["U"])
        const = {"clddp": api.STACKS_CLDDP, "clddp_box": api.STACKS_CLDDP, "clddp_retry": api.STACKS_CLDDP, "ipddp": api.STACKS_IPDDP,
                 "ipddp_hess": api.STACKS_IPDDP, "logddp": api.STACKS_LOGDDP, "logddp_hess": api.STACKS_LOGDDP, "msipddp": api.STACKS_MSIPDDP,
                 "path": api.STACKS_IPDDP_PATH, "path_hess": api.STACKS_IPDDP_PATH, "mspath": api.STACKS_MSIPDDP_PATH}[branch]
        retries = {"clddp_retry": (False, True), "clddp_box": (False, False)}.get(branch, (False,))
        opt = api.default_options()
        outs = []
        for rt in retries:
            ok = hs.backward(const, opt, c["reg"], c.get("mu") if m else None, retry=rt)
            o = {"ok": ok.copy(), "form": hs.sweep_form()}
            o.update(zip(ARRAYS, hs.gains()))
            o.update(hs.scalars())
            if m:
                o.update(zip(PATH_ARRAYS + ("dX",), hs.constraint_gains()))
            outs.append(o)
    finally:
        hs.close()
    return outs


def compare(got, refs, idx, label, failures):
    """got: one dict of GPU outputs of one sweep (batch arrays); refs: {b: reference dict} of that sweep."""
    for b in idx:
        r = refs[b]
        if bool(got["ok"][b]) != bool(r["ok"]) or got["reg"][b] != r["reg"]:
            failures.append("%s b=%d: ok %d / %d, reg %r / %r" % (label, b, got["ok"][b], r["ok"], got["reg"][b], r["reg"]))
            continue
        if not r["ok"]:
            continue
        names = list(ARRAYS) + list(SCALARS) + [n for n in PATH_ARRAYS + ("dX",) if n in r]
        for n in names:
            e = rel(got[n][b], r[n])
            if not e <= TOL:
                failures.append("%s b=%d: %s rel %.3g" % (label, b, n, e))
                break


def default_form(shape, B):
    """The handle's default (stacks.hip, cddp_hip_stacks_create_abi): the cooperative form and tile-minor stacks from nx = 6 on, for a shape
    without a one-lane kernel, and for the small shapes with path rows up to a batch threshold."""
    nx, nu, m = shape
    coop, lane = shape in COOP_SHAPES, shape in LANE_SHAPES
    return int(coop and (nx >= 6 or not lane or (m > 0 and B <= (16384 if nx <= 3 else 8192))))


def combos(shape, B):
    """(label, env, expected form): the default first, then every other (sweep, layout) the handle admits."""
    lane, coop = shape in LANE_SHAPES, shape in COOP_SHAPES
    d = default_form(shape, B)
    out = [("default", {}, d)]
    forms = (["lane"] if lane else []) + (["coop"] if coop else [])
    layouts = ["plain", "t4"] if coop else ["plain"]
    for f in forms:
        for l in layouts:
            if (f == "coop") == bool(d) and (l == "t4") == bool(d):
                continue   # that is the default
            out.append(("%s/%s" % (f, l), {"CDDP_HIP_STACKS_SWEEP": f, "CDDP_HIP_STACKS_LAYOUT": l}, 1 if f == "coop" else 0))
    return out


def check_options_agree(api):
    opt, tw = api.default_options(), twin_options()
    assert opt.reg_update_factor == tw["reg_update_factor"] and opt.reg_max_value == tw["reg_max_value"] and opt.reg_min_value == tw["reg_min_value"]
    assert opt.termination_scaling_max_factor == tw["termination_scaling_max_factor"]
    assert opt.barrier_min_fraction_to_boundary == tw["min_fraction_to_boundary"]
    for key, val in tw.items():
        if key.startswith("boxqp_") and hasattr(opt, key):
            assert getattr(opt, key) == val, key


CASES = [(s, br) for s in SHAPES for br in branches(s)]


@pytest.mark.parametrize("shape,branch", CASES, ids=["nx%d_nu%d_m%d-%s" % (s + (br,)) for s, br in CASES])
def test_shape_branch_against_the_reference(api, shape, branch, monkeypatch):
    check_options_agree(api)
    failures = []
    for B, N in datasets(shape):
        c, refs = cached_reference(shape, branch, B, N)
        for label, env, form in combos(shape, B):
            outs = run_gpu(api, shape, branch, c, env, monkeypatch)
            for i, got in enumerate(outs):
                tag = "B=%d N=%d %s sweep %d" % (B, N, label, i)
                if got["form"] != form:
                    failures.append("%s: ran form %d, expected %d" % (tag, got["form"], form))
                compare(got, {b: refs[b][i] for b in refs}, range(B), tag, failures)
        if branch == "clddp_retry":   # the data exercise the loop: the first sweep fails where l_uu is indefinite, the retry succeeds
            bad = bad_trajectories(B)
            assert not any(refs[b][0]["ok"] for b in bad) and all(refs[b][1]["ok"] for b in range(B)) and all(refs[b][1]["retries"] > 0 for b in bad)
        if branch == "clddp_box" and (B, N) == datasets(shape)[0]:
            free = np.array([refs[b][1]["free"] for b in range(B)])
            assert free.any() and not free.all(), "the box data should clamp some rows and leave others free"
        if branch.startswith("path") and (B, N) == datasets(shape)[0]:
            assert any(refs[b][0]["alpha_pr_max"] < 1.0 for b in range(B)), "some step caps should fall below 1"
    assert not failures, "%d mismatches:\n  %s" % (len(failures), "\n  ".join(failures[:40]))


FLIP_N = 4
GRID_B = 9
GRID_CASES = [((12, 4, 0), 40), ((13, 4, 0), 31)]


def flip_sample(B):
    """About 64 trajectories strided over the batch, and the last eight."""
    return sorted(set(range(0, B, B // 64)) | set(range(B - 8, B)))


@pytest.mark.parametrize("shape,B", [((4, 1, 2), 8192), ((4, 1, 2), 8256), ((3, 2, 5), 16384), ((3, 2, 5), 16448)],
                         ids=lambda v: str(v))
def test_default_form_flip_against_the_reference(api, shape, B, monkeypatch):
    """Small shapes with path rows take the cooperative form while the batch leaves the chip mostly empty under the one-lane one: both sides of
    the threshold, a strided sample of trajectories and the last eight against the reference."""
    idx = flip_sample(B)
    c, refs = cached_reference(shape, "path", B, FLIP_N, idx)
    got = run_gpu(api, shape, "path", c, {}, monkeypatch)[0]
    assert got["form"] == default_form(shape, B) == (1 if B in (8192, 16384) else 0)
    failures = []
    compare(got, {b: refs[b][0] for b in idx}, idx, "B=%d" % B, failures)
    assert not failures, "\n".join(failures[:40])


@pytest.mark.parametrize("shape,N", GRID_CASES, ids=lambda v: str(v))
def test_stacks_past_the_grid_limit(api, shape, N, monkeypatch):
    """F_xx of nx = 12 over 40 steps is 69120 stack rows, of nx = 13 over 31 steps 68107: more than a grid's y extent (65535) -- upload,
    sweep and download of every row against the reference."""
    B = GRID_B
    assert N * shape[0] ** 3 > 65535
    c, refs = cached_reference(shape, "ipddp_hess", B, N)
    failures = []
    for label, env, form in combos(shape, B):
        got = run_gpu(api, shape, "ipddp_hess", c, env, monkeypatch)[0]
        assert got["form"] == form
        compare(got, {b: refs[b][0] for b in refs}, range(B), label, failures)
    assert not failures, "\n".join(failures[:40])
