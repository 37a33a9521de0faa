"""The option table (tests/option_cases.py) on the CPU: it covers every field of cddp_hip_options, every row changes the oracle's solve,
and the oracle reads the row's options as the numpy twins do.

  * completeness: every field of pyapi.Options outside `_pad*` is moved by a row, is one of the four fields other tests cover, or is
    listed in option_cases.DEAD with what was tried and the reference line that makes it dead -- so a field added later fails here
    until it has a row (tests/test_plant_solver_matrix.py does the same for kernel sets);
  * liveness: the oracle's solve of a row differs from its solve of the same problem with the row's options at their defaults, on the
    same B = 3 perturbed starts: different counts or different bits of X.  A row that changes nothing would compare two equal solves;
  * the checker: for every row whose options the twins restate, the oracle against the twin on trajectory 0 over the row's whole solve
    -- counts equal, objective, X and U at the 1e-6 of tests/test_plant_solver_matrix.py.  The rows on the cart-pole and the unicycle,
    whose solves turn chaotic in their rounding, carry a static iteration cap (option_cases.CAPS) up to which they are well conditioned;
    a test holds every capped row to that claim.  Six rows whose override acts only after that point (option_cases.TWIN_PREFIX_ONLY)
    are shown to be ill conditioned and compared over the iterations before it."""
import numpy as np
import pytest

import option_cases as OC

B = 3
NAMES = [r.name for r in OC.ROWS]
TOL = 1e-6            # tests/test_plant_solver_matrix.py::TOL_SOLVE
MIN_PREFIX = 3        # iterations a capped or prefix comparison has at the least


def _fields(api):
    return [n for n, _ in api.Options._fields_ if not n.startswith("_pad")]


def _missing(fields):
    moved = {k for r in OC.ROWS for k in r.opts}
    return [f for f in fields if f not in moved and f not in OC.EXEMPT and f not in OC.DEAD]


def test_table_covers_every_option_field(api):
    fields = _fields(api)
    assert len(fields) >= 57 and not _missing(fields), _missing(fields)
    assert set(OC.EXEMPT) <= set(fields) and set(OC.DEAD) <= set(fields)
    # at most four options may be left dead, each with what was tried and a reference line; none of them is moved by a row
    assert len(OC.DEAD) <= 4 and all("ipddp_solver.cpp:" in why or "msipddp_solver.cpp:" in why for why in OC.DEAD.values())
    assert not {k for r in OC.ROWS for k in r.opts} & set(OC.DEAD)
    # names are unique, every family has rows, every option of a row is a field
    assert len(set(NAMES)) == len(NAMES)
    assert {r.family for r in OC.ROWS} == set(OC.FAMILIES)
    assert all(k in fields for r in OC.ROWS for k in list(r.opts) + list(r.setup))
    assert not OC._UNCHANGED & set(NAMES)


def test_a_field_added_later_is_missed_by_the_table(api):
    """The completeness test is live."""
    assert _missing(_fields(api) + ["ipddp_some_new_threshold"]) == ["ipddp_some_new_threshold"]


_memo = {}


def _oracle(api, row, override):
    key = (row.name, True) if override else (row.base, row.solver, row.start, tuple(sorted(row.setup.items())), False)
    if key not in _memo:
        p = OC.problem(api, row, override)
        _memo[key] = OC.oracle_solve(api, p, row, OC.starts(api, p, row, B), n_threads=B)
    return _memo[key]


@pytest.mark.parametrize("name", NAMES)
def test_row_changes_the_oracle_solve(api, oracle_built, name):
    row = OC.BY_NAME[name]
    rd, Xd = _oracle(api, row, False)[:2]
    rv, Xv = _oracle(api, row, True)[:2]
    assert np.all(np.isfinite(Xv)), name
    assert OC.counts(rd) != OC.counts(rv) or not np.array_equal(Xd, Xv), (name, row.opts, OC.counts(rd))


def test_every_option_has_a_row_that_decides_something(api, oracle_built):
    """Different bits are enough for a row to be live, but a kernel that ignored the option would still pass a 1e-6 comparison on such a
    row.  Every option therefore has a row on which the override changes a count of some trajectory or moves X by more than 1e-3."""
    decided = set()
    for row in OC.ROWS:
        rd, Xd = _oracle(api, row, False)[:2]
        rv, Xv = _oracle(api, row, True)[:2]
        if OC.counts(rd) != OC.counts(rv) or np.max(np.abs(Xd - Xv)) > 1e-3:
            decided |= set(row.opts)
    assert {k for r in OC.ROWS for k in r.opts} <= decided, sorted({k for r in OC.ROWS for k in r.opts} - decided)


@pytest.mark.parametrize("name", [r.name for r in OC.IGNORED])
def test_option_the_solver_does_not_read_changes_nothing(api, oracle_built, name):
    """... and the twin, which restates that solver's own ladder, agrees with the oracle on the row."""
    row = OC.BY_NAME[name]
    rd, Xd = _oracle(api, row, False)[:2]
    rv, Xv = _oracle(api, row, True)[:2]
    assert OC.counts(rd) == OC.counts(rv) and np.array_equal(Xd, Xv), name
    _twin_row(api, name)


def _history(api, p, x0, U0, X0):
    o = api.Oracle(p); o.set_initial(x0, U0, X0); r = o.solve()
    return o.history(), int(r["iterations"])


def stable_prefix(api, row):
    """How many leading iterations of the oracle's solve of trajectory 0 are the same solve under a relative 1e-12 change of x0: the
    iteration history (cost, merit, residuals, step sizes, mu, regularisation) agrees at 1e-9 row by row (a thousandfold amplification of the change).  The row's own max_iterations
    where the whole solve agrees and ends in the same iteration."""
    p = OC.problem(api, row); p.options.return_iteration_info = 1
    x0, U0, X0 = OC.starts(api, p, row, 1)
    u = None if U0 is None else U0[0]
    h0, it0 = _history(api, p, x0[0], u, None if X0 is None else X0[0])
    n = len(h0); same_end = True
    for eps in (1e-12, -1e-12, 3e-12):
        x1 = x0[0] + eps * np.maximum(1.0, np.abs(x0[0]))
        g = None
        if X0 is not None:
            g = X0[0].copy(); g[0] = x1
        h1, it1 = _history(api, p, x1, u, g)
        same_end = same_end and it1 == it0 and len(h1) == len(h0)
        k = 0
        while k < min(len(h0), len(h1)):
            a, b = h0[k], h1[k]
            fin = np.isfinite(a) & np.isfinite(b)
            if not np.array_equal(np.isfinite(a), np.isfinite(b)) or np.max(np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin])), initial=0.0) > 1e-9:
                break
            k += 1
        n = min(n, k)
    if same_end and n == len(h0):
        return int(p.options.max_iterations)
    return max(0, n - 1)          # history row 0 is the initial iterate: n agreeing rows are n - 1 iterations


def _against_twin(api, row):
    """(counts equal, worst errors, the figures) of the oracle against the twin on trajectory 0 of the row."""
    p = OC.problem(api, row)
    x0, U0, X0 = OC.starts(api, p, row, 1)
    u = None if U0 is None else U0[0]; g = None if X0 is None else X0[0]
    res, X, U, _ = OC.oracle_solve(api, p, row, (x0, U0, X0), n_threads=1)
    tw = OC.twin_solve(row, x0[0], u, g)
    got = OC.counts(res)[0]
    got = (got[0], api.STATUS_STRINGS[got[1]], got[2], got[3])
    worst = {"J": abs(res["final_objective"][0] - tw["final_objective"]) / max(1.0, abs(tw["final_objective"])),
             "X": float(np.max(np.abs(X[0] - tw["X"]))), "U": float(np.max(np.abs(U[0] - tw["U"])))}
    return got == tw["counts"], worst, (got, tw["counts"])


TWIN_ROWS = [r.name for r in OC.ROWS if OC.twin_reads(r)]
_whole = {}           # row name -> the whole solve agreed


def _twin_row(api, name):
    """The row's whole solve, oracle against twin; for the TWIN_PREFIX_ONLY rows its well-conditioned iterations."""
    if name in _whole:
        assert _whole[name] is not False, name
        return
    row = OC.BY_NAME[name]
    label = "whole solve"
    _whole[name] = False
    if name in OC.TWIN_PREFIX_ONLY:
        iters = stable_prefix(api, row)
        assert MIN_PREFIX <= iters < OC.problem(api, row).options.max_iterations, (name, iters)    # ill conditioned, as the table says
        row = row._replace(setup=dict(row.setup, max_iterations=iters)); label = "first %d iterations" % iters
    same, worst, figures = _against_twin(api, row)
    print("TWIN %s %s oracle %s twin %s %s" % ((name, label) + figures + (" ".join("%s %.1e" % kv for kv in worst.items()),)))
    assert same, (name, label, figures)
    assert all(np.isfinite(v) and v < TOL for v in worst.values()), (name, label, worst)
    _whole[name] = None if name in OC.TWIN_PREFIX_ONLY else True


@pytest.mark.parametrize("name", TWIN_ROWS)
def test_oracle_reads_the_row_as_the_twin_does(api, oracle_built, name):
    """Trajectory 0: counts equal, objective, X and U at 1e-6."""
    _twin_row(api, name)


@pytest.mark.parametrize("name", sorted(OC.CAPS))
def test_capped_row_is_a_well_conditioned_solve(api, oracle_built, name):
    """The cap of option_cases.CAPS is not past the point where the oracle's own iteration history moves under a relative 1e-12 change
    of x0: up to the cap the row is one solve, whoever computes it."""
    row = OC.BY_NAME[name]
    assert row.setup["max_iterations"] == OC.CAPS[name] >= MIN_PREFIX
    assert stable_prefix(api, row) == OC.CAPS[name], (name, stable_prefix(api, row))


def test_every_option_the_twins_read_is_compared_over_a_whole_solve(api, oracle_built):
    """Every option a twin restates has at least one row whose whole solve agrees with the twin's -- a solve the liveness test shows
    the option changes -- and the rows held over a prefix only are the listed six, each with the sibling the table names."""
    assert set(OC.TWIN_PREFIX_ONLY) <= set(TWIN_ROWS)
    assert all(v == "*" or (v in TWIN_ROWS and v not in OC.TWIN_PREFIX_ONLY) for v in OC.TWIN_PREFIX_ONLY.values())
    whole = [n for n in TWIN_ROWS if n not in OC.TWIN_PREFIX_ONLY]
    covered = {k for n in whole for k in OC.BY_NAME[n].opts}
    wanted = {k for n in TWIN_ROWS for k in OC.BY_NAME[n].opts}
    assert wanted <= covered, sorted(wanted - covered)
    assert wanted >= {k for k in OC.OPTION_NAMES if k not in OC.EXEMPT and k not in OC.DEAD}, sorted(set(OC.OPTION_NAMES) - wanted)


def test_pairs_without_a_live_row_are_the_listed_ones():
    """option_cases.NO_LIVE_ROW is exactly what the loops tried and dropped: a pair that gains or loses its rows fails here."""
    tried = {(k, r.family) for r in OC.TRIED for k in r.opts}
    live = {(k, r.family) for r in OC.ROWS for k in r.opts}
    assert tried - live == {(k, f) for f, ks in OC.NO_LIVE_ROW.items() for k in ks}


# ---------------------------------------------------------------------------------------------------------------- the capacities (host side)
def test_build_alphas_reports_the_untruncated_length(api):
    import ctypes as C
    import __graft_entry__ as g
    import os
    if not os.path.exists(api.HIP_LIB_PATH):
        g.build()
    lib = api.load_hip()
    o = api.default_options(); o.ls_max_iterations = 40; o.ls_step_reduction_factor = 0.8
    a = np.zeros(32)
    assert lib.cddp_hip_build_alphas(C.byref(o), None, 0) == 40
    assert lib.cddp_hip_build_alphas(C.byref(o), a.ctypes.data_as(C.POINTER(C.c_double)), 32) == 32 and np.isclose(a[-1], 0.8 ** 31, rtol=1e-14)
    o.ls_step_reduction_factor = 0.5                      # stops at ls_min_step_size = 1e-8 after 27 halvings
    assert lib.cddp_hip_build_alphas(C.byref(o), None, 0) == 28


@pytest.mark.parametrize("solver,opts,msg", [
    ("ipddp", dict(ls_max_iterations=33, ls_step_reduction_factor=0.8), "ls_max_iterations = 33 gives a ladder of 33 step sizes, more than CDDP_HIP_MAX_ALPHAS = 32"),
    ("msipddp", dict(ls_max_iterations=33, ls_step_reduction_factor=0.8), "ls_max_iterations = 33 gives a ladder of 33 step sizes, more than CDDP_HIP_MAX_ALPHAS = 32"),
    # LogDDP walks the plain geometric ladder (logddp_solver.cpp:177-182): 40 halvings are 40 step sizes there, 28 under the others
    ("logddp", dict(ls_max_iterations=40), "ls_max_iterations = 40 gives a ladder of 40 step sizes, more than CDDP_HIP_MAX_ALPHAS = 32"),
    ("ipddp", dict(ipddp_max_filter_size=8), r"ipddp_max_filter_size = 8: the filter holds max_filter_size \+ 1 points before it is pruned and has 8 slots, so at most 7"),
])
def test_create_refuses_what_a_handle_cannot_hold(api, solver, opts, msg):
    """cddp_hip_create checks the two fixed capacities before it touches a device, so the refusals show without one."""
    row = OC.Row("x", "pendulum40", solver, opts, "", "cold", {})
    with pytest.raises(api.HipError, match=msg):
        api.HipBatchSolver(OC.problem(api, row), 4)
