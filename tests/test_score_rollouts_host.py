"""CPU-side checks of cddp_hip_score_rollouts / cddp_hip_seed_best: HipBatchSolver.score_rollouts and seed_best validate shapes, dtypes
and the kind of their arguments in Python BEFORE any library call (the object under test has a library that fails on every access); the
two entries are exported, declared with the documented signatures and flags, bound with matching argtypes, and answer the refusals that
need no device with their own messages; the facade and the C++ mirror offer them.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, N, NX, NU = 6, 3, 5, 4, 2


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the arguments were validated" % name)


class Dims:
    N, nx, nu = N, NX, NU


@pytest.fixture()
def solver(api):
    h = api.HipBatchSolver.__new__(api.HipBatchSolver)       # no handle, no device: only what the validation reads
    h.lib = NoLibrary(); h.p = Dims(); h.B = B; h.h = None; h._device = 0; h._user_stream = False; h.plan_epoch = 0
    return h


def test_score_rollouts_validates_before_any_library_call(solver):
    U = np.zeros((B, S, N, NU)); x0 = np.zeros((B, NX))
    bad = [
        (dict(U=None), "U is None without feedback"),
        (dict(U=np.zeros((B, S, N))), "U: shape"),
        (dict(U=np.zeros((B, S, N + 1, NU))), "U: shape"),
        (dict(U=np.zeros((B + 1, S, N, NU))), "U: shape"),
        (dict(U=np.zeros((B, 0, N, NU))), "at least one candidate"),
        (dict(U=U.astype(np.float32)), "dtype float64"),
        (dict(U=U, x0=np.zeros((B, NX + 1))), "x0: shape"),
        (dict(U=U, x0=np.zeros((B, S + 1, NX))), "x0: shape"),
        (dict(U=U, x0=x0.astype(np.int64)), "dtype float64"),
        (dict(U=U, x0=x0, want=("cost", "merit")), "want"),
        (dict(U=U, x0=x0, ncand=S + 1), "ncand"),
        (dict(U=None, feedback=True, ncand=0), "at least one candidate"),
    ]
    for kw, needle in bad:
        with pytest.raises(ValueError, match=re.escape(needle)):
            solver.score_rollouts(**kw)
    # ... and a well-formed call does reach the library
    with pytest.raises(AssertionError, match="cddp_hip_score_rollouts"):
        solver.score_rollouts(U, x0=x0)
    with pytest.raises(AssertionError, match="cddp_hip_score_rollouts"):
        solver.score_rollouts(None, x0=np.zeros((B, S, NX)), feedback=True)


def test_seed_best_validates_before_any_library_call(solver):
    U = np.zeros((B, S, N, NU)); cost = np.zeros((B, S)); x0 = np.zeros((B, NX))
    bad = [
        (dict(U=None, cost=cost), "required"),
        (dict(U=U, cost=None), "required"),
        (dict(U=np.zeros((B, S, N * NU)), cost=cost), "U: shape"),
        (dict(U=U, cost=np.zeros((B, S + 1))), "cost: shape"),
        (dict(U=U, cost=cost.astype(np.float32)), "dtype float64"),
        (dict(U=U, cost=cost, viol=np.zeros((B,))), "viol: shape"),
        (dict(U=U, cost=cost, x0=np.zeros((B, S, NX))), "x0: shape"),
        (dict(U=U, cost=cost, viol_tol="loose"), "could not convert"),
    ]
    for kw, needle in bad:
        with pytest.raises(ValueError, match=re.escape(needle)):
            solver.seed_best(**kw)
    with pytest.raises(AssertionError, match="cddp_hip_seed_best"):
        solver.seed_best(U, cost, viol=cost, x0=x0, viol_tol=0.5)


def test_mixed_kinds_are_refused(solver):
    torch = pytest.importorskip("torch")
    U = np.zeros((B, S, N, NU)); cost = np.zeros((B, S))
    with pytest.raises(ValueError, match="numpy arrays"):
        solver.seed_best(U, torch.zeros((B, S), dtype=torch.float64))
    with pytest.raises(ValueError):
        solver.score_rollouts(torch.zeros((B, S, N, NU), dtype=torch.float64), x0=np.zeros((B, NX)))   # a CPU tensor is no device tensor either
    with pytest.raises(ValueError):
        solver.seed_best(torch.zeros((B, S, N, NU), dtype=torch.float64), cost)


# ---- the C boundary
SYMBOLS = ("cddp_hip_score_rollouts", "cddp_hip_seed_best")


@pytest.fixture(scope="module")
def lib(api):
    if not os.path.exists(api.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return api.load_hip()


def header():
    txt = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def declaration(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m, "%s is not declared in include/cddp_hip.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_library_and_binding_agree(api, lib):
    assert declaration("cddp_hip_score_rollouts") == ["cddp_hip_handle *h", "cddp_hip_plant *plant", "int flags", "int ncand", "const double *x0",
                                                      "const double *U", "double *cost", "double *viol", "double *X_out", "double *U_out"]
    assert declaration("cddp_hip_seed_best") == ["cddp_hip_handle *h", "int flags", "int ncand", "const double *x0", "const double *U",
                                                 "const double *cost", "const double *viol", "double viol_tol", "int32_t *winner"]
    assert re.search(r"CDDP_HIP_SCORE_DEVICE\s*=\s*1\s*,\s*CDDP_HIP_SCORE_FEEDBACK\s*=\s*2\s*,\s*CDDP_HIP_SCORE_X0_PER_CANDIDATE\s*=\s*4", header())
    assert (api.SCORE_DEVICE, api.SCORE_FEEDBACK, api.SCORE_X0_PER_CANDIDATE) == (1, 2, 4)
    raw = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", raw)                     # new entry points only
    assert "Terminal EQUALITIES are not part of viol" in re.sub(r"\s+", " ", raw)
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in api.EXPORTED_SYMBOLS, s
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(declaration(s)), s
    assert lib.cddp_hip_seed_best.argtypes[7] is C.c_double


def test_refusals_that_need_no_device(api, lib):
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    err = lambda: lib.cddp_hip_last_error().decode()
    assert lib.cddp_hip_score_rollouts(None, None, 0, 1, p, p, p, None, None, None) < 0 and "cddp_hip_score_rollouts: null handle" in err()
    assert lib.cddp_hip_seed_best(None, 0, 1, p, p, p, None, 0.0, None) < 0 and "cddp_hip_seed_best: null handle" in err()
    fake = C.c_void_p(8)       # never dereferenced: every refusal below comes before the handle is looked into
    assert lib.cddp_hip_score_rollouts(fake, None, 8, 1, p, p, p, None, None, None) < 0 and "unknown flag bits" in err()
    assert lib.cddp_hip_score_rollouts(fake, None, 0, 0, p, p, p, None, None, None) < 0 and "ncand = 0" in err()
    assert lib.cddp_hip_score_rollouts(fake, None, 0, 2, p, p, None, None, None, None) < 0 and "null cost" in err()
    assert lib.cddp_hip_score_rollouts(fake, None, 0, 2, p, None, p, None, None, None) < 0 and "U is NULL without CDDP_HIP_SCORE_FEEDBACK" in err()
    assert lib.cddp_hip_score_rollouts(fake, None, 4, 2, None, p, p, None, None, None) < 0 and "NULL x0" in err()
    assert lib.cddp_hip_seed_best(fake, 2, 1, p, p, p, None, 0.0, None) < 0 and "unknown flag bits" in err()
    assert lib.cddp_hip_seed_best(fake, 0, 0, p, p, p, None, 0.0, None) < 0 and "ncand = 0" in err()
    assert lib.cddp_hip_seed_best(fake, 0, 1, p, None, p, None, 0.0, None) < 0 and "null U" in err()
    assert lib.cddp_hip_seed_best(fake, 0, 1, p, p, None, None, 0.0, None) < 0 and "null cost" in err()


def test_facade_and_cpp_mirror_offer_the_entries():
    src = open(os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py")).read()
    assert "def solve_batch_sampled(self, x0s, U_candidates" in src
    hpp = open(os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")).read()
    assert "void scoreRollouts(" in hpp and "void seedBest(" in hpp
    mk = open(os.path.join(REPO, "cddp-cpp_amd", "csrc", "Makefile")).read()
    assert "inst_score.hip" in mk
