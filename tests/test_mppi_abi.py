"""The C boundary of the sampling-based plan refinement without a device: cddp_hip_sample_controls, cddp_hip_mppi_blend and
cddp_hip_mppi_refine are exported, declared with the documented signatures, bound with matching argtypes; cddp_hip_mppi_desc has its
pinned size and layout on both sides; every refusal that reads nothing of the handle answers with its own message; the Python front end
validates before any library call; the facade and the C++ mirror offer the entries.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cddp_hip_sample_controls", "cddp_hip_mppi_blend", "cddp_hip_mppi_refine")
B, S, N, NX, NU = 6, 3, 5, 4, 2


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
    assert declaration("cddp_hip_sample_controls") == ["cddp_hip_handle *h", "int flags", "const cddp_hip_mppi_desc *desc", "const double *U_mean",
                                                       "double *U_out"]
    assert declaration("cddp_hip_mppi_blend") == ["cddp_hip_handle *h", "int flags", "const cddp_hip_mppi_desc *desc", "const double *U_mean",
                                                  "const double *U_cand", "const double *cost", "const double *viol", "double *U_out", "double *stats"]
    assert declaration("cddp_hip_mppi_refine") == ["cddp_hip_handle *h", "cddp_hip_plant *plant", "int flags", "const cddp_hip_mppi_desc *desc",
                                                   "const double *x0", "const double *U_mean", "double *U_out", "double *cost_out", "double *viol_out",
                                                   "double *stats"]
    assert re.search(r"CDDP_HIP_MPPI_SEED\s*=\s*8\b", header()) and api.MPPI_SEED == 8
    assert api.MPPI_SEED & (api.SCORE_DEVICE | api.SCORE_FEEDBACK | api.SCORE_X0_PER_CANDIDATE) == 0
    raw = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", raw)                     # new entry points only
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in api.EXPORTED_SYMBOLS, s
        fn = getattr(lib, s)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(declaration(s)), s


def test_descriptor_size_is_pinned(api, tmp_path):
    d = api.MppiDesc
    assert C.sizeof(d) == 64
    offs = {n: getattr(d, n).offset for n, _ in d._fields_}
    assert offs == {"seed": 0, "stream": 8, "iters": 12, "ncand": 16, "keep_mean": 20, "lam": 24, "viol_tol": 32, "sigma": 40, "u_lower": 48,
                    "u_upper": 56}
    # ... and the C compiler lays the header's struct out alike
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cddp_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(cddp_hip_mppi_desc), " + ", ".join("offsetof(cddp_hip_mppi_desc, %s)" % n for n in
                                                              ("seed", "stream", "iters", "ncand", "keep_mean", "lambda", "viol_tol", "sigma", "u_lower", "u_upper"))
                   + "); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [64, 0, 8, 12, 16, 20, 24, 32, 40, 48, 56]


def desc(api, **kw):
    d = api.MppiDesc()
    sg = (C.c_double * 8)(*([0.5] * 8))
    d.seed = 1; d.stream = 0; d.iters = 1; d.ncand = 2; d.keep_mean = 0; d.lam = 1.0; d.viol_tol = 0.0
    d.sigma = C.cast(sg, C.POINTER(C.c_double))
    d._keep = sg
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_refusals_that_need_no_device(api, lib):
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    dp = C.cast(buf, C.POINTER(C.c_double))
    err = lambda: lib.cddp_hip_last_error().decode()
    fake = C.c_void_p(8)       # never dereferenced: every refusal below comes before the handle is looked into
    ok = desc(api)
    calls = {
        "cddp_hip_sample_controls": lambda h, flags, d: lib.cddp_hip_sample_controls(h, flags, d, p, p),
        "cddp_hip_mppi_blend": lambda h, flags, d: lib.cddp_hip_mppi_blend(h, flags, d, p, p, p, None, p, None),
        "cddp_hip_mppi_refine": lambda h, flags, d: lib.cddp_hip_mppi_refine(h, None, flags, d, p, p, p, None, None, None),
    }
    inf, nan = float("inf"), float("nan")
    for name, call in calls.items():
        a = lambda d: C.addressof(d) if d is not None else None
        assert call(None, 0, a(ok)) < 0 and name + ": null handle" in err()
        assert call(fake, 16, a(ok)) < 0 and name in err() and "unknown flag bits 0x10" in err()
        assert call(fake, api.SCORE_FEEDBACK, a(ok)) < 0 and "unknown flag bits 0x2" in err()        # scoring here is without feedback
        assert call(fake, 0, None) < 0 and name + ": null descriptor" in err()
        assert call(fake, 0, a(desc(api, iters=0))) < 0 and "iters = 0" in err()
        assert call(fake, 0, a(desc(api, ncand=0))) < 0 and "ncand = 0" in err()
        for bad in (0.0, -1.0, inf, nan):
            assert call(fake, 0, a(desc(api, lam=bad))) < 0 and "lambda" in err() and "not positive and finite" in err(), bad
        assert call(fake, 0, a(desc(api, viol_tol=nan))) < 0 and "viol_tol is NaN" in err()
        assert call(fake, 0, a(desc(api, sigma=None))) < 0 and "null sigma" in err()
        assert call(fake, 0, a(desc(api, u_lower=dp))) < 0 and "half a box" in err()
        assert call(fake, 0, a(desc(api, u_upper=dp))) < 0 and "half a box" in err()
    # only cddp_hip_mppi_refine knows CDDP_HIP_MPPI_SEED
    assert lib.cddp_hip_sample_controls(fake, api.MPPI_SEED, C.addressof(ok), p, p) < 0 and "unknown flag bits 0x8" in err()
    assert lib.cddp_hip_mppi_blend(fake, api.MPPI_SEED, C.addressof(ok), p, p, p, None, p, None) < 0 and "unknown flag bits 0x8" in err()


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


def test_python_validates_before_any_library_call(solver):
    U = np.zeros((B, N, NU)); x0 = np.zeros((B, NX)); Uc = np.zeros((B, S, N, NU)); cost = np.zeros((B, S))
    bad = [
        (solver.sample_controls, dict(sigma=0.5, ncand=0), "ncand"),
        (solver.sample_controls, dict(sigma=[0.5], ncand=S), "sigma"),
        (solver.sample_controls, dict(sigma=[0.5, -1.0], ncand=S), "sigma"),
        (solver.sample_controls, dict(sigma=0.5, ncand=S, u_lower=[0.0, 0.0]), "both given or both None"),
        (solver.sample_controls, dict(sigma=0.5, ncand=S, u_lower=[0.0, 1.0], u_upper=[1.0, 0.0]), "u_lower <= u_upper"),
        (solver.sample_controls, dict(sigma=0.5, ncand=S, U_mean=np.zeros((B, N + 1, NU))), "U_mean: shape"),
        (solver.sample_controls, dict(sigma=0.5, ncand=S, U_mean=U.astype(np.float32)), "dtype float64"),
        (solver.sample_controls, dict(sigma=0.5, ncand=S, seed=-1), "seed"),
        (solver.mppi_refine, dict(sigma=0.5, ncand=S, iters=0), "iters"),
        (solver.mppi_refine, dict(sigma=0.5, ncand=S, lam=0.0), "lam"),
        (solver.mppi_refine, dict(sigma=0.5, ncand=S, lam=float("nan")), "lam"),
        (solver.mppi_refine, dict(sigma=0.5, ncand=S, x0=np.zeros((B, NX + 1)), U_mean=U), "x0: shape"),
        (solver.mppi_blend, dict(U_mean=U, U_cand=None, cost=cost), "required"),
        (solver.mppi_blend, dict(U_mean=U, U_cand=np.zeros((B, S, N * NU)), cost=cost), "U_cand: shape"),
        (solver.mppi_blend, dict(U_mean=U, U_cand=Uc, cost=np.zeros((B, S + 1))), "cost: shape"),
        (solver.mppi_blend, dict(U_mean=U, U_cand=Uc, cost=cost, viol=np.zeros((B,))), "viol: shape"),
        (solver.mppi_blend, dict(U_mean=U, U_cand=Uc, cost=cost, lam=-2.0), "lam"),
    ]
    for fn, kw, needle in bad:
        with pytest.raises(ValueError, match=re.escape(needle)):
            fn(**kw)
    # ... and well-formed calls do reach the library
    with pytest.raises(AssertionError, match="cddp_hip_sample_controls"):
        solver.sample_controls(0.5, S, U_mean=U, seed=2 ** 64 - 1, stream=2 ** 32 - 1)
    with pytest.raises(AssertionError, match="cddp_hip_mppi_blend"):
        solver.mppi_blend(U, Uc, cost, viol=cost, lam=0.3, u_lower=[-1.0, -1.0], u_upper=[1.0, 1.0])
    with pytest.raises(AssertionError, match="cddp_hip_mppi_refine"):
        solver.mppi_refine([0.5, 0.25], S, x0=x0, U_mean=U, iters=2, seed_handle=True)


def test_mixed_kinds_are_refused(solver):
    torch = pytest.importorskip("torch")
    U = np.zeros((B, N, NU)); Uc = np.zeros((B, S, N, NU))
    with pytest.raises(ValueError):
        solver.mppi_blend(U, Uc, torch.zeros((B, S), dtype=torch.float64))
    with pytest.raises(ValueError):
        solver.mppi_refine(0.5, S, x0=torch.zeros((B, NX), dtype=torch.float64), U_mean=U)   # a CPU tensor is no device tensor


def test_facade_mirror_and_makefile_offer_the_entries():
    src = open(os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py")).read()
    assert "def solve_batch_mppi(self, x0s, U0, sigma, ncand" in src
    hpp = open(os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")).read()
    assert "void sampleControls(" in hpp and "void mppiBlend(" in hpp and "void mppiRefine(" in hpp
    mk = open(os.path.join(REPO, "cddp-cpp_amd", "csrc", "Makefile")).read()
    assert "inst_mppi.hip" in mk
