"""CPU-side checks of the boundary of the plan sensitivities (cddp_hip_plan_jvp, cddp_hip_plan_vjp): exported by the built library, declared
in include/cddp_hip.h with the documented signatures and flag, bound in pyapi with matching argtypes, each refusal that needs no device
answered with its own message instead of a crash, and offered by HipBatchSolver, the facade and the C++ mirror -- no GPU needed."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cddp_hip_plan_jvp", "cddp_hip_plan_vjp")


@pytest.fixture(scope="module")
def lib(api):
    if not os.path.exists(api.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return api.load_hip()


def header():
    txt = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)      # comments out (the parameter lists carry size comments)


def declaration(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m, "%s is not declared in include/cddp_hip.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_symbols_are_exported(api, lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), "libcddp_hip.so does not export %s" % s
        assert s in api.EXPORTED_SYMBOLS


def test_header_declares_the_documented_signatures():
    assert declaration("cddp_hip_plan_jvp") == ["cddp_hip_handle *h", "int flags", "int nvec", "const double *dx0", "double *dX", "double *dU"]
    assert declaration("cddp_hip_plan_vjp") == ["cddp_hip_handle *h", "int flags", "int nvec", "const double *gX", "const double *gU", "double *gx0"]
    assert re.search(r"enum\s*\{\s*CDDP_HIP_SENS_DEVICE\s*=\s*1\s*\}", header())
    raw = open(os.path.join(REPO, "include", "cddp_hip.h")).read()
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", raw)                     # new entry points only
    doc = re.sub(r"\s+", " ", raw)
    assert "LAST BACKWARD SWEEP" in doc and "cddp_hip_backward first" in doc           # which sweep the stacks belong to


def test_binding_argtypes_match_the_header(api, lib):
    for s in SYMBOLS:
        fn = getattr(lib, s)
        assert list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] and fn.restype is C.c_int, s
        assert len(fn.argtypes) == len(declaration(s)), s
    assert api.SENS_DEVICE == 1


def test_refusals_that_need_no_device_have_their_own_messages(api, lib):
    buf = (C.c_double * 8)()
    fake = C.c_void_p(8)       # never dereferenced: every refusal below comes before the handle is looked into
    p = C.addressof(buf)
    cases = [
        (lambda: lib.cddp_hip_plan_jvp(None, 0, 1, p, p, p), b"cddp_hip_plan_jvp: null handle"),
        (lambda: lib.cddp_hip_plan_vjp(None, 0, 1, p, p, p), b"cddp_hip_plan_vjp: null handle"),
        (lambda: lib.cddp_hip_plan_jvp(fake, 2, 1, p, p, p), b"cddp_hip_plan_jvp: unknown flag bits 0x2"),
        (lambda: lib.cddp_hip_plan_vjp(fake, 5, 1, p, p, p), b"cddp_hip_plan_vjp: unknown flag bits 0x4"),
        (lambda: lib.cddp_hip_plan_jvp(fake, 0, 0, p, p, p), b"cddp_hip_plan_jvp: nvec = 0"),
        (lambda: lib.cddp_hip_plan_vjp(fake, 1, -3, p, p, p), b"cddp_hip_plan_vjp: nvec = -3"),
        (lambda: lib.cddp_hip_plan_jvp(fake, 0, 1, None, p, p), b"cddp_hip_plan_jvp: null dx0 pointer"),
        (lambda: lib.cddp_hip_plan_vjp(fake, 0, 1, p, p, None), b"cddp_hip_plan_vjp: null gx0 pointer"),
        (lambda: lib.cddp_hip_plan_jvp(fake, 0, 1, p, None, None), b"cddp_hip_plan_jvp: dX and dU are both null"),
    ]
    for call, message in cases:
        lib.cddp_hip_mpc_advance(None, 7, 0, None)           # (another message in between: each entry sets its own)
        assert call() != 0
        assert message in lib.cddp_hip_last_error(), (message, lib.cddp_hip_last_error())
    assert list(buf) == [0.0] * 8


def test_solver_facade_and_mirror_offer_the_methods(api):
    for name in ("plan_jvp", "plan_vjp", "plan_jacobian_device"):
        assert callable(getattr(api.HipBatchSolver, name)), name
    import importlib.util, sys
    name = "pycddp_amd"
    if name in sys.modules:
        mod = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    assert callable(mod.CDDP.solve_batch_diff)
    sv = mod.CDDP([0.0, 0.0], [0.0, 0.0], 10, 0.02)
    with pytest.raises(RuntimeError):
        sv.solve_batch_diff(None)                            # no dynamical system yet: refused before anything else is looked at
    txt = open(os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")).read()
    for name in ("planJvp", "planVjp"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
