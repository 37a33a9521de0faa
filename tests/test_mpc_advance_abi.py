"""CPU-side checks of the device-resident MPC step's boundary (cddp_hip_mpc_advance, cddp_hip_mpc_run): exported by the built library,
declared in include/cddp_hip.h with the documented signatures, bound in pyapi with matching argtypes, and refusing a NULL handle with a
message instead of crashing -- no GPU needed."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    for s in ("cddp_hip_mpc_advance", "cddp_hip_mpc_run"):
        assert hasattr(lib, s), "libcddp_hip.so does not export %s" % s
        assert s in api.EXPORTED_SYMBOLS


def test_header_declares_the_documented_signatures():
    assert declaration("cddp_hip_mpc_advance") == ["cddp_hip_handle *h", "int mode", "int flags", "const double *x_next"]
    assert declaration("cddp_hip_mpc_run") == ["cddp_hip_handle *h", "int steps", "int mode", "int flags", "double *U_applied", "double *X_visited",
                                               "int32_t *iterations", "int32_t *status", "cddp_hip_stats *stats_sum"]
    h = header()
    m = re.search(r"enum\s+cddp_hip_mpc_mode\s*\{([^}]*)\}", h)
    assert m and [re.sub(r"\s+", "", e) for e in m.group(1).split(",")] == ["CDDP_HIP_MPC_KEEP_PLAN=0", "CDDP_HIP_MPC_SHIFT_EXISTING=1", "CDDP_HIP_MPC_SHIFT_PROVIDED=2"]
    assert re.search(r"CDDP_HIP_MPC_SHIFT_DUALS\s*=\s*1\b", h) and re.search(r"CDDP_HIP_MPC_X_DEVICE\s*=\s*2\b", h)
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", open(os.path.join(REPO, "include", "cddp_hip.h")).read())   # new entry points only


def test_binding_argtypes_match_the_header(api, lib):
    i32 = C.POINTER(C.c_int32); dp = C.POINTER(C.c_double)
    assert list(lib.cddp_hip_mpc_advance.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.c_void_p] and lib.cddp_hip_mpc_advance.restype is C.c_int
    assert list(lib.cddp_hip_mpc_run.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp, i32, i32, C.POINTER(api.Stats)]
    assert lib.cddp_hip_mpc_run.restype is C.c_int
    assert len(lib.cddp_hip_mpc_advance.argtypes) == len(declaration("cddp_hip_mpc_advance"))
    assert len(lib.cddp_hip_mpc_run.argtypes) == len(declaration("cddp_hip_mpc_run"))
    assert (api.MPC_KEEP_PLAN, api.MPC_SHIFT_EXISTING, api.MPC_SHIFT_PROVIDED) == (0, 1, 2) and (api.MPC_SHIFT_DUALS, api.MPC_X_DEVICE) == (1, 2)
    for name in ("mpc_advance", "mpc_run"):
        assert callable(getattr(api.HipBatchSolver, name))


def test_null_handle_is_refused_with_a_message(api, lib):
    assert lib.cddp_hip_mpc_advance(None, api.MPC_SHIFT_PROVIDED, 0, None) != 0
    assert len(lib.cddp_hip_last_error()) > 0
    assert lib.cddp_hip_mpc_run(None, 3, api.MPC_SHIFT_PROVIDED, 0, None, None, None, None, None) != 0
    assert b"null handle" in lib.cddp_hip_last_error()


def test_facade_offers_solve_mpc_batch():
    import importlib.util, sys
    name = "pycddp_amd"
    if name in sys.modules:
        mod = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    assert callable(mod.CDDP.solve_mpc_batch)
    sv = mod.CDDP([0.0, 0.0], [0.0, 0.0], 10, 0.02)
    with pytest.raises(ValueError):
        sv.solve_mpc_batch([[0.0, 0.0]], 2, warm_start="shifted")
