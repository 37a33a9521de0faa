"""CPU-side checks of the boundary of the device-resident inputs and outputs (cddp_hip_field_shape, cddp_hip_get_field_device,
cddp_hip_get_results_device, cddp_hip_set_initial_device): exported by the built library, declared in include/cddp_hip.h with the documented
signatures and field ids, bound in pyapi with matching argtypes, refusing a NULL handle with a message instead of crashing, and offered by
HipBatchSolver and the facade -- no GPU needed."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cddp_hip_field_shape", "cddp_hip_get_field_device", "cddp_hip_get_results_device", "cddp_hip_set_initial_device")
FIELDS = ["X", "U", "K", "KFF", "VX", "VXX", "A", "B", "S", "Y", "G", "LAMBDA"]


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
    assert declaration("cddp_hip_field_shape") == ["cddp_hip_handle *h", "int field", "int32_t *rows", "int32_t *cols"]
    assert declaration("cddp_hip_get_field_device") == ["cddp_hip_handle *h", "int field", "double *out_dev"]
    assert declaration("cddp_hip_get_results_device") == ["cddp_hip_handle *h", "double *cols_dev", "int32_t *icols_dev"]
    assert declaration("cddp_hip_set_initial_device") == ["cddp_hip_handle *h", "const double *x0_dev", "const double *U0_dev", "const double *X0_dev"]
    m = re.search(r"enum\s+cddp_hip_field\s*\{([^}]*)\}", header())
    assert m
    names = [re.sub(r"\s+", "", e) for e in m.group(1).split(",")]
    assert names[0] == "CDDP_HIP_FIELD_X=0"                 # the first is pinned at 0, the rest count up in this order
    assert [n.split("=")[0] for n in names] == ["CDDP_HIP_FIELD_" + f for f in FIELDS]
    assert all("=" not in n for n in names[1:])
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", open(os.path.join(REPO, "include", "cddp_hip.h")).read())   # new entry points only


def test_binding_argtypes_match_the_header(api, lib):
    i32 = C.POINTER(C.c_int32)
    want = {"cddp_hip_field_shape": [C.c_void_p, C.c_int, i32, i32], "cddp_hip_get_field_device": [C.c_void_p, C.c_int, C.c_void_p],
            "cddp_hip_get_results_device": [C.c_void_p, C.c_void_p, C.c_void_p], "cddp_hip_set_initial_device": [C.c_void_p] * 4}
    for s in SYMBOLS:
        fn = getattr(lib, s)
        assert list(fn.argtypes) == want[s] and fn.restype is C.c_int, s
        assert len(fn.argtypes) == len(declaration(s)), s
    assert list(api.FIELD_NAMES) == FIELDS and [api.FIELD_IDS[f] for f in FIELDS] == list(range(12))
    assert list(api.RESULT_DEVICE_COLS) + list(api.RESULT_DEVICE_ICOLS) == list(api.RESULT_DTYPE.names)    # struct order
    # the diagnostic that tells the tests which plane of a slotted field is live
    assert declaration("cddp_hip_get_live_slots") == ["cddp_hip_handle *h", "int32_t *slots", "int32_t *n_slots"]
    assert list(lib.cddp_hip_get_live_slots.argtypes) == [C.c_void_p, i32, i32] and "cddp_hip_get_live_slots" in api.EXPORTED_SYMBOLS
    assert lib.cddp_hip_get_live_slots(None, None, None) != 0 and b"null handle" in lib.cddp_hip_last_error()


def test_null_handle_is_refused_with_a_message(api, lib):
    r = C.c_int32(0); c = C.c_int32(0)
    calls = [lambda: lib.cddp_hip_field_shape(None, 0, C.byref(r), C.byref(c)), lambda: lib.cddp_hip_get_field_device(None, 0, None),
             lambda: lib.cddp_hip_get_results_device(None, None, None), lambda: lib.cddp_hip_set_initial_device(None, None, None, None)]
    for call in calls:
        lib.cddp_hip_mpc_advance(None, 7, 0, None)           # (another message in between: each entry sets its own)
        assert call() != 0
        assert b"null handle" in lib.cddp_hip_last_error()


def test_solver_and_facade_offer_the_device_methods(api):
    for name in ("set_initial_device", "field_device", "field_shape", "trajectory_device", "gains_device", "value_device", "linearization_device",
                 "duals_device", "costates_device", "results_device"):
        assert callable(getattr(api.HipBatchSolver, name)), name
    import importlib.util, sys
    name = "pycddp_amd"
    if name in sys.modules:
        mod = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    assert callable(mod.CDDP.solve_batch_device)
    sv = mod.CDDP([0.0, 0.0], [0.0, 0.0], 10, 0.02)
    with pytest.raises(ValueError):
        sv.solve_batch_device(None, want=("X", "Q"))         # an unknown field name is refused before anything else is looked at


def test_host_header_offers_the_device_methods():
    txt = open(os.path.join(REPO, "cddp-cpp_amd", "host", "cddp_hip.hpp")).read()
    for name in ("setInitialDevice", "getFieldDevice", "fieldShape", "resultsDevice"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
