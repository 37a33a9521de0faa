"""CPU-side checks of the movable reference's boundary (cddp_hip_set_reference, cddp_hip_get_reference, cddp_hip_mpc_set_reference_path,
cddp_hip_mpc_reference_cursor): exported by the built library, declared in include/cddp_hip.h with the documented signatures, bound in
pyapi with matching argtypes, the descriptor the size the header's struct has, and a NULL handle refused with a message instead of a
crash -- no GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cddp_hip_set_reference", "cddp_hip_get_reference", "cddp_hip_mpc_set_reference_path", "cddp_hip_mpc_reference_cursor")


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
    for s in ENTRIES:
        assert hasattr(lib, s), "libcddp_hip.so does not export %s" % s
        assert s in api.EXPORTED_SYMBOLS


def test_header_declares_the_documented_signatures():
    assert declaration("cddp_hip_set_reference") == ["cddp_hip_handle *h", "int flags", "const double *x_ref", "const double *x_ref_traj"]
    assert declaration("cddp_hip_get_reference") == ["cddp_hip_handle *h", "double *x_ref", "double *x_ref_traj", "int32_t *has_traj"]
    assert declaration("cddp_hip_mpc_set_reference_path") == ["cddp_hip_handle *h", "const cddp_hip_ref_path *desc"]
    assert declaration("cddp_hip_mpc_reference_cursor") == ["cddp_hip_handle *h", "int64_t *cursor"]
    h = header()
    assert re.search(r"CDDP_HIP_REF_DEVICE\s*=\s*1\b", h) and re.search(r"CDDP_HIP_REF_CLEAR_TRAJ\s*=\s*2\b", h)
    m = re.search(r"typedef\s+struct\s+cddp_hip_ref_path\s*\{([^}]*)\}\s*cddp_hip_ref_path\s*;", h)
    assert m and [re.sub(r"\s+", " ", s).strip() for s in m.group(1).split(";") if s.strip()] == \
        ["int32_t abi_version, flags", "int64_t rows", "int64_t start", "double rows_per_step", "const double *path"]
    assert re.search(r"#define\s+CDDP_HIP_ABI_VERSION\s+5\b", open(os.path.join(REPO, "include", "cddp_hip.h")).read())   # new entry points only


def test_descriptor_size_matches_the_header(api, tmp_path):
    """sizeof and the field offsets of cddp_hip_ref_path as a C compiler lays the header's struct out, against the ctypes structure"""
    src = tmp_path / "ref_path_size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cddp_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cddp_hip_ref_path), offsetof(cddp_hip_ref_path, abi_version),\n'
                   '  offsetof(cddp_hip_ref_path, flags), offsetof(cddp_hip_ref_path, rows), offsetof(cddp_hip_ref_path, start),\n'
                   '  offsetof(cddp_hip_ref_path, rows_per_step), offsetof(cddp_hip_ref_path, path)); return 0; }\n')
    exe = str(tmp_path / "ref_path_size")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    D = api.RefPathDesc
    assert got == [C.sizeof(D), D.abi_version.offset, D.flags.offset, D.rows.offset, D.start.offset, D.rows_per_step.offset, D.path.offset]
    assert C.sizeof(D) == 40


def test_binding_argtypes_match_the_header(api, lib):
    i32 = C.POINTER(C.c_int32); dp = C.POINTER(C.c_double)
    assert list(lib.cddp_hip_set_reference.argtypes) == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert list(lib.cddp_hip_get_reference.argtypes) == [C.c_void_p, dp, dp, i32]
    assert list(lib.cddp_hip_mpc_set_reference_path.argtypes) == [C.c_void_p, C.POINTER(api.RefPathDesc)]
    assert list(lib.cddp_hip_mpc_reference_cursor.argtypes) == [C.c_void_p, C.POINTER(C.c_int64)]
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(declaration(name))
    assert (api.REF_DEVICE, api.REF_CLEAR_TRAJ) == (1, 2)
    for name in ("set_reference", "get_reference", "mpc_set_reference_path", "mpc_reference_cursor"):
        assert callable(getattr(api.HipBatchSolver, name))


def test_null_handle_is_refused_with_a_message(api, lib):
    x = (C.c_double * 2)(0.0, 0.0)
    assert lib.cddp_hip_set_reference(None, 0, C.addressof(x), None) != 0
    assert b"cddp_hip_set_reference: null handle" in lib.cddp_hip_last_error()
    assert lib.cddp_hip_get_reference(None, x, None, None) != 0
    assert b"cddp_hip_get_reference: null handle" in lib.cddp_hip_last_error()
    d = api.RefPathDesc(); d.abi_version = api.ABI_VERSION; d.rows = 1; d.rows_per_step = 1.0; d.path = C.addressof(x)
    assert lib.cddp_hip_mpc_set_reference_path(None, C.byref(d)) != 0
    assert b"cddp_hip_mpc_set_reference_path: null handle" in lib.cddp_hip_last_error()
    c = C.c_int64(7)
    assert lib.cddp_hip_mpc_reference_cursor(None, C.byref(c)) != 0
    assert b"cddp_hip_mpc_reference_cursor: null" in lib.cddp_hip_last_error()


def test_facade_takes_a_reference_path():
    import importlib.util, inspect, sys
    name = "pycddp_amd"
    if name in sys.modules:
        mod = sys.modules[name]
    else:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "cddp-cpp_amd", "pycddp_amd.py"))
        mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    sig = inspect.signature(mod.CDDP.solve_mpc_batch)
    assert sig.parameters["reference_path"].default is None and sig.parameters["rows_per_step"].default == 1.0
