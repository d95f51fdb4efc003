"""CPU suite: the additive C ABI of ssde_path_occupancy_fine (include/ssde.h against smoothsde_amd/capi.py)."""
import ctypes as C
import os
import re

from smoothsde_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "ssde.h")) as f:
        return f.read()


def test_the_header_declares_both_calls_and_capi_exports_them():
    text = _header()
    assert re.search(r"\bint\s+ssde_path_occupancy_fine\s*\(\s*ssde_handle\s*\*h,\s*const double\s*\*par,\s*int32_t n_par_full,\s*uint64_t seed,"
                     r"\s*int64_t draw0,\s*int32_t n_draws,\s*const ssde_occ_grid\s*\*grid,\s*double max_step,\s*const double\s*\*weight,"
                     r"\s*const int32_t\s*\*group,\s*int32_t n_groups,\s*double\s*\*occ,\s*double\s*\*outside,\s*uint32_t flags\)\s*;", text)
    assert re.search(r"\bint\s+ssde_last_occupancy_points\s*\(\s*const ssde_handle\s*\*h,\s*int64_t\s*\*n_points,\s*int64_t\s*\*n_capped\)\s*;", text)
    assert "ssde_path_occupancy_fine" in capi.EXPORTED_SYMBOLS and "ssde_last_occupancy_points" in capi.EXPORTED_SYMBOLS


def test_the_abi_version_and_the_cap():
    text = _header()
    assert re.search(r"^#define SSDE_ABI_VERSION 12$", text, re.M) and capi.ABI_VERSION == 12
    assert re.search(r"^#define SSDE_OCC_MAX_SUB 64$", text, re.M) and capi.OCC_MAX_SUB == 64


def test_the_ctypes_mirror_is_the_headers_signature():
    lib = capi.load_library()
    assert hasattr(C.CDLL(capi.lib_path()), "ssde_path_occupancy_fine") and hasattr(C.CDLL(capi.lib_path()), "ssde_last_occupancy_points")
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert lib.ssde_path_occupancy_fine.restype == C.c_int
    assert lib.ssde_path_occupancy_fine.argtypes == [C.c_void_p, dp, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(capi.SsdeOccGrid),
                                                     C.c_double, dp, ip, C.c_int32, dp, dp, C.c_uint32]
    # ... which is ssde_path_occupancy's with max_step after the grid
    old = list(lib.ssde_path_occupancy.argtypes)
    assert lib.ssde_path_occupancy_fine.argtypes == old[:7] + [C.c_double] + old[7:]
    assert lib.ssde_last_occupancy_points.restype == C.c_int and lib.ssde_last_occupancy_points.argtypes == [C.c_void_p, lp, lp]
    assert lib.ssde_abi_version() == 12
    assert lib.ssde_last_occupancy_points(None, None, None) == 1                      # SSDE_ERR_ARG, and no device touched


def test_the_headers_symbols_are_the_exported_ones():
    declared = re.findall(r"\b(ssde_[a-z_]+)\s*\(", _header())
    assert set(declared) == set(capi.EXPORTED_SYMBOLS), set(declared) ^ set(capi.EXPORTED_SYMBOLS)


def test_the_python_layer_has_the_call():
    import inspect
    sig = inspect.signature(capi.Engine.path_occupancy_fine)
    assert list(sig.parameters) == ["self", "par", "n_draws", "grid", "max_step", "seed", "draw0", "weight", "group", "n_groups", "force_global"]
    assert hasattr(capi.Engine, "last_occupancy_points")
    from smoothsde_amd.sde import SDE
    assert inspect.signature(SDE.utilisation).parameters["max_step"].default is None
