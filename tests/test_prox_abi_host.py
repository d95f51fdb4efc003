"""CPU suite: the additive C ABI of ssde_path_proximity and ssde_last_proximity_plan (include/ssde.h against smoothsde_amd/capi.py and
the built library)."""
import ctypes as C
import os
import re

from smoothsde_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "ssde.h")) as f:
        return f.read()


def test_the_header_declares_both_calls():
    text = _header()
    assert re.search(r"\bint\s+ssde_path_proximity\s*\(\s*ssde_handle\s*\*h,\s*const double\s*\*par,\s*int32_t n_par_full,\s*uint64_t seed,"
                     r"\s*int64_t draw0,\s*int32_t n_draws,\s*const int64_t\s*\*qa_row,\s*const double\s*\*qa_off,"
                     r"\s*const int64_t\s*\*qb_row,\s*const double\s*\*qb_off,\s*const int64_t\s*\*pair_ptr,\s*int32_t n_pairs,"
                     r"\s*const double\s*\*weight,\s*const double\s*\*radii,\s*int32_t n_radii,\s*double\s*\*stats,\s*uint32_t flags\)\s*;", text)
    assert re.search(r"\bint\s+ssde_last_proximity_plan\s*\(\s*const ssde_handle\s*\*h,\s*int64_t\s*\*n_tiles,\s*int64_t\s*\*tiles_max,"
                     r"\s*int32_t\s*\*n_batches,\s*int32_t\s*\*route\)\s*;", text)
    assert re.search(r"^ \*   ssde_path_proximity <- \(new\)", text, re.M)               # the list at the head of the file
    assert "DESIGN.md §3.16" in text


def test_the_most_radii_is_eight():
    assert re.search(r"^#define SSDE_PROX_MAX_RADII 8$", _header(), re.M) and capi.PROX_MAX_RADII == 8


def test_the_abi_version_stays_twelve():
    assert re.search(r"^#define SSDE_ABI_VERSION 12$", _header(), re.M) and capi.ABI_VERSION == 12
    assert capi.load_library().ssde_abi_version() == 12


def test_the_symbols_and_their_ctypes_signatures():
    assert "ssde_path_proximity" in capi.EXPORTED_SYMBOLS and "ssde_last_proximity_plan" in capi.EXPORTED_SYMBOLS
    lib = capi.load_library()
    raw = C.CDLL(capi.lib_path())
    assert hasattr(raw, "ssde_path_proximity") and hasattr(raw, "ssde_last_proximity_plan")
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    assert lib.ssde_path_proximity.restype == C.c_int and lib.ssde_last_proximity_plan.restype == C.c_int
    assert list(lib.ssde_path_proximity.argtypes) == [C.c_void_p, dp, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, lp, dp, lp, dp, lp,
                                                      C.c_int32, dp, dp, C.c_int32, dp, C.c_uint32]
    assert list(lib.ssde_last_proximity_plan.argtypes) == [C.c_void_p, lp, lp, ip, ip]
    assert lib.ssde_last_proximity_plan(None, None, None, None, None) == 1              # SSDE_ERR_ARG for a NULL handle


def test_python_reaches_it():
    assert hasattr(capi.Engine, "path_proximity") and hasattr(capi.Engine, "last_proximity_plan")
    from smoothsde_amd.sde import SDE
    assert hasattr(SDE, "proximity") and "p_within" in SDE.proximity.__doc__
