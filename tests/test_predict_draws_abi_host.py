"""CPU suite: the additive C ABI of ssde_predict_draws (include/ssde.h against smoothsde_amd/capi.py and the built library)."""
import ctypes as C
import os
import re

from smoothsde_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "ssde.h")) as f:
        return f.read()


def test_the_header_declares_the_call():
    text = _header()
    assert re.search(r"\bint\s+ssde_predict_draws\s*\(\s*ssde_handle\s*\*h,\s*const double\s*\*par,\s*int32_t n_par_full,"
                     r"\s*const int64_t\s*\*q_row,\s*const double\s*\*q_off,\s*int64_t n_query,\s*uint64_t seed,\s*int64_t draw0,"
                     r"\s*int32_t n_draws,\s*double\s*\*draws_at,\s*uint32_t flags\)\s*;", text)
    assert "must go into ONE call to be jointly distributed" in text
    assert re.search(r"^ \*   ssde_predict_draws <- \(new\)", text, re.M)               # the list at the head of the file


def test_the_abi_version_stays_twelve():
    assert re.search(r"^#define SSDE_ABI_VERSION 12$", _header(), re.M) and capi.ABI_VERSION == 12
    assert capi.load_library().ssde_abi_version() == 12


def test_the_symbol_and_its_ctypes_signature():
    assert "ssde_predict_draws" in capi.EXPORTED_SYMBOLS
    lib = capi.load_library()
    assert hasattr(C.CDLL(capi.lib_path()), "ssde_predict_draws")
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert lib.ssde_predict_draws.restype == C.c_int
    assert list(lib.ssde_predict_draws.argtypes) == [C.c_void_p, dp, C.c_int32, lp, dp, C.c_int64, C.c_uint64, C.c_int64, C.c_int32, dp,
                                                     C.c_uint32]


def test_python_reaches_it():
    assert hasattr(capi.Engine, "predict_draws")
    from smoothsde_amd.sde import SDE
    assert hasattr(SDE, "sample_states_at") and hasattr(SDE, "predict_states")
    assert "sample_states" in SDE.sample_states_at.__doc__
