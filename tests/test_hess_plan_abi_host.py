"""CPU suite: the additive C ABI of ssde_last_hess_plan (include/ssde.h against smoothsde_amd/capi.py)."""
import ctypes as C
import os
import re

from smoothsde_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "ssde.h")) as f:
        return f.read()


def test_the_header_declares_the_call_and_capi_exports_it():
    assert re.search(r"\bint\s+ssde_last_hess_plan\s*\(\s*const ssde_handle\s*\*h,\s*int32_t\s*\*warm_up,\s*int32_t\s*\*windows_max,"
                     r"\s*int32_t\s*\*attempts,\s*double\s*\*check\)\s*;", _header())
    assert "ssde_last_hess_plan" in capi.EXPORTED_SYMBOLS


def test_the_abi_version_stays():
    assert re.search(r"^#define SSDE_ABI_VERSION 12$", _header(), re.M) and capi.ABI_VERSION == 12


def test_the_ctypes_mirror_is_the_headers_signature():
    lib = capi.load_library()
    assert hasattr(C.CDLL(capi.lib_path()), "ssde_last_hess_plan")
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    assert lib.ssde_last_hess_plan.restype == C.c_int and lib.ssde_last_hess_plan.argtypes == [C.c_void_p, ip, ip, ip, dp]
    assert lib.ssde_abi_version() == 12
    w = C.c_int32(7)
    assert lib.ssde_last_hess_plan(None, C.byref(w), None, None, None) == 1          # SSDE_ERR_ARG, nothing written, no device touched
    assert w.value == 7


def test_the_headers_symbols_are_the_exported_ones():
    declared = re.findall(r"\b(ssde_[a-z_]+)\s*\(", _header())
    assert set(declared) == set(capi.EXPORTED_SYMBOLS), set(declared) ^ set(capi.EXPORTED_SYMBOLS)


def test_the_python_layer_has_the_call():
    import inspect
    assert list(inspect.signature(capi.Engine.hess_plan).parameters) == ["self"]
