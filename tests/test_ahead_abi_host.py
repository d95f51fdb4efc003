"""ssde_forecast_scores in the C ABI and the Python surface: the header declares the call and its three caps, the
ABI version is still 12, the built library exports the symbol and refuses a call without a handle before anything is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from smoothsde_amd import capi
from smoothsde_amd.capi import AHEAD_MAX_H, AHEAD_MAX_STEP, AHEAD_MAX_THR     # the feature itself
from smoothsde_amd.sde import SDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_call_and_its_caps():
    hdr = open(os.path.join(ROOT, "include", "ssde.h")).read()
    assert re.search(r"^int ssde_forecast_scores\(ssde_handle \*h, const double \*par, int32_t n_par_full,\s*"
                     r"const int32_t \*horizon, int32_t n_h,\s*double \*z_ahead, double \*lpd_ahead,\s*"
                     r"const double \*thr, int32_t n_thr, double \*stats, uint32_t flags\);", hdr, re.M)
    for name, val in (("SSDE_AHEAD_MAX_H", 8), ("SSDE_AHEAD_MAX_STEP", 64), ("SSDE_AHEAD_MAX_THR", 8)):
        assert re.search(rf"^#define {name}\s+{val}\b", hdr, re.M), name
    assert (AHEAD_MAX_H, AHEAD_MAX_STEP, AHEAD_MAX_THR) == (8, 64, 8)
    assert re.search(r"^ \*   ssde_forecast_scores <- \(new\)", hdr, re.M)            # the "what they replace" list


def test_the_abi_version_is_still_12():
    hdr = open(os.path.join(ROOT, "include", "ssde.h")).read()
    assert re.search(r"^#define SSDE_ABI_VERSION 12$", hdr, re.M) and capi.ABI_VERSION == 12
    assert "ssde_forecast_scores" in capi.EXPORTED_SYMBOLS
    assert callable(getattr(capi.Engine, "forecast_scores", None)) and callable(getattr(capi, "forecast_scores", None))
    assert callable(getattr(SDE, "forecast_skill", None))


def test_the_built_library_exports_the_symbol_and_refuses_no_handle():
    assert os.path.exists(capi.lib_path()), "libssde_hip.so not built"
    lib = capi.load_library()
    assert hasattr(lib, "ssde_forecast_scores") and lib.ssde_abi_version() == 12
    out = np.zeros(4)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    hz = np.array([1, 2], dtype=np.int32)
    assert lib.ssde_forecast_scores(None, p, 4, hz.ctypes.data_as(C.POINTER(C.c_int32)), 2, p, None, None, 0, None, 0) == 1   # SSDE_ERR_ARG
    assert np.all(out == 0.0)


def test_models_without_a_latent_state_raise():
    rng = np.random.default_rng(1)
    data = {"ID": np.zeros(10), "time": np.arange(10.0), "z": np.exp(rng.standard_normal(10))}
    sde = SDE(data=data, type="CIR", response="z")
    with pytest.raises(NotImplementedError, match="no latent state in the model 'CIR'"):
        sde.forecast_skill()
