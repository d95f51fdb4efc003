"""ctypes loader of the test-only host build of the draws' lane math (tests/hostsim/hostsim_draws.cpp, a library of its own next to
libhostsim.so, built by tests/hostsim/Makefile)."""
import ctypes as C

import numpy as np

from hostsim_lib import TWIN_ARGTYPES, _dp, load_lib, ptr, twin_args


def load():
    return load_lib("libhostsim_draws.so", {"hostsim_draws": (C.c_int, TWIN_ARGTYPES + [C.c_uint64, C.c_int64, C.c_int, _dp, _dp]),
                                            "hostsim_draws_fac_doubles": (C.c_int, [C.c_int, C.c_int])})


def fac_doubles(model, d):
    from smoothsde_amd.capi import MODEL_CODES
    return load().hostsim_draws_fac_doubles(MODEL_CODES[model], d)


def draws(pb, par, seed=0, draw0=0, n_draws=1, normals=None):
    """Joint posterior draws by the lane math of csrc/ssde_draws.hpp (record -> factor -> draw, one track after the other): what
    draws_ref returns, (n_draws, n, sdim), NaN where no state exists.  The linear predictors, a0 and P0 as hostsim_lib.twin_args
    forms them."""
    args, keep = twin_args(pb, par)
    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
    assert nrm is None or nrm.shape == (n_draws, pb.n, pb.sdim)
    out = np.full((n_draws, pb.n, pb.sdim), np.nan)
    st = load().hostsim_draws(*args, int(seed), int(draw0), int(n_draws), ptr(nrm), ptr(out))
    assert st == 0
    return out
