"""ctypes loader of the test-only host build of ssde_smooth_loo's lane math (tests/hostsim/hostsim_loo.cpp, a library of its own
built by tests/hostsim/loo.mk together with the stand-alone sanitizer program loo_san)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import TWIN_ARGTYPES, _dp, _lp, ptr, twin_args

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
SAN = os.path.join(_DIR, "loo_san")


def load():
    """tests/hostsim/libhostsim_loo.so, after `make -f loo.mk` there (which compiles nothing in a built tree)"""
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "loo.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_loo.so"))
        lib.hostsim_loo.restype = C.c_int
        lib.hostsim_loo.argtypes = TWIN_ARGTYPES + [_lp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp]
        _LIB = lib
    return _LIB


def smooth_loo(pb, par, thresholds=None, crow=None):
    """ssde_smooth_loo by the lane math of csrc/ssde_loo.hpp over csrc/ssde_smooth.hpp (record -> loo_back_row -> loo_fold, one track
    after the other): what loo_ref returns -- {"mean": n x d, "cov": n x d x d, "resid": n x d, "lpd": n, "stats": n_seg x
    (4 + n_thr)} on the problem's rows, NaN where no row is served and the statistics of a track without a state row preset as the
    engine presets them.  `crow`: per row of pb the caller's row, -1 where the row is not the caller's (None: every row is its
    own)."""
    args, keep = twin_args(pb, par)
    thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64).ravel()
    cr = None if crow is None else np.ascontiguousarray(crow, dtype=np.int64)
    assert cr is None or cr.shape == (pb.n,)
    d, n = pb.n_dim, pb.n
    mean, cov, res, lpd = np.full((n, d), np.nan), np.full((n, d, d), np.nan), np.full((n, d), np.nan), np.full(n, np.nan)
    st = np.zeros((pb.n_seg, 4 + len(thr)))
    st[:, 2:4] = np.nan
    rc = load().hostsim_loo(*args, ptr(cr), ptr(thr) if len(thr) else None, len(thr), ptr(mean), ptr(cov), ptr(res), ptr(lpd), ptr(st))
    assert rc == 0, rc
    del keep
    return {"mean": mean, "cov": cov, "resid": res, "lpd": lpd, "stats": st}
