"""ctypes loader of the test-only host build of ssde_path_speed's lane math (tests/hostsim/hostsim_speed.cpp, a library of its own
built by tests/hostsim/speed.mk together with the stand-alone sanitizer program speed_san)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import TWIN_ARGTYPES, _dp, _lp, ptr, twin_args

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
_up = C.POINTER(C.c_uint32)
SAN = os.path.join(_DIR, "speed_san")


def load():
    """tests/hostsim/libhostsim_speed.so, after `make -f speed.mk` there (which compiles nothing in a built tree)"""
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "speed.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_speed.so"))
        lib.hostsim_speed.restype = C.c_int
        lib.hostsim_speed.argtypes = TWIN_ARGTYPES + [C.c_uint64, C.c_int64, C.c_int, _lp, C.c_int64, _dp, _dp, C.c_int, _dp, _up]
        _LIB = lib
    return _LIB


def path_speed(pb, par, seed=0, draw0=0, n_draws=1, thresholds=None, weight=None, crow=None, n_out=None, stats=True, rows=True):
    """ssde_path_speed by the lane math of csrc/ssde_speed.hpp over csrc/ssde_draws.hpp (record -> factor -> draw -> speed_step, one
    track after the other): (stats (n_draws, n_tracks, 5 + n_thr) with NaN for a track without a state row, row_below (n_out, n_thr)
    uint32), either None when not asked for (or, the counts, without a threshold).  `crow`: per row of pb the caller's row, -1 where
    the row is not the caller's (None: every row is its own) and `n_out` the caller's rows; `weight` is indexed by the caller's
    row.  The linear predictors, a0 and P0 as hostsim_lib.twin_args forms them."""
    args, keep = twin_args(pb, par)
    thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64).ravel()
    n_out = pb.n if n_out is None else int(n_out)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    cr = None if crow is None else np.ascontiguousarray(crow, dtype=np.int64)
    assert (w is None or w.shape == (n_out,)) and (cr is None or cr.shape == (pb.n,))
    out = np.full((n_draws, pb.n_seg, 5 + len(thr)), np.nan) if stats else None
    cnt = np.zeros((len(thr), n_out), dtype=np.uint32) if (rows and len(thr)) else None
    st = load().hostsim_speed(*args, int(seed), int(draw0), int(n_draws), ptr(cr), n_out, ptr(w), ptr(thr) if len(thr) else None, len(thr),
                              ptr(out), None if cnt is None else cnt.ctypes.data_as(_up))
    assert st == 0, st
    return out, (None if cnt is None else cnt.T)
