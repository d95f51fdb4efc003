"""ctypes loader of the test-only host build of ssde_forecast_scores' lane math and host plan (tests/hostsim/hostsim_ahead.cpp, a
library of its own built by tests/hostsim/ahead.mk together with the stand-alone sanitizer program ahead_san)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import TWIN_ARGTYPES, _dp, _lp, ptr, twin_args

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
SAN = os.path.join(_DIR, "ahead_san")
_ip = C.POINTER(C.c_int32)


def load():
    """tests/hostsim/libhostsim_ahead.so, after `make -f ahead.mk` there (which compiles nothing in a built tree)"""
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "ahead.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_ahead.so"))
        lib.hostsim_ahead.restype = C.c_int
        lib.hostsim_ahead.argtypes = TWIN_ARGTYPES + [_lp, _ip, C.c_int, _dp, C.c_int, _dp, _dp, _dp]
        lib.hostsim_ahead_block.restype = C.c_int
        lib.hostsim_ahead_blocks.restype = C.c_int64
        lib.hostsim_ahead_blocks.argtypes = [C.c_int64]
        lib.hostsim_ahead_partial_doubles.restype = C.c_int64
        lib.hostsim_ahead_partial_doubles.argtypes = [C.c_int64, C.c_int, C.c_int]
        lib.hostsim_ahead_check_horizons.restype = C.c_int
        lib.hostsim_ahead_check_horizons.argtypes = [_ip, C.c_int]
        lib.hostsim_ahead_block_offsets.restype = None
        lib.hostsim_ahead_block_offsets.argtypes = [_lp, C.c_int, _lp]
        lib.hostsim_ahead_chunks.restype = C.c_int
        lib.hostsim_ahead_chunks.argtypes = [_lp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int)]
        _LIB = lib
    return _LIB


def block():
    """ssde_plan::AHEAD_BLOCK"""
    return load().hostsim_ahead_block()


def check_horizons(hz):
    """ssde_plan::check_horizons against the header's caps: 0 accepted, 1 the count, 2 a horizon out of range, 3 not increasing"""
    if hz is None:
        return load().hostsim_ahead_check_horizons(None, 1)
    a = np.ascontiguousarray(hz, dtype=np.int32)
    return load().hostsim_ahead_check_horizons(a.ctypes.data_as(_ip), len(a))


def block_offsets(steps):
    s = np.ascontiguousarray(steps, dtype=np.int64)
    out = np.zeros(len(s) + 1, dtype=np.int64)
    load().hostsim_ahead_block_offsets(ptr(s), len(s), ptr(out))
    return out


def chunks(steps, R, SW, n_h, n_stat, budget):
    """the chunk boundaries (first groups, then G) of groups with these state rows under `budget` doubles"""
    s = np.ascontiguousarray(steps, dtype=np.int64)
    cut = (C.c_int * (len(s) + 1))()
    nc = load().hostsim_ahead_chunks(ptr(s), len(s), R, SW, n_h, n_stat, budget, cut)
    return list(cut[:nc + 1])


def forecast_scores(pb, par, horizons, thresholds=None, crow=None):
    """ssde_forecast_scores by the lane math of csrc/ssde_ahead.hpp (record + side row -> per block and start row ahead_load,
    ahead_score, ahead_step -> the blocks' sums in ascending order, one track after the other): {"z": n x n_h x d, "lpd": n x n_h,
    "stats": n_seg x n_h x (5 + n_thr)} on the problem's rows, NaN where a target is not scored, zero statistics for a track
    without a scored target.  `crow`: per row of pb the caller's row, -1 where the row is not the caller's (None: every row is
    its own)."""
    args, keep = twin_args(pb, par)
    hz = np.ascontiguousarray(horizons, dtype=np.int32)
    thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64).ravel()
    cr = None if crow is None else np.ascontiguousarray(crow, dtype=np.int64)
    assert cr is None or cr.shape == (pb.n,)
    d, n, nh = pb.n_dim, pb.n, len(hz)
    z, lpd = np.full((n, nh, d), np.nan), np.full((n, nh), np.nan)
    st = np.zeros((pb.n_seg, nh, 5 + len(thr)))
    rc = load().hostsim_ahead(*args, ptr(cr), hz.ctypes.data_as(_ip), nh, ptr(thr) if len(thr) else None, len(thr), ptr(z), ptr(lpd), ptr(st))
    assert rc == 0, rc
    del keep
    return {"z": z, "lpd": lpd, "stats": st}
