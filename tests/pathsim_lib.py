"""ctypes loader of the test-only host build of the path statistics' lane math (tests/hostsim/hostsim_path.cpp, a library of its own
next to libhostsim.so, built by tests/hostsim/Makefile)."""
import ctypes as C

import numpy as np

from hostsim_lib import TWIN_ARGTYPES, _dp, load_lib, ptr, twin_args

_bp = C.POINTER(C.c_uint8)


def load():
    return load_lib("libhostsim_path.so", {"hostsim_path": (C.c_int, TWIN_ARGTYPES + [C.c_uint64, C.c_int64, C.c_int, _bp, _dp, _dp, C.c_int, _dp])})


def path_stats(pb, par, seed=0, draw0=0, n_draws=1, regions=None, weight=None, is_row=None):
    """The statistics of ssde_path_stats by the lane math of csrc/ssde_path.hpp over csrc/ssde_draws.hpp (record -> factor -> draw
    -> path_step, one track after the other): (n_draws, n_tracks, 2 + n_regions), NaN for a track without a state row.  `weight`
    and `is_row` (the row is a row of the caller's data; None: every row is) are indexed by pb's rows.  The linear predictors, a0
    and P0 as hostsim_lib.twin_args forms them."""
    args, keep = twin_args(pb, par)
    n = pb.n
    reg = np.zeros((0, 4)) if regions is None else np.ascontiguousarray(regions, dtype=np.float64).reshape(-1, 4)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    flags = None if is_row is None else np.ascontiguousarray(is_row, dtype=np.uint8)
    assert (w is None or w.shape == (n,)) and (flags is None or flags.shape == (n,))
    out = np.full((n_draws, pb.n_seg, 2 + len(reg)), np.nan)
    st = load().hostsim_path(*args, int(seed), int(draw0), int(n_draws), ptr(flags, _bp), ptr(w), ptr(reg), len(reg), ptr(out))
    assert st == 0
    return out
