"""ctypes loader of the test-only host build of the path statistics' lane math (tests/hostsim/hostsim_path.cpp): compiles it itself,
with the flags of tests/hostsim/Makefile, into a library of its own next to libhostsim.so."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_CSRC = os.path.join(os.path.dirname(_DIR), os.pardir, "smoothsde_amd", "csrc")
_SRC = os.path.join(_DIR, "hostsim_path.cpp")
_SO = os.path.join(_DIR, "libhostsim_path.so")
_DEPS = [_SRC] + [os.path.join(_CSRC, f) for f in ("ssde_path.hpp", "ssde_draws.hpp", "ssde_smooth.hpp", "ssde_dense.hpp", "ssde_math.hpp")]
_LIB = None
_dp = C.POINTER(C.c_double)
_lp = C.POINTER(C.c_int64)


def build():
    """g++ -> tests/hostsim/libhostsim_path.so when it is missing or older than its sources"""
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(f) for f in _DEPS):
        return _SO
    cxx = os.environ.get("CXX", "g++")
    tmp = _SO + f".{os.getpid()}.tmp"
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-shared", "-o", tmp, _SRC], check=True)
    os.replace(tmp, _SO)
    return _SO


def load():
    global _LIB
    if _LIB is None:
        lib = C.CDLL(build())
        lib.hostsim_path.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _lp, _lp, _dp, _dp, _dp, _dp, C.c_double,
                                     _dp, _dp, C.c_uint64, C.c_int64, C.c_int, C.POINTER(C.c_uint8), _dp, _dp, C.c_int, _dp]
        lib.hostsim_path.restype = C.c_int
        _LIB = lib
    return _LIB


def path_stats(pb, par, seed=0, draw0=0, n_draws=1, regions=None, weight=None, is_row=None):
    """The statistics of ssde_path_stats by the lane math of csrc/ssde_path.hpp over csrc/ssde_draws.hpp (record -> factor -> draw
    -> path_step, one track after the other): (n_draws, n_tracks, 2 + n_regions), NaN for a track without a state row.  `weight`
    and `is_row` (the row is a row of the caller's data; None: every row is) are indexed by pb's rows.  The linear predictors, a0
    and P0 as drawsim_lib.draws forms them."""
    import torch
    from refimpl import linear_predictor
    from smoothsde_amd.capi import MODEL_CODES
    lib = load()
    d, sd, n = pb.n_dim, pb.sdim, pb.n
    par = np.asarray(par, dtype=np.float64)
    parmat = np.ascontiguousarray(linear_predictor(pb, torch.as_tensor(par)).detach().numpy())          # n x q
    row0 = np.ascontiguousarray(pb.seg_start, dtype=np.int64)
    nrows = np.diff(np.append(pb.seg_start, n)).astype(np.int64)
    z = (lambda a: 2 * a) if pb.model == "CTCRW" else (lambda a: a)
    if pb.P0 is None:
        P0 = np.diag([1.0, 10.0] * d) if pb.model == "CTCRW" else 10.0 * np.eye(d)
    else:
        P0 = np.asarray(pb.P0, dtype=np.float64)
    p0f = np.ascontiguousarray(P0.ravel(order="F"))
    if pb.a0 is None:
        a0 = np.zeros((pb.n_seg, sd))
        for a in range(d):
            a0[:, z(a)] = pb.obs[row0, a]
    else:
        a0 = np.ascontiguousarray(pb.a0, dtype=np.float64)
    harr = None if pb.H is None else np.ascontiguousarray(np.moveaxis(np.asarray(pb.H, dtype=np.float64), 2, 0))   # n x d x d
    reg = np.zeros((0, 4)) if regions is None else np.ascontiguousarray(regions, dtype=np.float64).reshape(-1, 4)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    flags = None if is_row is None else np.ascontiguousarray(is_row, dtype=np.uint8)
    assert (w is None or w.shape == (n,)) and (flags is None or flags.shape == (n,))
    out = np.full((n_draws, pb.n_seg, 2 + len(reg)), np.nan)
    st = lib.hostsim_path(MODEL_CODES[pb.model], d, int(pb.na_mode == 1), n, pb.n_seg, row0.ctypes.data_as(_lp),
                          nrows.ctypes.data_as(_lp), pb.times.ctypes.data_as(_dp), pb.obs.ctypes.data_as(_dp),
                          parmat.ctypes.data_as(_dp), None if harr is None else harr.ctypes.data_as(_dp),
                          float(np.exp(par[0]) ** 2), p0f.ctypes.data_as(_dp), a0.ctypes.data_as(_dp), int(seed), int(draw0),
                          int(n_draws), None if flags is None else flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                          None if w is None else w.ctypes.data_as(_dp), reg.ctypes.data_as(_dp), len(reg), out.ctypes.data_as(_dp))
    assert st == 0
    return out
