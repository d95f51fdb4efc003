"""ctypes loader of the test-only host build of ssde_predict's lane math (tests/hostsim/hostsim_predict.cpp): compiles it itself,
with the flags of tests/hostsim/Makefile, into a library of its own next to libhostsim.so."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_CSRC = os.path.join(os.path.dirname(_DIR), os.pardir, "smoothsde_amd", "csrc")
_SRC = os.path.join(_DIR, "hostsim_predict.cpp")
_SO = os.path.join(_DIR, "libhostsim_predict.so")
_DEPS = [_SRC] + [os.path.join(_CSRC, f) for f in ("ssde_predict.hpp", "ssde_smooth.hpp", "ssde_dense.hpp", "ssde_math.hpp")]
_LIB = None
_dp = C.POINTER(C.c_double)
_lp = C.POINTER(C.c_int64)


def build():
    """g++ -> tests/hostsim/libhostsim_predict.so when it is missing or older than its sources"""
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
        lib.hostsim_predict.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _lp, _lp, _dp, _dp, _dp, _dp, C.c_double,
                                        _dp, _dp, C.c_int64, _lp, _dp, _dp, _dp]
        lib.hostsim_predict.restype = C.c_int
        lib.hostsim_predict_packet_doubles.argtypes = [C.c_int, C.c_int]
        lib.hostsim_predict_packet_doubles.restype = C.c_int
        _LIB = lib
    return _LIB


def packet_doubles(model, d):
    from smoothsde_amd.capi import MODEL_CODES
    return load().hostsim_predict_packet_doubles(MODEL_CODES[model], d)


def predict(pb, par, rows, offs):
    """The queries by the lane math of csrc/ssde_predict.hpp (record + side row -> packet -> query, one track after the other): what
    predict_ref returns.  The linear predictors, a0 and P0 as drawsim_lib.draws forms them."""
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
    rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
    offs = np.ascontiguousarray(offs, dtype=np.float64).ravel()
    m = len(rows)
    mean = np.full((m, sd), np.nan); cov = np.full((m, sd, sd), np.nan)
    st = lib.hostsim_predict(MODEL_CODES[pb.model], d, int(pb.na_mode == 1), n, pb.n_seg, row0.ctypes.data_as(_lp),
                             nrows.ctypes.data_as(_lp), pb.times.ctypes.data_as(_dp), pb.obs.ctypes.data_as(_dp),
                             parmat.ctypes.data_as(_dp), None if harr is None else harr.ctypes.data_as(_dp),
                             float(np.exp(par[0]) ** 2), p0f.ctypes.data_as(_dp), a0.ctypes.data_as(_dp), m, rows.ctypes.data_as(_lp),
                             offs.ctypes.data_as(_dp), mean.ctypes.data_as(_dp), cov.ctypes.data_as(_dp))
    assert st == 0
    return {"mean": mean, "cov": cov}
