"""ctypes loader of the test-only host build of ssde_par_bands' lane math (tests/hostsim/hostsim_bands.cpp, a library of its own
built by tests/hostsim/bands.mk together with the stand-alone sanitizer program bands_san)."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
_dp = C.POINTER(C.c_double)
SAN = os.path.join(_DIR, "bands_san")


def load():
    """tests/hostsim/libhostsim_bands.so, after `make -f bands.mk` there (which compiles nothing in a built tree)"""
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "bands.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_bands.so"))
        lib.hostsim_bands.restype = C.c_int
        lib.hostsim_bands.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int, C.c_double, C.c_double] + [C.c_void_p] * 8
        lib.hostsim_bands_plan.restype = None
        lib.hostsim_bands_plan.argtypes = [C.c_int, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        _LIB = lib
    return _LIB


def plan(n_post, level):
    a, b = C.c_int32(0), C.c_int32(0)
    load().hostsim_bands_plan(int(n_post), float(level), C.byref(a), C.byref(b))
    return a.value, b.value


def par_bands(X_fe, X_re, link, coeff, level, z, resp=True):
    """ssde_par_bands by the lane math of csrc/ssde_bands.hpp, one row and one draw after the other: a dict of est, pw_low, pw_upp,
    se, sim_low, sim_upp (n, q), crit (q,), max_dev (q, n_post)"""
    q = len(X_fe)
    keep = []

    def blk(b):
        if b is None:
            return None, 0
        a = np.asfortranarray(np.asarray(b, dtype=np.float64))
        keep.append(a)
        return a.ctypes.data, a.shape[1]

    pf, pr = [blk(b) for b in X_fe], [blk(b) for b in X_re]
    n = max([a.shape[0] for a in keep], default=1)
    kf = np.array([1 if p is None else k for p, k in pf], dtype=np.int32)
    kr = np.array([k for _, k in pr], dtype=np.int32)
    xf = (C.c_void_p * q)(*[p for p, _ in pf])
    xr = (C.c_void_p * q)(*[p for p, _ in pr])
    cf = np.ascontiguousarray(coeff, dtype=np.float64)
    lk = np.ascontiguousarray(link, dtype=np.uint8)
    n_post = cf.shape[0] - 1
    assert cf.shape[1] == int(kf.sum() + kr.sum())
    out = {nm: np.zeros((q, n)) for nm in ("est", "pw_low", "pw_upp", "se", "sim_low", "sim_upp")}
    out["crit"] = np.zeros(q)
    out["max_dev"] = np.zeros((q, n_post))
    st = load().hostsim_bands(n, q, kf.ctypes.data, xf, kr.ctypes.data, xr, lk.ctypes.data, cf.ctypes.data, n_post, 1 if resp else 0,
                              float(level), float(z), *[out[nm].ctypes.data for nm in ("est", "pw_low", "pw_upp", "se", "sim_low", "sim_upp", "crit", "max_dev")])
    assert st == 0, st
    return {nm: (v if nm in ("crit", "max_dev") else v.T) for nm, v in out.items()}
