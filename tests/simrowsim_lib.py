"""ctypes loader of the test-only host build of ssde_simulate_rows' lane math (tests/hostsim/hostsim_simrows.cpp, a library of its
own built by tests/hostsim/simrows.mk together with the stand-alone sanitizer program simrows_san)."""
import ctypes as C
import os
import subprocess

import numpy as np

from simrows_ref import KIND

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
SAN = os.path.join(_DIR, "simrows_san")


def load():
    """tests/hostsim/libhostsim_simrows.so, after `make -f simrows.mk` there (which compiles nothing in a built tree)"""
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "simrows.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_simrows.so"))
        lib.hostsim_simrows.restype = C.c_int
        lib.hostsim_simrows.argtypes = ([C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
        lib.hostsim_simrows_factors.restype = None
        lib.hostsim_simrows_factors.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
        _LIB = lib
    return _LIB


def factors(model, dt, p1, p2=0.0):
    """(e, 1 - e, a, l11, l21, l22, sd) of one transition by simrows_factors"""
    out = np.zeros(7)
    load().hostsim_simrows_factors(KIND[model], float(dt), float(p1), float(p2), out.ctypes.data)
    return dict(zip(("e", "ome", "a", "l11", "l21", "l22", "sd"), out))


def simulate_rows(model, n_dim, row0, times, X_fe, X_re, link, coeff, sigma_obs=None, z0=0.0, seed=0, rep0=0, n_rep=1, thr=()):
    """ssde_simulate_rows by the lane math of csrc/ssde_simrows.hpp, one (track, replicate) after the other:
    {"obs": (n_rep, n, d), "stats": (n_rep, n_tracks, n_stat)}"""
    q, d = len(X_fe), int(n_dim)
    r0 = np.ascontiguousarray(row0, dtype=np.int64)
    tm = np.ascontiguousarray(times, dtype=np.float64)
    n, M, R = len(tm), len(r0) - 1, int(n_rep)
    keep = []

    def blk(b):
        if b is None:
            return None, 0
        a = np.asfortranarray(np.asarray(b, dtype=np.float64))
        assert a.shape[0] == n
        keep.append(a)
        return a.ctypes.data, a.shape[1]

    pf, pr = [blk(b) for b in X_fe], [blk(b) for b in X_re]
    kf = np.array([1 if p is None else k for p, k in pf], dtype=np.int32)
    kr = np.array([k for _, k in pr], dtype=np.int32)
    xf = (C.c_void_p * q)(*[p for p, _ in pf])
    xr = (C.c_void_p * q)(*[p for p, _ in pr])
    cf = np.ascontiguousarray(np.atleast_2d(np.asarray(coeff, dtype=np.float64)))
    lk = np.ascontiguousarray(link, dtype=np.uint8)
    so = None if sigma_obs is None else np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_obs, dtype=np.float64), (cf.shape[0],)))
    z = np.zeros(8)
    z[:d] = np.broadcast_to(np.asarray(z0, dtype=np.float64), (d,))
    th = np.ascontiguousarray(np.asarray(thr, dtype=np.float64).ravel())
    n_stat = 3 * d + 2 + len(th)
    obs, stats = np.full((R, d, n), np.nan), np.zeros((R, n_stat, M))
    st = load().hostsim_simrows(KIND[model], d, q, n, M, r0.ctypes.data, tm.ctypes.data, kf.ctypes.data, xf, kr.ctypes.data, xr, lk.ctypes.data,
                                cf.ctypes.data, cf.shape[0], cf.shape[1], None if so is None else so.ctypes.data, z.ctypes.data,
                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(rep0), R, th.ctypes.data, len(th), obs.ctypes.data, stats.ctypes.data)
    assert st == 0, st
    return {"obs": obs.transpose(0, 2, 1), "stats": stats.transpose(0, 2, 1)}
