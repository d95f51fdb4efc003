"""ctypes loader of the test-only host build of ssde_path_proximity's lane math and tile plan (tests/hostsim/hostsim_prox.cpp, a library
of its own built by tests/hostsim/prox.mk)."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
_dp, _lp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
SAN = os.path.join(_DIR, "prox_san")


def _ptr(a, t=None):
    return None if a is None else a.ctypes.data_as(t or (_dp if a.dtype == np.float64 else _lp))


def load():
    """tests/hostsim/libhostsim_prox.so, after `make -f prox.mk` there (which compiles nothing in a built tree)"""
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "prox.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_prox.so"))
        lib.hostsim_prox.restype = C.c_int
        lib.hostsim_prox.argtypes = [C.c_int, C.c_int, _dp, C.c_int64, C.c_int, _lp, C.c_int64, _dp, _dp, C.c_int, _dp]
        lib.hostsim_prox_plan.restype = C.c_int
        lib.hostsim_prox_plan.argtypes = [_lp, C.c_int64, C.c_int, C.c_int64, _lp, _lp, _lp, _lp, _ip, _lp]
        lib.hostsim_prox_quantum_exp.restype = C.c_int
        lib.hostsim_prox_quantum_exp.argtypes = [C.c_double, C.c_int64]
        _LIB = lib
    return _LIB


def proximity(draws_at, model, d, pair_ptr, radii=(), weight=None):
    """ssde_path_proximity's statistics (n_draws, n_pairs, 2 + n_radii) by the tile step, the wave butterfly, the combine, the fold and
    the finish of csrc/ssde_prox.hpp as k_path_prox.hip runs them, from the array predict_draws returns for the A queries followed by
    the B queries: (n_draws, 2 n_point, sdim)."""
    from smoothsde_amd.capi import MODEL_CODES
    n_draws, nq, sd = draws_at.shape
    pos = np.ascontiguousarray(draws_at.transpose(0, 2, 1), dtype=np.float64)      # element (k, c, q) at k + nq (c + sdim q)
    pp = np.ascontiguousarray(pair_ptr, dtype=np.int64)
    rad = np.ascontiguousarray(radii, dtype=np.float64).ravel()
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    n_pairs, n_stat = len(pp) - 1, 2 + len(rad)
    assert sd == (2 * d if model == "CTCRW" else d) and pp[-1] * 2 == nq
    out = np.zeros((n_draws, n_stat, n_pairs))
    st = load().hostsim_prox(MODEL_CODES[model], d, _ptr(pos), nq // 2, n_draws, _ptr(pp), n_pairs, _ptr(w),
                             _ptr(rad) if len(rad) else None, len(rad), _ptr(out))
    assert st == 0, st
    return out.transpose(0, 2, 1)


def plan(pair_ptr, tile=256):
    """plan_prox_tiles: a dict of tile_pair, tile_first, tile_idx0, tile_count, pair_tile, n_tiles, tiles_max"""
    pp = np.ascontiguousarray(pair_ptr, dtype=np.int64)
    n_pairs = len(pp) - 1
    counts = np.zeros(2, dtype=np.int64)
    lib = load()
    assert lib.hostsim_prox_plan(_ptr(pp), n_pairs, tile, 0, _ptr(counts), None, None, None, None, None) == 0
    nt = int(counts[0])
    tp, tf, ti = (np.zeros(max(nt, 1), dtype=np.int64) for _ in range(3))
    tc = np.zeros(max(nt, 1), dtype=np.int32)
    pt = np.zeros(n_pairs + 1, dtype=np.int64)
    assert lib.hostsim_prox_plan(_ptr(pp), n_pairs, tile, max(nt, 1), _ptr(counts), _ptr(tp), _ptr(tf), _ptr(ti), _ptr(tc, _ip), _ptr(pt)) == 0
    return dict(tile_pair=tp[:nt], tile_first=tf[:nt], tile_idx0=ti[:nt], tile_count=tc[:nt], pair_tile=pt, n_tiles=nt,
                tiles_max=int(counts[1]))


def quantum_exp(wmax, n_point):
    return load().hostsim_prox_quantum_exp(float(wmax), int(n_point))
