"""ctypes loader of the test-only host build of the occupancy grids' lane math (tests/hostsim/hostsim_occ.cpp, a library of its own
built by tests/hostsim/occ.mk)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import TWIN_ARGTYPES, ptr, twin_args
from occ_ref import quantum_exp

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
_dp = C.POINTER(C.c_double)
_bp = C.POINTER(C.c_uint8)
_up = C.POINTER(C.c_uint64)
_ip = C.POINTER(C.c_int32)


def load():
    """tests/hostsim/libhostsim_occ.so, after `make -f occ.mk` there (which compiles nothing in a built tree), loaded once"""
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "occ.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_occ.so"))
        lib.hostsim_occ.restype = C.c_int
        lib.hostsim_occ.argtypes = TWIN_ARGTYPES + [C.c_uint64, C.c_int64, C.c_int, _bp, _up, _ip, C.c_int, _dp, C.c_int, C.c_int, _up]
        lib.hostsim_occ_quantum_exp.restype = C.c_int
        lib.hostsim_occ_quantum_exp.argtypes = [C.c_double, C.c_int64, C.c_int64]
        lib.hostsim_occ_quantise.restype = None
        lib.hostsim_occ_quantise.argtypes = [_dp, C.c_int64, C.c_int, C.c_int, _up]
        lib.hostsim_occ_batch_cap.restype = C.c_int
        lib.hostsim_occ_batch_cap.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.hostsim_occ_groups.restype = None
        lib.hostsim_occ_groups.argtypes = [_ip, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int32, _ip]
        _LIB = lib
    return _LIB


def twin_quantum_exp(wmax, n, n_draws):
    return load().hostsim_occ_quantum_exp(float(wmax), int(n), int(n_draws))


def twin_quantise(w, e, fast=True):
    """fast: the engine's loop over all weights (occ_quantise_all); else the definition, one weight at a time (occ_quantise)"""
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = np.zeros(len(w), dtype=np.uint64)
    load().hostsim_occ_quantise(ptr(w), len(w), int(e), int(fast), ptr(out, _up))
    return out


def batch_cap(nw, ch, n_draws):
    return load().hostsim_occ_batch_cap(nw, ch, n_draws)


def plan_groups(lane_grp, wave, n_cells, tile_cells, force_global=False, mixed=-2):
    lg = np.ascontiguousarray(lane_grp, dtype=np.int32)
    out = np.full((len(lg) + wave - 1) // wave, 99, dtype=np.int32)
    load().hostsim_occ_groups(ptr(lg, _ip), len(lg), wave, n_cells, tile_cells, int(force_global), mixed, ptr(out, _ip))
    return out


def path_occupancy(pb, par, grid, seed=0, draw0=0, n_draws=1, weight=None, group=None, n_groups=1, is_row=None, n_rows=None):
    """ssde_path_occupancy by the lane math of csrc/ssde_occ.hpp over csrc/ssde_draws.hpp (record -> factor -> draw -> cell -> integer
    add, one track after the other): (occ (n_groups, ny, nx), outside (n_groups,)).  `weight` and `is_row` (the row is a row of the
    caller's data; None: every row is) are indexed by pb's rows; rows that are not the caller's may carry any weight.  n_rows: the
    rows of the caller's data (pb.n unless given), which set the quantum."""
    args, keep = twin_args(pb, par)
    n, d = pb.n, pb.n_dim
    flags = None if is_row is None else np.ascontiguousarray(is_row, dtype=np.uint8)
    w = np.ones(n) if weight is None else np.array(weight, dtype=np.float64)
    if flags is not None:
        w[flags == 0] = 0.0
    e = twin_quantum_exp(1.0 if weight is None else np.max(w, initial=0.0), n if n_rows is None else n_rows, n_draws)
    assert e == quantum_exp(1.0 if weight is None else np.max(w, initial=0.0), n if n_rows is None else n_rows, n_draws)
    wq = twin_quantise(w, e)
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    nx, ny = grid["nx"], (grid["ny"] if d == 2 else 1)
    g4 = np.array([grid["x0"], grid["dx"], grid["y0"], grid["dy"]], dtype=np.float64)
    counts = np.zeros(nx * ny * n_groups + n_groups, dtype=np.uint64)
    st = load().hostsim_occ(*args, int(seed), int(draw0), int(n_draws), ptr(flags, _bp), ptr(wq, _up), ptr(grp, _ip), n_groups,
                            ptr(g4), nx, ny, ptr(counts, _up))
    assert st == 0
    assert int(counts.max(initial=0)) < 2 ** 52
    occ = np.ldexp(counts[:nx * ny * n_groups].astype(np.float64), e).reshape(n_groups, ny, nx)
    return occ, np.ldexp(counts[nx * ny * n_groups:].astype(np.float64), e)
