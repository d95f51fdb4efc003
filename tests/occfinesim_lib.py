"""ctypes loader of the test-only host build of ssde_path_occupancy_fine's lane math and host plans (tests/hostsim/hostsim_occ_fine.cpp,
a library of its own built by tests/hostsim/occ_fine.mk)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import TWIN_ARGTYPES, _dp, _lp, ptr, twin_args
from occ_ref import quantise, quantum_exp

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
_bp = C.POINTER(C.c_uint8)
_up = C.POINTER(C.c_uint64)
_ip = C.POINTER(C.c_int32)


def load():
    """tests/hostsim/libhostsim_occ_fine.so, after `make -f occ_fine.mk` there (which compiles nothing in a built tree), loaded once"""
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "occ_fine.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_occ_fine.so"))
        lib.hostsim_occ_fine.restype = C.c_int
        lib.hostsim_occ_fine.argtypes = TWIN_ARGTYPES + [C.c_uint64, C.c_int64, C.c_int, _bp, _up, _ip, C.c_int, _dp, C.c_int, C.c_int,
                                                         C.c_double, C.c_int, _up, _lp]
        lib.hostsim_plan_all_slots.restype = None
        lib.hostsim_plan_all_slots.argtypes = [C.c_int64, _ip, _ip, _lp, _ip]
        lib.hostsim_plan_fine_weights.restype = None
        lib.hostsim_plan_fine_weights.argtypes = [C.c_int64, _ip, _ip, _lp, _dp, C.c_double, C.c_int, _lp, _up, C.c_uint64, _ip, _up, _up, _lp]
        lib.hostsim_occ_fine_substeps.restype = C.c_int
        lib.hostsim_occ_fine_substeps.argtypes = [C.c_double, C.c_double, C.c_int]
        lib.hostsim_occ_fine_batch_cap.restype = C.c_int
        lib.hostsim_occ_fine_batch_cap.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]
        _LIB = lib
    return _LIB


def plan_all_slots(ns, lane_grp):
    """(want_off [lanes + 1], want_step [slots]) of ssde_plan::plan_all_slots"""
    ns = np.ascontiguousarray(ns, dtype=np.int32); lg = np.ascontiguousarray(lane_grp, dtype=np.int32)
    want_off = np.full(len(ns) + 1, -7, dtype=np.int64)
    want_step = np.full(int(np.maximum(ns, 0).sum()) + 1, -7, dtype=np.int32)
    load().hostsim_plan_all_slots(len(ns), ptr(ns, _ip), ptr(lg, _ip), ptr(want_off), ptr(want_step, _ip))
    return want_off, want_step[:want_off[-1]]


def plan_fine_weights(ns, lane_grp, row0, slot_dt, max_step, row_map=None, wq=None, unit=1, max_sub=64):
    """(m, own, share per slot, n_points, n_capped) of plan_all_slots then ssde_plan::plan_fine_weights"""
    ns = np.ascontiguousarray(ns, dtype=np.int32); lg = np.ascontiguousarray(lane_grp, dtype=np.int32)
    row0 = np.ascontiguousarray(row0, dtype=np.int64); slot_dt = np.ascontiguousarray(slot_dt, dtype=np.float64)
    rm = None if row_map is None else np.ascontiguousarray(row_map, dtype=np.int64)
    w = None if wq is None else np.ascontiguousarray(wq, dtype=np.uint64)
    ns_n = len(slot_dt)
    m = np.zeros(ns_n, dtype=np.int32); own = np.zeros(ns_n, dtype=np.uint64); share = np.zeros(ns_n, dtype=np.uint64)
    pts = np.zeros(2, dtype=np.int64)
    load().hostsim_plan_fine_weights(len(ns), ptr(ns, _ip), ptr(lg, _ip), ptr(row0), ptr(slot_dt), float(max_step), max_sub, ptr(rm),
                                     ptr(w, _up), int(unit), ptr(m, _ip), ptr(own, _up), ptr(share, _up), ptr(pts))
    return m, own, share, int(pts[0]), int(pts[1])


def substeps(dt, max_step, max_sub=64):
    return load().hostsim_occ_fine_substeps(float(dt), float(max_step), max_sub)


def batch_cap(budget, n_slots, ez, ch, n_draws):
    return load().hostsim_occ_fine_batch_cap(int(budget), int(n_slots), ez, ch, n_draws)


def path_occupancy_fine(pb, par, grid, max_step, seed=0, draw0=0, n_draws=1, weight=None, group=None, n_groups=1, is_row=None,
                        n_rows=None, with_points=False):
    """ssde_path_occupancy_fine by the lane math of csrc (record + side row -> draws' walk with the store rule of the ends -> per slot
    and draw what one thread of path_occ_fine_kernel does, over the real plan_all_slots / plan_fine_weights): (occ (n_groups, ny, nx),
    outside (n_groups,)) [, (n_points, n_capped)].  `weight` and `is_row` are indexed by pb's rows; n_rows: the rows of the
    caller's data (pb.n unless given), which set the quantum."""
    args, keep = twin_args(pb, par)
    n, d = pb.n, pb.n_dim
    flags = None if is_row is None else np.ascontiguousarray(is_row, dtype=np.uint8)
    w = np.ones(n) if weight is None else np.array(weight, dtype=np.float64)
    if flags is not None:
        w[flags == 0] = 0.0
    e = quantum_exp(1.0 if weight is None else np.max(w, initial=0.0), n if n_rows is None else n_rows, n_draws)
    wq = quantise(w, e)
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    nx, ny = grid["nx"], (grid["ny"] if d == 2 else 1)
    g4 = np.array([grid["x0"], grid["dx"], grid["y0"], grid["dy"]], dtype=np.float64)
    counts = np.zeros(nx * ny * n_groups + n_groups, dtype=np.uint64)
    pts = np.zeros(2, dtype=np.int64)
    st = load().hostsim_occ_fine(*args, int(seed), int(draw0), int(n_draws), ptr(flags, _bp), ptr(wq, _up), ptr(grp, _ip), n_groups,
                                 ptr(g4), nx, ny, float(max_step), 64, ptr(counts, _up), ptr(pts))
    assert st == 0
    assert int(counts.max(initial=0)) < 2 ** 52
    occ = np.ldexp(counts[:nx * ny * n_groups].astype(np.float64), e).reshape(n_groups, ny, nx)
    res = (occ, np.ldexp(counts[nx * ny * n_groups:].astype(np.float64), e))
    return res + ((int(pts[0]), int(pts[1])),) if with_points else res
