"""ctypes loader of the test-only host build of ssde_predict_draws' lane math and host plan (tests/hostsim/hostsim_predict_draws.cpp, a
library of its own built by tests/hostsim/predict_draws.mk)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import TWIN_ARGTYPES, _dp, _lp, ptr, twin_args

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
_ip = C.POINTER(C.c_int32)


def load():
    """tests/hostsim/libhostsim_predict_draws.so, after `make -f predict_draws.mk` there (which compiles nothing in a built tree)"""
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "predict_draws.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_predict_draws.so"))
        lib.hostsim_predict_draws.restype = C.c_int
        lib.hostsim_predict_draws.argtypes = TWIN_ARGTYPES + [C.c_int64, _lp, _dp, C.c_uint64, C.c_int64, C.c_int, _dp]
        lib.hostsim_bridge_step.restype = C.c_int
        lib.hostsim_bridge_step.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int, _dp, _dp]
        lib.hostsim_plan_slot_offsets.restype = None
        lib.hostsim_plan_slot_offsets.argtypes = [C.c_int64, _lp, _ip, _lp, C.c_double, C.c_int64, _lp, _dp, _lp, _lp, _lp, _lp, _lp, _dp,
                                                  _lp, _lp]
        lib.hostsim_predict_draws_batch_cap.restype = C.c_int
        lib.hostsim_predict_draws_batch_cap.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int]
        _LIB = lib
    return _LIB


def predict_draws(pb, par, rows, offs, seed=0, draw0=0, n_draws=1):
    """ssde_predict_draws by the lane math of csrc/ssde_bridge.hpp over csrc/ssde_draws.hpp (record + side row -> draw walk with the
    store rule of the ends -> bridge_slot_walk over the host plan's lists, one track after the other): what predict_draws_ref returns,
    (n_draws, n_query, sdim)."""
    args, keep = twin_args(pb, par)
    rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
    offs = np.ascontiguousarray(offs, dtype=np.float64).ravel()
    out = np.full((n_draws, len(rows), pb.sdim), np.nan)
    st = load().hostsim_predict_draws(*args, len(rows), ptr(rows), ptr(offs), int(seed), int(draw0), int(n_draws), ptr(out))
    assert st == 0
    return out


def plan_slot_offsets(row0, ns, q_row, q_off, pad_row=None, pad_step=0.0):
    """plan_queries then plan_slot_offsets over the lanes (row0, ns): order, q_slot, q_rank per planned query; off_ptr, off_val the
    slots' CSR lists; q_ptr, q_dest the queries of every distinct offset; most: the longest list."""
    row0 = np.ascontiguousarray(row0, dtype=np.int64); ns = np.ascontiguousarray(ns, dtype=np.int32)
    q_row = np.ascontiguousarray(q_row, dtype=np.int64); q_off = np.ascontiguousarray(q_off, dtype=np.float64)
    pad = None if pad_row is None else np.ascontiguousarray(pad_row, dtype=np.int64)
    nl, nq = len(row0), len(q_row)
    counts = np.zeros(4, dtype=np.int64)
    order, q_slot, q_rank, q_dest = (np.zeros(nq, dtype=np.int64) for _ in range(4))
    off_ptr, q_ptr, off_val = np.zeros(nq + 1, dtype=np.int64), np.zeros(nq + 1, dtype=np.int64), np.zeros(nq)
    load().hostsim_plan_slot_offsets(nl, ptr(row0), ptr(ns, _ip), ptr(pad), float(pad_step), nq, ptr(q_row), ptr(q_off), ptr(counts),
                                     ptr(order), ptr(q_slot), ptr(q_rank), ptr(off_ptr), ptr(off_val), ptr(q_ptr), ptr(q_dest))
    nv, n_slots, nd, most = (int(c) for c in counts)
    return dict(order=order[:nv], q_slot=q_slot[:nv], q_rank=q_rank[:nv], off_ptr=off_ptr[:n_slots + 1], off_val=off_val[:nd],
                q_ptr=q_ptr[:nd + 1], q_dest=q_dest[:nv], most=most)


def batch_cap(budget, n_slots, sd, n_query, ch, n_draws):
    return load().hostsim_predict_draws_batch_cap(int(budget), int(n_slots), sd, int(n_query), ch, n_draws)


def bridge_step(model, d, par, x_prev, alpha_next, d1, d2, tail, z):
    from smoothsde_amd.capi import MODEL_CODES
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (par, x_prev, alpha_next, z)]
    out = np.zeros(len(a[1]))
    assert load().hostsim_bridge_step(MODEL_CODES[model], d, ptr(a[0]), ptr(a[1]), ptr(a[2]), float(d1), float(d2), int(tail), ptr(a[3]),
                                      ptr(out)) == 0
    return out
