"""ctypes loader of the test-only host build of ssde_predict's lane math and of the smoother calls' host-side plans
(tests/hostsim/hostsim_predict.cpp, a library of its own next to libhostsim.so, built by tests/hostsim/Makefile)."""
import ctypes as C

import numpy as np

from hostsim_lib import TWIN_ARGTYPES, _dp, _lp, load_lib, ptr, twin_args

_ip = C.POINTER(C.c_int32)


def load():
    return load_lib("libhostsim_predict.so", {
        "hostsim_predict": (C.c_int, TWIN_ARGTYPES + [C.c_int64, _lp, _dp, _dp, _dp]),
        "hostsim_predict_packet_doubles": (C.c_int, [C.c_int, C.c_int]),
        "hostsim_plan_queries": (None, [C.c_int64, _lp, _ip, _lp, C.c_double, C.c_int64, _lp, _dp, C.c_int, _ip, C.c_int, _lp, _lp, _lp, _dp,
                                        _lp, _ip, _lp]),
        "hostsim_chunk_groups": (C.c_int, [C.c_int, _lp, C.c_int64, _ip]),
        "hostsim_batch_cap": (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]),
        "hostsim_deal_queries": (C.c_int64, [C.c_int64, C.c_int64, _lp, _dp, C.c_int64, _lp, _lp, _dp]),
        "hostsim_place_columns": (None, [_dp, C.c_int64, C.c_int, _dp, C.c_int64, C.c_int, C.c_int64, _lp]),
        "hostsim_place_block": (None, [_dp, C.c_int64, C.c_int, C.c_int, _dp, C.c_int64, C.c_int, C.c_int64, _lp, C.c_int]),
        "hostsim_place_track_stats": (None, [_dp, C.c_int64, C.c_int64, _dp, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int64]),
        "hostsim_max_distinct_offsets": (C.c_int64, [_lp, _dp, C.c_int64])})


def packet_doubles(model, d):
    from smoothsde_amd.capi import MODEL_CODES
    return load().hostsim_predict_packet_doubles(MODEL_CODES[model], d)


def predict(pb, par, rows, offs):
    """The queries by the lane math of csrc/ssde_predict.hpp (record + side row -> packet -> query, one track after the other): what
    predict_ref returns.  The linear predictors, a0 and P0 as hostsim_lib.twin_args forms them."""
    args, keep = twin_args(pb, par)
    rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
    offs = np.ascontiguousarray(offs, dtype=np.float64).ravel()
    m, sd = len(rows), pb.sdim
    mean = np.full((m, sd), np.nan); cov = np.full((m, sd, sd), np.nan)
    st = load().hostsim_predict(*args, m, ptr(rows), ptr(offs), ptr(mean), ptr(cov))
    assert st == 0
    return {"mean": mean, "cov": cov}


# ---- the host-side plans (csrc/ssde_smooth_plan.hpp) ----------------------------------------------------------------------------
def plan_queries(row0, ns, q_row, q_off, pad_row=None, pad_step=0.0, cuts=(), wave=64):
    """plan_queries over the lanes (row0, ns), and chunk_queries for the chunks between the group boundaries `cuts`: order, q_slot,
    off (the sorted residuals), want_off, want_step, ranges (one row s0, s1, q0, q1 per chunk)."""
    row0 = np.ascontiguousarray(row0, dtype=np.int64); ns = np.ascontiguousarray(ns, dtype=np.int32)
    q_row = np.ascontiguousarray(q_row, dtype=np.int64); q_off = np.ascontiguousarray(q_off, dtype=np.float64)
    pad = None if pad_row is None else np.ascontiguousarray(pad_row, dtype=np.int64)
    cuts = np.ascontiguousarray(cuts, dtype=np.int32)
    nl, nq = len(row0), len(q_row)
    counts = np.zeros(2, dtype=np.int64)
    order, q_slot, off = np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int64), np.zeros(nq)
    want_off, want_step = np.zeros(nl + 1, dtype=np.int64), np.zeros(nq, dtype=np.int32)
    ranges = np.zeros((max(len(cuts) - 1, 0), 4), dtype=np.int64)
    load().hostsim_plan_queries(nl, ptr(row0), ptr(ns, _ip), ptr(pad), float(pad_step), nq, ptr(q_row), ptr(q_off), len(cuts),
                                ptr(cuts, _ip), wave, ptr(counts), ptr(order), ptr(q_slot), ptr(off), ptr(want_off),
                                ptr(want_step, _ip), ptr(ranges))
    nv, n_slots = int(counts[0]), int(counts[1])
    return dict(order=order[:nv], q_slot=q_slot[:nv], off=off[:nv], want_off=want_off, want_step=want_step[:n_slots], ranges=ranges)


def chunk_groups(goff, budget):
    goff = np.ascontiguousarray(goff, dtype=np.int64)
    cuts = np.zeros(len(goff), dtype=np.int32)
    k = load().hostsim_chunk_groups(len(goff) - 1, ptr(goff), int(budget), ptr(cuts, _ip))
    return cuts[:k]


def batch_cap(budget, per_draw, unit, ch, n_draws):
    return load().hostsim_batch_cap(int(budget), int(per_draw), unit, ch, n_draws)


# ---- a parent of several engines: the deal and the placement (csrc/ssde_smooth_plan.hpp) -------------------------------------------
def deal_queries(lo, m, q_row, q_off):
    """(idx, rows, offs) of the queries on rows [lo, lo + m)"""
    q_row = np.ascontiguousarray(q_row, dtype=np.int64); q_off = np.ascontiguousarray(q_off, dtype=np.float64)
    nq = len(q_row)
    idx, rows, offs = np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int64), np.zeros(nq)
    k = load().hostsim_deal_queries(int(lo), int(m), ptr(q_row), ptr(q_off), nq, ptr(idx), ptr(rows), ptr(offs))
    return idx[:k], rows[:k], offs[:k]


def _idx(idx):
    return None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)


def place_columns(dst, c0, src, lo=0, idx=None):
    """src (m, ncol) into columns c0 .. of dst (n, NCOL), both Fortran-ordered, in place: at rows lo .., or at rows idx"""
    assert dst.flags.f_contiguous and src.flags.f_contiguous and dst.dtype == src.dtype == np.float64
    idx = _idx(idx)
    load().hostsim_place_columns(ptr(dst), dst.shape[0], c0, ptr(src), src.shape[0], src.shape[1], int(lo), ptr(idx))


def place_block(dst, c0, src, lo=0, idx=None, nan_rule=True):
    """src (m, sd, sd) into the diagonal block at c0 of dst (n, SD, SD), both Fortran-ordered, in place; nan_rule: place_cov_block"""
    assert dst.flags.f_contiguous and src.flags.f_contiguous and dst.dtype == src.dtype == np.float64
    idx = _idx(idx)
    load().hostsim_place_block(ptr(dst), dst.shape[0], dst.shape[1], c0, ptr(src), src.shape[0], src.shape[1], int(lo), ptr(idx), int(nan_rule))


def place_track_stats(dst, track0, src, row_stat, lo):
    """src (mt, n_stat, n_rep) at tracks track0 .. of dst (NT, n_stat, n_rep), both Fortran-ordered, in place"""
    assert dst.flags.f_contiguous and src.flags.f_contiguous and dst.shape[1:] == src.shape[1:]
    load().hostsim_place_track_stats(ptr(dst), dst.shape[0], int(track0), ptr(src), src.shape[0], src.shape[1], src.shape[2], row_stat, int(lo))


def max_distinct_offsets(q_row, q_off):
    q_row = np.ascontiguousarray(q_row, dtype=np.int64); q_off = np.ascontiguousarray(q_off, dtype=np.float64)
    return int(load().hostsim_max_distinct_offsets(ptr(q_row), ptr(q_off), len(q_row)))
