"""CPU suite: the bulk cut at the transient's end (smoothsde_amd/csrc/ssde_windows.hpp: head_early_cut), through a host
build of window_geometry that takes the option and the list of built cuts (tests/hostsim/hostsim_headcut.cpp, headcut.mk).

Over the parameter grid of tests/test_head_plan_host.py: lag_cut == t0 exactly when the option is on, the model is CTCRW, lag_K > 0,
t0 > 0 with t0_delta == 0, t0 is one of the built cuts (and lag_K < t0: the statistics hold the lags below the cut), the window count is
not forced, and there is neither a Hessian request nor a plan that has given up; LAG_A otherwise.  No other field of the geometry
moves with the option."""
import ctypes as C
import os
import subprocess

import numpy as np

from hostsim_lib import WINDOW_EVAL, WINDOW_FACTS, _vec, window_geometry
from smoothsde_amd import capi
from test_head_plan_host import BENCH, CONSTS, CTCRW, LAG_A, _bench_par, _sweep

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_dp = C.POINTER(C.c_double)
_LIB = None
FIELDS = ("n_chunks", "window", "t0", "t0_delta", "dual", "n_chunks_d", "t0_d", "lag_K", "s_stat", "quiet_window", "quiet_w", "quiet_b0",
          "lag_cut", "plan_n_chunks", "plan_window", "plan_warmup")
CUTS = capi.LAG_CUTS
ALL_CUTS = (1 << len(CUTS)) - 1


def _load():
    global _LIB
    if _LIB is None:
        subprocess.run(["make", "-s", "-C", _DIR, "-f", "headcut.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_headcut.so"))
        lib.hostsim_headcut_geometry.argtypes = [_dp, C.POINTER(C.c_int), _dp, C.c_int, C.c_int, _dp, _dp]
        lib.hostsim_headcut_geometry.restype = None
        _LIB = lib
    return _LIB


def geometry(par, early, mask=ALL_CUTS, boost=1, gave_up=False, ev=None, **facts):
    f = np.concatenate([_vec(WINDOW_FACTS, facts), [float(early), float(mask), float(CUTS[0]), float(CUTS[1] - CUTS[0])]])
    c = np.asarray(CONSTS, dtype=np.int32)
    e = _vec(WINDOW_EVAL, ev or {})
    out = np.zeros(len(FIELDS))
    _load().hostsim_headcut_geometry(f.ctypes.data_as(_dp), c.ctypes.data_as(C.POINTER(C.c_int)), par.ctypes.data_as(_dp), boost, int(gave_up),
                                     e.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    return {k: int(v) for k, v in zip(FIELDS, out)}


def expected_cut(g, facts, early, mask, gave_up, ev):
    ok = (early and facts["model"] == CTCRW and g["lag_K"] > 0 and g["t0"] > 0 and g["t0_delta"] == 0 and not facts.get("chunks_forced", 0)
          and not (ev or {}).get("hess_req", 0) and not gave_up and g["t0"] in CUTS and (mask >> CUTS.index(g["t0"])) & 1
          and g["lag_K"] < g["t0"])
    return g["t0"] if ok else LAG_A


def test_the_bench_head_is_cut_at_its_transient_window():
    seen = set()
    for k in (-6, 0, 7, 50, 99):
        par = _bench_par(k)
        for gain_last in range(20, 33):
            ev = dict(gain_last=gain_last)
            on, off = geometry(par, 1, ev=ev, **BENCH), geometry(par, 0, ev=ev, **BENCH)
            assert on["lag_cut"] == on["t0"] in CUTS and off["lag_cut"] == LAG_A, (on, off)
            assert on["s_stat"] + on["lag_K"] <= on["lag_cut"] and on["lag_K"] < on["lag_cut"]
            assert {k_: v for k_, v in on.items() if k_ != "lag_cut"} == {k_: v for k_, v in off.items() if k_ != "lag_cut"}
            # the fields the existing suite pins are what the unchanged entry gives
            old = window_geometry(CONSTS, par, ev=ev, **BENCH)
            assert all(on[k_] == old[k_] for k_ in old if k_ not in ("first", "plan"))
            # a forced window count, a Hessian request, a plan that has given up, a cut that is not built: the late cut
            assert geometry(par, 1, ev=ev, **dict(BENCH, chunks_forced=1))["lag_cut"] == LAG_A
            assert geometry(par, 1, ev=dict(ev, hess_req=1), **BENCH)["lag_cut"] == LAG_A
            assert geometry(par, 1, gave_up=True, ev=ev, **BENCH)["lag_cut"] == LAG_A
            assert geometry(par, 1, mask=ALL_CUTS & ~(1 << CUTS.index(on["t0"])), ev=ev, **BENCH)["lag_cut"] == LAG_A
            assert geometry(par, 1, mask=0, ev=ev, **BENCH)["lag_cut"] == LAG_A
            seen.add(on["t0"])
    assert seen


def test_a_boosted_warm_up_moves_the_cut_or_falls_back_to_the_late_one():
    par = _bench_par(0)
    cuts = []
    for boost in (1, 2, 4, 16):
        g = geometry(par, 1, boost=boost, ev=dict(gain_last=24), **BENCH)
        assert g["lag_cut"] == expected_cut(g, BENCH, 1, ALL_CUTS, False, dict(gain_last=24))
        cuts.append(g["lag_cut"])
    assert cuts[0] < LAG_A and cuts[-1] == LAG_A and sorted(cuts) == cuts


def test_more_groups_than_wave_slots_keep_the_late_cut():
    """c4: the transient window stays on the wave of window 1 (t0_delta > 0)"""
    g = geometry(_bench_par(0), 1, ev=dict(gain_last=20), **dict(BENCH, n_groups=1563, max_chunks=2, want_chunks=1))
    assert g["lag_K"] > 0 and g["t0_delta"] > 0 and g["lag_cut"] == LAG_A


def test_the_cut_follows_its_conditions_and_moves_no_other_field_over_the_sweep():
    rng = np.random.default_rng(20250809)
    n_cut = n_late = n_off_list = 0
    for par, facts, boost, ev in _sweep(rng, 3000):
        mask = int(rng.choice([ALL_CUTS, ALL_CUTS, ALL_CUTS, ALL_CUTS, 0, int(rng.integers(0, ALL_CUTS + 1))]))
        gave_up = bool(rng.random() < 0.1)
        if rng.random() < 0.1:
            ev = dict(ev, hess_req=1)
        if rng.random() < 0.15:
            facts = dict(facts, chunks_forced=1)
        on = geometry(par, 1, mask=mask, boost=boost, gave_up=gave_up, ev=ev, **facts)
        off = geometry(par, 0, mask=mask, boost=boost, gave_up=gave_up, ev=ev, **facts)
        old = window_geometry(CONSTS, par, boost=boost, gave_up=gave_up, ev=ev, **facts)
        assert off["lag_cut"] == LAG_A
        assert on["lag_cut"] == expected_cut(on, facts, 1, mask, gave_up, ev), (facts, on)
        assert {k: v for k, v in on.items() if k != "lag_cut"} == {k: v for k, v in off.items() if k != "lag_cut"}, (facts, on, off)
        assert all(on[k] == old[k] for k in old if k not in ("first", "plan")), (facts, on, old)
        assert (on["plan_n_chunks"], on["plan_window"], on["plan_warmup"]) == tuple(old["plan"][k] for k in ("n_chunks", "window", "warmup"))
        if on["lag_cut"] < LAG_A:
            n_cut += 1
            assert on["s_stat"] + on["lag_K"] <= on["lag_cut"] and on["lag_cut"] % 16 == 0
        elif on["lag_K"] > 0 and on["t0"] > 0 and on["t0_delta"] == 0:
            n_late += 1
            n_off_list += on["t0"] not in CUTS
    assert n_cut > 30 and n_late > 50 and n_off_list > 5, (n_cut, n_late, n_off_list)
