"""GPU suite: the edges of the REVERSE sweep (csrc/k_iso_adj.hip, iso_adj_kernel -- the default kernel of every batch whose tau /
nu / drift vary by row) that the shapes of test_gpu_adjoint.py do not reach.

A. Windows of 2 GiB and more.  A group's tile is rows x C x 64 doubles whatever the number of tracks in it, so ONE window over a long
   track spans rows x C x 512 bytes; one window per track is an ordinary plan (slow forgetting, a plan that gave up, SSDE_CHUNKS=1,
   ssde_widen_windows(h, 0)).  A 32-bit row offset from one buffer resource over the window is negative past 2^31 and wraps past
   2^32: finite, wrong numbers, no fault.  One 430 000-row track of C = 20 channels (4.4 GB of tile), the same batch on many verified
   windows (the control), on two windows of 2.2 GB each and on one of 4.4 GB, each against ONE oracle evaluation.  The oracle walks
   the track on one thread (measured on a CPU: 37 s with all 25 parameters free, 10 s with six), so all but six parameters -- one of
   every kind of accumulator the kernel keeps -- are held fixed.  The window's span depends on the columns in the tile, not on the
   free entries, and every column of every row still enters the value and the six derivatives through the row's predictors.
   tests/test_adj_offsets_host.py checks the address arithmetic itself over the whole range of rows x C.
B. A handle with a history.  With order == 0 the kernel writes the forward half of each hand-over record only; the adjoint halves keep
   what earlier evaluations -- and their FAILED attempts -- left, and the check must not read them.
C. Tracks of 1 .. 9 rows and of WIN_ALIGN - 1 .. WIN_ALIGN + 1 (the backward block is 2 - 4 rows, the window grain WIN_ALIGN), ten
   groups of which the last holds one lane (the grid pads the groups to eight), long tracks among them so that windows exist.

Tolerances as everywhere (test_gpu_adjoint.py): value 1e-10 * max(1,|v|); gradient 1e-8 * max|g| + 1e-10; the same value from two
window plans 1e-13 * max(1,|v|), the same gradient 1e-12 * max|g| (test_reverse_sweep_vs_oracle_and_forward_tangents)."""
import os
import re

import numpy as np
import pytest

from smoothsde_amd import capi
from test_gpu_colvar import _batch, _close, _is_colvar, _oracle

pytestmark = pytest.mark.gpu
K_ADJ = 17
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smoothsde_amd", "csrc", "ssde_device.hpp")) as _f:
    WIN_ALIGN = int(re.search(r"constexpr int WIN_ALIGN = (\d+);", _f.read()).group(1))


@pytest.fixture(autouse=True)
def _take_the_lane_track_path_from_32_tracks(monkeypatch):
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "32")
    monkeypatch.setenv("SSDE_CV_ADJ", "2")                      # the few-column shapes too


def _value_close(val, oval):
    assert abs(val - oval) <= 1e-10 * max(1.0, abs(oval)), (val, oval)


def _same_as_on(inf, ref_inf, val, ref_val, grad=None, ref_grad=None):
    """the same batch and parameters on two handles: bitwise the same where the window plans are, the bars between plans otherwise"""
    if (inf["window"], inf["lanes_per_track"]) == (ref_inf["window"], ref_inf["lanes_per_track"]):
        assert val == ref_val, (val, ref_val)
        assert grad is None or np.array_equal(grad, ref_grad)
    else:
        assert abs(val - ref_val) <= 1e-13 * max(1.0, abs(ref_val)), (val, ref_val, inf, ref_inf)
        assert grad is None or np.max(np.abs(grad - ref_grad)) <= 1e-12 * np.max(np.abs(ref_grad))


# ---- A. windows of 2 GiB and more ------------------------------------------------------------------------------------------------------
LONG_ROWS, LONG_C = 430000, 20          # C: two response columns + 9 + 9 streamed columns, no time stamp (regular grid)


@pytest.fixture(scope="module")
def long_track():
    """One CTCRW track of LONG_ROWS rows, tau and nu each a 9-column spline of a per-row covariate: 430 simulated tracks of 1000 rows
    laid end to end (each starts where the one before ended), all but six parameters fixed, and the oracle's value and gradient."""
    pb0, par = _batch("CTCRW", 2, LONG_ROWS // 1000, 1000, 9, 9, seed=29)
    obs = pb0.obs.reshape(-1, 1000, 2).copy()
    obs -= obs[:, :1, :]
    obs[1:] += np.cumsum(obs[:-1, -1, :], axis=0)[:, None, :]
    fixed = np.ones(pb0.n_par_full, dtype=np.uint8)
    free = [0, pb0.off_fe + pb0.fe_off[0], pb0.off_fe + pb0.fe_off[2], pb0.off_fe + pb0.fe_off[3], pb0.off_re + 4, pb0.off_re + 9 + 6]
    fixed[free] = 0       # log sigma_obs, a drift intercept, the intercepts of log tau and log nu, a spline coefficient of each
    pb = capi.Problem("CTCRW", np.zeros(LONG_ROWS), pb0.times, obs.reshape(-1, 2), X_fe=pb0.X_fe, X_re=pb0.X_re, S_list=pb0.S_list,
                      par_fixed=fixed)
    assert pb.n == LONG_ROWS and len(pb.seg_start) == 1
    oval, ograd = _oracle(pb, par)
    assert np.all(ograd[fixed.astype(bool)] == 0.0) and np.all(ograd[free] != 0.0)
    ograd.setflags(write=False)
    par.setflags(write=False)
    return pb, par, fixed.astype(bool), oval, ograd


def _long_engine(pb, monkeypatch, chunks=None):
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "1")
    if chunks is not None:
        monkeypatch.setenv("SSDE_CHUNKS", str(chunks))
    eng = capi.Engine(pb)
    assert _is_colvar(eng)
    inf = eng.info()
    # the tile really has LONG_C channels of 64 lanes a row: less than one more channel's worth on top of rows x C x 512 bytes (the
    # spare rows, the hand-over records, the partial sums)
    span = LONG_ROWS * LONG_C * 512
    assert inf["uniform_dt"] == 1 and inf["n_groups"] == 1 and inf["n_tracks"] == 1
    assert span <= inf["hbm_bytes"] < span + LONG_ROWS * 512, (inf["hbm_bytes"], span)
    return eng


def _check_long(eng, long_track):
    pb, par, fixed, oval, ograd = long_track
    val, grad = eng.eval(par)
    inf = eng.info()
    print("long track:", inf["lanes_per_track"], "windows, warm-up", inf["window"], "retries", inf["window_retries"], "check",
          inf["window_check"], "value", val, "oracle", oval, "gradient error", np.max(np.abs(grad - ograd)), "of", np.max(np.abs(ograd)))
    assert inf["kernel_id"] == K_ADJ and inf["window_check"] <= 1e-11, inf
    _close(val, grad, oval, ograd)
    assert np.all(grad[fixed] == 0.0)
    return inf


def test_long_track_on_many_verified_windows_is_the_oracles(long_track, monkeypatch):
    """The control: the default plan, every window far below 2 GiB -- the batch and the oracle agree at this length."""
    eng = _long_engine(long_track[0], monkeypatch)
    inf = _check_long(eng, long_track)
    assert inf["window"] > 0 and inf["lanes_per_track"] >= 8
    assert (LONG_ROWS // inf["lanes_per_track"] + 3 * inf["window"] + WIN_ALIGN) * LONG_C * 512 < 2 ** 31
    eng.close()


def test_two_windows_between_2_gib_and_4_gib_each(long_track, monkeypatch):
    eng = _long_engine(long_track[0], monkeypatch, chunks=2)
    inf = _check_long(eng, long_track)
    assert inf["lanes_per_track"] == 2 and inf["window"] > 0
    # each window: its half of the rows at least, its warm-up or its backward tail and an alignment unit at most on top
    assert (LONG_ROWS // 2 - WIN_ALIGN) * LONG_C * 512 >= 2 ** 31
    assert (LONG_ROWS // 2 + 2 * inf["window"] + 2 * WIN_ALIGN) * LONG_C * 512 < 2 ** 32
    eng.close()


def test_one_window_past_4_gib(long_track, monkeypatch):
    pb, par, fixed, oval, ograd = long_track
    eng = _long_engine(pb, monkeypatch, chunks=1)
    inf = _check_long(eng, long_track)
    assert inf["lanes_per_track"] == 1 and inf["window"] == 0
    assert LONG_ROWS * LONG_C * 512 >= 2 ** 32
    eng.forget()                                                   # (the same parameters again: not the memoised value)
    n0 = eng.info()["n_evals"]
    v0 = eng.eval(par, order=0)
    inf = eng.info()
    assert inf["n_evals"] == n0 + 1 and inf["kernel_id"] == K_ADJ and inf["window"] == 0 and inf["window_check"] <= 1e-11
    _value_close(v0, oval)
    eng.close()


# ---- B. a handle with a history ----------------------------------------------------------------------------------------------------------
def _device_value(eng, pb, par):
    """ssde_eval_device, value only, on a stream of its own: (the data term + the penalty, the check slot)"""
    import torch
    out = torch.zeros(2 + pb.n_par_full, dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream()
    eng.eval_device(par, out.data_ptr(), order=0, stream=st.cuda_stream)
    st.synchronize()
    host = out.cpu().numpy()
    return host[0] + eng.penalty(par, want_grad=False)[0], host[-1]


def test_value_only_evaluations_after_a_repaired_gradient_evaluation(monkeypatch):
    """A gradient evaluation whose backward tail is useless (SSDE_ADJ_TAIL=4) fails its hand-over check and is repaired with fewer,
    longer windows: the records past the new window count keep the adjoints that disagreed.  Once the plan is as narrow as before, a
    value-only evaluation -- which writes no adjoints -- must not be judged on them: no retry, an agreeing check, the plan and the
    value of a handle without a history.
    The batch of test_short_backward_tail_is_detected_and_repaired with longer tracks and a window count of the test's own.  The
    reverse sweep's own plan picks its window count by cost, whatever the warm-up, until the warm-up passes the track and ONE window is
    left (that batch: 46 windows, 46, 46, then 1 at 16 x the warm-up).  With SSDE_CHUNKS=8 the count follows the warm-up -- a window
    holds two of them -- and 5600 rows leave two windows at the 16 x the tail of 4 rows needs (warm-up 96 -> 1296 rows): 8, 8, 8, 2.
    Records 2 .. 7 then keep the adjoints of the attempt at 4 x, which disagreed."""
    pb, par = _batch("CTCRW", 2, 40, 5600, 6, 6, seed=17)
    par[0] = 0.3                                                # sigma_obs = 1.35: slow forgetting
    oval, ograd = _oracle(pb, par)
    monkeypatch.setenv("SSDE_ADJ_TAIL", "4")
    monkeypatch.setenv("SSDE_CHUNKS", "8")
    eng = capi.Engine(pb)
    assert _is_colvar(eng)
    first = eng.eval(par)
    inf1 = eng.info()
    assert inf1["kernel_id"] == K_ADJ and inf1["window_retries"] >= 1, inf1
    assert inf1["lanes_per_track"] > 1 and inf1["window"] > 0 and inf1["window_check"] <= capi.WINDOW_TOL, inf1      # repaired, not given up
    _close(*first, oval, ograd)
    for k in range(24):                                         # (the boost halves at every call and stops at 1; it is at most 2^20)
        eng.relax_windows()
    eng.forget()
    # a handle without a history, at its first evaluation
    fresh = capi.Engine(pb)
    fv = fresh.eval(par, order=0)
    finf = fresh.info()
    assert finf["kernel_id"] == K_ADJ and finf["window_retries"] == 0 and finf["window_check"] <= capi.WINDOW_TOL, finf
    _value_close(fv, oval)
    assert 1 < inf1["lanes_per_track"] < finf["lanes_per_track"], (inf1, finf)      # fewer, longer windows than the plan that failed
    # 1. the synchronous call
    v0 = eng.eval(par, order=0)
    inf0 = eng.info()
    print("history:", inf1, "\nvalue only after it:", inf0, "\nfresh:", finf)
    assert inf0["n_evals"] == inf1["n_evals"] + 1
    assert inf0["window_retries"] == inf1["window_retries"], (inf0, inf1)
    assert inf0["window_check"] <= capi.WINDOW_TOL, inf0
    assert (inf0["window"], inf0["lanes_per_track"]) == (finf["window"], finf["lanes_per_track"]), (inf0, finf)
    _same_as_on(inf0, finf, v0, fv)
    _value_close(v0, oval)
    # 2. the asynchronous call: its caller rejects on the check slot
    vd, chk = _device_value(eng, pb, par)
    assert chk <= capi.WINDOW_TOL, chk
    assert abs(vd - v0) <= 1e-13 * max(1.0, abs(v0)), (vd, v0)
    # 3. a gradient evaluation afterwards (the tail is still crippled: it may retry again)
    eng.forget()
    val, grad = eng.eval(par)
    assert eng.info()["window_check"] <= capi.WINDOW_TOL or eng.info()["lanes_per_track"] == 1
    _close(val, grad, oval, ograd)
    eng.close(); fresh.close()


def test_value_only_evaluations_between_plans_of_different_window_counts(monkeypatch):
    """order = 1 at theta_A, order = 0 at a theta_B whose plan has another window count, order = 0 at theta_A again: each is what a
    handle without a history returns, without a retry.  (SSDE_CHUNKS=12: at most twelve windows, each at least two warm-ups long --
    the reverse sweep's own plan keeps its window count whatever the warm-up.)"""
    pb, par_a = _batch("CTCRW", 2, 96, 1500, 6, 6, seed=17)
    par_b = par_a.copy()
    par_b[0] = 0.3                                              # sigma_obs 0.12 -> 1.35: slower forgetting, longer warm-ups, fewer windows
    monkeypatch.setenv("SSDE_CHUNKS", "12")
    eng = capi.Engine(pb)
    seen = []
    for par, order in ((par_a, 1), (par_b, 0), (par_a, 0)):
        fresh = capi.Engine(pb)
        ref = fresh.eval(par, order=order)
        rinf = fresh.info()
        assert rinf["kernel_id"] == K_ADJ and rinf["window_retries"] == 0 and rinf["window_check"] <= capi.WINDOW_TOL, rinf
        eng.forget()
        n0 = eng.info()["n_evals"]
        got = eng.eval(par, order=order)
        inf = eng.info()
        assert inf["n_evals"] == n0 + 1 and inf["kernel_id"] == K_ADJ and inf["window_retries"] == 0 and inf["window_check"] <= capi.WINDOW_TOL, inf
        if order:
            _same_as_on(inf, rinf, got[0], ref[0], got[1], ref[1])
            _close(*got, *_oracle(pb, par))
        else:
            _same_as_on(inf, rinf, got, ref)
            _value_close(got, _oracle(pb, par)[0])
        seen.append((inf["lanes_per_track"], inf["window"]))
        fresh.close()
    print("plans (windows, warm-up):", seen)
    assert 1 < seen[1][0] < seen[0][0] and seen[1][1] > seen[0][1] and seen[2] == seen[0], seen      # theta_B's plan really has another window count
    eng.close()


# ---- C. the kernel's small edges -----------------------------------------------------------------------------------------------------------
SHORT = [1, 2, 3, 4, 5, 6, 7, 8, 9, WIN_ALIGN - 1, WIN_ALIGN, WIN_ALIGN + 1]
N_EDGE_TRACKS, LONGEST = 64 * 9 + 1, 600


def _edge_batch(model, d, k1, k2, missing):
    """577 tracks -- ten groups, the last with one lane --: every eighth 600 rows long (so that windows exist), the others cycling
    through SHORT; 6 streamed columns"""
    pb0, par = _batch(model, d, N_EDGE_TRACKS, LONGEST, k1, k2, seed=43)
    lens = np.array([SHORT[(i - i // 8) % len(SHORT)] for i in range(N_EDGE_TRACKS)])
    lens[7::8] = LONGEST
    assert set(SHORT) <= set(lens.tolist())
    keep = np.concatenate([np.arange(LONGEST) < L for L in lens])
    obs = pb0.obs[keep].copy()
    n = int(keep.sum())
    ident = pb0.id[keep]
    if missing:                                                    # 3 % of the rows without column 0, never a track's first
        na = np.random.default_rng(5).random(n) < 0.03
        na[np.r_[0, 1 + np.flatnonzero(np.diff(ident) != 0)]] = False
        obs[na, 0] = np.nan
    cut = lambda X: None if X is None else X[keep]
    pb = capi.Problem(model, ident, np.arange(1.0, n + 1), obs, X_fe=[cut(X) for X in pb0.X_fe], X_re=[cut(X) for X in pb0.X_re],
                      S_list=pb0.S_list)
    assert len(pb.seg_start) == N_EDGE_TRACKS
    return pb, par


@pytest.mark.parametrize("missing", [False, True], ids=["complete", "missing"])
@pytest.mark.parametrize("model,d,k1,k2", [("CTCRW", 2, 3, 3), ("OU_SSM", 1, 3, 3), ("BM_SSM", 2, 6, 0)])
def test_tracks_of_a_few_rows_and_a_last_group_of_one_lane(model, d, k1, k2, missing):
    pb, par = _edge_batch(model, d, k1, k2, missing)
    oval, ograd = _oracle(pb, par)
    eng = capi.Engine(pb)
    assert _is_colvar(eng)
    val, grad = eng.eval(par)
    inf = eng.info()
    assert inf["kernel_id"] == K_ADJ and inf["n_groups"] == 10 and inf["window_check"] <= 1e-11, inf
    assert inf["lanes_per_track"] > 1 and inf["window"] > 0, inf
    _close(val, grad, oval, ograd)
    eng.forget()
    n0 = inf["n_evals"]
    v0 = eng.eval(par, order=0)
    inf = eng.info()
    assert inf["n_evals"] == n0 + 1 and inf["kernel_id"] == K_ADJ and inf["window_check"] <= 1e-11, inf
    _value_close(v0, oval)
    eng.close()
