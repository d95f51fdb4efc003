"""GPU suite: exact second derivatives over TIME WINDOWS (ssde_hess on the lane = direction path: hess_tv_device of csrc/ssde_hess.hip,
k_tv_hess.hip), the drift Hessian of the shared-covariance lanes (iso_drift_hess_kernel) and the 8 x 8 tiles of the direct families
(k_direct_hess.hip), against an outside reference that exists at any length: oracle_hess_quad, second central differences of the
restated likelihood in IEEE binary128 (oracle/oracle_quad.cpp; within 6e-14 of autograd Hessians where those are in reach,
tests/test_oracle_hess_quad.py).

The bar is the path's own: max|H - H_ref| <= 1e-9 max|H_ref|; 1e-10 on the direct families.  Every test prints its
gap; the table of DESIGN.md §3.5c is these prints.  What ran is read from Engine.hess_plan() (ssde_last_hess_plan): warm-up, windows
of the longest track, attempts, hand-over check."""
import numpy as np
import pytest
import torch

from hess_cases import direct_problem, direction_entries, free_entries, ragged_problem
from oracle_lib import oracle_hess_quad
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu
TOL = 1e-9

# name -> arguments of hess_cases.ragged_problem.  640-row long tracks hold two warm-ups of a case's plan (2 W <= 639 steps) except
# under BM_SSM's general P0 (variances of several units next to sigma_obs = 0.05: W = 336), whose long tracks are 960 rows.
RAGGED_CASES = {
    "CTCRW_d1": dict(model="CTCRW", d=1), "CTCRW_d2": dict(model="CTCRW", d=2),
    "OU_SSM_d1": dict(model="OU_SSM", d=1), "OU_SSM_d2": dict(model="OU_SSM", d=2),
    "BM_SSM_d1": dict(model="BM_SSM", d=1), "BM_SSM_d2": dict(model="BM_SSM", d=2),
    # the full-covariance lanes (HessLaneDense)
    "CTCRW_d2_H": dict(model="CTCRW", d=2, full="H"), "OU_SSM_d2_H": dict(model="OU_SSM", d=2, full="H"),
    "BM_SSM_d2_P0": dict(model="BM_SSM", d=2, full="P0", long_rows=960),
    # any-NaN mode with rows whose FIRST response column alone is NaN (hess_cases.ragged_problem says why the first)
    "CTCRW_d2_na_col": dict(model="CTCRW", d=2, na_first_column_only=True),
}


def _gap(H, Href):
    return float(np.max(np.abs(H - Href)) / np.max(np.abs(Href)))


@pytest.fixture(scope="module")
def batches():
    """name -> (problem, par, free entries, binary128 Hessian over them): built once per case, never written to"""
    cache = {}

    def get(name, **over):
        key = (name, tuple(sorted(over.items())))
        if key not in cache:
            kw = dict(RAGGED_CASES[name])
            par0 = over.pop("par0", None)
            kw.update(over)
            pb, par = ragged_problem(kw.pop("model"), kw.pop("d"), **kw)
            if par0 is not None:
                par = par.copy()
                par[0] = par0
            idx = free_entries(pb)
            Href = oracle_hess_quad(pb, par, idx)
            for a in (par, Href):
                a.setflags(write=False)
            cache[key] = (pb, par, idx, Href)
        return cache[key]

    return get


def _report(name, eng, gap):
    p = eng.hess_plan()
    print("\n[hess-windows] %-28s gap %.2e  warm_up %4d  windows_max %3d  attempts %d  check %.2e" % (
        name, gap, p["warm_up"], p["windows_max"], p["attempts"], p["check"]))
    return p


# ---- batch R: ragged tracks, irregular intervals, missing rows on window edges -------------------------------------------------------
@pytest.mark.parametrize("name", list(RAGGED_CASES))
def test_windowed_hessian_of_a_ragged_batch_matches_the_binary128_reference(name, batches):
    pb, par, idx, Href = batches(name)
    assert pb.n_seg == 7 and np.isnan(pb.obs[:, 0]).sum() == 32
    if name.endswith("na_col"):
        assert 0 < np.isnan(pb.obs[:, 1]).sum() < np.isnan(pb.obs[:, 0]).sum() and pb.na_mode == capi.NA_ANY_NAN
    eng = capi.Engine(pb)
    try:
        assert eng.info()["path"] == 3 and eng.info()["exact_hess_scope"] == 3, eng.info()
        assert eng.hess_plan() == dict(warm_up=0, windows_max=0, attempts=0, check=0.0)       # before any call
        H = eng.hess(par, idx)
        gap = _gap(H, Href)
        p = _report(name, eng, gap)
    finally:
        eng.close()
    assert p["windows_max"] >= 4 and p["attempts"] == 1 and p["warm_up"] > 0, p
    assert 2 * p["warm_up"] <= max(np.diff(np.append(pb.seg_start, pb.n))) - 1, p
    assert p["check"] <= 1e-10, p
    assert np.array_equal(H, H.T)
    assert gap <= TOL, gap


# ---- pair-block edges -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctcrw_d2_full(batches):
    """the 15-direction Hessian of the CTCRW d = 2 batch (120 pairs: a second block of 56 lanes), one engine for the subsets"""
    pb, par, idx, Href = batches("CTCRW_d2")
    dirs = direction_entries(pb)
    assert len(dirs) == 15 and len(idx) == 17
    eng = capi.Engine(pb)
    H = eng.hess(par, dirs)
    yield pb, par, idx, Href, dirs, eng, H
    eng.close()


@pytest.mark.parametrize("n_entries, n_pairs", [(15, 120), (11, 66), (10, 55)])
def test_pair_blocks_with_few_live_lanes(n_entries, n_pairs, ctcrw_d2_full):
    """120 pairs: a second block with 56 lanes; 66: a second block with 2 lanes; 55: one block with dead lanes"""
    pb, par, idx, Href, dirs, eng, H = ctcrw_d2_full
    # a subset that keeps log_sigma_obs, one mu and entries of both smooths, in an order of its own
    sub = (dirs[::2] + dirs[1::2])[:n_entries] if n_entries < 15 else dirs[::-1]
    assert len(sub) * (len(sub) + 1) // 2 == n_pairs
    Hs = eng.hess(par, sub)
    p = eng.hess_plan()
    assert p["windows_max"] >= 4 and p["attempts"] == 1, p
    pos = [dirs.index(k) for k in sub]
    d = float(np.max(np.abs(Hs - H[np.ix_(pos, pos)])) / np.max(np.abs(H)))
    rpos = [idx.index(k) for k in sub]
    gap = _gap(Hs, Href[np.ix_(rpos, rpos)])
    print("\n[hess-windows] %d entries, %d pairs: against the 15-entry Hessian %.2e, against the reference %.2e" % (n_entries, n_pairs, d, gap))
    assert np.array_equal(Hs, Hs.T)
    assert d <= 1e-13, d                                         # another tiling: another rounding
    assert gap <= TOL, gap


# ---- the retry loop -----------------------------------------------------------------------------------------------------------------------
SLOW = float(np.log(2.0))       # par[0] = log sigma_obs = log 2: slow forgetting


def _retry(name, batches, monkeypatch, window):
    pb, par, idx, Href = batches("CTCRW_d2", par0=SLOW)
    monkeypatch.setenv("SSDE_HESS_WINDOW", str(window))
    eng = capi.Engine(pb)
    try:
        H = eng.hess(par, idx)
        gap = _gap(H, Href)
        p = _report(name, eng, gap)
    finally:
        eng.close()
    assert np.array_equal(H, H.T)
    return p, gap


def test_a_short_first_warm_up_is_caught_and_widened(batches, monkeypatch):
    p, gap = _retry("retry SSDE_HESS_WINDOW=16", batches, monkeypatch, 16)
    assert p["attempts"] >= 2, p
    assert p["check"] <= 1e-10 or p["warm_up"] == 0, p
    assert gap <= TOL, gap


def test_a_warm_up_that_cannot_be_widened_ends_in_one_sequential_window(batches, monkeypatch):
    """At par[0] = log 2 no first warm-up ends in one window on 640-row tracks: 16 -> 64 -> 256 passes, and 96 -- the smallest whose
    quadruple no longer fits a track twice -- passes outright (check 1.5e-16).  At par[0] = log 4 a warm-up of 96 rows fails the
    check, and the second attempt is one sequential window per track."""
    pb, par, idx, Href = batches("CTCRW_d2", par0=float(np.log(4.0)))
    monkeypatch.setenv("SSDE_HESS_WINDOW", "96")
    eng = capi.Engine(pb)
    try:
        H = eng.hess(par, idx)
        gap = _gap(H, Href)
        p = _report("retry sigma_obs 4, window 96", eng, gap)
    finally:
        eng.close()
    assert p["attempts"] == 2 and p["warm_up"] == 0 and p["windows_max"] == 1, p
    assert np.array_equal(H, H.T)
    assert gap <= TOL, gap


# ---- second derivatives from another engine ----------------------------------------------------------------------------------------------
def test_companion_handle_runs_windows(batches):
    """a constant-coefficient handle on the register kernels, created with SSDE_FLAG_EXACT_HESS: the Hessian pass runs on its
    companion's rows, over windows, and the plan is reported through the handle"""
    pb0, par = ragged_problem("CTCRW", 2, lengths=[640, 640], smooth=False)
    pb1, _ = ragged_problem("CTCRW", 2, lengths=[640, 640], smooth=False, flags=capi.FLAG_EXACT_HESS)
    idx = free_entries(pb1)
    Href = oracle_hess_quad(pb1, par, idx)
    e0, e1 = capi.Engine(pb0), capi.Engine(pb1)
    try:
        assert e0.info()["path"] == 1 and e0.info()["exact_hess_scope"] == 0
        assert e1.info()["path"] == 1 and e1.info()["exact_hess_scope"] == 3
        v0, g0 = e0.eval(par)
        v1, g1 = e1.eval(par)
        assert v0 == v1 and np.array_equal(g0, g1)
        H = e1.hess(par, idx)
        gap = _gap(H, Href)
        p = _report("companion CTCRW d2 const", e1, gap)
        v2, g2 = e1.eval(par)
        assert v2 == v0 and np.array_equal(g2, g0)                  # ... and leaves the evaluation as it was
    finally:
        e0.close(); e1.close()
    assert p["windows_max"] >= 4 and p["attempts"] == 1 and p["check"] <= 1e-10, p
    assert np.array_equal(H, H.T)
    assert gap <= TOL, gap


def test_track_shards_sum_and_report_the_largest_plan(batches):
    pb, par, idx, Href = batches("OU_SSM_d1")
    one, two = capi.Engine(pb), capi.Engine(pb, devices=[0, 0])
    try:
        H1 = one.hess(par, idx)
        p1 = one.hess_plan()
        H2 = two.hess(par, idx)
        gap = _gap(H2, Href)
        p2 = _report("shards OU_SSM d1", two, gap)
    finally:
        one.close(); two.close()
    d = float(np.max(np.abs(H2 - H1)) / np.max(np.abs(H1)))
    print("[hess-windows] two shards against one engine %.2e" % d)
    assert d <= 1e-12, d
    assert gap <= TOL, gap
    # each shard holds one of the two 640-row tracks: the same warm-up, and with fewer tracks per engine at least as many windows
    assert p2["attempts"] == 1 and p2["warm_up"] == p1["warm_up"] and p2["windows_max"] >= p1["windows_max"] >= 4, (p1, p2)
    assert p2["check"] <= 1e-10


def test_a_batch_of_short_tracks_runs_one_window(batches):
    """every track shorter than two warm-ups: one sequential window each, and the plan says so"""
    pb, par = ragged_problem("CTCRW", 2, lengths=[1, 2, 3, 37, 90, 61], missing=False)
    idx = free_entries(pb)
    Href = oracle_hess_quad(pb, par, idx)
    eng = capi.Engine(pb)
    try:
        H = eng.hess(par, idx)
        gap = _gap(H, Href)
        p = _report("short tracks CTCRW d2", eng, gap)
    finally:
        eng.close()
    assert p["windows_max"] == 1 and p["attempts"] == 1 and p["check"] == 0.0, p
    assert np.array_equal(H, H.T)
    assert gap <= TOL, gap


# ---- the drift Hessian of the shared-covariance lanes (iso_drift_hess_kernel) ----------------------------------------------------------
# measured: 200 rows are the shortest tracks (of 100, 150, 200, 400) whose evaluation runs several windows (2; warm-up 48), whatever the
# track count (1, 2, 4, 8); four tracks rather than one, which would leave 63 of the wave's 64 lanes dead
DRIFT_TRACKS, DRIFT_ROWS = 4, 200


def test_drift_hessian_over_time_windows_matches_the_binary128_reference(monkeypatch):
    """the windowed batch of test_gpu_laplace's long drift test (CTCRW d = 2, mu_1 / mu_2 smooth with 9 / 5 columns), cut to
    DRIFT_TRACKS x DRIFT_ROWS rows -- its evaluation still runs several windows -- so that the binary128 reference takes seconds"""
    from test_gpu_drift import _batch
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", str(DRIFT_TRACKS))
    pb, par = _batch("CTCRW", 2, DRIFT_TRACKS, DRIFT_ROWS, (9, 5), seed=11)
    idx = [k for k in range(pb.off_re, pb.off_re + pb.n_re)] + [pb.off_fe, pb.off_fe + 1]
    Href = oracle_hess_quad(pb, par, idx)
    eng = capi.Engine(pb)
    try:
        assert eng.info()["path"] == 1 and eng.info()["exact_hess_scope"] == 1, eng.info()
        H = eng.hess(par, idx)
        info = eng.info()
        assert eng.hess_plan() == dict(warm_up=0, windows_max=0, attempts=0, check=0.0)       # not the hyper-dual lanes' pass
    finally:
        eng.close()
    gap = _gap(H, Href)
    print("\n[hess-windows] drift CTCRW d2 %d x %d: gap %.2e, windows %d, warm-up %d" % (DRIFT_TRACKS, DRIFT_ROWS, gap, info["lanes_per_track"], info["window"]))
    assert info["lanes_per_track"] > 1 and info["window"] > 0, info
    assert gap <= TOL, gap


# ---- the direct families' 8 x 8 tiles (k_direct_hess.hip) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_entries", [7, 8, 9, 16, 17])
@pytest.mark.parametrize("model, d", [("OU", 1), ("BM", 2)])
def test_direct_family_tiles_match_both_references(model, d, n_entries):
    """7 / 8 / 9 / 16 / 17 wanted entries: one tile with a dead row, one full tile, a second tile row of one, four full tiles, a
    third tile row of one"""
    from refimpl import direct_nllk, penalty
    pb, par = direct_problem(model, d, n_entries - 4)
    idx = list(range(pb.n_par_full))
    assert len(idx) == n_entries and pb.n_seg == 3 and np.isnan(pb.obs[:, 0]).sum() == 6
    Href = oracle_hess_quad(pb, par, idx)
    p0 = torch.tensor(par)

    def f(x):
        p = p0.clone()
        p[idx] = x
        return direct_nllk(pb, p) + penalty(pb, p)

    Ha = torch.autograd.functional.hessian(f, torch.tensor(par[idx])).numpy()
    eng = capi.Engine(pb)
    try:
        assert eng.info()["exact_hess_scope"] == 2
        H = eng.hess(par, idx)
        Hr = eng.hess(par, idx[::-1])
        assert eng.hess_plan() == dict(warm_up=0, windows_max=0, attempts=0, check=0.0)
    finally:
        eng.close()
    gq, ga = _gap(H, Href), _gap(H, Ha)
    rev = float(np.max(np.abs(Hr[::-1, ::-1] - H)) / np.max(np.abs(H)))
    print("\n[hess-windows] direct %s d%d, %2d entries: binary128 %.2e, autograd %.2e, reversed order %.2e" % (model, d, n_entries, gq, ga, rev))
    assert gq <= 1e-10 and ga <= 1e-10, (gq, ga)
    assert rev <= 1e-13, rev


def test_direct_family_hessian_is_bitwise_symmetric_and_the_same_at_every_call():
    """Found with this file: an 8 x 8 tile on the diagonal holds (k, l) and (l, k) as two accumulations that differ in their last
    bit, and direct_hess_reduce_kernel let both blocks store to both places -- which one stayed depended on the order the blocks
    finished in (1 ulp from run to run, H[k, l] != H[l, k] possible).  Now the upper one fills both."""
    pb, par = direct_problem("OU", 1, 13)
    idx = list(range(pb.n_par_full))
    eng = capi.Engine(pb)
    try:
        Hs = [eng.hess(par, idx) for _ in range(3)]
    finally:
        eng.close()
    e2 = capi.Engine(pb)
    try:
        Hs.append(e2.hess(par, idx))
    finally:
        e2.close()
    for H in Hs:
        assert np.array_equal(H, H.T)
        assert np.array_equal(H, Hs[0])
