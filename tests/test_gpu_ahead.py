"""GPU suite (-m gpu): ssde_forecast_scores on every handle layout it serves.

The device against the host twin of its lane math (tests/aheadsim_lib.py, itself checked against the numpy definition of
tests/ahead_ref.py on the CPU: test_ahead_host.py) at test_gpu_loo.py's limits (loo_cases: z 1e-9, lpd and the sums 1e-11 (1 +
max|ref|), NaN patterns and counts exactly; thresholds midway between neighbouring twin q); against shipped code alone (ssde_smooth
on a second handle whose rows t - k + 1 .. t - 1 are NaN; ssde_eval / ssde_penalty at horizon 1); the edges, bitwise determinism,
isolation, refusals, and SDE.forecast_skill on simulated data.  Handles are small: 66 tracks of 1, 2, 3, 14 and 2 blocks + 5 rows,
so two wavefront groups, the second nearly empty."""
import ctypes as C
import math

import numpy as np
import pytest

import aheadsim_lib as AS
import loo_cases as LC
from cases import make_spec, problem_from_spec
from smoothsde_amd import capi
from test_ahead_host import compare

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
MODELS = LC.MODELS
HORIZONS = (1, 2, 5, 33)
B = 32                                                       # ssde_plan::AHEAD_BLOCK (test_ahead_host.py asserts it)
LENGTHS = ([2 * B + 5, 14, 3, 2, 1] * 14)[:66]
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _na_rows(lengths):
    """NA rows inside the first long track (two in a row, one later), inside and at the end of the first 14-row track, in the middle
    of the first 3-row track; never a track's first row"""
    st = np.r_[0, np.cumsum(lengths)]
    i69, i14, i3 = lengths.index(2 * B + 5), lengths.index(14), lengths.index(3)
    return (st[i69] + 30, st[i69] + 31, st[i69] + 50, st[i14] + 9, st[i14] + 13, st[i3] + 1)


def _spec(name, model, d, seed, **kw):
    return make_spec(name, model, d, seed=seed, lengths=LENGTHS, na_rows=_na_rows(LENGTHS), **kw)


def _twin(pb, par, horizons=HORIZONS, n_thr=8):
    with np.errstate(invalid="ignore"):
        z = AS.forecast_scores(pb, par, horizons)["z"]
        thr = LC.midway_thresholds(np.sum(z ** 2, axis=2).ravel(), n_thr)
    return AS.forecast_scores(pb, par, horizons, thr), thr


def _dev(out):
    """the engine's outputs in the twin's layout: z n x n_h x d, stats n_tracks x n_h x n_stat"""
    return {"z": None if out["z"] is None else out["z"].transpose(0, 2, 1), "lpd": out["lpd"],
            "stats": None if out["stats"] is None else out["stats"].transpose(0, 2, 1)}


def _check(eng, pb, par, tag, horizons=HORIZONS):
    ref, thr = _twin(pb, par, horizons)
    out = eng.forecast_scores(par, horizons, thresholds=thr)
    gaps = {}
    compare(_dev(out), ref, gaps)
    print("GAPS", tag, {k: f"{v:.1e}" for k, v in gaps.items()})
    return out, ref, thr


def _same(a, b):
    for k in ("z", "lpd", "stats"):
        if a[k] is not None and b[k] is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- 1. device versus twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d,grid", [(2, "regular"), (2, "irregular"), (1, "irregular")])
def test_tiled_handles_match_the_twin(model, d, grid):
    spec = _spec(f"gah_{model}_{d}_{grid}", model, d, 400 + d, irregular=grid == "irregular")
    pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    info = eng.info()
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == pb.n and info["n_groups"] == 2, info
    out, ref, _ = _check(eng, pb, par, f"{model} d={d} {grid}")
    eng.close()
    # a NA target is not scored and is stepped through as an intermediate row; the one-row tracks give zero statistics
    na = list(_na_rows(LENGTHS))
    assert np.all(np.isnan(out["lpd"][na])) and np.isfinite(out["lpd"][na[1] + 1, 1]) and np.isfinite(out["lpd"][na[1] + 2, 2])
    assert np.all(out["stats"][4] == 0.0) and out["stats"][0, 0, 3] > 0


def test_a_lattice_padded_handle_counts_the_callers_rows():
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks("CTCRW", 2, ([90, 16, 3, 2, 1] * 14)[:66], 0.5, 0.15, seed=9, na_frac=0.05)
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = _par("CTCRW", 2, np.random.default_rng(2))
    eng = capi.Engine(pb)
    info = eng.info()
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] > pb.n, info     # absent fixes are padded rows of the handle
    out, ref, _ = _check(eng, pb, par, "lattice")
    eng.close()
    assert out["stats"][:, 0, :].sum(axis=0).tolist() == np.isfinite(out["lpd"]).sum(axis=0).tolist()
    assert out["stats"][0, 0, 3] > 0                                          # horizon 33 inside the long tracks


def test_a_path_tv_handle_with_row_varying_parameters(monkeypatch):
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = make_spec("gah_tv", "CTCRW", 2, seed=29, lengths=[300, 20, 2 * B + 5, 35, 1, 14, 2, 3], variant="tv", na_rows=(7, 299, 310, 350))
    pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    info = eng.info()
    assert info["path"] == PATH_TV and info["const_coeff"] == 0, info
    _check(eng, pb, par, "tv")
    eng.close()


@pytest.mark.parametrize("model", MODELS)
def test_force_dense_with_a_per_row_h_array(model):
    spec = _spec(f"gah_dense_{model}", model, 2, 91, with_H=True)
    pb, par = problem_from_spec(spec, flags=capi.FLAG_FORCE_DENSE), np.asarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    info = eng.info()
    assert info["path"] == PATH_DENSE and info["n_groups"] == 2, info
    _check(eng, pb, par, f"dense {model}")
    eng.close()


@pytest.mark.parametrize("model,d", [("CTCRW", 2), ("OU_SSM", 1)])
def test_a_general_p0_and_a_per_row_h_array(model, d):
    spec = _spec(f"gah_p0_{model}", model, d, 93, with_H=True, with_P0=True)
    pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    print("LAYOUT", eng.info()["path"])
    _check(eng, pb, par, f"P0 {model}")
    eng.close()


# ---- 2. against shipped code, independent of the twin -----------------------------------------------------------------------------
def _blanked_resid(model, ID, times, obs, par, t, k, **kw):
    """ssde_smooth's whitened innovation at row t on a handle whose rows t - k + 1 .. t - 1 are NaN"""
    o = np.array(obs, dtype=np.float64, copy=True)
    o[t - k + 1:t] = np.nan
    eng = capi.Engine(capi.Problem(model, ID, times, o, **kw))
    r = eng.smooth(par, cov=False)["resid"][t]
    eng.close()
    return r


def test_z_ahead_is_the_smoothers_innovation_on_a_handle_with_the_rows_blanked():
    spec = _spec("gah_blank", "CTCRW", 2, 402, irregular=True)
    pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    out = eng.forecast_scores(par, HORIZONS, lpd=False, stats=False)
    eng.close()
    st = np.r_[0, np.cumsum(LENGTHS)]
    # (t, k): inside block 0; start in block 0 (row 32 = step 31) and target in block 1; horizon 33 across the boundary; a short track
    pairs = [(20, 2), (36, 5), (60, 33), (int(st[1]) + 8, 2)]
    for t, k in pairs:
        r = _blanked_resid("CTCRW", spec["ID"], spec["times"], spec["obs"], par, t, k)
        z = out["z"][t, :, HORIZONS.index(k)]
        print("BLANKED", t, k, z, r)
        assert np.all(np.isfinite(r)) and np.max(np.abs(z - r)) <= LC.RESID_TOL, (t, k, z, r)


def test_z_ahead_on_a_lattice_padded_handle_is_the_blanked_handles_innovation():
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks("CTCRW", 2, ([90, 16, 3, 2, 1] * 14)[:66], 0.5, 0.15, seed=9)
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = _par("CTCRW", 2, np.random.default_rng(2))
    eng = capi.Engine(pb)
    assert eng.info()["n_rows_tiled"] > pb.n
    out = eng.forecast_scores(par, HORIZONS, lpd=False, stats=False)
    eng.close()
    for t, k in [(25, 5), (50, 33)]:
        r = _blanked_resid("CTCRW", ID, times, obs, par, t, k)
        z = out["z"][t, :, HORIZONS.index(k)]
        print("BLANKED lattice", t, k, z, r)
        assert np.all(np.isfinite(r)) and np.max(np.abs(z - r)) <= LC.RESID_TOL, (t, k, z, r)


# ---- 3. horizon 1 closes the books ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_horizon_one_is_the_innovation_and_the_likelihood(model):
    spec = _spec(f"gah_books_{model}", model, 2, 404, irregular=True)
    pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    out = eng.forecast_scores(par, (1, 7))
    resid = eng.smooth(par, cov=False)["resid"]
    val = eng.eval(par, order=1)[0]
    pen = eng.penalty(par, want_grad=False)[0]
    eng.close()
    z1 = out["z"][:, :, 0]
    assert np.array_equal(np.isnan(z1), np.isnan(resid))
    ok = ~np.isnan(resid)
    gap_z = np.max(np.abs(z1[ok] - resid[ok])) / (1.0 + np.max(np.abs(resid[ok])))
    scored = out["stats"][:, 0, 0].sum()
    want = -(val - pen) - scored * pb.n_dim * math.log(2 * math.pi) / 2
    got = out["stats"][:, 1, 0].sum()
    print("BOOKS", model, gap_z, got, want, abs(got - want) / abs(want))
    assert scored == ok[:, 0].sum() and gap_z <= 1e-10
    assert abs(got - want) <= 1e-10 * abs(want)


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------------
def test_a_horizon_longer_than_every_track_and_the_largest_horizon():
    spec = make_spec("gah_short", "CTCRW", 2, seed=406, lengths=[14, 3, 2, 1] * 4, na_rows=(5,))
    pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    out = eng.forecast_scores(par, (64,), thresholds=[1.0])
    eng.close()
    assert np.all(np.isnan(out["z"])) and np.all(np.isnan(out["lpd"])) and np.all(out["stats"] == 0.0)
    assert out["stats"].shape == (16, 6, 1)
    spec = _spec("gah_64", "CTCRW", 2, 407)
    pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    _check(eng, pb, par, "horizon 64", horizons=(64,))
    eng.close()


@pytest.mark.parametrize("model", MODELS)
def test_a_target_without_a_positive_definite_s_is_not_scored(model):
    pb, par = LC.negative_p0_case(model)                     # sigma_obs tiny, P0 negative: S < 0 on every track's first state rows
    eng = capi.Engine(pb)
    out, ref, _ = _check(eng, pb, par, f"negP0 {model}", horizons=(1, 2, 5))
    eng.close()
    st = np.asarray(pb.seg_start)
    assert np.all(np.isnan(out["lpd"][st + 1, 0])) and np.isfinite(out["lpd"]).sum() > 0


# ---- 5. determinism, all bitwise ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["const", "lattice"])
def test_budget_devices_outputs_and_repeats_are_bitwise(layout):
    if layout == "const":
        spec = _spec("gah_det", "CTCRW", 2, 408)
        pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
    else:
        from test_gpu_lattice import _par, lattice_tracks
        ID, times, obs = lattice_tracks("OU_SSM", 2, ([90, 16, 3, 2, 1] * 14)[:66], 0.5, 0.15, seed=8, na_frac=0.05)
        pb, par = capi.Problem("OU_SSM", ID, times, obs), _par("OU_SSM", 2, np.random.default_rng(2))
    thr = [0.5, 2.0, 6.0]
    eng = capi.Engine(pb)
    one = eng.forecast_scores(par, HORIZONS, thresholds=thr)
    again = eng.forecast_scores(par, HORIZONS, thresholds=thr)
    _same(one, again)
    for kw in ({"lpd": False, "stats": False}, {"z": False, "stats": False}, {"z": False, "lpd": False}):
        alone = eng.forecast_scores(par, HORIZONS, thresholds=thr if kw.get("stats", True) else None, **kw)
        assert sum(v is not None for v in alone.values()) == 1
        _same(one, alone)
    # the records and side rows of the first group alone pass 1 MiB (68 steps x (31 + 11) x 64 doubles on CTCRW): two chunks
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    _same(one, eng.forecast_scores(par, HORIZONS, thresholds=thr))
    eng.close()
    eng = capi.Engine(pb, devices=[0, 0])
    assert eng.info()["n_devices"] == 2
    _same(one, eng.forecast_scores(par, HORIZONS, thresholds=thr))
    eng.close()


# ---- 6. isolation -------------------------------------------------------------------------------------------------------------------
def test_a_call_leaves_every_other_result_as_it_was():
    spec = _spec("gah_iso", "CTCRW", 2, 410, irregular=False)
    pb, par = problem_from_spec(spec), np.array(spec["par"], dtype=np.float64)
    par_b = par.copy(); par_b[1] += 0.01
    eng = capi.Engine(pb)
    va, ga = eng.eval(par, order=1)
    sm = eng.smooth(par)
    dr = eng.smooth_draws(par, 3, seed=11)
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.forecast_scores(par, HORIZONS, thresholds=[1.0, 4.0])
    after = eng.info()
    assert after["n_evals"] == before["n_evals"] and after["n_memo_hits"] == before["n_memo_hits"]
    vb2, gb2 = eng.eval(par_b, order=1)                                            # still the memo's: a hit
    assert eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1 and vb2 == vb and np.array_equal(gb2, gb)
    va2, ga2 = eng.eval(par, order=1)
    assert va2 == va and np.array_equal(ga2, ga)
    sm2 = eng.smooth(par)
    dr2 = eng.smooth_draws(par, 3, seed=11)
    eng.close()
    for k in ("mean", "cov", "resid"):
        assert np.array_equal(sm[k], sm2[k], equal_nan=True), k
    assert np.array_equal(dr, dr2, equal_nan=True)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_argument_checks_come_before_the_device():
    spec = make_spec("gah_args", "CTCRW", 2, seed=53, lengths=[20, 35, 1, 14], na_rows=(2, 19))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    p = np.ascontiguousarray(spec["par"], dtype=np.float64)
    n = pb.n
    z, lpd, st = np.full((n, 2, 2), 7.0, order="F"), np.full((n, 2), 7.0, order="F"), np.full((2, 13, pb.n_seg), 7.0)
    thr = np.array([1.0, 2.0])
    f = eng.lib.ssde_forecast_scores
    P = lambda a: a.ctypes.data_as(_dp)
    I = lambda *k: np.array(k, dtype=np.int32).ctypes.data_as(_ip)
    ok_h = (I(1, 2), 2)
    bad = [
        (None, *ok_h, P(z), None, None, 0, None, 0),                        # NULL par
        (P(p), None, 2, P(z), None, None, 0, None, 0),                      # NULL horizon
        (P(p), I(1), 0, P(z), None, None, 0, None, 0),                      # n_h outside 1 .. 8
        (P(p), I(*range(1, 10)), 9, P(z), None, None, 0, None, 0),
        (P(p), I(0, 2), 2, P(z), None, None, 0, None, 0),                   # a horizon out of range
        (P(p), I(1, 65), 2, P(z), None, None, 0, None, 0),
        (P(p), I(2, 2), 2, P(z), None, None, 0, None, 0),                   # not strictly increasing
        (P(p), I(5, 2), 2, P(z), None, None, 0, None, 0),
        (P(p), *ok_h, None, None, None, 0, None, 0),                        # all three outputs NULL
        (P(p), *ok_h, P(z), None, P(thr), -1, P(st), 0),                    # n_thr outside 0 .. 8
        (P(p), *ok_h, P(z), None, P(np.zeros(9)), 9, P(st), 0),
        (P(p), *ok_h, P(z), None, None, 2, P(st), 0),                       # thr NULL with n_thr > 0
        (P(p), *ok_h, P(z), None, P(np.array([1.0, -0.5])), 2, P(st), 0),   # a bad threshold: negative, NaN, infinite
        (P(p), *ok_h, P(z), None, P(np.array([np.nan, 1.0])), 2, P(st), 0),
        (P(p), *ok_h, P(z), None, P(np.array([1.0, np.inf])), 2, P(st), 0),
        (P(p), *ok_h, P(z), P(lpd), P(thr), 2, None, 0),                    # thresholds without stats
        (P(p), *ok_h, P(z), None, None, 0, None, 1),                        # a flag
    ]
    before = eng.info()
    for a in bad:
        assert f(eng._h, a[0], pb.n_par_full, *a[1:]) == 1, a[1:]            # SSDE_ERR_ARG
    assert f(eng._h, P(p), pb.n_par_full + 1, *ok_h, P(z), None, None, 0, None, 0) == 1
    assert np.all(z == 7.0) and np.all(lpd == 7.0) and np.all(st == 7.0)     # nothing was written
    assert eng.info()["n_evals"] == before["n_evals"]
    eng.close()


def test_models_and_layouts_that_are_not_served():
    from cases import eseal_spec
    for sp in (eseal_spec("gah_eseal", 211, [14, 9, 11]), make_spec("gah_cir", "CIR", 1, seed=221, lengths=[9, 2, 14]),
               make_spec("gah_ou", "OU", 1, seed=222, lengths=[9, 2, 14]),
               make_spec("gah_coupled", "CTCRW", 3, seed=223, lengths=[20, 9, 1, 14], with_H=True)):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.forecast_scores(sp["par"], (1, 2))
        assert ei.value.status == 2, sp["name"]                        # SSDE_ERR_MODEL
        eng.close()


def test_column_pairs_serve_z_alone_and_it_is_the_pair_handles():
    spec = make_spec("gah_pairs", "CTCRW", 4, seed=43, lengths=[20, 35, 1, 14, 2, 27, 9] * 10, na_rows=(2, 19))
    pb = problem_from_spec(spec)
    par = np.ascontiguousarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    assert eng.info()["n_rows_tiled"] == 2 * pb.n                      # two column pairs
    got = eng.forecast_scores(par, (1, 3, 10), lpd=False, stats=False)
    for kw in ({"lpd": True, "stats": False}, {"lpd": False, "stats": True}):
        with pytest.raises(capi.EngineError) as ei:
            eng.forecast_scores(par, (1, 3, 10), **kw)
        assert ei.value.status == 2 and "column pairs" in str(ei.value)     # SSDE_ERR_MODEL
    eng.close()
    for c0 in (0, 2):
        pp = capi.Problem("CTCRW", spec["ID"], spec["times"], spec["obs"][:, c0:c0 + 2])
        e2 = capi.Engine(pp)
        one = e2.forecast_scores(par[[0, 1 + c0, 2 + c0, 5, 6]], (1, 3, 10), lpd=False, stats=False)
        e2.close()
        assert np.array_equal(got["z"][:, c0:c0 + 2, :], one["z"], equal_nan=True), c0


# ---- 8. SDE.forecast_skill ----------------------------------------------------------------------------------------------------------
def test_forecast_skill_is_calibrated_on_data_simulated_from_the_model():
    """64 tracks x 200 rows simulated by ssde_simulate at tau = 2, nu = 1, sigma_obs = 0.1 and scored at those parameters.  One
    target per track and horizon (the track's last row) enters each check, so the targets are independent: mean q within 4
    standard errors of d = 2 (the variance of a chi-square_2 is 4) and the 95 % coverage within 4 binomial standard errors."""
    from smoothsde_amd.sde import SDE
    M, T, d, hz = 64, 200, 2, (1, 5, 20)
    ID, times, obs = capi.simulate_device("CTCRW", M, T, d, tau=2.0, nu=1.0, sigma_obs=0.1, seed=20)
    ID, times, obs = ID.cpu().numpy(), times.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy())
    data = {"ID": ID, "time": times, "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~1", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.0, 0.0, np.log(2.0), np.log(1.0)])
    sde.setup()
    par = sde._current_par_full().copy()
    par[0] = np.log(0.1)
    sde.par_full_ = par
    sk = sde.forecast_skill(horizons=hz, level=0.95)
    assert sk["horizons"] == list(hz) and abs(sk["threshold"] - 5.991464547107979) < 1e-9
    assert sk["tracks"]["n"].shape == (M, 3) and np.all(sk["pooled"]["n"] == [M * (T - k) for k in hz])
    print("SKILL pooled", {k: np.asarray(v).round(4).tolist() for k, v in sk["pooled"].items()})
    out = sde.engine_.forecast_scores(par, hz, stats=False)
    last = np.arange(M) * T + T - 1
    q = np.sum(out["z"][last] ** 2, axis=1)                               # M x n_h
    assert np.all(np.isfinite(q))
    for j, k in enumerate(hz):
        mean_q, cover = q[:, j].mean(), np.mean(q[:, j] <= sk["threshold"])
        print("SKILL last rows", k, mean_q, cover)
        assert abs(mean_q - d) <= 4 * math.sqrt(4.0 / M), (k, mean_q)
        assert abs(cover - 0.95) <= 4 * math.sqrt(0.95 * 0.05 / M), (k, cover)
    # the pooled sums are the per-row outputs added up
    lp = out["lpd"]
    assert np.allclose(sk["pooled"]["log_score"], np.nanmean(lp, axis=0), rtol=1e-10)
    assert np.all(sk["pooled"]["lead"] > 0) and np.all(np.diff(sk["pooled"]["rmse"]) > 0)
