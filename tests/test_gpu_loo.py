"""GPU suite (-m gpu): ssde_smooth_loo on every handle layout it serves, against the numpy definition of
tests/loo_ref.py (itself checked against the dense joint Gaussian with a block deleted, and the host twin of the lane math against
it, on the CPU: test_loo_host.py, test_loo_hostsim.py).

Every case asserts the layout it ran on (info(): path, n_rows_tiled, n_devices) and goes through loo_cases.compare: mean
1e-10 (1 + max|ref|), covariance 1e-9 max|ref|, residual 1e-9, lpd and the statistics k = 1, 2 at 1e-11 (1 + max|ref|); NaN patterns,
served rows, the rows of the maxima and the threshold counts exactly (thresholds midway between neighbouring reference q_j)."""
import ctypes as C

import numpy as np
import pytest

import loo_cases as LC
from cases import make_spec, problem_from_spec
from loo_ref import loo_ref
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
MODELS = LC.MODELS
KEYS = ("mean", "cov", "resid", "lpd", "stats")
_dp = C.POINTER(C.c_double)


def _show(tag, info, **more):
    keys = ("path", "kernel_id", "const_coeff", "n_rows", "n_rows_tiled", "n_groups", "n_devices")
    print("LAYOUT", tag, {k: info[k] for k in keys}, more)


def _ref(pb, par, n_thr=8):
    """loo_ref with thresholds midway between its own q_j"""
    with np.errstate(invalid="ignore"):
        thr = LC.midway_thresholds(loo_ref(pb, par)["q"], n_thr)
        return loo_ref(pb, par, thr), thr


def _check(eng, pb, par, tag, gaps=None):
    ref, thr = _ref(pb, par)
    got = eng.smooth_loo(par, thresholds=thr)
    g = {} if gaps is None else gaps
    LC.compare(got, ref, list(pb.seg_start) + [pb.n], g)
    print("GAPS", tag, {k: f"{v:.1e}" for k, v in g.items()})
    return got, ref, thr


def _same(a, b):
    for k in KEYS:
        if a[k] is not None or b[k] is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("grid", ["regular", "irregular"])
def test_ragged_tracks_with_na_rows_and_a_one_row_track(model, d, grid):
    spec = make_spec(f"gloo_{model}_{d}_{grid}", model, d, seed=70 + d, lengths=[20, 35, 1, 14], irregular=grid == "irregular",
                     na_rows=(2, 19, 40))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"ragged {model} d={d} {grid}", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == pb.n and info["n_groups"] == 1
    got, ref, _ = _check(eng, pb, spec["par"], f"ragged {model} d={d} {grid}")
    eng.close()
    for k in ("mean", "cov", "resid", "lpd"):
        assert np.all(np.isnan(got[k][[0, 2, 19, 20, 40, 55, 56]])), k       # first rows, NA rows, the one-row track
    assert np.array_equal(got["stats"][2, :4], [0, 0, np.nan, np.nan], equal_nan=True) and np.all(got["stats"][2, 4:] == 0)
    assert got["stats"][:, 0].sum() == 66 - 3                             # 70 rows, four first rows, three NA rows


def _lengths150():
    return [int(v) for v in np.random.default_rng(83).integers(5, 41, size=150)]


@pytest.mark.parametrize("d", [2, 4])
def test_150_tracks_in_three_groups_chunked_and_not_are_bitwise(d):
    """150 tracks of 5 ... 40 rows: three wavefront groups, the last partly filled.  The budget's unit is 1 MiB = 131072 doubles.
    d = 2: the register kernel on tiled rows; its records of 31 doubles are small enough for two groups of such tracks to share a
    MiB, so the budget gives two chunks there (all three groups do not fit).  d = 4 with a coupling H: one filter of eight states
    with records of 96 doubles, where no two groups fit -- tracks go to lanes longest first, the groups' longest tracks are asserted
    below -- so every group is a chunk of its own: three chunks.  The count is not read from the engine (it reports none): the
    assertion repeats the rule of chunk_groups (csrc/ssde_smooth_plan.hpp: a chunk is closed before the group that would take
    it past the budget) on the groups' record sizes, steps of the longest track x R x 64 doubles."""
    lengths = _lengths150()
    spec = make_spec(f"gloo_150_{d}", "CTCRW", d, seed=83, lengths=lengths, with_H=d == 4, na_rows=(2, lengths[0] - 1))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"150 tracks d={d}", info)
    assert info["n_groups"] == 3 and info["n_rows_tiled"] == pb.n and info["path"] == (PATH_ISO if d == 2 else PATH_DENSE)
    steps = np.sort(np.array(lengths) - 1)[::-1]
    s0, s1, s2 = steps[0], steps[64], steps[128]
    R = 31 if d == 2 else 96
    assert (s0 + s1 + s2) * R * 64 > 131072 and (d == 2 or min(s0 + s1, s1 + s2) * R * 64 > 131072)
    one, ref, thr = _check(eng, pb, spec["par"], f"150 tracks d={d}")
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.smooth_loo(spec["par"], thresholds=thr)
    eng.close()
    _same(one, many)


def test_a_lattice_padded_handle_serves_the_callers_rows():
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks("CTCRW", 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=9, na_frac=0.05)
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = _par("CTCRW", 2, np.random.default_rng(2))
    eng = capi.Engine(pb)
    info = eng.info()
    _show("lattice", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] > pb.n       # absent fixes are padded rows of the handle
    got, ref, _ = _check(eng, pb, par, "lattice")
    eng.close()
    # the row of a maximum is a row of the caller's data, inside its track; padded rows are in no count
    bounds = np.r_[pb.seg_start, pb.n]
    ok = ~np.isnan(got["stats"][:, 3])
    assert ok.sum() >= 48 and np.all(got["stats"][ok, 3] > bounds[:-1][ok]) and np.all(got["stats"][ok, 3] < bounds[1:][ok])
    assert got["stats"][:, 0].sum() == np.isfinite(got["lpd"]).sum() == ref["white"].sum()


def test_a_path_tv_handle(monkeypatch):
    # tau ~ x: one long track and short ones on the row-varying route (lane = track of the length-sorted order)
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = make_spec("gloo_tv", "CTCRW", 2, seed=29, lengths=[300, 20, 35, 1, 14, 2], variant="tv", na_rows=(7, 299, 310))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show("tv", info)
    assert info["path"] == PATH_TV and info["const_coeff"] == 0
    _check(eng, pb, spec["par"], "tv")
    eng.close()


@pytest.mark.parametrize("model", MODELS)
def test_force_dense(model):
    spec = make_spec(f"gloo_dense_{model}", model, 2, seed=91, lengths=[20, 35, 1, 14, 2, 27, 9] * 10, with_H=True, na_rows=(2, 19))
    pb = problem_from_spec(spec, flags=capi.FLAG_FORCE_DENSE)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"dense {model}", info)
    assert info["path"] == PATH_DENSE and info["n_groups"] == 2
    _check(eng, pb, spec["par"], f"dense {model}")
    eng.close()


@pytest.mark.parametrize("model", MODELS)
def test_a_coupled_filter_of_five_columns(model):
    # a per-row H couples the columns: one filter of width 5 (k_smooth_loo_wide.hip)
    spec = make_spec(f"gloo_wide_{model}", model, 5, seed=35, lengths=([20, 35, 1, 14, 2, 27, 9] * 10)[:67], with_H=True, na_rows=(2, 19))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"wide {model}", info)
    assert info["path"] == PATH_DENSE and info["sdim"] == pb.sdim and info["n_devices"] <= 1
    _check(eng, pb, spec["par"], f"wide {model}")
    eng.close()


def test_an_uncoupled_wide_response_serves_the_rows_and_refuses_the_sums():
    spec = make_spec("gloo_pairs", "CTCRW", 4, seed=43, lengths=[20, 35, 1, 14, 2, 27, 9] * 10, na_rows=(2, 19))
    pb = problem_from_spec(spec)
    par = np.ascontiguousarray(spec["par"], dtype=np.float64)
    eng = capi.Engine(pb)
    info = eng.info()
    _show("pairs", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == 2 * pb.n      # two column pairs
    got = eng.smooth_loo(par, lpd=False, stats=False)
    ref = loo_ref(pb, par)
    assert got["lpd"] is None and got["stats"] is None
    LC.compare(got, ref)
    served = ref["served"]
    pair = np.arange(4) // 2
    cross = pair[:, None] != pair[None, :]
    assert np.all(got["cov"][served][:, cross] == 0.0) and np.all(np.isnan(got["cov"][~served]))
    # the reference's cross blocks are zero up to rounding only: the model is uncoupled
    assert np.max(np.abs(ref["cov"][served][:, cross])) <= 1e-9 * np.max(np.abs(ref["cov"][served]))
    for kw in ({"lpd": True, "stats": False}, {"lpd": False, "stats": True}):
        with pytest.raises(capi.EngineError) as ei:
            eng.smooth_loo(par, **kw)
        assert ei.value.status == 2 and "column pairs" in str(ei.value)     # SSDE_ERR_MODEL
    eng.close()


@pytest.mark.parametrize("layout", ["const", "lattice"])
def test_two_shards_on_one_device_are_bitwise_the_single_handle(layout):
    if layout == "const":
        spec = make_spec("gloo_shards", "CTCRW", 2, seed=47, lengths=[20, 35, 1, 14, 2, 27, 9] * 10, na_rows=(2, 19))
        pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
    else:
        from test_gpu_lattice import _par, lattice_tracks
        ID, times, obs = lattice_tracks("OU_SSM", 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
        pb, par = capi.Problem("OU_SSM", ID, times, obs), _par("OU_SSM", 2, np.random.default_rng(2))
    eng = capi.Engine(pb)
    one, ref, thr = _check(eng, pb, par, f"shards {layout} single")
    eng.close()
    eng = capi.Engine(pb, devices=[0, 0])
    info = eng.info()
    _show(f"shards {layout}", info)
    assert info["n_devices"] == 2 and info["path"] == PATH_ISO
    assert info["n_rows_tiled"] == pb.n if layout == "const" else info["n_rows_tiled"] > pb.n
    two = eng.smooth_loo(par, thresholds=thr)
    eng.close()
    _same(one, two)


def test_direct_families_and_eseal_are_refused():
    from cases import eseal_spec
    for sp in (eseal_spec("gloo_eseal", 211, [14, 9, 11]), make_spec("gloo_cir", "CIR", 1, seed=221, lengths=[9, 2, 14])):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.smooth_loo(sp["par"])
        assert ei.value.status == 2                                   # SSDE_ERR_MODEL
        eng.close()


def test_argument_checks_come_before_the_device():
    spec = make_spec("gloo_args", "CTCRW", 2, seed=53, lengths=[20, 35, 1, 14], na_rows=(2, 19))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show("argument checks", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == pb.n
    p = np.ascontiguousarray(spec["par"], dtype=np.float64)
    n = pb.n
    mean, lpd, st = np.full((n, 2), 7.0, order="F"), np.full(n, 7.0), np.full((12, pb.n_seg), 7.0)
    thr = np.array([1.0, 2.0])
    f = eng.lib.ssde_smooth_loo
    P = lambda a: a.ctypes.data_as(_dp)
    bad = [
        (p, None, None, None, None, None, 0, None, 0),                      # all five outputs NULL
        (p, P(mean), None, None, None, P(thr), -1, P(st), 0),               # n_thr outside 0 .. 8
        (p, P(mean), None, None, None, P(np.zeros(9)), 9, P(st), 0),
        (p, P(mean), None, None, None, None, 2, P(st), 0),                  # thr NULL with n_thr > 0
        (p, P(mean), None, None, None, P(np.array([1.0, -0.5])), 2, P(st), 0),      # a bad threshold: negative, NaN, infinite
        (p, P(mean), None, None, None, P(np.array([np.nan, 1.0])), 2, P(st), 0),
        (p, P(mean), None, None, None, P(np.array([1.0, np.inf])), 2, P(st), 0),
        (p, P(mean), None, None, P(lpd), P(thr), 2, None, 0),               # thresholds without stats
        (p, P(mean), None, None, None, None, 0, None, 1),                   # a flag
    ]
    before = eng.info()
    for a in bad:
        assert f(eng._h, P(a[0]), pb.n_par_full, *a[1:]) == 1, a[6:]         # SSDE_ERR_ARG
    assert f(eng._h, P(p), pb.n_par_full + 1, P(mean), None, None, None, None, 0, None, 0) == 1
    assert np.all(mean == 7.0) and np.all(lpd == 7.0) and np.all(st == 7.0)   # nothing was written
    after = eng.info()
    assert after["n_evals"] == before["n_evals"]
    # ... and each output alone is the full call's
    full = eng.smooth_loo(p, thresholds=thr)
    assert f(eng._h, P(p), pb.n_par_full, None, None, None, P(lpd), None, 0, None, 0) == 0
    assert np.array_equal(lpd, full["lpd"], equal_nan=True)
    st2 = np.zeros((6, pb.n_seg))
    assert f(eng._h, P(p), pb.n_par_full, None, None, None, None, P(thr), 2, P(st2), 0) == 0
    assert np.array_equal(st2.T, full["stats"], equal_nan=True)
    V = np.zeros((n, 2, 2), order="F")
    assert f(eng._h, P(p), pb.n_par_full, None, P(V), None, None, None, 0, None, 0) == 0
    assert np.array_equal(V, full["cov"], equal_nan=True)
    eng.close()


def _sde_at(ID, times, obs, sigma_obs):
    """a CTCRW of two columns as an SDE object, its parameters held at the simulation's (no fit)"""
    from smoothsde_amd.sde import SDE
    data = {"ID": ID, "time": times, "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~1", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.0, 0.0, np.log(2.0), np.log(1.0)])
    sde.setup()
    par = sde._current_par_full().copy()
    par[0] = np.log(sigma_obs)
    sde.par_full_ = par
    return sde, par


def test_a_planted_outlier_is_named():
    from smoothsde_amd.synth import simulate
    sigma_obs = 0.1
    ID, times, obs = simulate("CTCRW", 3, 40, 2, tau=2.0, nu=1.0, sigma_obs=sigma_obs, seed=12)
    bad = 40 + 23                                                     # row 23 of the second track, moved by 50 sigma_obs
    obs[bad, 0] += 50 * sigma_obs
    sde, par = _sde_at(ID, times, obs, sigma_obs)
    info = sde.engine_.info()
    _show("outlier", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == len(ID)
    out = sde.loo()
    LC.compare(out, loo_ref(sde.problem_, par), [0, 40, 80, 120])
    fwd = sde.residuals()
    assert out["stats"][1, 3] == bad                                  # the track's largest q_j sits on the planted row
    assert np.linalg.norm(out["resid"][bad]) > np.linalg.norm(fwd[bad]) > 5.0      # both sides of the track predict the fix
    found = sde.outliers(level=0.999)
    assert bad in found["rows"] and found["counts"][1] >= 1 and np.all(found["q"] > found["threshold"])


def test_sde_loo_elpd_is_the_sum_of_lpd():
    from smoothsde_amd.synth import simulate
    ID, times, obs = simulate("CTCRW", 5, 40, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=14)
    obs[[5, 79]] = np.nan
    sde, par = _sde_at(ID, times, obs, 0.1)
    info = sde.engine_.info()
    _show("elpd", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == len(ID)
    out = sde.loo(thresholds=[2.0, 6.0])
    ref = loo_ref(sde.problem_, par, [2.0, 6.0])
    assert np.min(np.abs(ref["q"][ref["white"]][:, None] - np.array([2.0, 6.0]))) > 1e-7    # no count hangs on rounding
    LC.compare(out, ref, list(sde.problem_.seg_start) + [sde.problem_.n])
    ok = np.isfinite(out["lpd"])
    assert ok.sum() == 5 * 39 - 2
    assert abs(out["elpd"] - out["lpd"][ok].sum()) <= LC.LPD_TOL * ok.sum() * (1.0 + np.max(np.abs(out["lpd"][ok])))
    assert out["elpd"] == out["stats"][:, 1].sum()


@pytest.mark.parametrize("layout", ["const", "tv"])
def test_a_loo_call_leaves_every_other_result_as_it_was(layout, monkeypatch):
    if layout == "tv":
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = make_spec("gloo_iso_tv", "CTCRW", 2, seed=29, lengths=[120, 20, 35, 1, 14], variant="tv", na_rows=(7, 119))
    else:
        spec = make_spec("gloo_iso", "CTCRW", 2, seed=31, lengths=[20, 35, 1, 14, 2, 27, 9] * 10, irregular=False, na_rows=(2, 19))
    pb = problem_from_spec(spec)
    par = np.array(spec["par"], dtype=np.float64)
    par_b = par.copy(); par_b[1] += 0.01
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"non-interference {layout}", info)
    if layout == "tv":
        assert info["path"] == PATH_TV and info["const_coeff"] == 0
    else:
        assert info["path"] == PATH_ISO and info["n_rows_tiled"] == pb.n
    va, ga = eng.eval(par, order=1)
    sm = eng.smooth(par)
    dr = eng.smooth_draws(par, 3, seed=11)
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.smooth_loo(par, thresholds=[1.0, 4.0])
    after = eng.info()
    assert after["n_evals"] == before["n_evals"] and after["n_memo_hits"] == before["n_memo_hits"]
    vb2, gb2 = eng.eval(par_b, order=1)                                            # still the memo's: a hit
    assert eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1 and vb2 == vb and np.array_equal(gb2, gb)
    va2, ga2 = eng.eval(par, order=1)                                              # evaluated afresh
    assert eng.info()["n_evals"] > before["n_evals"]
    assert va2 == va and np.array_equal(ga2, ga)
    sm2 = eng.smooth(par)
    dr2 = eng.smooth_draws(par, 3, seed=11)
    eng.close()
    for k in ("mean", "cov", "resid"):
        assert np.array_equal(sm[k], sm2[k], equal_nan=True), k
    assert np.array_equal(dr, dr2, equal_nan=True)
