"""GPU suite (-m gpu): ssde_predict, the smoothed state at any time from the smoother's records, on every handle
layout it serves, against the numpy reference of tests/predict_ref.py (itself, and the host twin of the lane math, checked against
the joint Gaussian of the augmented problem on the CPU: test_predict_host.py, test_predict_hostsim.py).

Every case asserts the layout it ran on (info(): path, kernel_id after an evaluation, tiled rows) and goes through
predict_cases.compare: mean 1e-10 (1 + max|ref|), covariance 1e-9 max|ref|, NaN patterns identical.  Shapes: 65 / 70 / 130 / 150
tracks (two or three groups of lanes, the last partly filled), track lengths 1, 2, 3, 9 among them, a few thousand rows at most
(the reference loops over rows)."""
import ctypes as C

import numpy as np
import pytest

from cases import eseal_spec, make_spec, problem_from_spec
from predict_cases import compare, expected_nan, intervals, query_set
from predict_ref import predict_ref
from smoothsde_amd import capi
from smoothsde_amd.synth import simulate

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
ERR_ARG, ERR_MODEL = 1, 2
MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS70 = [20, 35, 1, 14, 2, 27, 9] * 10           # 70 tracks: a full group and a partly filled one
LENGTHS65 = [9, 3, 1, 2, 12] * 13                    # 65 tracks: one lane in the second group
N70 = sum(LENGTHS70)


def _show(tag, info, **more):
    keys = ("path", "kernel_id", "const_coeff", "uniform_dt", "n_rows", "n_rows_tiled", "n_groups", "n_devices", "n_tracks", "sdim")
    print("LAYOUT", tag, {k: info[k] for k in keys}, more)


def _same(a, b):
    assert np.array_equal(a["mean"], b["mean"], equal_nan=True)
    if a["cov"] is not None or b["cov"] is not None:
        assert np.array_equal(a["cov"], b["cov"], equal_nan=True)


def _run(pb, par, rows, offs, **kw):
    eng = capi.Engine(pb, **kw)
    try:
        return eng.predict(par, rows, offs), eng.info(), eng
    except Exception:
        eng.close()
        raise


def _const_spec(model, d, what, lengths=LENGTHS70, seed=3):
    n = sum(lengths)
    na = (5, 19, 40, 41, n - 1) if what == "missing" else ()
    return make_spec(f"gp_{model}_{d}_{what}", model, d, seed=seed + d, lengths=lengths, irregular=(what == "irregular"), na_rows=na)


# ---- path 1: constant coefficients ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("what", ["irregular", "missing"])
def test_constant_coefficients(model, d, what):
    spec = _const_spec(model, d, what)
    pb = problem_from_spec(spec)
    rows, offs = query_set(pb, seed=d, per_row=False)
    got, info, eng = _run(pb, spec["par"], rows, offs)
    eng.close()
    _show(f"const {model} d={d} {what}", info, n_query=len(rows))
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_groups"] == 2
    compare(got, predict_ref(pb, spec["par"], rows, offs), f"GPU vs predict_ref: const {model} d={d} {what}")
    assert np.array_equal(np.isnan(got["mean"][:, 0]), expected_nan(pb, rows, offs))


@pytest.mark.parametrize("model", MODELS)
def test_regular_complete_tracks_keep_the_shared_covariance_kernel(model):
    # 130 complete tracks on a regular grid: the evaluation runs iso_shared_kernel (kernel_id 3) before and after the predict call
    ID, times, obs = simulate(model, 130, 40, 2, seed=12)
    pb = capi.Problem(model, ID, times, obs)
    q = capi.n_sde_par(model, 2)
    par = np.r_[-1.0, 0.05, -0.05, 0.4, 0.1][:1 + q]
    rows, offs = query_set(pb, seed=2, per_row=False)
    eng = capi.Engine(pb)
    v0, g0 = eng.eval(par)
    assert eng.info()["kernel_id"] == 3
    got = eng.predict(par, rows, offs)
    info = eng.info()
    eng.forget()
    v1, g1 = eng.eval(par)
    assert eng.info()["kernel_id"] == 3 and v1 == v0 and np.array_equal(g1, g0)
    eng.close()
    _show(f"shared {model}", info, n_query=len(rows))
    assert info["path"] == PATH_ISO and info["kernel_id"] == 3 and info["uniform_dt"] == 1 and info["n_groups"] == 3
    compare(got, predict_ref(pb, par, rows, offs), f"GPU vs predict_ref: shared {model}")


# ---- shapes: group boundaries, short tracks, query counts -----------------------------------------------------------------------
@pytest.mark.parametrize("n_query", [1, 63, 64, 65, 257])
def test_query_counts_on_65_tracks_with_short_tracks(n_query):
    spec = _const_spec("CTCRW", 2, "irregular", lengths=LENGTHS65, seed=7)
    pb = problem_from_spec(spec)
    rows, offs = query_set(pb, seed=11)
    assert len(rows) >= 257
    # the last queries of the shuffled set; n_query = 1 asks for one interior state only (every other track has no query)
    rows, offs = rows[-n_query:], offs[-n_query:]
    got, info, eng = _run(pb, spec["par"], rows, offs)
    eng.close()
    _show(f"65 tracks n_query={n_query}", info)
    assert info["path"] == PATH_ISO and info["n_groups"] == 2 and info["n_tracks"] == 65
    compare(got, predict_ref(pb, spec["par"], rows, offs), f"GPU vs predict_ref: n_query={n_query}")


def test_sorted_unsorted_duplicated_and_crowded_queries():
    spec = _const_spec("OU_SSM", 2, "irregular", lengths=LENGTHS65, seed=9)
    pb = problem_from_spec(spec)
    first, last, dt = intervals(pb)
    rows, offs = query_set(pb, seed=13, shuffle=False)
    j = int(np.flatnonzero(~first & ~last)[40])
    crowd = np.linspace(0.0, dt[j], 20)                                  # 20 queries in one interval, its two ends among them
    track3 = (rows >= pb.seg_start[3]) & (rows < pb.seg_start[4])         # ... and a track with no query at all
    rows = np.r_[rows[~track3], np.full(20, j), rows[:30]]                # the first 30 once more
    offs = np.r_[offs[~track3], crowd, offs[:30]]
    eng = capi.Engine(pb)
    srt = eng.predict(spec["par"], rows, offs)
    p = np.random.default_rng(5).permutation(len(rows))
    mixed = eng.predict(spec["par"], rows[p], offs[p])
    info = eng.info()
    eng.close()
    _show("sorted / unsorted", info, n_query=len(rows))
    assert info["path"] == PATH_ISO and info["n_groups"] == 2
    assert np.array_equal(mixed["mean"], srt["mean"][p], equal_nan=True) and np.array_equal(mixed["cov"], srt["cov"][p], equal_nan=True)
    assert np.array_equal(srt["mean"][-30:], srt["mean"][:30], equal_nan=True)
    compare(srt, predict_ref(pb, spec["par"], rows, offs), "GPU vs predict_ref: crowded")


# ---- a lattice handle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_a_lattice_handle_answers_inside_the_absent_fix_gaps(model):
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks(model, 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
    obs[39 if ID[39] == ID[38] else 38] = np.nan
    pb = capi.Problem(model, ID, times, obs)
    par = _par(model, 2, np.random.default_rng(2))
    first, last, dt = intervals(pb)
    rows, offs = query_set(pb, seed=17, per_row=False)
    gaps = np.flatnonzero(~first & ~last & (dt > 0.75))                   # intervals of two to four lattice steps
    assert len(gaps) >= 20
    # in every such gap: on a lattice point, just before and after one, in the last step, at the gap's end
    rows = np.r_[rows, np.repeat(gaps, 5)]
    offs = np.r_[offs, (np.array([0.5, 0.49, 0.61, 0.0, 1.0])[None, :] * np.c_[np.ones((len(gaps), 3)), dt[gaps] - 0.2, dt[gaps]]).ravel()]
    got, info, eng = _run(pb, par, rows, offs)
    eng.close()
    _show(f"lattice {model}", info, n_query=len(rows))
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] > pb.n
    compare(got, predict_ref(pb, par, rows, offs), f"GPU vs predict_ref: lattice {model}")
    assert np.array_equal(np.isnan(got["mean"][:, 0]), expected_nan(pb, rows, offs))


# ---- the full-covariance lanes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_force_dense(model):
    spec = _const_spec(model, 2, "missing")
    pb = problem_from_spec(spec, flags=capi.FLAG_FORCE_DENSE)
    rows, offs = query_set(pb, seed=19, per_row=False)
    got, info, eng = _run(pb, spec["par"], rows, offs)
    eng.close()
    _show(f"dense {model}", info)
    assert info["path"] == PATH_DENSE and info["n_rows_tiled"] == pb.n
    compare(got, predict_ref(pb, spec["par"], rows, offs), f"GPU vs predict_ref: dense {model}")


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    spec = make_spec(f"gp_hp_{model}_{d}", model, d, seed=41 + d, lengths=LENGTHS70, with_H=True, with_P0=True, na_rows=(5, 19, N70 - 1))
    pb = problem_from_spec(spec)
    rows, offs = query_set(pb, seed=23, per_row=False)
    got, info, eng = _run(pb, spec["par"], rows, offs)
    eng.close()
    _show(f"H P0 {model} d={d}", info)
    # with H_array a batch of eight tracks or more sits on the tiles of the full-covariance lane = track kernels (reported as path 1);
    # the records and side rows come from dense_kernel on those tiles, per-row H and the general P0 included
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_tracks"] == 70
    compare(got, predict_ref(pb, spec["par"], rows, offs), f"GPU vs predict_ref: H P0 {model} d={d}")


# ---- row-varying parameters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,d", [("CTCRW", 2), ("OU_SSM", 1), ("BM_SSM", 2)])
def test_drift_columns_in_the_tiles(model, d, monkeypatch):
    from test_gpu_smooth_layouts import _drift_problem
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "32")
    pb, par, ncols = _drift_problem(model, d, "missing", seed=60 + d, smooth_dims=(0, 1)[:d])
    rows, offs = query_set(pb, seed=29, per_row=False)
    eng = capi.Engine(pb)
    eng.eval(par)
    got = eng.predict(par, rows, offs)
    info = eng.info()
    eng.close()
    _show(f"drift {model} d={d}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 0 and info["kernel_id"] == 10 and info["n_rows_tiled"] == pb.n
    compare(got, predict_ref(pb, par, rows, offs), f"GPU vs predict_ref: drift {model} d={d}")


@pytest.mark.parametrize("model", MODELS)
def test_row_varying_tau_nu_on_the_register_lanes(model, monkeypatch):
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "32")
    spec = make_spec(f"gp_tv_{model}", model, 2, seed=13, lengths=LENGTHS70, variant="tv", irregular=False, na_rows=(5, 19, 60, N70 - 1))
    pb = problem_from_spec(spec)
    rows, offs = query_set(pb, seed=31, per_row=False)
    eng = capi.Engine(pb)
    eng.eval(spec["par"])
    got = eng.predict(spec["par"], rows, offs)
    info = eng.info()
    eng.close()
    _show(f"colvar {model}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 0 and info["kernel_id"] in (11, 12, 17) and info["n_rows_tiled"] == pb.n
    compare(got, predict_ref(pb, spec["par"], rows, offs), f"GPU vs predict_ref: colvar {model}")


@pytest.mark.parametrize("model,extra", [("CTCRW", "H"), ("OU_SSM", ""), ("BM_SSM", "P0")])
def test_tv_route_with_150_tracks(model, extra, monkeypatch):
    from test_gpu_smooth_layouts import _tv_many
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = _tv_many(model, seed=29, with_H=extra == "H", with_P0=extra == "P0")
    pb = problem_from_spec(spec)
    rows, offs = query_set(pb, seed=37, per_row=False)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"tv many {model} {extra}", info, n_query=len(rows))
    assert info["path"] == PATH_TV and info["n_tracks"] == 150           # three groups of lanes by length; one-row tracks among them
    one = eng.predict(spec["par"], rows, offs)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.predict(spec["par"], rows, offs)
    eng.close()
    _same(one, many)
    compare(one, predict_ref(pb, spec["par"], rows, offs), f"GPU vs predict_ref: tv {model} {extra}")


# ---- column pairs and shards ----------------------------------------------------------------------------------------------------
def test_uncoupled_ctcrw_d4_runs_as_column_pairs():
    spec = make_spec("gp_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70, na_rows=(2, 19))
    pb = problem_from_spec(spec)
    rows, offs = query_set(pb, seed=41, per_row=False)
    got, info, eng = _run(pb, spec["par"], rows, offs)
    eng.close()
    _show("pairs", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == 2 * pb.n and info["sdim"] == 8
    compare(got, predict_ref(pb, spec["par"], rows, offs), "GPU vs predict_ref: pairs")
    pair = np.arange(8) // 4
    ok = ~np.isnan(got["mean"][:, 0])
    assert np.all(got["cov"][ok][:, pair[:, None] != pair[None, :]] == 0.0)          # cross-pair blocks: exactly zero ...
    assert np.all(np.isnan(got["cov"][~ok]))                                         # ... and all NaN where there is no state


@pytest.mark.parametrize("layout", ["const", "pairs", "tv", "lattice"])
def test_two_shards_are_bitwise_the_single_device_handle(layout, monkeypatch):
    if layout == "tv":
        from test_gpu_smooth_layouts import _tv_many
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = _tv_many("OU_SSM", seed=37)
    elif layout == "pairs":
        spec = make_spec("gp_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70, na_rows=(2, 19))
    elif layout == "lattice":
        from test_gpu_lattice import _par, lattice_tracks
        ID, times, obs = lattice_tracks("CTCRW", 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
        spec = dict(model="CTCRW", ID=ID, times=times, obs=obs, par=_par("CTCRW", 2, np.random.default_rng(2)))
    else:
        spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    rows, offs = query_set(pb, seed=43, per_row=False)
    one, info1, e1 = _run(pb, spec["par"], rows, offs)
    e1.close()
    two, info2, e2 = _run(pb, spec["par"], rows, offs, devices=[0, 0])
    e2.close()
    _show(f"shards {layout}", info2)
    assert info2["n_devices"] == 2 and info1["n_devices"] <= 1
    _same(one, two)


# ---- invariance, all bitwise ----------------------------------------------------------------------------------------------------
def test_budget_chunks_calls_and_a_null_covariance_are_bitwise():
    # the batch of test_gpu_smooth_layouts.py::test_chunks_on_ragged_tiled_groups_are_bitwise: six groups, 1 MiB cuts them into chunks
    rng = np.random.default_rng(31)
    lengths = np.r_[rng.integers(71, 90, 64), rng.integers(45, 61, 63), [60], rng.integers(10, 16, 64), rng.integers(3, 8, 64),
                    rng.integers(2, 4, 64), [1, 2, 5, 1, 3]]
    lengths = [int(v) for v in rng.permutation(lengths)]
    starts = np.r_[0, np.cumsum(lengths)]
    k5 = next(k for k, L in enumerate(lengths) if L >= 5)
    spec = make_spec("gp_chunks", "CTCRW", 2, seed=31, lengths=lengths, irregular=True,
                     na_rows=(int(starts[k5]) + 2, int(starts[k5]) + 3, int(starts[k5 + 1]) - 1))
    pb = problem_from_spec(spec)
    rows, offs = query_set(pb, seed=47, per_row=False)
    one, info, eng = _run(pb, spec["par"], rows, offs)
    _show("chunks ragged", info, n_query=len(rows))
    assert info["path"] == PATH_ISO and info["n_groups"] == 6
    h = len(rows) // 3
    a, b = eng.predict(spec["par"], rows[:h], offs[:h]), eng.predict(spec["par"], rows[h:], offs[h:])
    nocov = eng.predict(spec["par"], rows, offs, cov=False)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.predict(spec["par"], rows, offs)
    eng.close()
    _same(one, many)
    _same(one, {"mean": np.concatenate([a["mean"], b["mean"]]), "cov": np.concatenate([a["cov"], b["cov"]])})
    assert nocov["cov"] is None and np.array_equal(nocov["mean"], one["mean"], equal_nan=True)
    compare(one, predict_ref(pb, spec["par"], rows, offs), "GPU vs predict_ref: chunks ragged")


# ---- isolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["const", "tv"])
def test_a_predict_call_leaves_eval_and_smooth_as_they_were(layout, monkeypatch):
    if layout == "tv":
        from test_gpu_smooth_layouts import _tv_many
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = _tv_many("CTCRW", seed=29)
    else:
        spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    rows, offs = query_set(pb, seed=53, per_row=False)
    par = np.array(spec["par"], dtype=np.float64)
    par_b = par.copy(); par_b[1] += 0.01
    eng = capi.Engine(pb)
    va, ga = eng.eval(par, order=1)
    sm = eng.smooth(par)
    dr = eng.smooth_draws(par, 2, seed=3)
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.predict(par, rows, offs)
    after = eng.info()
    assert after["n_evals"] == before["n_evals"] and after["n_memo_hits"] == before["n_memo_hits"]
    vb2, gb2 = eng.eval(par_b, order=1)                                            # still the memo's: a hit
    assert eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1 and vb2 == vb and np.array_equal(gb2, gb)
    va2, ga2 = eng.eval(par, order=1)                                              # evaluated afresh
    assert eng.info()["n_evals"] > before["n_evals"] and eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1
    assert va2 == va and np.array_equal(ga2, ga)
    sm2 = eng.smooth(par)
    dr2 = eng.smooth_draws(par, 2, seed=3)
    eng.close()
    for k in ("mean", "cov", "resid"):
        assert np.array_equal(sm[k], sm2[k], equal_nan=True), k
    assert np.array_equal(dr, dr2, equal_nan=True)


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_unserved_models_and_bad_arguments():
    for sp in (make_spec("gp_ou", "OU", 1, seed=201, lengths=[9, 2, 14]), make_spec("gp_cir", "CIR", 1, seed=221, lengths=[9, 2, 14]),
               eseal_spec("gp_eseal", 211, [14, 9, 11]),
               make_spec("gp_coupled3", "CTCRW", 3, seed=33, lengths=LENGTHS70[:14], with_H=True, na_rows=(2, 19))):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.predict(sp["par"], [3], [0.1])
        eng.close()
        assert ei.value.status == ERR_MODEL, sp["name"]
    spec = _const_spec("CTCRW", 2, "irregular")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    for rows, offs in (([], []), ([-1], [0.0]), ([pb.n], [0.0]), ([3], [-0.1]), ([3], [np.nan]), ([3], [np.inf])):
        with pytest.raises(capi.EngineError) as ei:
            eng.predict(spec["par"], rows, offs)
        assert ei.value.status == ERR_ARG, (rows, offs)
    par = np.ascontiguousarray(spec["par"])
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    r = np.array([3], dtype=np.int64); o = np.array([0.1]); m = np.zeros(4)
    args = [par.ctypes.data_as(dp), pb.n_par_full, r.ctypes.data_as(lp), o.ctypes.data_as(dp), 1, m.ctypes.data_as(dp), None]
    for null in (2, 3, 5):                                                         # q_row, q_off, a_pred
        a = list(args); a[null] = None
        assert eng.lib.ssde_predict(eng._h, *a) == ERR_ARG
    assert eng.lib.ssde_predict(eng._h, *args) == 0 and np.all(np.isfinite(m))
    eng.close()


# ---- the det F <= 0 corner ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dense", [False, True])
def test_negative_p0_follows_the_reference(model, dense):
    ID, times, obs = simulate(model, 70, 12, 1, seed=4)
    keep = np.ones(len(ID), dtype=bool)
    keep[2 * 12 + 1:3 * 12] = False; keep[4 * 12 + 2:5 * 12] = False
    ID, times, obs = ID[keep], times[keep], obs[keep]
    obs[11] = np.nan
    sdim = 2 if model == "CTCRW" else 1
    P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
    par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
    pb = capi.Problem(model, ID, times, obs, P0=P0, flags=capi.FLAG_FORCE_DENSE if dense else 0)
    rows, offs = query_set(pb, seed=59)
    got, info, eng = _run(pb, par, rows, offs)
    eng.close()
    _show(f"detF {model} dense={dense}", info)
    assert info["path"] == (PATH_DENSE if dense else PATH_ISO)
    ref = predict_ref(pb, par, rows, offs)
    if model == "CTCRW":
        assert np.isnan(ref["mean"][:, 0]).sum() > expected_nan(pb, rows, offs).sum()       # the rows that rejected their update
    compare(got, ref, f"GPU vs predict_ref: negative P0 {model} dense={dense}")


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_sde_predict_states_on_a_ctcrw_with_tau_smooth_in_x():
    from cases import _tracks
    from smoothsde_amd.sde import SDE
    rng = np.random.default_rng(61)
    ID, times, obs = _tracks(rng, "CTCRW", 2, LENGTHS70, irregular=True)
    n = len(ID)
    obs[[5, 19]] = np.nan
    data = {"ID": ID, "time": times, "x": np.clip((np.sin(np.linspace(0, 7, n)) + 1) / 2, 0, 1), "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~x", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.05, -0.05, 0.3, 0.4, 0.1])
    sde.setup()
    pb = sde.problem_
    first, last, dt = intervals(pb)
    rows, offs = query_set(pb, seed=67, per_row=False)
    keep = ~expected_nan(pb, rows, offs) & ~(~last[rows] & (offs >= dt[rows]))       # times that name (row, offset) uniquely
    rows, offs = rows[keep], offs[keep]
    qid = np.r_[ID[rows], ID[0], 1e6]
    qt = np.r_[times[rows] + offs, times[0] - 1.0, 5.0]                              # before a track's first row; an unknown ID
    out = sde.predict_states(qid, qt)
    par = sde._current_par_full()
    back = qt[:-2] - times[rows]                                                     # the offsets predict_states forms
    direct = sde.engine_.predict(par, rows, back)
    info = sde.engine_.info()
    _show("SDE tau ~ x", info)
    assert info["path"] == PATH_TV
    assert np.array_equal(out["mean"][:-2], direct["mean"], equal_nan=True) and np.array_equal(out["cov"][:-2], direct["cov"], equal_nan=True)
    assert np.all(np.isnan(out["mean"][-2:])) and np.all(np.isnan(out["cov"][-2:])) and np.all(np.isfinite(out["mean"][:-2]))
    compare({"mean": out["mean"][:-2], "cov": out["cov"][:-2]}, predict_ref(pb, par, rows, back), "GPU vs predict_ref: SDE.predict_states")
    bm = SDE(formulas={"mu": "~1", "sigma": "~1"}, data={"ID": ID, "time": times, "Z": np.cumsum(np.ones(n))}, type="BM", response="Z")
    with pytest.raises(NotImplementedError):
        bm.predict_states(ID[:2], times[:2])
