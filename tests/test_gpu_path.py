"""GPU suite (-m gpu): ssde_path_stats on every handle layout it serves.

Each comparison case checks the call twice: against the definition (tests/path_ref.py) on the GPU's OWN draws (ssde_smooth_draws on
the same handle, seed and draw0), and against the definition on the numpy reference draws (tests/draws_ref.py).  Limit
1e-9 (1 + max|ref|) per statistic with identical NaN patterns -- the limit §3.10 and test_gpu_draws.py put on the draws themselves;
a length is a sum of at most 64 differences of draws.  Every case first asserts that no reference position is within 1e-5 of a
region edge (path_cases.py), runs a few thousand rows at most and five draws (one full chunk of DRAW_CH = 4 and one partly filled)
and asserts the layout it ran on (info()).  Shapes as test_gpu_draws.py."""
import ctypes as C

import numpy as np
import pytest

from cases import _tracks, eseal_spec, make_spec, problem_from_spec
from draws_ref import draws_ref
from path_cases import clear_of_edges, compare, dt_weights, make_regions
from path_ref import path_ref
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS70 = [20, 35, 1, 14, 2, 27, 9] * 10
N70 = sum(LENGTHS70)
ERR_ARG, ERR_MODEL = 1, 2
_REF = {}


def _ref(key, pb, par, **kw):
    """the reference draws of a case, computed once and left unchanged"""
    if key not in _REF:
        with np.errstate(invalid="ignore"):
            _REF[key] = draws_ref(pb, par, **kw)
        _REF[key].setflags(write=False)
    return _REF[key]


def _show(tag, info, **more):
    keys = ("path", "kernel_id", "const_coeff", "uniform_dt", "n_rows", "n_rows_tiled", "n_groups", "n_devices", "n_tracks", "sdim")
    print("LAYOUT", tag, {k: info[k] for k in keys}, more)


def _const_spec(model, d, what, seed=3, lengths=LENGTHS70):
    na = (5, 19, 40, 41, sum(lengths) - 1) if what == "missing" else ()
    return make_spec(f"gp_{model}_{d}_{what}_{len(lengths)}", model, d, seed=seed + d, lengths=lengths, irregular=(what == "irregular"), na_rows=na)


def _check(eng, pb, par, ref_draws, obs, tag, n_draws=5, seed=11, draw0=0, n_regions=8):
    """path_stats against the definition on the handle's own draws and on the reference draws (the caller's rows of both)"""
    model, d = pb.model, pb.n_dim
    reg = make_regions(obs, d, n_regions)
    assert clear_of_edges(ref_draws, model, d, reg), tag                           # a condition on the inputs
    w = dt_weights(pb.seg_start, pb.times)
    got = eng.path_stats(par, n_draws, seed=seed, draw0=draw0, regions=reg if n_regions else None, weight=w)
    assert got.shape == (n_draws, pb.n_seg, 2 + n_regions)
    own = eng.smooth_draws(par, n_draws, seed=seed, draw0=draw0)
    compare(got, path_ref(own, pb.seg_start, model, d, regions=reg, weight=w), f"{tag} | own draws")
    compare(got, path_ref(ref_draws, pb.seg_start, model, d, regions=reg, weight=w), f"{tag} | reference")
    return got


# ---- path 1: constant coefficients ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("what", ["regular", "irregular", "missing"])
def test_constant_coefficients(model, d, what):
    spec = _const_spec(model, d, what)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"const {model} d={d} {what}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_groups"] == 2
    assert info["n_tracks"] == 70
    got = _check(eng, pb, spec["par"], _ref(("const", model, d, what), pb, spec["par"], seed=11, n_draws=5), spec["obs"],
                 f"const {model} d={d} {what}")
    eng.close()
    one_row = np.array(LENGTHS70) == 1
    assert np.all(np.isnan(got[:, one_row, :])) and np.all(np.isfinite(got[:, ~one_row, :]))
    assert np.all(got[:, np.array(LENGTHS70) == 2, :2] == 0.0)                     # one state row: no length, no displacement
    inside = got[:, ~one_row, 2:]
    assert np.any(inside > 0) and np.any(inside == 0)


@pytest.mark.parametrize("n_tracks", [65, 130])
def test_65_and_130_tracks(n_tracks):
    lengths = (LENGTHS70 * 2)[:n_tracks]
    spec = _const_spec("CTCRW", 2, "missing", seed=4, lengths=lengths)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"{n_tracks} tracks", info)
    assert info["path"] == PATH_ISO and info["n_tracks"] == n_tracks and info["n_groups"] == (n_tracks + 63) // 64
    _check(eng, pb, spec["par"], _ref(("tracks", n_tracks), pb, spec["par"], seed=11, n_draws=5), spec["obs"], f"{n_tracks} tracks")
    eng.close()


@pytest.mark.parametrize("n_draws", [1, 4, 5])
@pytest.mark.parametrize("n_regions", [0, 1, 8])
def test_draw_and_region_counts(n_draws, n_regions):
    spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    assert info["path"] == PATH_ISO and info["n_groups"] == 2 and info["n_tracks"] == 70
    ref = _ref(("const", "CTCRW", 2, "missing"), pb, spec["par"], seed=11, n_draws=5)[:n_draws]
    _check(eng, pb, spec["par"], ref, spec["obs"], f"{n_draws} draws {n_regions} regions", n_draws=n_draws, n_regions=n_regions)
    eng.close()


# ---- a lattice handle -----------------------------------------------------------------------------------------------------------
def _lattice(model):
    from test_gpu_draws import _written_out
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks(model, 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=9, na_frac=0.05)
    pb = capi.Problem(model, ID, times, obs)
    par = _par(model, 2, np.random.default_rng(2))
    ID2, t2, obs2, rows = _written_out(ID, times, obs, 0.5)
    pb2 = capi.Problem(model, ID2, t2, obs2)
    return pb, par, obs, pb2, rows


@pytest.mark.parametrize("model", MODELS)
def test_a_lattice_handle_skips_its_padded_rows(model):
    pb, par, obs, pb2, rows = _lattice(model)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"lattice {model}", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] > pb.n
    assert pb2.n == info["n_rows_tiled"] and pb2.n_seg == pb.n_seg                 # the written-out rows ARE the handle's lattice
    ref = _ref(("lattice", model), pb2, par, seed=11, n_draws=5)[:, rows, :]
    got = _check(eng, pb, par, ref, obs, f"lattice {model}")                       # weights indexed by the caller's rows
    eng.close()
    # the padded rows, had they counted, would have lengthened the paths
    full = path_ref(_ref(("lattice", model), pb2, par, seed=11, n_draws=5), pb2.seg_start, model, 2)
    assert np.nanmax(full[:, :, 0] - got[:, :, 0]) > 1e-6


# ---- path 2, per-row H, a general P0 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_force_dense(model):
    spec = _const_spec(model, 2, "missing")
    pb = problem_from_spec(spec, flags=capi.FLAG_FORCE_DENSE)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"dense {model}", info)
    assert info["path"] == PATH_DENSE and info["n_groups"] == 2
    _check(eng, pb, spec["par"], _ref(("const", model, 2, "missing"), pb, spec["par"], seed=11, n_draws=5), spec["obs"], f"dense {model}")
    eng.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    spec = make_spec(f"gp_hp_{model}_{d}", model, d, seed=21, lengths=LENGTHS70, with_H=True, with_P0=True, na_rows=(3, 19, 40, 41))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"H P0 {model} d={d}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_tracks"] == 70
    _check(eng, pb, spec["par"], _ref(("hp", model, d), pb, spec["par"], seed=11, n_draws=5), spec["obs"], f"H P0 {model} d={d}")
    eng.close()


# ---- path 3: row-varying coefficients, 150 tracks ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_tv_route_with_150_tracks(model, monkeypatch):
    from test_gpu_smooth_layouts import _tv_many
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = _tv_many(model, seed=29)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"tv {model}", info)
    assert info["path"] == PATH_TV and info["n_tracks"] == 150 and info["const_coeff"] == 0
    got = _check(eng, pb, spec["par"], _ref(("tv", model), pb, spec["par"], seed=11, n_draws=5), spec["obs"], f"tv {model}")
    # three groups of lanes by length: 1 MiB of records makes each group of the CTCRW its own chunk (test_gpu_smooth_layouts.py)
    reg, w = make_regions(spec["obs"], 2, 8), dt_weights(pb.seg_start, pb.times)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.path_stats(spec["par"], 5, seed=11, regions=reg, weight=w)
    eng.close()
    assert np.array_equal(got, many, equal_nan=True)


# ---- the det F <= 0 corner ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_negative_p0_follows_the_reference(model):
    from smoothsde_amd.synth import simulate
    ID, times, obs = simulate(model, 70, 12, 1, seed=4)
    keep = np.ones(len(ID), dtype=bool)
    keep[2 * 12 + 1:3 * 12] = False; keep[4 * 12 + 2:5 * 12] = False
    ID, times, obs = ID[keep], times[keep], obs[keep]
    obs[11] = np.nan
    sdim = 2 if model == "CTCRW" else 1
    P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
    par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
    pb = capi.Problem(model, ID, times, obs, P0=P0)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"negative P0 {model}", info)
    assert info["path"] == PATH_ISO
    got = _check(eng, pb, par, _ref(("negp0", model), pb, par, seed=11, n_draws=5), obs, f"negative P0 {model}")
    eng.close()
    nan = np.isnan(got)
    assert np.array_equal(nan.any(axis=2), nan.all(axis=2))                        # all of a (track, draw) or nothing


# ---- invariance, all bitwise ------------------------------------------------------------------------------------------------------
def test_budget_chunks_on_six_ragged_groups_are_bitwise():
    # the batch of test_gpu_draws.py::test_budget_chunks_on_six_ragged_groups_and_draw_batches_are_bitwise: 1 MiB = 131072 doubles
    # cuts the records into three chunks, produced again for every batch of draws
    rng = np.random.default_rng(31)
    lengths = np.r_[rng.integers(71, 90, 64), rng.integers(45, 61, 63), [60], rng.integers(10, 16, 64), rng.integers(3, 8, 64),
                    rng.integers(2, 4, 64), [1, 2, 5, 1, 3]]
    lengths = [int(v) for v in rng.permutation(lengths)]
    starts = np.r_[0, np.cumsum(lengths)]
    k5 = next(k for k, L in enumerate(lengths) if L >= 5)
    spec = make_spec("gp_chunks", "CTCRW", 2, seed=31, lengths=lengths, irregular=True,
                     na_rows=(int(starts[k5]) + 2, int(starts[k5]) + 3, int(starts[k5 + 1]) - 1))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show("chunks ragged", info)
    assert info["path"] == PATH_ISO and info["n_groups"] == 6
    one = _check(eng, pb, spec["par"], _ref("chunks", pb, spec["par"], seed=11, n_draws=5), spec["obs"], "chunks ragged")
    reg, w = make_regions(spec["obs"], 2, 8), dt_weights(pb.seg_start, pb.times)
    # 325 tracks x 10 statistics: 1 MiB holds 40 draws, so 44 draws go in two batches (40 + 4), each over the three chunks
    assert pb.n_seg == 325
    wide = eng.path_stats(spec["par"], 44, seed=11, regions=reg, weight=w)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.path_stats(spec["par"], 5, seed=11, regions=reg, weight=w)
    wide_many = eng.path_stats(spec["par"], 44, seed=11, regions=reg, weight=w)
    eng.close()
    assert np.array_equal(one, many, equal_nan=True) and np.array_equal(wide, wide_many, equal_nan=True)
    assert np.array_equal(wide[:5], one, equal_nan=True)


@pytest.mark.parametrize("model", MODELS)
def test_draw_numbering_weights_and_region_order_are_bitwise(model):
    spec = _const_spec(model, 2, "missing")
    pb = problem_from_spec(spec)
    reg, w = make_regions(spec["obs"], 2, 8), dt_weights(pb.seg_start, pb.times)
    eng = capi.Engine(pb)
    whole = eng.path_stats(spec["par"], 8, seed=5, regions=reg, weight=w)
    a = eng.path_stats(spec["par"], 4, seed=5, draw0=0, regions=reg, weight=w)
    b = eng.path_stats(spec["par"], 4, seed=5, draw0=4, regions=reg, weight=w)
    assert np.array_equal(whole, np.concatenate([a, b]), equal_nan=True)           # [0, 8) = [0, 4) + [4, 8)
    assert np.array_equal(whole, eng.path_stats(spec["par"], 8, seed=5, regions=reg, weight=w), equal_nan=True)   # two identical calls
    none = eng.path_stats(spec["par"], 5, seed=5, regions=reg)
    ones = eng.path_stats(spec["par"], 5, seed=5, regions=reg, weight=np.ones(pb.n))
    assert np.array_equal(none, ones, equal_nan=True) and not np.array_equal(none, whole[:5], equal_nan=True)
    perm = np.random.default_rng(5).permutation(8)
    mixed = eng.path_stats(spec["par"], 8, seed=5, regions=reg[perm], weight=w)
    assert np.array_equal(mixed[:, :, :2], whole[:, :, :2], equal_nan=True)
    assert np.array_equal(mixed[:, :, 2:], whole[:, :, 2:][:, :, perm], equal_nan=True)
    other = eng.path_stats(spec["par"], 1, seed=6, regions=reg, weight=w)
    eng.close()
    assert not np.array_equal(other[0], whole[0], equal_nan=True)


@pytest.mark.parametrize("layout", ["const", "tv", "lattice"])
def test_two_shards_are_bitwise_the_single_device_handle(layout, monkeypatch):
    if layout == "tv":
        from test_gpu_smooth_layouts import _tv_many
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = _tv_many("OU_SSM", seed=37)
        pb, par, obs = problem_from_spec(spec), spec["par"], spec["obs"]
    elif layout == "lattice":
        pb, par, obs, _, _ = _lattice("CTCRW")
    else:
        spec = _const_spec("CTCRW", 2, "missing")
        pb, par, obs = problem_from_spec(spec), spec["par"], spec["obs"]
    reg, w = make_regions(obs, 2, 8), dt_weights(pb.seg_start, pb.times)
    e1 = capi.Engine(pb)
    info1 = e1.info()
    one = e1.path_stats(par, 5, seed=11, regions=reg, weight=w)
    e1.close()
    e2 = capi.Engine(pb, devices=[0, 0])
    info2 = e2.info()
    _show(f"shards {layout}", info2)
    two = e2.path_stats(par, 5, seed=11, regions=reg, weight=w)
    e2.close()
    assert info2["n_devices"] == 2 and info1["n_devices"] <= 1 and info2["n_tracks"] == info1["n_tracks"] == pb.n_seg
    if layout == "lattice":
        assert info1["n_rows_tiled"] > pb.n and info2["n_rows_tiled"] > pb.n
    if layout == "tv":
        assert info1["path"] == PATH_TV and info2["path"] == PATH_TV
    assert np.any(np.isfinite(one)) and np.array_equal(one, two, equal_nan=True)


# ---- isolation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["const", "tv"])
def test_a_path_stats_call_leaves_every_other_result_as_it_was(layout, monkeypatch):
    if layout == "tv":
        from test_gpu_smooth_layouts import _tv_many
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = _tv_many("CTCRW", seed=29)
    else:
        spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    par = np.array(spec["par"], dtype=np.float64)
    par_b = par.copy(); par_b[1] += 0.01
    reg, w = make_regions(spec["obs"], 2, 8), dt_weights(pb.seg_start, pb.times)
    rows, offs = np.array([1, 7, 30, 31, pb.n - 1]), np.array([0.0, 0.1, 0.2, 0.05, 1.5])
    eng = capi.Engine(pb)
    va, ga = eng.eval(par, order=1)
    sm = eng.smooth(par)
    dr = eng.smooth_draws(par, 5, seed=11)
    pr = eng.predict(par, rows, offs)
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.path_stats(par, 5, seed=11, regions=reg, weight=w)
    after = eng.info()
    assert after["n_evals"] == before["n_evals"] and after["n_memo_hits"] == before["n_memo_hits"]
    vb2, gb2 = eng.eval(par_b, order=1)                                            # still the memo's: a hit
    assert eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1 and vb2 == vb and np.array_equal(gb2, gb)
    va2, ga2 = eng.eval(par, order=1)                                              # evaluated afresh
    assert eng.info()["n_evals"] > before["n_evals"] and eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1
    assert va2 == va and np.array_equal(ga2, ga)
    sm2 = eng.smooth(par)
    dr2 = eng.smooth_draws(par, 5, seed=11)
    pr2 = eng.predict(par, rows, offs)
    eng.close()
    for k in ("mean", "cov", "resid"):
        assert np.array_equal(sm[k], sm2[k], equal_nan=True), k
    assert np.array_equal(dr, dr2, equal_nan=True)
    for k in ("mean", "cov"):
        assert np.array_equal(pr[k], pr2[k], equal_nan=True), k


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_unserved_models_and_bad_arguments():
    for sp in (make_spec("gp_ou", "OU", 1, seed=201, lengths=[9, 2, 14]), eseal_spec("gp_eseal", 211, [14, 9, 11]),
               make_spec("gp_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70[:14], na_rows=(2, 19)),
               make_spec("gp_coupled3", "CTCRW", 3, seed=33, lengths=LENGTHS70[:14], with_H=True, na_rows=(2, 19))):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.path_stats(sp["par"], 5)
        eng.close()
        assert ei.value.status == ERR_MODEL, sp["name"]
    spec = _const_spec("CTCRW", 2, "regular")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    box = [0.0, 1.0, 0.0, 1.0]
    for kw in (dict(n_draws=0), dict(n_draws=1, draw0=-1), dict(n_draws=2, draw0=(1 << 28) - 2),
               dict(n_draws=1, regions=[box] * 9), dict(n_draws=1, regions=[[0.0, np.nan, 0.0, 1.0]]),
               dict(n_draws=1, regions=[[0.0, 1.0, np.nan, 1.0]]), dict(n_draws=1, regions=[box, [2.0, 1.0, 0.0, 1.0]]),
               dict(n_draws=1, regions=[[0.0, 1.0, np.inf, -np.inf]])):
        with pytest.raises(capi.EngineError) as ei:
            eng.path_stats(spec["par"], **kw)
        assert ei.value.status == ERR_ARG, kw
    # what the Python layer cannot send: NULL pointers, a negative region count, regions without a table, a flag
    dp = C.POINTER(C.c_double)
    par = np.ascontiguousarray(spec["par"], dtype=np.float64)
    out = np.zeros((1, 3, pb.n_seg))
    reg = np.array(box)
    P, O, R = par.ctypes.data_as(dp), out.ctypes.data_as(dp), reg.ctypes.data_as(dp)
    call = lambda p, regions, n_regions, stats, flags: eng.lib.ssde_path_stats(eng._h, p, eng.n_par_full, 0, 0, 1, regions, n_regions, None, stats, flags)
    assert call(None, R, 1, O, 0) == ERR_ARG and call(P, R, 1, None, 0) == ERR_ARG
    assert call(P, None, 1, O, 0) == ERR_ARG and call(P, R, -1, O, 0) == ERR_ARG and call(P, R, 1, O, 1) == ERR_ARG
    assert call(P, R, 1, O, 0) == 0 and np.isfinite(out[0, :, 0]).all()
    last = eng.path_stats(spec["par"], 1, draw0=(1 << 28) - 2, regions=[[-np.inf, np.inf, -np.inf, np.inf], [0.5, 0.5, 0.0, 1.0]])
    eng.close()
    # the last draw number there is; the whole plane holds every state row, an empty box (lo == hi) none
    state_rows = np.array(LENGTHS70) - 1.0
    assert np.array_equal(last[0, :, 2], np.where(state_rows > 0, state_rows, np.nan), equal_nan=True)
    assert np.array_equal(last[0, :, 3], np.where(state_rows > 0, 0.0, np.nan), equal_nan=True)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_sde_path_summary_on_a_ctcrw_with_tau_smooth_in_x():
    from smoothsde_amd.sde import SDE
    rng = np.random.default_rng(61)
    ID, times, obs = _tracks(rng, "CTCRW", 2, LENGTHS70, irregular=True)
    n = len(ID)
    obs[[5, 19]] = np.nan
    data = {"ID": ID, "time": times, "x": np.clip((np.sin(np.linspace(0, 7, n)) + 1) / 2, 0, 1), "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~x", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.05, -0.05, 0.3, 0.4, 0.1])
    sde.setup()
    reg = make_regions(obs, 2, 4)
    got = sde.path_summary(3, seed=2, regions=reg)
    par = sde._current_par_full()
    w = dt_weights(sde.problem_.seg_start, times)
    direct = sde.engine_.path_stats(par, 3, seed=2, regions=reg, weight=w)
    info = sde.engine_.info()
    _show("SDE tau ~ x", info)
    assert info["const_coeff"] == 0 and info["path"] == PATH_TV
    assert got["length"].shape == (3, 70) and got["in_region"].shape == (3, 70, 4)
    assert np.array_equal(got["length"], direct[:, :, 0], equal_nan=True) and np.array_equal(got["displacement"], direct[:, :, 1], equal_nan=True)
    assert np.array_equal(got["in_region"], direct[:, :, 2:], equal_nan=True)
    ref = draws_ref(sde.problem_, par, seed=2, n_draws=3)
    assert clear_of_edges(ref, "CTCRW", 2, reg)
    compare(direct, path_ref(ref, sde.problem_.seg_start, "CTCRW", 2, regions=reg, weight=w), "SDE tau ~ x")
    rows = sde.path_summary(3, seed=2, regions=reg, weight=None)["in_region"]
    assert np.array_equal(rows, sde.engine_.path_stats(par, 3, seed=2, regions=reg)[:, :, 2:], equal_nan=True)
    with pytest.raises(NotImplementedError):
        SDE(data={"ID": np.zeros(10), "time": np.arange(10.0), "z": np.exp(rng.standard_normal(10))}, type="CIR", response="z").path_summary(2)
