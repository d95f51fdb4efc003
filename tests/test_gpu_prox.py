"""GPU suite (-m gpu): ssde_path_proximity, the posterior paths of two tracks paired and reduced per pair and draw on the device
(DESIGN.md §3.16), on every handle layout it serves.

The main comparison takes the SAME engine's predict_draws of the A queries followed by the B queries and reduces it with the numpy
reference of tests/prox_ref.py (itself the yardstick of the host twin: test_prox_hostsim.py): the index of the closest point and the
fixed-point sums bitwise, the minimum distance within 1e-12 relative (the device may contract the sum of squares into an fma), NaN
patterns identical -- after prox_ref.undecided (tol 1e-12) is asserted 0 on the reference.  One smaller case goes against
bridge_ref.predict_draws_ref instead, which shares nothing with the engine: minimum within 1e-9 (1 + max), the rest bitwise with
undecided (tol 1e-8) asserted 0.  Shapes as test_gpu_predict_draws.py: 65 / 70 tracks of at most 12 rows (two groups of lanes, the
second partly filled), ND = 5."""
import ctypes as C

import numpy as np
import pytest

import prox_ref
from bridge_ref import predict_draws_ref
from cases import eseal_spec, make_spec, problem_from_spec
from prox_cases import (EDGE_SIZES, RADII, RADII8, STAT_DRAWS, STAT_SEED, concat, points, side_queries, stat_problem, stat_ratio,
                        track_of_row)
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_TV = 1, 3
ERR_ARG, ERR_MODEL = 1, 2
MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS70 = [12, 7, 1, 9, 2, 11, 5] * 10             # 70 tracks: a full group and a partly filled one
LENGTHS65 = [9, 3, 1, 2, 12] * 13                    # 65 tracks: one lane in the second group
ND, SEED, TOL = 5, 11, 1e-12
SIZES = [40, 0, 300, 1, 257, 90]


def _last_error(eng):
    msg = eng.lib.ssde_last_error(eng._h)
    return msg.decode() if msg else ""


def _const_spec(model, d, what, lengths=LENGTHS70, seed=3):
    n = sum(lengths)
    na = (5, 11, 40, 41, n - 1) if what == "missing" else ()           # row 11 ends the first track
    return make_spec(f"gpx_{model}_{d}_{what}", model, d, seed=seed + d, lengths=lengths, irregular=(what != "regular"), na_rows=na)


def _check(eng, pb, par, pts, tag, radii=RADII, weight="random", nd=ND, seed=SEED, draw0=2):
    """path_proximity against prox_ref on the same engine's predict_draws of the concatenated queries"""
    ra, oa, rb, ob, pp = pts
    if isinstance(weight, str):
        weight = np.random.default_rng(len(ra)).uniform(0.0, 2.0, len(ra))
    got = eng.path_proximity(par, ra, oa, rb, ob, pp, nd, seed=seed, draw0=draw0, radii=radii, weight=weight)
    assert got.shape == (nd, len(pp) - 1, 2 + len(radii))
    at = eng.predict_draws(par, *concat(ra, oa, rb, ob), nd, seed=seed, draw0=draw0)
    assert prox_ref.undecided(at, pb.model, pb.n_dim, pp, radii, tol=TOL) == 0, tag
    prox_ref.compare(got, prox_ref.proximity(at, pb.model, pb.n_dim, pp, radii, weight), f"GPU vs prox_ref: {tag}", rel=TOL)
    return got


# ---- constant coefficients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d,what", [(2, "regular"), (2, "irregular"), (2, "missing"), (1, "regular"), (1, "irregular"), (1, "missing")])
def test_constant_coefficients(model, d, what):
    spec = _const_spec(model, d, what)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    got = _check(eng, pb, spec["par"], points(pb, SIZES, seed=d, forecast=0.1), f"const {model} d={d} {what}")
    plan = eng.last_proximity_plan()
    eng.close()
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_groups"] == 2
    assert plan == {"n_tiles": 1 + 2 + 1 + 2 + 1, "tiles_max": 2, "n_batches": 1, "route": 1}
    assert np.all(np.isnan(got[:, 1])) and np.all(np.isfinite(np.delete(got, 1, axis=1)))


def test_a_lattice_handle():
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks("CTCRW", 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = _par("CTCRW", 2, np.random.default_rng(2))
    eng = capi.Engine(pb)
    info = eng.info()
    got = _check(eng, pb, par, points(pb, SIZES, seed=5, forecast=0.1), "lattice")
    eng.close()
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] > pb.n
    assert np.all(np.isfinite(np.delete(got, 1, axis=1)))


def test_a_tv_handle(monkeypatch):
    from test_gpu_smooth_layouts import _tv_many
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = _tv_many("CTCRW", seed=29)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    assert info["path"] == PATH_TV and info["n_tracks"] == 150
    got = _check(eng, pb, spec["par"], points(pb, SIZES, seed=6, forecast=0.1), "tv")
    eng.close()
    assert np.all(np.isfinite(np.delete(got, 1, axis=1)))


@pytest.mark.parametrize("layout", ["const", "tv"])
def test_two_shards_are_route_2_and_bitwise_the_single_device_handle(layout, monkeypatch):
    if layout == "tv":
        from test_gpu_smooth_layouts import _tv_many
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = _tv_many("OU_SSM", seed=37)
    else:
        spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    pts = points(pb, SIZES, seed=7, forecast=0.1)                          # the sides are drawn over every track: pairs straddle shards
    ra, oa, rb, ob, pp = pts
    w = np.random.default_rng(3).uniform(0.0, 2.0, len(ra))
    e1 = capi.Engine(pb)
    one = e1.path_proximity(spec["par"], ra, oa, rb, ob, pp, ND, seed=SEED, radii=RADII, weight=w)
    n1, p1 = e1.info()["n_devices"], e1.last_proximity_plan()
    e1.close()
    e2 = capi.Engine(pb, devices=[0, 0])
    assert e2.last_proximity_plan() == {"n_tiles": 0, "tiles_max": 0, "n_batches": 0, "route": 0}
    two = _check(e2, pb, spec["par"], pts, f"two shards {layout}", weight=w, draw0=0)
    n2, p2 = e2.info()["n_devices"], e2.last_proximity_plan()
    e2.close()
    assert n2 == 2 and n1 <= 1 and p1["route"] == 1 and p2["route"] == 2 and p2["n_tiles"] == p1["n_tiles"]
    half = track_of_row(pb, ra) < pb.n_seg // 2
    assert half.any() and (~half).any()
    assert np.array_equal(one, two, equal_nan=True) and np.isfinite(one).any()


# ---- against a reference that shares nothing with the engine ---------------------------------------------------------------------
def test_a_small_case_against_the_numpy_bridge_reference():
    spec = _const_spec("CTCRW", 2, "missing", seed=7)
    pb = problem_from_spec(spec)
    ra, oa, rb, ob, pp = points(pb, [150, 0, 1, 149], seed=9, forecast=0.1)             # 300 points
    w = np.random.default_rng(4).uniform(0.0, 2.0, 300)
    ref_at = predict_draws_ref(pb, spec["par"], *concat(ra, oa, rb, ob), seed=SEED, draw0=1, n_draws=ND)
    assert prox_ref.undecided(ref_at, "CTCRW", 2, pp, RADII, tol=1e-8) == 0
    eng = capi.Engine(pb)
    got = eng.path_proximity(spec["par"], ra, oa, rb, ob, pp, ND, seed=SEED, draw0=1, radii=RADII, weight=w)
    eng.close()
    prox_ref.compare(got, prox_ref.proximity(ref_at, "CTCRW", 2, pp, RADII, w), "GPU vs prox_ref on predict_draws_ref", rel=1e-9, scale_abs=True)


# ---- edges where the kernels can go wrong ---------------------------------------------------------------------------------------
def _edge_points(pb):
    """pairs of 0, 1, 255, 256, 257 and 600 points; the last one's are distinct offsets inside the intervals of two 12- and 11-row tracks"""
    a = points(pb, EDGE_SIZES[:-1], seed=13, forecast=0.1)
    b = points(pb, EDGE_SIZES[-1:], seed=14, tracks_a=[0], tracks_b=[5])
    return tuple(np.r_[x, y] for x, y in zip(a[:4], b[:4])) + (np.r_[a[4], a[4][-1] + b[4][1:]],)


@pytest.mark.parametrize("n_draws", [1, 4, 5])
def test_pair_sizes_around_a_tile_and_draw_counts_around_a_wave_s_chunk(n_draws):
    spec = _const_spec("CTCRW", 2, "irregular")
    pb = problem_from_spec(spec)
    assert LENGTHS70[0] == 12 and LENGTHS70[5] == 11
    pts = _edge_points(pb)
    assert np.diff(pts[4]).tolist() == EDGE_SIZES and len(np.unique(pts[1][-600:])) == 600
    eng = capi.Engine(pb)
    got = _check(eng, pb, spec["par"], pts, f"edge sizes n_draws={n_draws}", nd=n_draws)
    plan = eng.last_proximity_plan()
    _check(eng, pb, spec["par"], pts, f"edge sizes, 8 radii n_draws={n_draws}", radii=RADII8, nd=n_draws)
    none = _check(eng, pb, spec["par"], pts, f"edge sizes, no radius n_draws={n_draws}", radii=[], nd=n_draws)
    eng.close()
    assert plan == {"n_tiles": 0 + 1 + 1 + 1 + 2 + 3, "tiles_max": 3, "n_batches": 1, "route": 1}
    assert none.shape == (n_draws, 6, 2) and np.array_equal(none, got[:, :, :2], equal_nan=True)
    assert np.all(np.isnan(got[:, 0])) and np.all(np.isfinite(got[:, 1:]))


def test_a_track_with_itself_both_lane_groups_and_a_forecast():
    spec = _const_spec("OU_SSM", 2, "irregular", lengths=LENGTHS65, seed=8)
    pb = problem_from_spec(spec)
    rng = np.random.default_rng(15)
    trk = track_of_row(pb, np.arange(pb.n))
    # pair 0: track 4 with itself, both sides identical; pair 1: track 4 at two different times; pair 2: track 0 (first lane group)
    # with track 64 (the one lane of the second group); pair 3: forecasts only, past the last rows of tracks 0 and 64
    r4, o4 = side_queries(pb, 30, rng, tracks=[4])
    r4b, o4b = side_queries(pb, 30, rng, tracks=[4])
    r0, o0 = side_queries(pb, 30, rng, tracks=[0])
    r64, o64 = side_queries(pb, 30, rng, tracks=[64])
    assert np.all(trk[r64] == 64) and pb.n_seg == 65
    e0, e64 = int(pb.seg_start[1]) - 1, pb.n - 1
    ra = np.r_[r4, r4, r0, np.full(5, e0)]; oa = np.r_[o4, o4, o0, np.linspace(0.0, 4.0, 5)]
    rb = np.r_[r4, r4b, r64, np.full(5, e64)]; ob = np.r_[o4, o4b, o64, np.linspace(0.5, 4.5, 5)]
    pp = np.array([0, 30, 60, 90, 95], dtype=np.int64)
    radii = [0.0, 1.3, np.inf]
    eng = capi.Engine(pb)
    info = eng.info()
    # Identical sides give distance 0 in any arithmetic, every point tied: exact by construction, and exactly what `undecided` counts.
    # So the count is asserted 0 on the other three pairs, and the whole call is then compared as everywhere else.
    par = spec["par"]
    got = eng.path_proximity(par, ra, oa, rb, ob, pp, ND, seed=SEED, draw0=2, radii=radii)
    at = eng.predict_draws(par, *concat(ra, oa, rb, ob), ND, seed=SEED, draw0=2)
    rest = np.concatenate([at[:, 30:95], at[:, 95 + 30:]], axis=1)
    assert prox_ref.undecided(rest, "OU_SSM", 2, pp[1:] - 30, radii, tol=TOL) == 0
    prox_ref.compare(got, prox_ref.proximity(at, "OU_SSM", 2, pp, radii), "GPU vs prox_ref: self, groups, forecast", rel=TOL)
    eng.close()
    assert info["n_groups"] == 2 and info["n_tracks"] == 65 and np.all(np.isfinite(got))
    assert np.all(got[:, 0, 0] == 0.0) and np.all(got[:, 0, 1] == 0.0) and np.all(got[:, 0, 2] == got[:, 0, 4])     # identical sides
    assert np.all(got[:, 1, 0] > 0.0)


# ---- invariances, all bitwise ---------------------------------------------------------------------------------------------------
def test_budget_draw_ranges_repeats_and_unit_weights_are_bitwise():
    spec = _const_spec("CTCRW", 2, "irregular")
    pb = problem_from_spec(spec)
    ra, oa, rb, ob, pp = pts = points(pb, [1500, 0, 1300, 1200], seed=17, forecast=0.05)
    par = spec["par"]
    w = np.random.default_rng(5).uniform(0.0, 3.0, len(ra))
    eng = capi.Engine(pb)

    def call(nd, draw0=0, weight=w):
        return eng.path_proximity(par, ra, oa, rb, ob, pp, nd, seed=SEED, draw0=draw0, radii=RADII, weight=weight)
    one = _check(eng, pb, par, pts, "4000 points", weight=w, draw0=0)
    assert eng.last_proximity_plan()["n_batches"] == 1
    assert np.array_equal(one, call(ND), equal_nan=True)                                   # a repeated call
    assert np.array_equal(one, np.concatenate([call(2, 0), call(3, 2)]), equal_nan=True)   # draws [0, 5) = [0, 2) + [2, 5)
    ones = call(ND, weight=np.ones(len(ra)))
    assert np.array_equal(call(ND, weight=None), ones, equal_nan=True) and not np.array_equal(ones, one, equal_nan=True)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = call(ND)
    plan = eng.last_proximity_plan()
    eng.close()
    assert plan["n_batches"] > 1 and plan["n_tiles"] == 6 + 6 + 5 and plan["tiles_max"] == 6
    assert np.array_equal(one, many, equal_nan=True)


# ---- isolation ------------------------------------------------------------------------------------------------------------------
def test_a_call_leaves_every_other_call_as_it_was():
    spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    ra, oa, rb, ob, pp = points(pb, SIZES, seed=19, forecast=0.1)
    par = np.array(spec["par"], dtype=np.float64)
    par_b = par.copy(); par_b[1] += 0.01
    eng = capi.Engine(pb)

    def others():
        return (eng.smooth_draws(par, 2, seed=3), eng.predict_draws(par, *concat(ra, oa, rb, ob), 2, seed=3), eng.path_stats(par, 4, seed=3))
    va, ga = eng.eval(par, order=1)
    was = others()
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.path_proximity(par, ra, oa, rb, ob, pp, ND, seed=SEED, radii=RADII)
    after = eng.info()
    assert after["n_evals"] == before["n_evals"] and after["n_memo_hits"] == before["n_memo_hits"]
    vb2, gb2 = eng.eval(par_b, order=1)                                            # still the memo's: a hit
    assert eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1 and vb2 == vb and np.array_equal(gb2, gb)
    va2, ga2 = eng.eval(par, order=1)                                              # evaluated afresh
    assert va2 == va and np.array_equal(ga2, ga)
    now = others()
    eng.close()
    for x, y in zip(was, now):
        assert np.array_equal(x, y, equal_nan=True)


# ---- the mean of the squared distance over many draws ----------------------------------------------------------------------------
def test_the_mean_squared_distance_of_512_draws():
    # Two tracks, one common clock time, STAT_DRAWS = 512 draws of seed STAT_SEED = 7.  The tracks are independent given par, so
    # E dist^2 = |m_a - m_b|^2 + tr(V_a + V_b) on the position columns, m and V from ssde_predict.  The bound is 5 standard errors of the
    # Monte Carlo mean, estimated from the draws.  The draws are a fixed function of the seed: the host twin gives the ratio this
    # seed has (test_prox_hostsim.py::test_the_statistical_seed_passes_on_the_twin) before it is used here.
    pb, par, rows, offs = stat_problem()
    eng = capi.Engine(pb)
    pred = eng.predict(par, rows, offs)
    got = eng.path_proximity(par, rows[:1], offs[:1], rows[1:], offs[1:], [0, 1], STAT_DRAWS, seed=STAT_SEED)
    eng.close()
    assert got.shape == (STAT_DRAWS, 1, 2) and np.all(np.isfinite(got)) and np.all(got[:, 0, 1] == 0.0)
    ratio = stat_ratio(got[:, 0, 0], pred["mean"], pred["cov"])
    print(f"STAT proximity ratio {ratio:.3f}")
    assert ratio <= 5.0


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_unserved_models_and_bad_arguments():
    for sp in (make_spec("gpx_cir", "CIR", 1, seed=221, lengths=[9, 2, 14]), eseal_spec("gpx_eseal", 211, [14, 9, 11]),
               make_spec("gpx_coupled3", "CTCRW", 3, seed=33, lengths=LENGTHS70[:14], with_H=True, na_rows=(2, 11))):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.path_proximity(sp["par"], [3], [0.1], [4], [0.1], [0, 1], 2)
        assert _last_error(eng)
        eng.close()
        assert ei.value.status == ERR_MODEL, sp["name"]
    spec = _const_spec("CTCRW", 2, "irregular")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    par = np.ascontiguousarray(spec["par"])
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    ra = np.array([3, 4, 5], dtype=np.int64); oa = np.array([0.1, 0.2, 0.0])
    rb = np.array([14, 15, 16], dtype=np.int64); ob = np.array([0.0, 0.1, 0.2])
    pp = np.array([0, 2, 3], dtype=np.int64); w = np.array([1.0, 0.5, 2.0]); rad = np.array([0.37, np.inf])
    out = np.zeros(2 * 4 * 2)

    def args(**over):
        a = dict(par=par.ctypes.data_as(dp), n_par=pb.n_par_full, seed=7, draw0=0, n_draws=2, ra=ra, oa=oa, rb=rb, ob=ob, pp=pp, n_pairs=2, w=w,
                 rad=rad, n_radii=2, out=out.ctypes.data_as(dp), flags=0)
        a.update(over)
        for k in ("ra", "rb", "pp"):
            a[k] = None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.int64)
        for k in ("oa", "ob", "w", "rad"):
            a[k] = None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.float64)
        keep.append(a)
        p = lambda v, t: None if v is None else v.ctypes.data_as(t)
        return [a["par"], a["n_par"], a["seed"], a["draw0"], a["n_draws"], p(a["ra"], lp), p(a["oa"], dp), p(a["rb"], lp), p(a["ob"], dp),
                p(a["pp"], lp), a["n_pairs"], p(a["w"], dp), p(a["rad"], dp), a["n_radii"], a["out"], a["flags"]]
    keep = []
    call = lambda **over: eng.lib.ssde_path_proximity(eng._h, *args(**over))
    assert eng.lib.ssde_path_proximity(None, *args()) == ERR_ARG
    cases = [
        (dict(par=None), "no parameter vector"), (dict(ra=None), "no queries"), (dict(oa=None), "no queries"), (dict(rb=None), "no queries"),
        (dict(ob=None), "no queries"), (dict(pp=None), "no pair list"), (dict(out=None), "no output"),
        (dict(n_par=pb.n_par_full + 1), "wrong length"),
        (dict(n_pairs=0), "n_pairs >= 1"), (dict(n_pairs=-1), "n_pairs >= 1"),
        (dict(pp=[1, 2, 3]), "pair_ptr"), (dict(pp=[0, 3, 2]), "pair_ptr"), (dict(pp=[0, 0, 0]), "pair_ptr"),
        (dict(ra=[-1, 4, 5]), "row outside"), (dict(rb=[14, 15, pb.n]), "row outside"),
        (dict(oa=[0.1, -0.2, 0.0]), "offset"), (dict(ob=[0.0, np.nan, 0.2]), "offset"), (dict(oa=[np.inf, 0.2, 0.0]), "offset"),
        (dict(n_draws=0), "n_draws >= 1"), (dict(n_draws=-1), "n_draws >= 1"), (dict(draw0=-1), "draw0 >= 0"),
        (dict(n_draws=1, draw0=(1 << 28) - 1), "2^28"), (dict(n_draws=2, draw0=(1 << 28) - 2), "2^28"),
        (dict(n_radii=-1), "n_radii"), (dict(n_radii=9), "n_radii"), (dict(rad=None), "n_radii"),
        (dict(rad=[0.37, np.nan]), "radius"), (dict(rad=[-0.1, 1.0]), "radius"),
        (dict(w=[1.0, -0.5, 2.0]), "weight"), (dict(w=[1.0, np.inf, 2.0]), "weight"), (dict(w=[np.nan, 0.5, 2.0]), "weight"),
        (dict(flags=1), "unknown flag"),
    ]
    for over, word in cases:
        assert call(**over) == ERR_ARG, over
        assert "ssde_path_proximity" in _last_error(eng) or "wrong length" in _last_error(eng), over
        assert word in _last_error(eng), (over, _last_error(eng))
    # the handle stays usable: the call itself, NULL weights, no radii, +inf as a radius
    assert call() == 0 and np.all(np.isfinite(out))
    assert call(w=None) == 0 and call(rad=None, n_radii=0) == 0 and call(rad=[np.inf, 0.0]) == 0
    got = eng.path_proximity(par, ra, oa, rb, ob, pp, 2, seed=7, radii=rad, weight=w)
    assert call() == 0 and np.array_equal(out.reshape(2, 4, 2).transpose(0, 2, 1), got)
    eng.close()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_sde_proximity():
    from cases import _tracks
    from smoothsde_amd.sde import SDE
    rng = np.random.default_rng(61)
    ID, times, obs = _tracks(rng, "CTCRW", 2, [12, 7, 1, 9, 2, 11, 5], irregular=True)
    n = len(ID)
    for k in np.unique(ID):                                              # the tracks on one clock, so that their windows overlap
        m = ID == k
        times[m] -= times[m][0] - 0.1 * k
        obs[m] -= 10.0 * k - 0.3 * k                                     # ... and near each other
    data = {"ID": ID, "time": times, "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~1", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.05, -0.05, 0.3, 0.1])
    sde.setup()
    ids = list(dict.fromkeys(ID.tolist()))
    t_of = {k: times[ID == k] for k in ids}
    pairs = [(ids[0], ids[5]), (ids[0], ids[0]), (ids[3], 10 ** 6), (ids[1], ids[2]), (ids[5], ids[3])]
    radii = [0.37, 1.3, np.inf]
    out = sde.proximity(pairs, radii, 4, seed=9)
    ra, oa, rb, ob, pp, w = sde.proximity_queries_
    st = sde.engine_.path_proximity(sde._current_par_full(), ra, oa, rb, ob, pp, 4, seed=9, radii=radii, weight=w)
    assert np.array_equal(out["min_dist"], st[:, :, 0], equal_nan=True) and np.array_equal(out["time_within"], st[:, :, 2:], equal_nan=True)
    assert out["min_dist"].shape == (4, 5) and out["time_within"].shape == (4, 5, 3) and out["p_within"].shape == (5, 3)
    # an unknown ID and a one-row track: NaN, and the call went through
    assert len(out["times"][2]) == 0 and len(out["times"][3]) == 0
    assert np.all(np.isnan(out["min_dist"][:, [2, 3]])) and np.all(np.isnan(out["p_within"][[2, 3]])) and np.all(np.isnan(out["t_min"][:, [2, 3]]))
    for p in (0, 1, 4):
        a, b = t_of[pairs[p][0]], t_of[pairs[p][1]]
        lo, hi = max(a[1], b[1]), min(a[-1], b[-1])
        u = np.union1d(a, b)
        assert np.array_equal(out["times"][p], u[(u >= lo) & (u <= hi)])
        if len(out["times"][p]):
            assert np.all(np.isfinite(out["min_dist"][:, p])) and np.all(out["p_within"][p, 2] == 1.0)
            assert np.all(np.isin(out["t_min"][:, p], out["times"][p]))
            total = out["times"][p][-1] - out["times"][p][0]
            assert np.allclose(out["time_within"][:, p, 2], total, rtol=1e-12, atol=0)           # r = inf: the whole window, to the quantum
    assert len(out["times"][1]) > 0 and np.all(out["min_dist"][:, 1] == 0.0) and np.all(out["p_within"][1] == 1.0)
    # given times: the ones before either second stamp are dropped, later ones are forecasts; points are counted
    a, b = t_of[ids[0]], t_of[ids[5]]
    grid = np.r_[min(a[0], b[0]) - 1.0, np.linspace(max(a[1], b[1]), max(a[-1], b[-1]) + 2.0, 7)]
    cnt = sde.proximity([(ids[0], ids[5])], [np.inf], 3, seed=9, times=grid, weight=None)
    assert np.array_equal(cnt["times"][0], grid[1:]) and np.all(cnt["time_within"][:, 0, 0] == 7.0)
    assert n == len(times)
