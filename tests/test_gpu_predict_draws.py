"""GPU suite (-m gpu): ssde_predict_draws, joint posterior draws of the state at any time, on every handle layout it
serves, against the numpy reference of tests/bridge_ref.py (itself, and the host twin of the lane math, checked against the joint
Gaussian of the augmented problem on the CPU: test_predict_draws_host.py, test_predict_draws_hostsim.py).

Every comparison goes through bridge_ref.compare_draws: the twin's limit 1e-9 (1 + max|ref|), NaN patterns identical; every layout also
asks (row, 0) over every row and (row, Delta) over every interior row and wants ssde_smooth_draws' numbers back, bitwise.  Shapes:
65 / 70 / 130 / 150 tracks (two or three groups of lanes, the last partly filled), tracks of at most 12 rows except on the lattice and
PATH_TV layouts, which need longer ones."""
import ctypes as C

import numpy as np
import pytest

from bridge_ref import STAT_DRAWS, STAT_SEED, bridge_queries, compare_draws, predict_draws_ref, stat_problem, stat_ratio
from cases import eseal_spec, make_spec, problem_from_spec
from predict_cases import expected_nan, intervals
from smoothsde_amd import capi
from smoothsde_amd.synth import simulate

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
ERR_ARG, ERR_MODEL = 1, 2
MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS70 = [12, 7, 1, 9, 2, 11, 5] * 10             # 70 tracks: a full group and a partly filled one
LENGTHS65 = [9, 3, 1, 2, 12] * 13                    # 65 tracks: one lane in the second group
N70 = sum(LENGTHS70)
ND, SEED = 5, 11


def _last_error(eng):
    msg = eng.lib.ssde_last_error(eng._h)
    return msg.decode() if msg else ""


def _const_spec(model, d, what, lengths=LENGTHS70, seed=3):
    n = sum(lengths)
    na = (5, 11, 40, 41, n - 1) if what == "missing" else ()           # row 11 ends the first track
    return make_spec(f"gpd_{model}_{d}_{what}", model, d, seed=seed + d, lengths=lengths, irregular=(what != "regular"), na_rows=na)


def _check(eng, pb, par, rows, offs, tag, nd=ND, seed=SEED, draw0=2, ref=None):
    """GPU vs the reference on the queries (ref: the problem and queries the reference takes in their place); then the rows' own draws
    back, bitwise: offset 0 on every row, the interval on interior rows"""
    got = eng.predict_draws(par, rows, offs, nd, seed=seed, draw0=draw0)
    assert got.shape == (nd, len(rows), pb.sdim)
    rpb, rrows, roffs = ref or (pb, rows, offs)
    compare_draws(got, predict_draws_ref(rpb, par, rrows, roffs, seed=seed, draw0=draw0, n_draws=nd), f"GPU vs predict_draws_ref: {tag}")
    paths = eng.smooth_draws(par, nd, seed=seed, draw0=draw0)
    every = np.arange(pb.n)
    assert np.array_equal(eng.predict_draws(par, every, np.zeros(pb.n), nd, seed=seed, draw0=draw0), paths, equal_nan=True), tag
    first, last, dt = intervals(pb)
    inner = np.flatnonzero(~first & ~last)
    assert np.array_equal(eng.predict_draws(par, inner, dt[inner], nd, seed=seed, draw0=draw0), paths[:, inner + 1], equal_nan=True), tag
    return got


# ---- path 1: constant coefficients ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d,what", [(2, "regular"), (2, "irregular"), (2, "missing"), (1, "missing")])
def test_constant_coefficients(model, d, what):
    spec = _const_spec(model, d, what)
    pb = problem_from_spec(spec)
    rows, offs = bridge_queries(pb, seed=d)
    eng = capi.Engine(pb)
    info = eng.info()
    got = _check(eng, pb, spec["par"], rows, offs, f"const {model} d={d} {what}")
    eng.close()
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_groups"] == 2
    assert np.array_equal(np.isnan(got[0, :, 0]), expected_nan(pb, rows, offs))


@pytest.mark.parametrize("model", MODELS)
def test_130_regular_complete_tracks(model):
    ID, times, obs = simulate(model, 130, 12, 2, seed=12)
    pb = capi.Problem(model, ID, times, obs)
    par = np.r_[-1.0, 0.05, -0.05, 0.4, 0.1][:1 + capi.n_sde_par(model, 2)]
    rows, offs = bridge_queries(pb, seed=2, frac=0.5)
    eng = capi.Engine(pb)
    info = eng.info()
    _check(eng, pb, par, rows, offs, f"130 tracks {model}")
    eng.close()
    assert info["path"] == PATH_ISO and info["uniform_dt"] == 1 and info["n_groups"] == 3


# ---- shapes: query counts, draw counts, crowded intervals ------------------------------------------------------------------------
@pytest.mark.parametrize("n_query", [1, 63, 64, 65, 257])
def test_query_counts_on_65_tracks_with_short_tracks(n_query):
    spec = _const_spec("CTCRW", 2, "irregular", lengths=LENGTHS65, seed=7)
    pb = problem_from_spec(spec)
    rows, offs = bridge_queries(pb, seed=11)
    assert len(rows) >= 257
    rows, offs = rows[-n_query:], offs[-n_query:]
    if n_query == 1:                                                    # one interior state: every other track has no query
        first, last, dt = intervals(pb)
        j = int(np.flatnonzero(~first & ~last)[30])
        rows, offs = np.array([j]), np.array([0.4 * dt[j]])
    eng = capi.Engine(pb)
    info = eng.info()
    got = eng.predict_draws(spec["par"], rows, offs, ND, seed=SEED)
    eng.close()
    assert info["path"] == PATH_ISO and info["n_groups"] == 2 and info["n_tracks"] == 65
    compare_draws(got, predict_draws_ref(pb, spec["par"], rows, offs, seed=SEED, n_draws=ND), f"GPU vs predict_draws_ref: n_query={n_query}")


@pytest.mark.parametrize("n_draws", [1, 4, 5])
def test_draw_counts_at_the_edges_of_a_wave_s_chunk(n_draws):
    spec = _const_spec("OU_SSM", 2, "missing", lengths=LENGTHS65, seed=8)
    pb = problem_from_spec(spec)
    rows, offs = bridge_queries(pb, seed=12)
    eng = capi.Engine(pb)
    info = eng.info()
    _check(eng, pb, spec["par"], rows, offs, f"65 tracks n_draws={n_draws}", nd=n_draws, draw0=3)
    eng.close()
    assert info["n_groups"] == 2 and info["n_tracks"] == 65


def test_sorted_unsorted_crowded_intervals_and_a_track_without_a_query():
    spec = _const_spec("CTCRW", 2, "irregular", lengths=LENGTHS65, seed=9)
    pb = problem_from_spec(spec)
    first, last, dt = intervals(pb)
    rows, offs = bridge_queries(pb, seed=13, shuffle=False)
    j = int(np.flatnonzero(~first & ~last)[40])
    e = int(np.flatnonzero(last & ~first)[5])
    track3 = (rows >= pb.seg_start[3]) & (rows < pb.seg_start[4])         # a track with no query at all
    keep = ~track3 & (rows != j) & (rows != e)
    crowd = np.linspace(0.0, dt[j], 20)                                  # 20 offsets in one interval, its two ends among them
    chain = np.cumsum(np.r_[0.0, np.full(49, 0.37)])                      # a forecast chain of 50 offsets
    rows = np.r_[rows[keep], np.full(20, j), np.full(50, e), rows[keep][:30]]             # ... and the first 30 once more
    offs = np.r_[offs[keep], crowd, chain, offs[keep][:30]]
    eng = capi.Engine(pb)
    srt = eng.predict_draws(spec["par"], rows, offs, ND, seed=SEED)
    p = np.random.default_rng(5).permutation(len(rows))
    mixed = eng.predict_draws(spec["par"], rows[p], offs[p], ND, seed=SEED)
    eng.close()
    assert np.array_equal(mixed, srt[:, p], equal_nan=True)
    assert np.array_equal(srt[:, -30:], srt[:, :30], equal_nan=True)
    compare_draws(srt, predict_draws_ref(pb, spec["par"], rows, offs, seed=SEED, n_draws=ND), "GPU vs predict_draws_ref: crowded")


# ---- a lattice handle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_a_lattice_handle_answers_inside_the_absent_fix_gaps(model):
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks(model, 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
    obs[39 if ID[39] == ID[38] else 38] = np.nan
    pb = capi.Problem(model, ID, times, obs)
    par = _par(model, 2, np.random.default_rng(2))
    first, last, dt = intervals(pb)
    rows, offs = bridge_queries(pb, seed=17, frac=0.3)
    gaps = np.flatnonzero(~first & ~last & (dt > 0.75))                   # intervals of two to four lattice steps
    gaps = gaps[~np.isin(gaps, rows)][:40]
    assert len(gaps) >= 20
    # in every such gap: on a lattice point, just before and after one, in the last step, at the gap's end
    rows = np.r_[rows, np.repeat(gaps, 5)]
    offs = np.r_[offs, (np.array([0.5, 0.49, 0.61, 0.0, 1.0])[None, :] * np.c_[np.ones((len(gaps), 3)), dt[gaps] - 0.2, dt[gaps]]).ravel()]
    # The slots of a lattice handle are its LATTICE rows: the draw holds a state at every absent fix, and the bridges
    # run inside the lattice steps.  The reference takes the tracks with the absent fixes written out as NA rows, and every query at
    # the written-out row the plan's rule sends it to: whole steps inside the offset move the row, the rest is the offset.
    from test_gpu_draws import _written_out
    ID2, t2, obs2, at = _written_out(ID, times, obs, 0.5)
    pb2 = capi.Problem(model, ID2, t2, obs2)
    w = np.floor(offs / 0.5 + 1e-9).astype(np.int64)
    rest = np.maximum(offs - w * 0.5, 0.0)
    nxt = at[np.minimum(rows + 1, pb.n - 1)]
    inner = ~first[rows] & ~last[rows]
    past = inner & ((at[rows] + w > nxt) | ((at[rows] + w == nxt) & (rest > 1e-9 * 0.5)))
    rest[inner & (at[rows] + w == nxt)] = 0.0
    rows2 = np.where(inner, at[rows] + w, at[rows])
    offs2 = np.where(inner, rest, offs)
    rows2[past] = 0; offs2[past] = 0.0                                   # past the next fix: NaN, as a query on a first row is
    eng = capi.Engine(pb)
    info = eng.info()
    assert pb2.n == info["n_rows_tiled"]
    got = _check(eng, pb, par, rows, offs, f"lattice {model}", ref=(pb2, rows2, offs2))
    eng.close()
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] > pb.n
    assert np.array_equal(np.isnan(got[0, :, 0]), expected_nan(pb, rows, offs))


# ---- the full-covariance lanes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_force_dense(model):
    spec = _const_spec(model, 2, "missing")
    pb = problem_from_spec(spec, flags=capi.FLAG_FORCE_DENSE)
    rows, offs = bridge_queries(pb, seed=19)
    eng = capi.Engine(pb)
    info = eng.info()
    _check(eng, pb, spec["par"], rows, offs, f"dense {model}")
    eng.close()
    assert info["path"] == PATH_DENSE and info["n_rows_tiled"] == pb.n


@pytest.mark.parametrize("model,d", [("CTCRW", 2), ("OU_SSM", 2), ("BM_SSM", 2), ("CTCRW", 1)])
def test_per_row_h_and_a_general_p0(model, d):
    spec = make_spec(f"gpd_hp_{model}_{d}", model, d, seed=41 + d, lengths=LENGTHS70, with_H=True, with_P0=True, na_rows=(5, 11, N70 - 1))
    pb = problem_from_spec(spec)
    rows, offs = bridge_queries(pb, seed=23)
    eng = capi.Engine(pb)
    info = eng.info()
    _check(eng, pb, spec["par"], rows, offs, f"H P0 {model} d={d}")
    eng.close()
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == pb.n and info["n_tracks"] == 70


# ---- row-varying parameters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,extra", [("CTCRW", "H"), ("OU_SSM", ""), ("BM_SSM", "P0")])
def test_tv_route_with_150_tracks(model, extra, monkeypatch):
    from test_gpu_smooth_layouts import _tv_many
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = _tv_many(model, seed=29, with_H=extra == "H", with_P0=extra == "P0")
    pb = problem_from_spec(spec)
    rows, offs = bridge_queries(pb, seed=37, frac=0.15)
    eng = capi.Engine(pb)
    info = eng.info()
    assert info["path"] == PATH_TV and info["n_tracks"] == 150
    one = _check(eng, pb, spec["par"], rows, offs, f"tv {model} {extra}")
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.predict_draws(spec["par"], rows, offs, ND, seed=SEED, draw0=2)
    eng.close()
    assert np.array_equal(one, many, equal_nan=True)


# ---- column pairs and shards ----------------------------------------------------------------------------------------------------
def test_uncoupled_ctcrw_d4_runs_as_column_pairs():
    spec = make_spec("gpd_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70, na_rows=(2, 11))
    pb = problem_from_spec(spec)
    rows, offs = bridge_queries(pb, seed=41)
    eng = capi.Engine(pb)
    info = eng.info()
    _check(eng, pb, spec["par"], rows, offs, "pairs")
    eng.close()
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == 2 * pb.n and info["sdim"] == 8


@pytest.mark.parametrize("layout", ["const", "pairs", "tv", "lattice"])
def test_two_shards_are_bitwise_the_single_device_handle(layout, monkeypatch):
    frac = 1.0
    if layout == "tv":
        from test_gpu_smooth_layouts import _tv_many
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec, frac = _tv_many("OU_SSM", seed=37), 0.15
    elif layout == "pairs":
        spec = make_spec("gpd_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70, na_rows=(2, 11))
    elif layout == "lattice":
        from test_gpu_lattice import _par, lattice_tracks
        ID, times, obs = lattice_tracks("CTCRW", 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
        spec, frac = dict(model="CTCRW", ID=ID, times=times, obs=obs, par=_par("CTCRW", 2, np.random.default_rng(2))), 0.3
    else:
        spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    rows, offs = bridge_queries(pb, seed=43, frac=frac)
    e1 = capi.Engine(pb)
    one = e1.predict_draws(spec["par"], rows, offs, ND, seed=SEED)
    n1 = e1.info()["n_devices"]
    e1.close()
    e2 = capi.Engine(pb, devices=[0, 0])
    two = e2.predict_draws(spec["par"], rows, offs, ND, seed=SEED)
    n2 = e2.info()["n_devices"]
    e2.close()
    assert n2 == 2 and n1 <= 1
    assert np.array_equal(one, two, equal_nan=True) and np.isfinite(one).any()


# ---- invariance, all bitwise ----------------------------------------------------------------------------------------------------
def test_budget_chunks_draw_batches_and_calls_are_bitwise():
    # the batch of test_gpu_smooth_layouts.py::test_chunks_on_ragged_tiled_groups_are_bitwise: six groups, 1 MiB cuts them into chunks
    rng = np.random.default_rng(31)
    lengths = np.r_[rng.integers(71, 90, 64), rng.integers(45, 61, 63), [60], rng.integers(10, 16, 64), rng.integers(3, 8, 64),
                    rng.integers(2, 4, 64), [1, 2, 5, 1, 3]]
    lengths = [int(v) for v in rng.permutation(lengths)]
    spec = make_spec("gpd_chunks", "CTCRW", 2, seed=31, lengths=lengths, irregular=True)
    pb = problem_from_spec(spec)
    rows, offs = bridge_queries(pb, seed=47, frac=0.1)
    eng = capi.Engine(pb)
    info = eng.info()
    assert info["path"] == PATH_ISO and info["n_groups"] == 6
    par = spec["par"]
    one = eng.predict_draws(par, rows, offs, 8, seed=SEED)
    lo, hi = eng.predict_draws(par, rows, offs, 4, seed=SEED, draw0=0), eng.predict_draws(par, rows, offs, 4, seed=SEED, draw0=4)
    assert np.array_equal(one, np.concatenate([lo, hi]), equal_nan=True)                     # draws [0, 8) = [0, 4) + [4, 8)
    cut = rows < np.median(rows)                                                           # whole intervals on either side
    a, b = eng.predict_draws(par, rows[cut], offs[cut], 8, seed=SEED), eng.predict_draws(par, rows[~cut], offs[~cut], 8, seed=SEED)
    two = np.empty_like(one); two[:, cut] = a; two[:, ~cut] = b
    assert np.array_equal(one, two, equal_nan=True)                                        # two calls = one
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.predict_draws(par, rows, offs, 8, seed=SEED)
    eng.close()
    assert np.array_equal(one, many, equal_nan=True)
    compare_draws(one[:2], predict_draws_ref(pb, par, rows, offs, seed=SEED, n_draws=2), "GPU vs predict_draws_ref: chunks ragged")


# ---- isolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["const", "tv"])
def test_a_call_leaves_every_other_call_as_it_was(layout, monkeypatch):
    frac = 1.0
    if layout == "tv":
        from test_gpu_smooth_layouts import _tv_many
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec, frac = _tv_many("CTCRW", seed=29), 0.15
    else:
        spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    rows, offs = bridge_queries(pb, seed=53, frac=frac)
    par = np.array(spec["par"], dtype=np.float64)
    par_b = par.copy(); par_b[1] += 0.01
    grid = dict(x0=-20.0, dx=2.0, y0=-20.0, dy=2.0, nx=20, ny=20)
    eng = capi.Engine(pb)

    def others():
        return (eng.smooth(par), eng.smooth_draws(par, 2, seed=3), eng.predict(par, rows, offs), eng.path_stats(par, 4, seed=3),
                eng.path_occupancy(par, 4, grid, seed=3))
    va, ga = eng.eval(par, order=1)
    was = others()
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.predict_draws(par, rows, offs, ND, seed=SEED)
    after = eng.info()
    assert after["n_evals"] == before["n_evals"] and after["n_memo_hits"] == before["n_memo_hits"]
    vb2, gb2 = eng.eval(par_b, order=1)                                            # still the memo's: a hit
    assert eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1 and vb2 == vb and np.array_equal(gb2, gb)
    va2, ga2 = eng.eval(par, order=1)                                              # evaluated afresh
    assert va2 == va and np.array_equal(ga2, ga)
    now = others()
    eng.close()

    def flat(x):
        if isinstance(x, dict):
            return [v for k in sorted(x) for v in flat(x[k])]
        if isinstance(x, (tuple, list)):
            return [v for y in x for v in flat(y)]
        return [] if x is None else [np.asarray(x)]
    fa, fb = flat(was), flat(now)
    assert len(fa) == len(fb) and len(fa) >= 8
    for x, y in zip(fa, fb):
        assert np.array_equal(x, y, equal_nan=True)


# ---- the mean of many draws -------------------------------------------------------------------------------------------------------
def test_the_mean_of_4096_draws_is_the_predicted_mean():
    # the bound is derived: a mean of 4096 independent draws has standard deviation sqrt(V_ii / 4096); 6 of them over the 512 numbers
    # compared is a 1e-6 event.  The draws are a fixed function of the seed; the host twin gives ratio 2.80 for this seed
    pb, par, rows, offs = stat_problem()
    eng = capi.Engine(pb)
    pred = eng.predict(par, rows, offs)
    draws = eng.predict_draws(par, rows, offs, STAT_DRAWS, seed=STAT_SEED)
    eng.close()
    assert np.all(np.isfinite(draws))
    ratio = stat_ratio(draws, pred["mean"], pred["cov"])
    print(f"STAT largest ratio {ratio:.3f}")
    assert ratio <= 6.0


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_unserved_models_and_bad_arguments():
    for sp in (make_spec("gpd_ou", "OU", 1, seed=201, lengths=[9, 2, 14]), make_spec("gpd_cir", "CIR", 1, seed=221, lengths=[9, 2, 14]),
               eseal_spec("gpd_eseal", 211, [14, 9, 11]),
               make_spec("gpd_coupled3", "CTCRW", 3, seed=33, lengths=LENGTHS70[:14], with_H=True, na_rows=(2, 11))):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.predict_draws(sp["par"], [3], [0.1], 2)
        assert _last_error(eng)
        eng.close()
        assert ei.value.status == ERR_MODEL, sp["name"]
    spec = _const_spec("CTCRW", 2, "irregular")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    for rows, offs in (([], []), ([-1], [0.0]), ([pb.n], [0.0]), ([3], [-0.1]), ([3], [np.nan]), ([3], [np.inf])):
        with pytest.raises(capi.EngineError) as ei:
            eng.predict_draws(spec["par"], rows, offs, 2)
        assert ei.value.status == ERR_ARG and _last_error(eng), (rows, offs)
    for n_draws, draw0 in ((0, 0), (-1, 0), (1, -1), (1, (1 << 28) - 1), (2, (1 << 28) - 2)):
        with pytest.raises(capi.EngineError) as ei:
            eng.predict_draws(spec["par"], [3], [0.1], n_draws, draw0=draw0)
        assert ei.value.status == ERR_ARG and _last_error(eng), (n_draws, draw0)
    par = np.ascontiguousarray(spec["par"])
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    r = np.array([3], dtype=np.int64); o = np.array([0.1]); m = np.zeros(4 * 2)
    args = [par.ctypes.data_as(dp), pb.n_par_full, r.ctypes.data_as(lp), o.ctypes.data_as(dp), 1, 7, 0, 2, m.ctypes.data_as(dp), 0]
    for null in (0, 2, 3, 8):                                                      # par, q_row, q_off, draws_at
        a = list(args); a[null] = None
        assert eng.lib.ssde_predict_draws(eng._h, *a) == ERR_ARG
    bad = list(args); bad[9] = 1                                                   # a flag: none is defined
    assert eng.lib.ssde_predict_draws(eng._h, *bad) == ERR_ARG and _last_error(eng)
    bad = list(args); bad[1] = pb.n_par_full + 1
    assert eng.lib.ssde_predict_draws(eng._h, *bad) == ERR_ARG and _last_error(eng)
    assert eng.lib.ssde_predict_draws(eng._h, *args) == 0 and np.all(np.isfinite(m))
    eng.close()


# ---- the det F <= 0 corner ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_negative_p0_follows_the_reference(model):
    ID, times, obs = simulate(model, 70, 12, 1, seed=4)
    keep = np.ones(len(ID), dtype=bool)
    keep[2 * 12 + 1:3 * 12] = False; keep[4 * 12 + 2:5 * 12] = False
    ID, times, obs = ID[keep], times[keep], obs[keep]
    obs[11] = np.nan
    sdim = 2 if model == "CTCRW" else 1
    P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
    par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
    pb = capi.Problem(model, ID, times, obs, P0=P0)
    rows, offs = bridge_queries(pb, seed=59)
    eng = capi.Engine(pb)
    got = eng.predict_draws(par, rows, offs, ND, seed=SEED)
    eng.close()
    ref = predict_draws_ref(pb, par, rows, offs, seed=SEED, n_draws=ND)
    if model == "CTCRW":
        assert np.isnan(ref[0, :, 0]).sum() > expected_nan(pb, rows, offs).sum()            # the rows that rejected their update
    compare_draws(got, ref, f"GPU vs predict_draws_ref: negative P0 {model}")


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_sde_sample_states_at():
    from cases import _tracks
    from smoothsde_amd.sde import SDE
    rng = np.random.default_rng(61)
    ID, times, obs = _tracks(rng, "CTCRW", 2, LENGTHS70, irregular=True)
    n = len(ID)
    obs[[5, 11]] = np.nan
    data = {"ID": ID, "time": times, "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~1", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.05, -0.05, 0.3, 0.1])
    sde.setup()
    pb = sde.problem_
    first, last, dt = intervals(pb)
    # the data's own times return sample_states' numbers
    own = sde.sample_states_at(ID, times, 3, seed=9)
    assert np.array_equal(own, sde.sample_states(3, seed=9), equal_nan=True) and np.isfinite(own[:, ~first]).all()
    rows, offs = bridge_queries(pb, seed=67)
    keep = ~expected_nan(pb, rows, offs) & ~(~last[rows] & (offs >= dt[rows]))       # times that name (row, offset) uniquely
    rows, offs = rows[keep], offs[keep]
    qid = np.r_[ID[rows], ID[0], 1e6]
    qt = np.r_[times[rows] + offs, times[0] - 1.0, 5.0]                              # before a track's first row; an unknown ID
    out = sde.sample_states_at(qid, qt, 3, seed=9)
    par = sde._current_par_full()
    back = qt[:-2] - times[rows]                                                     # the offsets the lookup forms
    assert np.array_equal(out[:, :-2], sde.engine_.predict_draws(par, rows, back, 3, seed=9), equal_nan=True)
    assert np.all(np.isnan(out[:, -2:])) and np.all(np.isfinite(out[:, :-2]))
    compare_draws(out[:, :-2], predict_draws_ref(pb, par, rows, back, seed=9, n_draws=3), "GPU vs predict_draws_ref: SDE.sample_states_at")
    bm = SDE(formulas={"mu": "~1", "sigma": "~1"}, data={"ID": ID, "time": times, "Z": np.cumsum(np.ones(n))}, type="BM", response="Z")
    with pytest.raises(NotImplementedError):
        bm.sample_states_at(ID[:2], times[:2], 2)
