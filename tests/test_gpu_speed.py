"""GPU suite (-m gpu): ssde_path_speed on every handle layout it serves.

Each comparison case checks the call twice: against the definition (tests/speed_ref.py) on the GPU's OWN draws (ssde_smooth_draws on
the same handle, seed and draw0), and against the definition on the numpy reference draws (tests/draws_ref.py).  Limit
1e-9 (1 + max|ref|) per statistic with identical NaN patterns -- the limit §3.10 and test_gpu_draws.py put on the draws themselves;
a statistic is a sum of at most 64 speeds or unit vectors of draws -- and the row of the maximum and the per-row counts exact.
Every case first asserts its two preconditions on the reference draws (speed_cases.py: no speed within 1e-5 (1 + thr) of a
threshold, the two largest speeds of a (track, draw) more than 1e-5 (1 + max) apart), runs a few thousand rows at most and five
draws (one full chunk of DRAW_CH = 4 and one partly filled) and asserts the layout it ran on (info()).  Shapes as test_gpu_path.py."""
import ctypes as C

import numpy as np
import pytest

from cases import _tracks, eseal_spec, make_spec, problem_from_spec
from draws_ref import draws_ref
from speed_cases import clear_maxima, clear_of_thresholds, compare, dt_weights, make_thresholds
from speed_ref import speed_ref, state_rows
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
LENGTHS70 = [20, 35, 1, 14, 2, 27, 9] * 10
ERR_ARG, ERR_MODEL = 1, 2
_REF = {}
# The draws' seed of every comparison case: the first from 11 (2 for the SDE case) whose reference draws meet both preconditions of
# speed_cases.py with half as much room again (1.5e-5), found on the CPU with tests/draws_ref.py before the GPU run.  A case whose inputs change needs its seed found anew.
SEEDS = {("const", 1, "regular"): 13, ("const", 1, "irregular"): 11, ("const", 1, "missing"): 12, ("const", 2, "regular"): 11,
         ("const", 2, "irregular"): 16, ("const", 2, "missing"): 16, ("tracks", 65): 12, ("tracks", 130): 11, "lattice": 14, ("hp", 1): 12,
         ("hp", 2): 15, "tv": 56, "negp0": 11, "sde": 3}
_dp, _up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)


def _ref(key, pb, par):
    """the five reference draws of a case at its seed, computed once and left unchanged"""
    if key not in _REF:
        with np.errstate(invalid="ignore"):
            _REF[key] = draws_ref(pb, par, seed=SEEDS[key], n_draws=5)
        _REF[key].setflags(write=False)
    return _REF[key]


def _show(tag, info, **more):
    keys = ("path", "kernel_id", "const_coeff", "uniform_dt", "n_rows", "n_rows_tiled", "n_groups", "n_devices", "n_tracks", "sdim")
    print("LAYOUT", tag, {k: info[k] for k in keys}, more)


def _const_spec(d, what, seed=3, lengths=LENGTHS70):
    na = (5, 19, 40, 41, sum(lengths) - 1) if what == "missing" else ()
    return make_spec(f"gs_CTCRW_{d}_{what}_{len(lengths)}", "CTCRW", d, seed=seed + d, lengths=lengths, irregular=(what == "irregular"), na_rows=na)


def _thresholds(pb, ref_draws, n_thr, tag):
    """the case's thresholds from its reference draws, with both preconditions asserted on them (conditions on the inputs)"""
    d = pb.n_dim
    thr = make_thresholds(ref_draws, pb.seg_start, d, n_thr)
    assert clear_of_thresholds(ref_draws, pb.seg_start, d, thr), tag
    assert clear_maxima(ref_draws, pb.seg_start, d), tag
    return thr


def _check(eng, pb, par, ref_draws, tag, seed, n_draws=5, draw0=0, n_thr=8):
    """path_speed against the definition on the handle's own draws and on the reference draws (the caller's rows of both)"""
    d = pb.n_dim
    thr = _thresholds(pb, ref_draws, n_thr, tag)
    w = dt_weights(pb.seg_start, pb.times)
    got = eng.path_speed(par, n_draws, seed=seed, draw0=draw0, thresholds=thr if n_thr else None, weight=w)
    assert got[0].shape == (n_draws, pb.n_seg, 5 + n_thr)
    assert (got[1] is None) if n_thr == 0 else (got[1].shape == (pb.n, n_thr))
    own = eng.smooth_draws(par, n_draws, seed=seed, draw0=draw0)
    ref_own, ref_ref = (speed_ref(dr, pb.seg_start, d, thresholds=thr, weight=w) for dr in (own, ref_draws))
    if n_thr == 0:
        ref_own, ref_ref = (ref_own[0], None), (ref_ref[0], None)
    compare(got, ref_own, f"{tag} | own draws")
    compare(got, ref_ref, f"{tag} | reference")
    return got, thr


def _raw(eng, par, n_draws, thr, weight, stats=True, rows=True, seed=11, draw0=0):
    """ssde_path_speed itself with either output absent: (stats or None, row_below or None)"""
    pb = eng.problem
    p = np.ascontiguousarray(par, dtype=np.float64)
    t = np.ascontiguousarray(thr, dtype=np.float64)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    buf = np.zeros((n_draws, 5 + len(t), pb.n_seg)) if stats else None
    cnt = np.full((len(t), pb.n), 77, dtype=np.uint32) if rows else None               # the call overwrites it
    st = eng.lib.ssde_path_speed(eng._h, p.ctypes.data_as(_dp), eng.n_par_full, seed, draw0, n_draws, t.ctypes.data_as(_dp), len(t),
                                 None if w is None else w.ctypes.data_as(_dp), None if buf is None else buf.ctypes.data_as(_dp),
                                 None if cnt is None else cnt.ctypes.data_as(_up), 0)
    assert st == 0, st
    return (None if buf is None else buf.transpose(0, 2, 1)), (None if cnt is None else cnt.T)


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


# ---- path 1: constant coefficients ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("what", ["regular", "irregular", "missing"])
def test_constant_coefficients(d, what):
    spec = _const_spec(d, what)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"const CTCRW d={d} {what}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_groups"] == 2
    assert info["n_tracks"] == 70
    (got, below), thr = _check(eng, pb, spec["par"], _ref(("const", d, what), pb, spec["par"]), f"const CTCRW d={d} {what}", SEEDS["const", d, what])
    eng.close()
    lengths = np.array(LENGTHS70)
    one_row = lengths == 1
    assert np.all(np.isnan(got[:, one_row, :])) and np.all(np.isfinite(got[:, ~one_row, :]))
    assert np.array_equal(got[0, lengths == 2, 2], np.asarray(pb.seg_start)[lengths == 2] + 1.0)   # one state row: its own maximum
    has = state_rows(pb.seg_start, pb.n)
    assert np.all(below[~has] == 0) and np.all(below[has, 6] == 5) and np.all(below[:, 5] == 0)   # +inf: every draw; 0: none
    band = got[:, ~one_row, 5:10]
    assert np.any(band > 0) and np.any(band == 0)
    if d == 1:
        assert np.all(got[:, ~one_row, 4] == 0.0)


@pytest.mark.parametrize("n_tracks", [65, 130])
def test_65_and_130_tracks(n_tracks):
    lengths = (LENGTHS70 * 2)[:n_tracks]
    spec = _const_spec(2, "missing", seed=4, lengths=lengths)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"{n_tracks} tracks", info)
    assert info["path"] == PATH_ISO and info["n_tracks"] == n_tracks and info["n_groups"] == (n_tracks + 63) // 64
    _check(eng, pb, spec["par"], _ref(("tracks", n_tracks), pb, spec["par"]), f"{n_tracks} tracks", SEEDS["tracks", n_tracks])
    eng.close()


@pytest.mark.parametrize("n_draws", [1, 4, 5])
@pytest.mark.parametrize("n_thr", [0, 1, 8])
def test_draw_and_threshold_counts(n_draws, n_thr):
    spec = _const_spec(2, "missing")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    assert info["path"] == PATH_ISO and info["n_groups"] == 2 and info["n_tracks"] == 70
    ref = _ref(("const", 2, "missing"), pb, spec["par"])[:n_draws]
    _check(eng, pb, spec["par"], ref, f"{n_draws} draws {n_thr} thresholds", SEEDS["const", 2, "missing"], n_draws=n_draws, n_thr=n_thr)
    eng.close()


# ---- a lattice handle -----------------------------------------------------------------------------------------------------------
def _lattice():
    from test_gpu_draws import _written_out
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks("CTCRW", 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=9, na_frac=0.05)
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = _par("CTCRW", 2, np.random.default_rng(2))
    ID2, t2, obs2, rows = _written_out(ID, times, obs, 0.5)
    pb2 = capi.Problem("CTCRW", ID2, t2, obs2)
    return pb, par, pb2, rows


def test_a_lattice_handle_skips_its_padded_rows():
    pb, par, pb2, rows = _lattice()
    eng = capi.Engine(pb)
    info = eng.info()
    _show("lattice CTCRW", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] > pb.n
    assert pb2.n == info["n_rows_tiled"] and pb2.n_seg == pb.n_seg                 # the written-out rows ARE the handle's lattice
    full_draws = _ref("lattice", pb2, par)
    (got, below), thr = _check(eng, pb, par, full_draws[:, rows, :], "lattice CTCRW", SEEDS["lattice"])   # weights, counts and max_row by the caller's rows
    eng.close()
    # the padded rows, had they counted, would have been counted below +inf
    _, full_below = speed_ref(full_draws, pb2.seg_start, 2, thresholds=thr)
    assert full_below[:, 6].sum() > below[:, 6].sum() and below[:, 6].sum() == 5 * (pb.n - pb.n_seg)
    ok = ~np.isnan(got[:, :, 2])
    assert np.all(got[:, :, 2][ok] < pb.n)


# ---- path 2, per-row H, a general P0 ----------------------------------------------------------------------------------------------
def test_force_dense():
    spec = _const_spec(2, "missing")
    pb = problem_from_spec(spec, flags=capi.FLAG_FORCE_DENSE)
    eng = capi.Engine(pb)
    info = eng.info()
    _show("dense CTCRW", info)
    assert info["path"] == PATH_DENSE and info["n_groups"] == 2
    _check(eng, pb, spec["par"], _ref(("const", 2, "missing"), pb, spec["par"]), "dense CTCRW", SEEDS["const", 2, "missing"])
    eng.close()


@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(d):
    spec = make_spec(f"gs_hp_CTCRW_{d}", "CTCRW", d, seed=21, lengths=LENGTHS70, with_H=True, with_P0=True, na_rows=(3, 19, 40, 41))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"H P0 CTCRW d={d}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_tracks"] == 70
    _check(eng, pb, spec["par"], _ref(("hp", d), pb, spec["par"]), f"H P0 CTCRW d={d}", SEEDS["hp", d])
    eng.close()


# ---- path 3: row-varying coefficients, 150 tracks ---------------------------------------------------------------------------------
def _tv_spec(seed):
    from test_gpu_smooth_layouts import _tv_many
    return _tv_many("CTCRW", seed=seed)


def test_tv_route_with_150_tracks(monkeypatch):
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = _tv_spec(29)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show("tv CTCRW", info)
    assert info["path"] == PATH_TV and info["n_tracks"] == 150 and info["const_coeff"] == 0
    got, thr = _check(eng, pb, spec["par"], _ref("tv", pb, spec["par"]), "tv CTCRW", SEEDS["tv"])
    # three groups of lanes by length: 1 MiB of records makes each group its own chunk (test_gpu_smooth_layouts.py)
    w = dt_weights(pb.seg_start, pb.times)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.path_speed(spec["par"], 5, seed=SEEDS["tv"], thresholds=thr, weight=w)
    eng.close()
    assert _same(got, many)


# ---- the det F <= 0 corner ----------------------------------------------------------------------------------------------------------
def _negative_p0():
    from smoothsde_amd.synth import simulate
    ID, times, obs = simulate("CTCRW", 70, 12, 1, seed=4)
    keep = np.ones(len(ID), dtype=bool)
    keep[2 * 12 + 1:3 * 12] = False; keep[4 * 12 + 2:5 * 12] = False
    ID, times, obs = ID[keep], times[keep], obs[keep]
    obs[11] = np.nan
    return capi.Problem("CTCRW", ID, times, obs, P0=np.diag([-5.0, 1.0])), np.array([-2.0, 0.7, 0.3, 0.1])


def test_negative_p0_follows_the_reference():
    pb, par = _negative_p0()
    eng = capi.Engine(pb)
    info = eng.info()
    _show("negative P0 CTCRW", info)
    assert info["path"] == PATH_ISO
    (got, below), _ = _check(eng, pb, par, _ref("negp0", pb, par), "negative P0 CTCRW", SEEDS["negp0"])
    eng.close()
    nan = np.isnan(got)
    assert np.array_equal(nan.any(axis=2), nan.all(axis=2))                        # all of a (track, draw) or nothing


# ---- invariance, all bitwise ------------------------------------------------------------------------------------------------------
def _ragged_spec():
    # the batch of test_gpu_draws.py::test_budget_chunks_on_six_ragged_groups_and_draw_batches_are_bitwise: 1 MiB = 131072 doubles
    # cuts the records into three chunks, produced again for every batch of draws
    rng = np.random.default_rng(31)
    lengths = np.r_[rng.integers(71, 90, 64), rng.integers(45, 61, 63), [60], rng.integers(10, 16, 64), rng.integers(3, 8, 64),
                    rng.integers(2, 4, 64), [1, 2, 5, 1, 3]]
    lengths = [int(v) for v in rng.permutation(lengths)]
    starts = np.r_[0, np.cumsum(lengths)]
    k5 = next(k for k, L in enumerate(lengths) if L >= 5)
    return make_spec("gs_chunks", "CTCRW", 2, seed=31, lengths=lengths, irregular=True,
                     na_rows=(int(starts[k5]) + 2, int(starts[k5]) + 3, int(starts[k5 + 1]) - 1))


def test_budget_chunks_on_six_ragged_groups_are_bitwise():
    # (bitwise only: five draws of these 9799 rows put some speed within 1e-5 of some quantile threshold under almost every seed, so
    # the thresholds here are plain numbers and nothing is compared with a reference)
    spec = _ragged_spec()
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show("chunks ragged", info)
    assert info["path"] == PATH_ISO and info["n_groups"] == 6 and pb.n_seg == 325
    thr, w = np.array([0.3, 0.0, np.inf, 1.1, 0.05, 2.5, 0.7, 50.0]), dt_weights(pb.seg_start, pb.times)
    # 325 tracks x 13 statistics beside the counts' n x 8 x 4 bytes: 1 MiB holds fewer than 44 draws, so 44 draws go in two or
    # more batches, each over the three chunks
    assert (131072 - pb.n * 4) // (325 * 13) < 44
    one = eng.path_speed(spec["par"], 5, seed=11, thresholds=thr, weight=w)
    wide = eng.path_speed(spec["par"], 44, seed=11, thresholds=thr, weight=w)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.path_speed(spec["par"], 5, seed=11, thresholds=thr, weight=w)
    wide_many = eng.path_speed(spec["par"], 44, seed=11, thresholds=thr, weight=w)
    wide_rows = _raw(eng, spec["par"], 44, thr, w, stats=False)
    eng.close()
    assert _same(one, many) and _same(wide, wide_many) and np.array_equal(wide_rows[1], wide[1])
    assert np.array_equal(wide[0][:5], one[0], equal_nan=True)
    has = state_rows(pb.seg_start, pb.n)
    assert np.all(wide[1][has, 2] == 44) and np.all(wide[1][~has] == 0) and np.all(wide[1][:, 1] == 0)
    assert np.any(wide[1][:, 0] > 0) and np.any(wide[1][:, 0] < 44) and np.all(np.isfinite(one[0][:, np.diff(np.r_[pb.seg_start, pb.n]) > 1, :]))


def test_draw_numbering_weights_threshold_order_and_halves_are_bitwise():
    spec = _const_spec(2, "missing")
    pb = problem_from_spec(spec)
    par = spec["par"]
    thr = make_thresholds(_ref(("const", 2, "missing"), pb, par), pb.seg_start, 2, 8)
    w = dt_weights(pb.seg_start, pb.times)
    eng = capi.Engine(pb)
    whole = eng.path_speed(par, 8, seed=5, thresholds=thr, weight=w)
    a = eng.path_speed(par, 4, seed=5, draw0=0, thresholds=thr, weight=w)
    b = eng.path_speed(par, 4, seed=5, draw0=4, thresholds=thr, weight=w)
    assert np.array_equal(whole[0], np.concatenate([a[0], b[0]]), equal_nan=True)  # [0, 8) = [0, 4) + [4, 8)
    assert np.array_equal(whole[1], a[1] + b[1])                                   # ... with the counts added on the host
    assert _same(whole, eng.path_speed(par, 8, seed=5, thresholds=thr, weight=w))  # two identical calls
    # stats alone, row_below alone and both together
    both = _raw(eng, par, 8, thr, w, seed=5)
    only_s = _raw(eng, par, 8, thr, w, rows=False, seed=5)
    only_b = _raw(eng, par, 8, thr, w, stats=False, seed=5)
    assert _same(both, whole) and only_s[1] is None and only_b[0] is None
    assert np.array_equal(only_s[0], whole[0], equal_nan=True) and np.array_equal(only_b[1], whole[1])
    assert np.array_equal(eng.path_speed(par, 8, seed=5, thresholds=thr, weight=w, rows=False)[0], whole[0], equal_nan=True)
    none = eng.path_speed(par, 5, seed=5, thresholds=thr)
    ones = eng.path_speed(par, 5, seed=5, thresholds=thr, weight=np.ones(pb.n))
    assert _same(none, ones) and not np.array_equal(none[0], whole[0][:5], equal_nan=True)
    perm = np.random.default_rng(5).permutation(8)
    mixed = eng.path_speed(par, 8, seed=5, thresholds=thr[perm], weight=w)
    assert np.array_equal(mixed[0][:, :, :5], whole[0][:, :, :5], equal_nan=True)
    assert np.array_equal(mixed[0][:, :, 5:], whole[0][:, :, 5:][:, :, perm], equal_nan=True) and np.array_equal(mixed[1], whole[1][:, perm])
    other = eng.path_speed(par, 1, seed=6, thresholds=thr, weight=w)
    eng.close()
    assert not np.array_equal(other[0][0], whole[0][0], equal_nan=True)


@pytest.mark.parametrize("layout", ["const", "tv", "lattice"])
def test_two_shards_are_bitwise_the_single_device_handle(layout, monkeypatch):
    if layout == "tv":
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = _tv_spec(37)
        pb, par = problem_from_spec(spec), spec["par"]
    elif layout == "lattice":
        pb, par, _, _ = _lattice()
    else:
        spec = _const_spec(2, "missing")
        pb, par = problem_from_spec(spec), spec["par"]
    thr, w = np.array([0.3, 0.0, np.inf, 1.1, 0.05, 2.5, 0.7, 50.0]), dt_weights(pb.seg_start, pb.times)
    e1 = capi.Engine(pb)
    info1 = e1.info()
    one = e1.path_speed(par, 5, seed=11, thresholds=thr, weight=w)
    e1.close()
    e2 = capi.Engine(pb, devices=[0, 0])
    info2 = e2.info()
    _show(f"shards {layout}", info2)
    two = e2.path_speed(par, 5, seed=11, thresholds=thr, weight=w)
    two_b = _raw(e2, par, 5, thr, w, stats=False)
    e2.close()
    assert info2["n_devices"] == 2 and info1["n_devices"] <= 1 and info2["n_tracks"] == info1["n_tracks"] == pb.n_seg
    if layout == "lattice":
        assert info1["n_rows_tiled"] > pb.n and info2["n_rows_tiled"] > pb.n
    if layout == "tv":
        assert info1["path"] == PATH_TV and info2["path"] == PATH_TV
    assert np.any(np.isfinite(one[0])) and np.any(one[1][:, 0] > 0) and _same(one, two) and np.array_equal(two_b[1], one[1])


# ---- isolation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["const", "tv"])
def test_a_path_speed_call_leaves_every_other_result_as_it_was(layout, monkeypatch):
    if layout == "tv":
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = _tv_spec(29)
    else:
        spec = _const_spec(2, "missing")
    pb = problem_from_spec(spec)
    par = np.array(spec["par"], dtype=np.float64)
    par_b = par.copy(); par_b[1] += 0.01
    thr, w = np.array([0.3, np.inf, 1.1]), dt_weights(pb.seg_start, pb.times)
    rows, offs = np.array([1, 7, 30, 31, pb.n - 1]), np.array([0.0, 0.1, 0.2, 0.05, 1.5])
    eng = capi.Engine(pb)
    va, ga = eng.eval(par, order=1)
    sm = eng.smooth(par)
    dr = eng.smooth_draws(par, 5, seed=11)
    pr = eng.predict(par, rows, offs)
    ps = eng.path_stats(par, 5, seed=11, weight=w)
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.path_speed(par, 5, seed=11, thresholds=thr, weight=w)
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
    ps2 = eng.path_stats(par, 5, seed=11, weight=w)
    eng.close()
    for k in ("mean", "cov", "resid"):
        assert np.array_equal(sm[k], sm2[k], equal_nan=True), k
    assert np.array_equal(dr, dr2, equal_nan=True) and np.array_equal(ps, ps2, equal_nan=True)
    for k in ("mean", "cov"):
        assert np.array_equal(pr[k], pr2[k], equal_nan=True), k


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_unserved_models_and_bad_arguments():
    for sp in (make_spec("gs_ou", "OU", 1, seed=201, lengths=[9, 2, 14]), eseal_spec("gs_eseal", 211, [14, 9, 11]),
               make_spec("gs_oussm", "OU_SSM", 2, seed=5, lengths=LENGTHS70[:14]), make_spec("gs_bmssm", "BM_SSM", 1, seed=6, lengths=LENGTHS70[:14]),
               make_spec("gs_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70[:14], na_rows=(2, 19)),
               make_spec("gs_coupled3", "CTCRW", 3, seed=33, lengths=LENGTHS70[:14], with_H=True, na_rows=(2, 19))):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.path_speed(sp["par"], 5, thresholds=[1.0])
        eng.close()
        assert ei.value.status == ERR_MODEL, sp["name"]
    spec = _const_spec(2, "regular")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    for kw in (dict(n_draws=0), dict(n_draws=1, draw0=-1), dict(n_draws=2, draw0=(1 << 28) - 2),
               dict(n_draws=1, thresholds=[1.0] * 9), dict(n_draws=1, thresholds=[1.0, np.nan]), dict(n_draws=1, thresholds=[-1e-300]),
               dict(n_draws=1, thresholds=[-np.inf])):
        with pytest.raises(capi.EngineError) as ei:
            eng.path_speed(spec["par"], **kw)
        assert ei.value.status == ERR_ARG, kw
    # what the Python layer cannot send: NULL pointers, a negative threshold count, thresholds without a table, counts without a
    # threshold, a flag
    par = np.ascontiguousarray(spec["par"], dtype=np.float64)
    out, cnt, thr = np.zeros((1, 6, pb.n_seg)), np.zeros((1, pb.n), dtype=np.uint32), np.array([np.inf])
    P, O, B, T = par.ctypes.data_as(_dp), out.ctypes.data_as(_dp), cnt.ctypes.data_as(_up), thr.ctypes.data_as(_dp)
    call = lambda p, t, n_thr, stats, below, flags: eng.lib.ssde_path_speed(eng._h, p, eng.n_par_full, 0, 0, 1, t, n_thr, None, stats, below, flags)
    assert call(None, T, 1, O, B, 0) == ERR_ARG and call(P, T, 1, None, None, 0) == ERR_ARG
    assert call(P, None, 1, O, B, 0) == ERR_ARG and call(P, T, -1, O, B, 0) == ERR_ARG and call(P, T, 1, O, B, 1) == ERR_ARG
    assert call(P, T, 0, O, B, 0) == ERR_ARG and call(P, None, 0, None, B, 0) == ERR_ARG
    assert eng.lib.ssde_path_speed(None, P, eng.n_par_full, 0, 0, 1, T, 1, None, O, B, 0) == ERR_ARG
    assert call(P, T, 1, O, B, 0) == 0 and np.isfinite(out[0][:, np.array(LENGTHS70) > 1]).all()
    assert call(P, T, 1, O, None, 0) == 0 and call(P, T, 1, None, B, 0) == 0 and call(P, None, 0, O, None, 0) == 0
    # the last draw number there is; +inf counts every state row of every draw (0 on first rows), 0 none
    last, below = eng.path_speed(spec["par"], 3, draw0=(1 << 28) - 4, thresholds=[np.inf, 0.0])
    eng.close()
    state = np.array(LENGTHS70) - 1.0
    has = state_rows(pb.seg_start, pb.n)
    assert np.array_equal(last[0, :, 5], np.where(state > 0, state, np.nan), equal_nan=True)
    assert np.array_equal(last[0, :, 6], np.where(state > 0, 0.0, np.nan), equal_nan=True)
    assert np.array_equal(below[:, 0], np.where(has, 3, 0)) and np.all(below[:, 1] == 0) and np.array_equal(cnt[0], np.where(has, 1, 0))


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def _sde():
    from smoothsde_amd.sde import SDE
    rng = np.random.default_rng(61)
    ID, times, obs = _tracks(rng, "CTCRW", 2, LENGTHS70, irregular=True)
    n = len(ID)
    obs[[5, 19]] = np.nan
    data = {"ID": ID, "time": times, "x": np.clip((np.sin(np.linspace(0, 7, n)) + 1) / 2, 0, 1), "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~x", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.05, -0.05, 0.3, 0.4, 0.1])
    return sde, times


def test_sde_speed_summary_on_a_ctcrw_with_tau_smooth_in_x():
    sde, times = _sde()
    sde.setup()
    par = sde._current_par_full()
    pb = sde.problem_
    ref_draws = draws_ref(pb, par, seed=SEEDS["sde"], n_draws=3)
    thr = _thresholds(pb, ref_draws, 8, "SDE tau ~ x")[:4]
    got = sde.speed_summary(3, seed=SEEDS["sde"], thresholds=thr)
    w = dt_weights(pb.seg_start, times)
    direct = sde.engine_.path_speed(par, 3, seed=SEEDS["sde"], thresholds=thr, weight=w)
    info = sde.engine_.info()
    _show("SDE tau ~ x", info)
    assert info["const_coeff"] == 0 and info["path"] == PATH_TV
    has = state_rows(pb.seg_start, pb.n)
    wsum = np.add.reduceat(np.where(has, w, 0.0), np.asarray(pb.seg_start))
    assert got["mean_speed"].shape == (3, 70) and got["time_below"].shape == (3, 70, 4) and got["p_below"].shape == (pb.n, 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(got["mean_speed"], direct[0][:, :, 0] / wsum, equal_nan=True)
        assert np.array_equal(got["persistence"], np.hypot(direct[0][:, :, 3], direct[0][:, :, 4]) / wsum, equal_nan=True)
    assert np.array_equal(got["max_speed"], direct[0][:, :, 1], equal_nan=True) and np.array_equal(got["max_row"], direct[0][:, :, 2], equal_nan=True)
    assert np.array_equal(got["time_below"], direct[0][:, :, 5:], equal_nan=True)
    assert np.all(np.isnan(got["p_below"][~has])) and np.array_equal(got["p_below"][has], direct[1][has] / 3.0)
    ok = ~np.isnan(got["persistence"])
    assert np.all(got["persistence"][ok] <= 1.0 + 1e-12) and np.all(got["mean_speed"][ok] <= got["max_speed"][ok] * (1.0 + 1e-12))
    compare(direct, speed_ref(ref_draws, pb.seg_start, 2, thresholds=thr, weight=w), "SDE tau ~ x")
    rows = sde.speed_summary(3, seed=SEEDS["sde"], thresholds=thr, weight=None)["time_below"]
    assert np.array_equal(rows, sde.engine_.path_speed(par, 3, seed=SEEDS["sde"], thresholds=thr)[0][:, :, 5:], equal_nan=True)
    from smoothsde_amd.sde import SDE
    rng = np.random.default_rng(3)
    ID, t2, obs = _tracks(rng, "OU_SSM", 1, [12, 9], irregular=False)
    ou = SDE(data={"ID": ID, "time": t2, "z": obs[:, 0]}, type="OU_SSM", response="z")
    ou.setup()
    with pytest.raises(capi.EngineError) as ei:
        ou.speed_summary(2)
    assert ei.value.status == ERR_MODEL
