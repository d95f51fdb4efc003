"""GPU suite (-m gpu): ssde_path_occupancy_fine on every handle layout it serves.  Every comparison is BITWISE.

Unless noted, each case checks the call two ways: `occ` and `outside` equal the definition (tests/occ_fine_ref.py) on the numpy
reference draws (draws_ref at the rows, bridge_ref.predict_draws_ref at the inner points of rule 2) after the assertion that no
reference point is within 1e-6 of a cell line (occ_cases.py); and they equal the definition on the handle's OWN ssde_smooth_draws and
ssde_predict_draws at rule 2's offsets.  Each case also checks conservation in whole quanta, the kernel form and
ssde_last_occupancy_points against the definition's plan.  max_step is 0.4 of the median interior interval unless said otherwise (m up
to 5 on the irregular grids, 3 on the regular ones); shapes are test_gpu_occ.py's: about a thousand rows and five draws."""
import ctypes as C
import warnings

import numpy as np
import pytest

from cases import _tracks, eseal_spec, make_spec, problem_from_spec
from occ_cases import clear_of_lines, make_grid
from occ_fine_ref import all_points, fine_plan, occ_fine_counts, reference_draws, to_float
from occ_ref import grid_of, quantise
from path_cases import dt_weights
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS70 = [20, 35, 1, 14, 2, 27, 9] * 10
ERR_ARG, ERR_MODEL = 1, 2
TILE, GLOBAL, BOTH = 1, 2, 3
FINE_DRAWS, TILE_CELLS, MAX_SUB = 8, 8192, 64             # csrc/ssde_device.hpp: OCC_FINE_DRAWS, OCC_TILE_CELLS; ssde.h: SSDE_OCC_MAX_SUB
_REF = {}


def _max_step(pb, factor=0.4):
    """factor x the median interval between two state rows of a track"""
    b = np.r_[pb.seg_start, pb.n]
    inner = np.concatenate([np.arange(b[t] + 1, b[t + 1] - 1) for t in range(len(b) - 1)])
    return factor * float(np.median(np.diff(pb.times)[inner]))


def _ref(key, pb, par, max_step, is_row=None, **kw):
    """the definition's plan and the reference draws of a case, computed once and left unchanged"""
    if key not in _REF:
        plan = fine_plan(pb.times, pb.seg_start, max_step, is_row=is_row)
        rows, inner = reference_draws(pb, par, plan, **kw)
        rows.setflags(write=False); inner.setflags(write=False)
        _REF[key] = (plan, rows, inner)
    return _REF[key]


def _show(tag, info, **more):
    keys = ("path", "kernel_id", "const_coeff", "uniform_dt", "n_rows", "n_rows_tiled", "n_groups", "n_devices", "n_tracks", "sdim")
    print("LAYOUT", tag, {k: info[k] for k in keys}, more)


def _const_spec(model, d, what, seed=3, lengths=LENGTHS70):
    na = (5, 19, 40, 41, sum(lengths) - 1) if what == "missing" else ()
    return make_spec(f"gf_{model}_{d}_{what}_{len(lengths)}", model, d, seed=seed + d, lengths=lengths, irregular=(what == "irregular"), na_rows=na)


def _same(got, ref, tag):
    assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape, tag
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), tag


def _definition(plan, rows, inner, pb, grid, w, group, n_groups, n_rows=None):
    """the definition on a provider's draws, after its conservation in whole quanta: (occ, outside)"""
    occ, out, e = occ_fine_counts(rows, inner, plan, pb.seg_start, pb.model, pb.n_dim, grid, weight=w, group=group, n_groups=n_groups,
                                  n_rows=n_rows)
    state = plan["owner"] == np.arange(pb.n)
    wq = quantise(np.ones(pb.n) if w is None else w, e)
    seg_of = np.searchsorted(np.r_[pb.seg_start, pb.n], np.arange(pb.n), side="right") - 1
    for g in range(n_groups):
        mine = state & ((np.zeros(pb.n, dtype=int) if group is None else np.asarray(group)[seg_of]) == g)
        assert int(occ[g].sum()) + int(out[g]) == rows.shape[0] * int(wq[mine].sum(dtype=np.uint64)), ("conservation", g)
    return to_float(occ, out, e)


def _check(eng, pb, par, obs, tag, form, key, max_step=None, n_draws=5, seed=11, draw0=0, cells=(16, 12), grid=None, group=None,
           n_groups=1, force_global=False, own=True):
    """path_occupancy_fine against the definition on the reference draws and (own) on the handle's own draws"""
    model, d = pb.model, pb.n_dim
    max_step = _max_step(pb) if max_step is None else max_step
    plan, rows, inner = _ref((key, max_step, seed, draw0, n_draws), pb, par, max_step, seed=seed, draw0=draw0, n_draws=n_draws)
    pts = all_points(rows, inner)
    if grid is None:
        grid, _ = make_grid(obs, pts, model, d, cells=cells)
    assert clear_of_lines(pts, model, d, grid), tag                               # a condition on the inputs
    w = dt_weights(pb.seg_start, pb.times)
    got = eng.path_occupancy_fine(par, n_draws, grid, max_step, seed=seed, draw0=draw0, weight=w, group=group, n_groups=n_groups,
                                  force_global=force_global)
    assert form is None or eng.last_occupancy_form() == form, (tag, eng.last_occupancy_form())
    assert got[0].shape == (n_groups, grid["ny"] if d == 2 else 1, grid["nx"]) and got[1].shape == (n_groups,)
    gplan = plan if group is None else fine_plan(pb.times, pb.seg_start, max_step, group=group)
    assert eng.last_occupancy_points() == (gplan["n_points"], gplan["n_capped"]), (tag, eng.last_occupancy_points())
    _same(got, _definition(plan, rows, inner, pb, grid, w, group, n_groups), f"{tag} | reference")
    if own:
        own_rows = eng.smooth_draws(par, n_draws, seed=seed, draw0=draw0)
        own_inner = eng.predict_draws(par, plan["q_rows"], plan["q_offs"], n_draws, seed=seed, draw0=draw0)
        _same(got, _definition(plan, own_rows, own_inner, pb, grid, w, group, n_groups), f"{tag} | own draws")
    print(f"OCCFINE {tag}: max m {plan['m'].max()} points {plan['n_points']} inside {got[0].sum():.6g} outside {got[1].sum():.6g}")
    return got, grid


def _lane_order(lengths):
    return np.argsort(-np.asarray(lengths), kind="stable")


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
    (occ, out), _ = _check(eng, pb, spec["par"], spec["obs"], f"const {model} d={d} {what}", TILE, ("const", model, d, what))
    eng.close()
    assert np.any(occ > 0) and out[0] > 0


@pytest.mark.parametrize("n_tracks", [65, 130])
def test_65_and_130_tracks_with_both_forms_in_one_call(n_tracks):
    lengths = ([20, 35, 14, 3, 27, 9] * 11)[:65] if n_tracks == 65 else (LENGTHS70 * 2)[:n_tracks]
    spec = _const_spec("CTCRW", 2, "irregular", seed=4, lengths=lengths)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"{n_tracks} tracks", info)
    assert info["path"] == PATH_ISO and info["n_tracks"] == n_tracks and info["n_groups"] == (n_tracks + 63) // 64
    order = _lane_order(lengths)
    group = np.zeros(n_tracks, dtype=np.int32)
    if n_tracks == 65:
        group[order[:64]] = np.arange(64) % 2
        group[order[64]] = 2
    else:
        group[order[64:]] = 1 + np.arange(n_tracks - 64) % 2                       # first wavefront pooled, the rest alternating
        group[order[70]] = -1                                                      # and one track left out
    key = ("tracks", n_tracks)
    res, grid = _check(eng, pb, spec["par"], spec["obs"], f"{n_tracks} tracks", BOTH, key, group=group, n_groups=3)
    assert np.all(res[0].sum(axis=(1, 2)) > 0)
    # tile form = global form, pooled and grouped
    pooled = _check(eng, pb, spec["par"], spec["obs"], "pooled", TILE, key, grid=grid, own=False)[0]
    forced = _check(eng, pb, spec["par"], spec["obs"], "pooled, forced global", GLOBAL, key, grid=grid, force_global=True, own=False)[0]
    _same(forced, pooled, "both forms")
    forced3 = _check(eng, pb, spec["par"], spec["obs"], "grouped, forced global", GLOBAL, key, grid=grid, group=group, n_groups=3,
                     force_global=True, own=False)[0]
    eng.close()
    _same(forced3, res, "both forms, grouped")


def _stepped(model, d, pattern, lengths, seed):
    """tracks whose intervals cycle through `pattern`"""
    spec = make_spec(f"gf_step_{model}_{d}", model, d, seed=seed, lengths=lengths, irregular=False)
    t, k = np.array(spec["times"], dtype=np.float64), 0
    b = np.r_[0, np.cumsum(lengths)]
    for a, z in zip(b[:-1], b[1:]):
        dts = np.array([pattern[(k + i) % len(pattern)] for i in range(z - a)])
        t[a:z] = (0.0 if a == 0 else t[a - 1] + 5.0) + np.cumsum(dts)
        k += 1
    spec["times"] = t
    return spec


def test_m_mixed_over_1_to_5_in_one_wave():
    # neighbouring lanes start the pattern one entry apart, so every step of the wave holds all five m
    spec = _stepped("CTCRW", 2, [0.5, 1.5, 2.5, 3.5, 4.5], [12, 17, 9, 14] * 9, seed=13)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    (occ, out), _ = _check(eng, pb, spec["par"], spec["obs"], "m 1 .. 5", TILE, "mixed", max_step=1.0)
    eng.close()
    plan = _REF[("mixed", 1.0, 11, 0, 5)][0]
    assert sorted(set(plan["m"][plan["m"] > 0])) == [1, 2, 3, 4, 5]


def test_one_interval_at_the_cap():
    spec = _stepped("OU_SSM", 2, [1.0], [12, 17, 9, 14] * 3, seed=14)
    t = np.array(spec["times"]); t[20:] += 99.0                                    # row 19 -> 20, inside the second track: 100 x max_step
    spec["times"] = t
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    _check(eng, pb, spec["par"], spec["obs"], "the cap", TILE, "cap", max_step=1.0)
    assert eng.last_occupancy_points()[1] == 1
    plan = _REF[("cap", 1.0, 11, 0, 5)][0]
    assert plan["m"].max() == MAX_SUB and plan["n_capped"] == 1
    eng.close()


@pytest.mark.parametrize("force_global", [False, True])
def test_an_infinite_max_step_is_path_occupancy(force_global):
    spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    w = dt_weights(pb.seg_start, pb.times)
    q = np.nanquantile(spec["obs"], [.02, .98], axis=0)
    grid = grid_of(q[0, 0], (q[1, 0] - q[0, 0]) / 16, 16, q[0, 1], (q[1, 1] - q[0, 1]) / 12, 12)
    group = (np.arange(70) % 3 - (np.arange(70) % 11 == 0)).clip(-1).astype(np.int32)
    eng = capi.Engine(pb)
    for kw in (dict(), dict(group=group, n_groups=3), dict(weight=None)):
        kw = dict(dict(weight=w), **kw)
        old = eng.path_occupancy(spec["par"], 5, grid, seed=11, force_global=force_global, **kw)
        form = eng.last_occupancy_form()
        new = eng.path_occupancy_fine(spec["par"], 5, grid, np.inf, seed=11, force_global=force_global, **kw)
        assert eng.last_occupancy_form() == form
        _same(new, old, f"max_step = inf {sorted(kw)}")
        huge = eng.path_occupancy_fine(spec["par"], 5, grid, 1e9, seed=11, force_global=force_global, **kw)
        _same(huge, old, "every m = 1")
    assert eng.last_occupancy_points() == (pb.n - 70, 0)
    eng.close()


def test_the_lds_tile_cap():
    spec = _const_spec("CTCRW", 2, "irregular")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    key = ("const", "CTCRW", 2, "irregular")
    at = _check(eng, pb, spec["par"], spec["obs"], "at the cap", TILE, key, cells=(128, 64), own=False)[0]
    past = _check(eng, pb, spec["par"], spec["obs"], "one cell past the cap", GLOBAL, key, cells=(2731, 3), own=False)[0]
    eng.close()
    assert 128 * 64 == TILE_CELLS and 2731 * 3 == TILE_CELLS + 1


@pytest.mark.parametrize("n_draws", [1, 4, 5, FINE_DRAWS + 1])
@pytest.mark.parametrize("force_global", [False, True])
def test_draw_counts(n_draws, force_global):
    spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    _check(eng, pb, spec["par"], spec["obs"], f"{n_draws} draws", GLOBAL if force_global else TILE, ("draws", "CTCRW"), n_draws=n_draws,
           force_global=force_global, own=not force_global)
    eng.close()


def test_a_non_zero_draw0():
    spec = _const_spec("OU_SSM", 2, "missing")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    _check(eng, pb, spec["par"], spec["obs"], "draw0 = 3", TILE, ("draw0", "OU_SSM"), n_draws=6, seed=7, draw0=3)
    eng.close()


# ---- other layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_force_dense(model):
    spec = _const_spec(model, 2, "missing")
    pb = problem_from_spec(spec, flags=capi.FLAG_FORCE_DENSE)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"dense {model}", info)
    assert info["path"] == PATH_DENSE and info["n_groups"] == 2
    _check(eng, pb, spec["par"], spec["obs"], f"dense {model}", TILE, ("const", model, 2, "missing"))
    eng.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    spec = make_spec(f"gf_hp_{model}_{d}", model, d, seed=21, lengths=LENGTHS70, with_H=True, with_P0=True, na_rows=(3, 19, 40, 41))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"H P0 {model} d={d}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_tracks"] == 70
    _check(eng, pb, spec["par"], spec["obs"], f"H P0 {model} d={d}", TILE, ("hp", model, d))
    eng.close()


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
    key = ("tv", model)
    got, grid = _check(eng, pb, spec["par"], spec["obs"], f"tv {model}", TILE, key)
    grp = (np.arange(150) % 7).astype(np.int32)
    per = _check(eng, pb, spec["par"], spec["obs"], f"tv {model} seven groups", GLOBAL, key, grid=grid, group=grp, n_groups=7, own=False)[0]
    # 1 MiB of records and side rows: several chunks of groups (test_gpu_smooth_layouts.py)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    w = dt_weights(pb.seg_start, pb.times)
    many = eng.path_occupancy_fine(spec["par"], 5, grid, _max_step(pb), seed=11, weight=w)
    many7 = eng.path_occupancy_fine(spec["par"], 5, grid, _max_step(pb), seed=11, weight=w, group=grp, n_groups=7)
    eng.close()
    _same(many, got, "tv chunks")
    _same(many7, per, "tv chunks, global form")


def _lattice(model):
    from test_gpu_draws import _written_out
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks(model, 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=9, na_frac=0.05)
    pb = capi.Problem(model, ID, times, obs)
    par = _par(model, 2, np.random.default_rng(2))
    ID2, t2, obs2, rows = _written_out(ID, times, obs, 0.5)
    pb2 = capi.Problem(model, ID2, t2, obs2)
    return pb, par, obs, pb2, rows


def _lattice_reference(model, pb, par, obs, pb2, rows, max_step, group=None, n_groups=1):
    """the definition on the written-out lattice (the handle's resident rows) with the caller's rows flagged: weight spreads over the
    L_j lattice slots of a gap of several steps, the padded rows' own points included"""
    is_row = np.zeros(pb2.n, dtype=bool)
    is_row[rows] = True
    plan, prow, inner = _ref(("lattice", model, max_step), pb2, par, max_step, is_row=is_row, seed=11, n_draws=5)
    pts = all_points(prow, inner)
    grid, _ = make_grid(obs, pts, model, 2)
    assert clear_of_lines(pts, model, 2, grid)
    w2 = np.zeros(pb2.n)
    w2[rows] = dt_weights(pb.seg_start, pb.times)
    gplan = plan if group is None else fine_plan(pb2.times, pb2.seg_start, max_step, is_row=is_row, group=group)
    occ, out, e = occ_fine_counts(prow, inner, plan, pb2.seg_start, model, 2, grid, weight=w2, group=group, n_groups=n_groups, n_rows=pb.n)
    return grid, to_float(occ, out, e), plan, (gplan["n_points"], gplan["n_capped"])


@pytest.mark.parametrize("model", MODELS)
def test_a_lattice_handle_spreads_a_gap_over_its_lattice_slots(model):
    pb, par, obs, pb2, rows = _lattice(model)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"lattice {model}", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] > pb.n
    assert pb2.n == info["n_rows_tiled"] and pb2.n_seg == pb.n_seg                 # the written-out rows ARE the handle's lattice
    assert pb2.n - pb.n > 50                                                       # absent fixes: gaps of several lattice steps
    grid, ref, plan, counts = _lattice_reference(model, pb, par, obs, pb2, rows, 0.2)
    w = dt_weights(pb.seg_start, pb.times)
    got = eng.path_occupancy_fine(par, 5, grid, 0.2, seed=11, weight=w)
    assert eng.last_occupancy_form() == TILE and eng.last_occupancy_points() == counts
    _same(got, ref, f"lattice {model}")
    assert plan["m"].max() == 3                                                    # the lattice step, not the caller's interval
    # every m = 1: the points are the lattice rows, padded ones included, and a gap's weight is shared among them
    grid1, ref1, _, counts1 = _lattice_reference(model, pb, par, obs, pb2, rows, 10.0)
    got1 = eng.path_occupancy_fine(par, 5, grid1, 10.0, seed=11, weight=w)
    assert eng.last_occupancy_points() == counts1 and counts1[0] == pb2.n - pb2.n_seg
    _same(got1, ref1, f"lattice {model}, m = 1")
    eng.close()


def test_negative_p0_points_without_a_position_land_outside():
    # the det F <= 0 corner of §3.9, d = 1: whatever pivots fail, fail alike on both sides.  Not every model meets the corner on this
    # shape (test_occ_fine_hostsim.py counts the same way), so the three share one test that asserts it IS met
    from smoothsde_amd.synth import simulate
    seen = 0
    for model in MODELS:
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
        (occ, out), _ = _check(eng, pb, par, obs, f"negative P0 {model}", TILE, ("negp0", model), cells=(16, 1))
        eng.close()
        plan, rows, inner = _REF[(("negp0", model), _max_step(pb), 11, 0, 5)]
        # the points of the reference without a position, per point over the draws, and the quanta the definition gives them
        state = plan["owner"] == np.arange(pb.n)
        nan_inner = np.count_nonzero(~np.isfinite(inner[:, :, 0]), axis=0)
        nan_rows = np.count_nonzero(~np.isfinite(rows[:, :, 0]), axis=0) * state
        w = dt_weights(pb.seg_start, pb.times)
        e = int(np.frexp(w.max())[1]) + (pb.n * 5).bit_length() - 52                 # (above the -1074 floor)
        share = quantise(w, e).astype(object) // plan["m"].clip(1).astype(object)
        lost = sum(int(share[plan["q_rows"][k]]) * int(c) for k, c in enumerate(nan_inner) if c) + \
            sum(int(share[j]) * int(nan_rows[j]) for j in np.flatnonzero(nan_rows))
        print(f"negative P0 {model}: {nan_inner.sum()} inner and {nan_rows.sum()} row points without a position, {lost} quanta")
        assert out[0] >= np.ldexp(float(lost), e)                                   # at least their shares are outside
        seen += int(nan_inner.sum() > 0) + int(nan_rows.sum() > 0)
    assert seen >= 2                                                                # the corner is met, at rows AND inside intervals


# ---- invariance, all bitwise ------------------------------------------------------------------------------------------------------
def test_budget_chunks_on_six_ragged_groups_are_bitwise():
    rng = np.random.default_rng(31)
    lengths = np.r_[rng.integers(71, 90, 64), rng.integers(45, 61, 63), [60], rng.integers(10, 16, 64), rng.integers(3, 8, 64),
                    rng.integers(2, 4, 64), [1, 2, 5, 1, 3]]
    lengths = [int(v) for v in rng.permutation(lengths)]
    starts = np.r_[0, np.cumsum(lengths)]
    k5 = next(k for k, L in enumerate(lengths) if L >= 5)
    spec = make_spec("gf_chunks", "CTCRW", 2, seed=31, lengths=lengths, irregular=True,
                     na_rows=(int(starts[k5]) + 2, int(starts[k5]) + 3, int(starts[k5 + 1]) - 1))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show("chunks ragged", info)
    assert info["path"] == PATH_ISO and info["n_groups"] == 6 and pb.n_seg == 325
    w = dt_weights(pb.seg_start, pb.times)
    q = np.nanquantile(spec["obs"], [.02, .98], axis=0)
    grid = grid_of(q[0, 0], (q[1, 0] - q[0, 0]) / 16, 16, q[0, 1], (q[1, 1] - q[0, 1]) / 12, 12)
    group = (np.arange(325) % 3).astype(np.int32)
    ms = _max_step(pb)
    one = eng.path_occupancy_fine(spec["par"], 13, grid, ms, seed=11, weight=w)
    pts = eng.last_occupancy_points()
    mixed = eng.path_occupancy_fine(spec["par"], 13, grid, ms, seed=11, weight=w, group=group, n_groups=3)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)                                   # several chunks, and batches of a few draws
    one_c = eng.path_occupancy_fine(spec["par"], 13, grid, ms, seed=11, weight=w)
    assert eng.last_occupancy_points() == pts
    mixed_c = eng.path_occupancy_fine(spec["par"], 13, grid, ms, seed=11, weight=w, group=group, n_groups=3)
    eng.close()
    assert one[0].sum() > 0
    _same(one_c, one, "chunks")
    _same(mixed_c, mixed, "chunks, global form")


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
    w = dt_weights(pb.seg_start, pb.times)
    q = np.nanquantile(obs, [.02, .98], axis=0)
    grid = grid_of(q[0, 0], (q[1, 0] - q[0, 0]) / 16, 16, q[0, 1], (q[1, 1] - q[0, 1]) / 12, 12)
    group = np.arange(pb.n_seg) % 3 - (np.arange(pb.n_seg) % 11 == 0) * 1
    group = np.maximum(group, -1).astype(np.int32)
    ms = 0.2 if layout == "lattice" else _max_step(pb)
    out = {}
    for devices in (None, [0, 0]):
        eng = capi.Engine(pb) if devices is None else capi.Engine(pb, devices=devices)
        info = eng.info()
        _show(f"shards {layout} {devices}", info)
        pooled = eng.path_occupancy_fine(par, 5, grid, ms, seed=11, weight=w)
        form_p, pts_p = eng.last_occupancy_form(), eng.last_occupancy_points()
        grouped = eng.path_occupancy_fine(par, 5, grid, ms, seed=11, weight=w, group=group, n_groups=3)
        out[devices is None] = (info, pooled, grouped, form_p, eng.last_occupancy_form(), pts_p, eng.last_occupancy_points())
        eng.close()
    (info1, p1, g1, fp1, fg1, pp1, pg1), (info2, p2, g2, fp2, fg2, pp2, pg2) = out[True], out[False]
    assert info2["n_devices"] == 2 and info1["n_devices"] <= 1 and info2["n_tracks"] == info1["n_tracks"] == pb.n_seg
    assert fp1 == TILE and fp2 == TILE and fg1 == GLOBAL and fg2 == GLOBAL
    assert pp1 == pp2 and pg1 == pg2 and pp1[0] > pg1[0] > 0                       # the shards' counts add up
    assert p1[0].sum() > 0
    _same(p2, p1, f"shards {layout} pooled")
    _same(g2, g1, f"shards {layout} grouped")


def test_repeated_calls_and_draw_ranges():
    spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    w = dt_weights(pb.seg_start, pb.times)
    q = np.nanquantile(spec["obs"], [.02, .98], axis=0)
    grid = grid_of(q[0, 0], (q[1, 0] - q[0, 0]) / 16, 16, q[0, 1], (q[1, 1] - q[0, 1]) / 12, 12)
    ms = _max_step(pb)
    eng = capi.Engine(pb)
    first = eng.path_occupancy_fine(spec["par"], 8, grid, ms, seed=5, weight=w)
    _same(eng.path_occupancy_fine(spec["par"], 8, grid, ms, seed=5, weight=w), first, "two identical calls")
    # draws [0, 8) = [0, 4) + [4, 8), bitwise where every point's share is a whole number of both calls' quanta: w_j = N_j
    plan = fine_plan(pb.times, pb.seg_start, ms)
    wn = plan["m"].astype(np.float64)
    whole = eng.path_occupancy_fine(spec["par"], 8, grid, ms, seed=5, weight=wn)
    a = eng.path_occupancy_fine(spec["par"], 4, grid, ms, seed=5, draw0=0, weight=wn)
    b = eng.path_occupancy_fine(spec["par"], 4, grid, ms, seed=5, draw0=4, weight=wn)
    other = eng.path_occupancy_fine(spec["par"], 8, grid, ms, seed=6, weight=wn)
    eng.close()
    assert np.array_equal(whole[0], a[0] + b[0]) and np.array_equal(whole[1], a[1] + b[1])
    assert whole[0].sum() + whole[1].sum() == 8 * plan["n_points"]                  # every point of every draw, once
    assert not np.array_equal(other[0], whole[0])


# ---- isolation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["const", "tv"])
def test_a_call_leaves_every_other_result_as_it_was(layout, monkeypatch):
    from path_cases import make_regions
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
    q = np.nanquantile(spec["obs"], [.02, .98], axis=0)
    grid = grid_of(q[0, 0], (q[1, 0] - q[0, 0]) / 16, 16, q[0, 1], (q[1, 1] - q[0, 1]) / 12, 12)
    rows, offs = np.array([1, 7, 30, 31, pb.n - 1]), np.array([0.0, 0.1, 0.2, 0.05, 1.5])
    eng = capi.Engine(pb)
    va, ga = eng.eval(par, order=1)
    sm = eng.smooth(par)
    dr = eng.smooth_draws(par, 5, seed=11)
    pr = eng.predict(par, rows, offs)
    pd = eng.predict_draws(par, rows, offs, 5, seed=11)
    ps = eng.path_stats(par, 5, seed=11, regions=reg, weight=w)
    oc = eng.path_occupancy(par, 5, grid, seed=11, weight=w)
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.path_occupancy_fine(par, 5, grid, _max_step(pb), seed=11, weight=w)
    eng.path_occupancy_fine(par, 5, grid, _max_step(pb), seed=11, weight=w, group=np.arange(pb.n_seg) % 2, n_groups=2)
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
    pd2 = eng.predict_draws(par, rows, offs, 5, seed=11)
    ps2 = eng.path_stats(par, 5, seed=11, regions=reg, weight=w)
    oc2 = eng.path_occupancy(par, 5, grid, seed=11, weight=w)
    eng.close()
    for k in ("mean", "cov", "resid"):
        assert np.array_equal(sm[k], sm2[k], equal_nan=True), k
    assert np.array_equal(dr, dr2, equal_nan=True) and np.array_equal(ps, ps2, equal_nan=True) and np.array_equal(pd, pd2, equal_nan=True)
    for k in ("mean", "cov"):
        assert np.array_equal(pr[k], pr2[k], equal_nan=True), k
    _same(oc2, oc, "path_occupancy")


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_unserved_models_and_bad_arguments():
    g1, g2 = grid_of(0.0, 1.0, 4), grid_of(0.0, 1.0, 4, 0.0, 1.0, 3)
    for sp, g in ((make_spec("gf_ou", "OU", 1, seed=201, lengths=[9, 2, 14]), g1), (eseal_spec("gf_eseal", 211, [14, 9, 11]), g1),
                  (make_spec("gf_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70[:14], na_rows=(2, 19)), g2),
                  (make_spec("gf_coupled3", "CTCRW", 3, seed=33, lengths=LENGTHS70[:14], with_H=True, na_rows=(2, 19)), g2)):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.path_occupancy_fine(sp["par"], 5, g, 0.5)
        eng.close()
        assert ei.value.status == ERR_MODEL, sp["name"]
    spec = _const_spec("CTCRW", 2, "regular")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    ok = dict(n_draws=1, grid=g2, max_step=0.5)
    wbad = lambda v: np.r_[v, np.ones(pb.n - 1)]
    gbad = lambda v: np.r_[v, np.zeros(pb.n_seg - 1)].astype(np.int32)
    bad = [dict(n_draws=0), dict(draw0=-1), dict(n_draws=2, draw0=(1 << 28) - 2),
           dict(grid=dict(g2, nx=0)), dict(grid=dict(g2, nx=4097)), dict(grid=dict(g2, ny=0)), dict(grid=dict(g2, ny=4097)),
           dict(grid=dict(g2, dx=0.0)), dict(grid=dict(g2, dx=-1.0)), dict(grid=dict(g2, dx=np.inf)), dict(grid=dict(g2, dx=np.nan)),
           dict(grid=dict(g2, dy=0.0)), dict(grid=dict(g2, dy=np.nan)), dict(grid=dict(g2, x0=np.inf)), dict(grid=dict(g2, x0=np.nan)),
           dict(grid=dict(g2, y0=-np.inf)), dict(n_groups=0), dict(n_groups=2), dict(grid=dict(g2, nx=4096, ny=4096), group=gbad(0), n_groups=17),
           dict(group=gbad(-2), n_groups=1), dict(group=gbad(1), n_groups=1), dict(group=gbad(3), n_groups=3),
           dict(weight=wbad(-1e-300)), dict(weight=wbad(np.nan)), dict(weight=wbad(np.inf)),
           dict(max_step=0.0), dict(max_step=-1.0), dict(max_step=np.nan), dict(max_step=-np.inf)]
    for kw in bad:
        with pytest.raises(capi.EngineError) as ei:
            eng.path_occupancy_fine(spec["par"], **dict(ok, **kw))
        assert ei.value.status == ERR_ARG, kw
    assert eng.last_occupancy_form() == 0 and eng.last_occupancy_points() == (0, 0)     # nothing ran
    # what the Python layer cannot send: NULL pointers, an unknown flag
    dp = C.POINTER(C.c_double)
    par = np.ascontiguousarray(spec["par"], dtype=np.float64)
    occ, out = np.zeros(12), np.zeros(1)
    G = capi.SsdeOccGrid(0.0, 1.0, 0.0, 1.0, 4, 3)
    P, O, U = par.ctypes.data_as(dp), occ.ctypes.data_as(dp), out.ctypes.data_as(dp)
    call = lambda h, p, g, o, u, flags: eng.lib.ssde_path_occupancy_fine(h, p, eng.n_par_full, 0, 0, 1, g, 0.5, None, None, 1, o, u, flags)
    assert call(None, P, C.byref(G), O, U, 0) == ERR_ARG and call(eng._h, None, C.byref(G), O, U, 0) == ERR_ARG
    assert call(eng._h, P, None, O, U, 0) == ERR_ARG and call(eng._h, P, C.byref(G), None, U, 0) == ERR_ARG
    assert call(eng._h, P, C.byref(G), O, U, 2) == ERR_ARG and call(eng._h, P, C.byref(G), O, U, 3) == ERR_ARG
    assert eng.lib.ssde_last_occupancy_points(None, None, None) == ERR_ARG
    assert call(eng._h, P, C.byref(G), O, None, 0) == 0 and call(eng._h, P, C.byref(G), O, U, 1) == 0    # `outside` may be NULL
    assert eng.lib.ssde_last_occupancy_points(eng._h, None, None) == 0
    state_rows = float(pb.n - 70)
    assert occ.sum() + out[0] == state_rows
    # a grid over the whole plane counts every point's share: with unit weights, the state rows; one far from the data counts none
    everything = eng.path_occupancy_fine(spec["par"], 1, grid_of(-1e6, 2e6, 1, -1e6, 2e6, 1), 0.5, draw0=(1 << 28) - 2)
    nothing = eng.path_occupancy_fine(spec["par"], 3, grid_of(1e7, 1.0, 5, 1e7, 1.0, 5), np.inf)
    eng.close()
    assert everything[0][0, 0, 0] == state_rows and everything[1][0] == 0.0
    assert np.all(nothing[0] == 0.0) and nothing[1][0] == 3 * state_rows
    spec1 = _const_spec("OU_SSM", 1, "regular")
    eng = capi.Engine(problem_from_spec(spec1))
    with pytest.raises(capi.EngineError) as ei:
        eng.path_occupancy_fine(spec1["par"], 1, dict(g1, ny=2), 0.5)
    assert ei.value.status == ERR_ARG
    a = eng.path_occupancy_fine(spec1["par"], 2, dict(g1, x0=2.0, y0=np.nan, dy=-1.0), 0.5)
    b = eng.path_occupancy_fine(spec1["par"], 2, dict(g1, x0=2.0), 0.5)
    eng.close()
    _same(a, b, "d = 1 reads no y")


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_sde_utilisation_with_a_max_step():
    from smoothsde_amd.sde import SDE
    rng = np.random.default_rng(61)
    ID, times, obs = _tracks(rng, "CTCRW", 2, LENGTHS70, irregular=True)
    n = len(ID)
    obs[[5, 19]] = np.nan
    data = {"ID": ID, "time": times, "x": np.clip((np.sin(np.linspace(0, 7, n)) + 1) / 2, 0, 1), "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~x", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.05, -0.05, 0.3, 0.4, 0.1])
    sde.setup()
    pb, par = sde.problem_, sde._current_par_full()
    ms = _max_step(pb)
    plan, rows, inner = _ref("sde", pb, par, ms, seed=2, n_draws=3)
    pts = all_points(rows, inner)
    grid, _ = make_grid(obs, pts, "CTCRW", 2)
    ext = (grid["x0"], grid["x0"] + 16 * grid["dx"], grid["y0"], grid["y0"] + 12 * grid["dy"])
    g2 = grid_of(ext[0], (ext[1] - ext[0]) / 16, 16, ext[2], (ext[3] - ext[2]) / 12, 12)       # the grid utilisation() forms
    assert clear_of_lines(pts, "CTCRW", 2, g2)
    # None takes today's path and returns today's bits
    today = sde.utilisation(3, seed=2, cells=(16, 12), extent=ext)
    again = sde.utilisation(3, seed=2, cells=(16, 12), extent=ext, max_step=None)
    w = dt_weights(pb.seg_start, times)
    old = sde.engine_.path_occupancy(par, 3, g2, seed=2, weight=w)
    assert sorted(today) == ["density", "outside", "x_edges", "y_edges"]
    assert np.array_equal(today["density"], again["density"]) and np.array_equal(today["outside"], again["outside"])
    state_w = w.copy()
    state_w[pb.seg_start] = 0.0
    share = np.add.reduceat(state_w, pb.seg_start)
    total = 3 * np.bincount(np.zeros(70, dtype=np.int64), weights=share)[0]
    assert np.array_equal(today["density"], old[0] / total)
    # a positive number: the refined paths
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*sub-steps.*")
        ud = sde.utilisation(3, seed=2, cells=(16, 12), extent=ext, max_step=ms)
    assert ud["n_points"] == plan["n_points"] and ud["density"].shape == (1, 12, 16)
    assert abs(ud["density"].sum() + ud["outside"][0] - 1.0) <= 1e-12
    ref = _definition(plan, rows, inner, pb, g2, w, None, 1)
    assert np.array_equal(ud["density"], ref[0] / total) and np.array_equal(ud["outside"], ref[1] / total)
    assert not np.array_equal(ud["density"], today["density"])
    by_lab = sde.utilisation(3, seed=2, cells=(16, 12), by=np.arange(70) % 3, max_step=ms)
    assert np.allclose(by_lab["density"].sum(axis=(1, 2)) + by_lab["outside"], 1.0, rtol=0, atol=1e-12)
    with pytest.warns(UserWarning, match="sub-steps"):
        capped = sde.utilisation(3, seed=2, cells=(16, 12), extent=ext, max_step=ms / 200)
    assert abs(capped["density"].sum() + capped["outside"][0] - 1.0) <= 1e-12
