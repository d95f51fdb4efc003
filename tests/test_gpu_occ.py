"""GPU suite (-m gpu): ssde_path_occupancy on every handle layout it serves.

Unless noted, each case checks the call three ways: `occ` and `outside` equal, BITWISE, the definition (tests/occ_ref.py) on the GPU's
OWN draws (ssde_smooth_draws on the same handle, seed and draw0); they equal, bitwise, the definition on the numpy reference draws
(tests/draws_ref.py) after the assertion that no reference position is within 1e-6 of a cell line (occ_cases.py); and info() and
last_occupancy_form() show the layout and the kernel form the case is about.  A few thousand rows and five draws (one full chunk of
DRAW_CH = 4 and one partly filled) unless said otherwise; shapes as test_gpu_path.py."""
import ctypes as C

import numpy as np
import pytest

from cases import _tracks, eseal_spec, make_spec, problem_from_spec
from draws_ref import draws_ref
from occ_cases import clear_of_lines, make_grid
from occ_ref import grid_of, occ_ref
from path_cases import dt_weights
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS70 = [20, 35, 1, 14, 2, 27, 9] * 10
ERR_ARG, ERR_MODEL = 1, 2
TILE, GLOBAL, BOTH = 1, 2, 3
NW, DRAW_CH, TILE_CELLS = 4, 4, 8192                       # csrc/ssde_device.hpp: OCC_NW, DRAW_CH, OCC_TILE_CELLS
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


def _same(got, ref, tag):
    assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape, tag
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), tag


def _check(eng, pb, par, ref_draws, obs, tag, form, n_draws=5, seed=11, draw0=0, cells=(16, 12), grid=None, group=None, n_groups=1,
           force_global=False, own=None):
    """path_occupancy against the definition on the handle's own draws and on the reference draws (the caller's rows of both)"""
    model, d = pb.model, pb.n_dim
    if grid is None:
        grid, shift = make_grid(obs, ref_draws, model, d, cells=cells)
    assert clear_of_lines(ref_draws, model, d, grid), tag                          # a condition on the inputs
    w = dt_weights(pb.seg_start, pb.times)
    got = eng.path_occupancy(par, n_draws, grid, seed=seed, draw0=draw0, weight=w, group=group, n_groups=n_groups, force_global=force_global)
    assert form is None or eng.last_occupancy_form() == form, (tag, eng.last_occupancy_form())
    assert got[0].shape == (n_groups, grid["ny"] if d == 2 else 1, grid["nx"]) and got[1].shape == (n_groups,)
    if own is None:
        own = eng.smooth_draws(par, n_draws, seed=seed, draw0=draw0)
    kw = dict(weight=w, group=group, n_groups=n_groups)
    _same(got, occ_ref(own, pb.seg_start, model, d, grid, **kw), f"{tag} | own draws")
    _same(got, occ_ref(ref_draws, pb.seg_start, model, d, grid, **kw), f"{tag} | reference")
    print(f"OCC {tag}: inside {got[0].sum():.6g} outside {got[1].sum():.6g}")
    return got


def _lane_order(lengths):
    """the tracks in the order the tiled layout gives them lanes (no missing rows: longest first, ties in the data's order)"""
    return np.argsort(-np.asarray(lengths), kind="stable")


# ---- path 1: constant coefficients ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("what", ["regular", "irregular", "missing"])
def test_constant_coefficients(model, d, what):
    spec = _const_spec(model, d, what)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    assert eng.last_occupancy_form() == 0                                          # none yet
    info = eng.info()
    _show(f"const {model} d={d} {what}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_groups"] == 2
    assert info["n_tracks"] == 70
    occ, out = _check(eng, pb, spec["par"], _ref(("const", model, d, what), pb, spec["par"], seed=11, n_draws=5), spec["obs"],
                      f"const {model} d={d} {what}", TILE)
    eng.close()
    assert np.any(occ > 0) and out[0] > 0                                           # both branches


# ---- forms and groups on one handle -----------------------------------------------------------------------------------------------
def test_forms_and_groups():
    spec = _const_spec("CTCRW", 2, "irregular")
    pb = problem_from_spec(spec)
    ref = _ref(("const", "CTCRW", 2, "irregular"), pb, spec["par"], seed=11, n_draws=5)
    eng = capi.Engine(pb)
    assert eng.info()["n_groups"] == 2
    own = eng.smooth_draws(spec["par"], 5, seed=11)
    args = (eng, pb, spec["par"], ref, spec["obs"])
    pooled = _check(*args, "pooled", TILE, own=own)
    forced = _check(*args, "pooled, forced global", GLOBAL, force_global=True, own=own)
    _same(forced, pooled, "both forms")
    per_track = _check(*args, "one group per track", GLOBAL, group=np.arange(70), n_groups=70, own=own)
    assert np.array_equal(per_track[0].sum(axis=0), pooled[0][0]) and per_track[1].sum() == pooled[1][0]     # whole quanta: exact
    order = _lane_order(LENGTHS70)
    split = np.zeros(70, dtype=np.int32)
    split[order[64:]] = 1                                                          # whole wavefronts each
    _check(*args, "two groups, whole wavefronts", TILE, group=split, n_groups=2, own=own)
    alt = np.zeros(70, dtype=np.int32)
    alt[order[1::2]] = 1                                                           # neighbours in a wavefront differ
    _check(*args, "two groups alternating", GLOBAL, group=alt, n_groups=2, own=own)
    some = np.zeros(70, dtype=np.int32)
    some[[0, 5, 33, 69]] = -1
    left = _check(*args, "some tracks left out", TILE, group=some, n_groups=1, own=own)
    assert left[0].sum() < pooled[0].sum()
    alt_some = alt.copy()
    alt_some[[0, 5, 33, 69]] = -1
    _check(*args, "alternating, some left out", GLOBAL, group=alt_some, n_groups=3, own=own)
    eng.close()


@pytest.mark.parametrize("n_tracks", [65, 130])
def test_65_and_130_tracks_with_both_forms(n_tracks):
    # (the layout gives lanes by length, so the last wavefront of 65 tracks is ONE lane, which cannot mix two grids: there the first
    # wavefront alternates and the last lane has a grid of its own; no one-row track, so that lane has a state)
    lengths = ([20, 35, 14, 3, 27, 9] * 11)[:65] if n_tracks == 65 else (LENGTHS70 * 2)[:n_tracks]
    spec = _const_spec("CTCRW", 2, "irregular", seed=4, lengths=lengths)
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"{n_tracks} tracks", info)
    assert info["path"] == PATH_ISO and info["n_tracks"] == n_tracks and info["n_groups"] == (n_tracks + 63) // 64
    ref = _ref(("tracks", n_tracks), pb, spec["par"], seed=11, n_draws=5)
    own = eng.smooth_draws(spec["par"], 5, seed=11)
    order = _lane_order(lengths)
    group = np.zeros(n_tracks, dtype=np.int32)
    if n_tracks == 65:
        group[order[:64]] = np.arange(64) % 2
        group[order[64]] = 2
    else:
        group[order[64:]] = 1 + np.arange(n_tracks - 64) % 2                       # first wavefront pooled, the rest alternating
    got = _check(eng, pb, spec["par"], ref, spec["obs"], f"{n_tracks} tracks", BOTH, group=group, n_groups=3, own=own)
    assert np.all(got[0].sum(axis=(1, 2)) > 0)
    if n_tracks == 130:                                                            # three wavefronts, a grid each: the tile form
        split = np.repeat([0, 1, 2], [64, 64, 2])[np.argsort(order)]
        each = _check(eng, pb, spec["par"], ref, spec["obs"], "a grid per wavefront", TILE, group=split, n_groups=3, own=own)
        assert np.all(each[0].sum(axis=(1, 2))[:2] > 0)
        swapped = split.copy()
        swapped[order[0]] = 1                                                      # one lane of the first wavefront in the second's grid
        _check(eng, pb, spec["par"], ref, spec["obs"], "one lane swapped", BOTH, group=swapped, n_groups=3, own=own)
    eng.close()


def test_the_lds_tile_cap():
    spec = _const_spec("CTCRW", 2, "irregular")
    pb = problem_from_spec(spec)
    ref = _ref(("const", "CTCRW", 2, "irregular"), pb, spec["par"], seed=11, n_draws=5)
    eng = capi.Engine(pb)
    own = eng.smooth_draws(spec["par"], 5, seed=11)
    at = _check(eng, pb, spec["par"], ref, spec["obs"], "at the cap", TILE, cells=(128, 64), own=own)
    past = _check(eng, pb, spec["par"], ref, spec["obs"], "one cell past the cap", GLOBAL, cells=(2731, 3), own=own)
    eng.close()
    assert 128 * 64 == TILE_CELLS and 2731 * 3 == TILE_CELLS + 1
    assert at[0].sum() + at[1].sum() == past[0].sum() + past[1].sum()              # conservation, whole quanta


# ---- draw counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_draws", [1, 4, 5, NW * DRAW_CH, NW * DRAW_CH + 1])
@pytest.mark.parametrize("force_global", [False, True])
def test_draw_counts(n_draws, force_global):
    spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    ref = _ref(("const17", "CTCRW", 2, "missing"), pb, spec["par"], seed=11, n_draws=NW * DRAW_CH + 1)
    grid, _ = make_grid(spec["obs"], ref, "CTCRW", 2)                              # one grid for every count
    _check(eng, pb, spec["par"], ref[:n_draws], spec["obs"], f"{n_draws} draws", GLOBAL if force_global else TILE, n_draws=n_draws,
           grid=grid, force_global=force_global)
    eng.close()


def test_a_non_zero_draw0():
    spec = _const_spec("OU_SSM", 2, "missing")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    ref = _ref(("draw0", "OU_SSM"), pb, spec["par"], seed=7, draw0=3, n_draws=6)
    _check(eng, pb, spec["par"], ref, spec["obs"], "draw0 = 3", TILE, n_draws=6, seed=7, draw0=3)
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
    _check(eng, pb, spec["par"], _ref(("const", model, 2, "missing"), pb, spec["par"], seed=11, n_draws=5), spec["obs"], f"dense {model}", TILE)
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
    _check(eng, pb, spec["par"], _ref(("hp", model, d), pb, spec["par"], seed=11, n_draws=5), spec["obs"], f"H P0 {model} d={d}", TILE)
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
    ref = _ref(("tv", model), pb, spec["par"], seed=11, n_draws=5)
    got = _check(eng, pb, spec["par"], ref, spec["obs"], f"tv {model}", TILE)
    grid, _ = make_grid(spec["obs"], ref, model, 2)
    w = dt_weights(pb.seg_start, pb.times)
    per = eng.path_occupancy(spec["par"], 5, grid, seed=11, weight=w, group=np.arange(150) % 7, n_groups=7)
    assert eng.last_occupancy_form() == GLOBAL
    _same(per, occ_ref(ref, pb.seg_start, model, 2, grid, weight=w, group=np.arange(150) % 7, n_groups=7), f"tv {model} seven groups")
    # three groups of lanes by length: 1 MiB of records makes each group of the CTCRW its own chunk (test_gpu_smooth_layouts.py)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.path_occupancy(spec["par"], 5, grid, seed=11, weight=w)
    eng.close()
    _same(many, got, "tv chunks")


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
    full = _ref(("lattice", model), pb2, par, seed=11, n_draws=5)
    got = _check(eng, pb, par, full[:, rows, :], obs, f"lattice {model}", TILE)   # weights indexed by the caller's rows
    grid, _ = make_grid(obs, full[:, rows, :], model, 2)
    rows_only = eng.path_occupancy(par, 5, grid, seed=11)
    eng.close()
    # unit weights count the caller's state rows and no padded row
    assert rows_only[0].sum() + rows_only[1].sum() == 5 * (pb.n - pb.n_seg)
    assert got[0].sum() > 0


@pytest.mark.parametrize("model", MODELS)
def test_negative_p0_rows_without_a_position_land_outside(model):
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
    ref = _ref(("negp0", model), pb, par, seed=11, n_draws=5)
    _check(eng, pb, par, ref, obs, f"negative P0 {model}", TILE, cells=(16, 1))
    grid, _ = make_grid(obs, ref, model, 1, cells=(16, 1))
    occ, out = eng.path_occupancy(par, 5, grid, seed=11)                            # unit weights: whole numbers
    eng.close()
    state = np.ones(pb.n, dtype=bool)
    state[pb.seg_start] = False
    bad = np.count_nonzero(~np.isfinite(ref[:, state, 0]))
    assert occ.sum() + out[0] == 5 * state.sum() and out[0] >= bad                  # conservation; the non-finite rows are outside


# ---- invariance, all bitwise ------------------------------------------------------------------------------------------------------
def test_budget_chunks_and_draw_batches_on_six_ragged_groups_are_bitwise():
    # the batch of test_gpu_path.py::test_budget_chunks_on_six_ragged_groups_are_bitwise: 1 MiB = 131072 doubles cuts the records
    # into three chunks, produced again for every batch of draws
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
    assert info["path"] == PATH_ISO and info["n_groups"] == 6 and pb.n_seg == 325
    ref = _ref("chunks", pb, spec["par"], seed=11, n_draws=5)
    group = np.arange(325) % 3
    one = _check(eng, pb, spec["par"], ref, spec["obs"], "chunks ragged", TILE)
    mixed = _check(eng, pb, spec["par"], ref, spec["obs"], "chunks ragged, three groups", None, group=group, n_groups=3)
    assert eng.last_occupancy_form() in (GLOBAL, BOTH)        # (the last wavefront's few short tracks may share a grid)
    grid, _ = make_grid(spec["obs"], ref, "CTCRW", 2)
    w = dt_weights(pb.seg_start, pb.times)
    # one launch takes DRAW_CH * 2^15 draws: five more go in a second batch, each batch over the chunks
    many_draws = (DRAW_CH << 15) + 5
    wide = eng.path_occupancy(spec["par"], many_draws, grid, seed=11)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    one_c = eng.path_occupancy(spec["par"], 5, grid, seed=11, weight=w)
    mixed_c = eng.path_occupancy(spec["par"], 5, grid, seed=11, weight=w, group=group, n_groups=3)
    wide_c = eng.path_occupancy(spec["par"], many_draws, grid, seed=11)
    head = eng.path_occupancy(spec["par"], DRAW_CH << 15, grid, seed=11)
    tail = eng.path_occupancy(spec["par"], 5, grid, seed=11, draw0=DRAW_CH << 15)
    eng.close()
    _same(one_c, one, "chunks")
    _same(mixed_c, mixed, "chunks, global form")
    _same(wide_c, wide, "chunks and batches")
    assert np.array_equal(wide[0], head[0] + tail[0]) and np.array_equal(wide[1], head[1] + tail[1])
    assert wide[0].sum() + wide[1].sum() == many_draws * (pb.n - 325)              # every state row of every draw, once


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
    out = {}
    for devices in (None, [0, 0]):
        eng = capi.Engine(pb) if devices is None else capi.Engine(pb, devices=devices)
        info = eng.info()
        _show(f"shards {layout} {devices}", info)
        pooled = eng.path_occupancy(par, 5, grid, seed=11, weight=w)
        form_p = eng.last_occupancy_form()
        grouped = eng.path_occupancy(par, 5, grid, seed=11, weight=w, group=group, n_groups=3)
        out[devices is None] = (info, pooled, grouped, form_p, eng.last_occupancy_form())
        eng.close()
    (info1, p1, g1, fp1, fg1), (info2, p2, g2, fp2, fg2) = out[True], out[False]
    assert info2["n_devices"] == 2 and info1["n_devices"] <= 1 and info2["n_tracks"] == info1["n_tracks"] == pb.n_seg
    if layout == "lattice":
        assert info1["n_rows_tiled"] > pb.n and info2["n_rows_tiled"] > pb.n
    if layout == "tv":
        assert info1["path"] == PATH_TV and info2["path"] == PATH_TV
    assert fp1 == TILE and fp2 == TILE and fg1 == GLOBAL and fg2 == GLOBAL
    assert p1[0].sum() > 0
    _same(p2, p1, f"shards {layout} pooled")
    _same(g2, g1, f"shards {layout} grouped")


@pytest.mark.parametrize("model", MODELS)
def test_repeated_calls_and_draw_ranges_are_bitwise(model):
    spec = _const_spec(model, 2, "missing")
    pb = problem_from_spec(spec)
    w = dt_weights(pb.seg_start, pb.times)
    ref = _ref(("const", model, 2, "missing"), pb, spec["par"], seed=11, n_draws=5)
    grid, _ = make_grid(spec["obs"], ref, model, 2)
    eng = capi.Engine(pb)
    first = eng.path_occupancy(spec["par"], 8, grid, seed=5, weight=w)
    _same(eng.path_occupancy(spec["par"], 8, grid, seed=5, weight=w), first, "two identical calls")
    whole = eng.path_occupancy(spec["par"], 8, grid, seed=5)
    a = eng.path_occupancy(spec["par"], 4, grid, seed=5, draw0=0)
    b = eng.path_occupancy(spec["par"], 4, grid, seed=5, draw0=4)
    assert np.array_equal(whole[0], a[0] + b[0]) and np.array_equal(whole[1], a[1] + b[1])       # [0, 8) = [0, 4) + [4, 8)
    ones = eng.path_occupancy(spec["par"], 8, grid, seed=5, weight=np.ones(pb.n))
    _same(ones, whole, "weight None is ones")
    zero = eng.path_occupancy(spec["par"], 8, grid, seed=5, weight=np.zeros(pb.n))
    other = eng.path_occupancy(spec["par"], 8, grid, seed=6)
    eng.close()
    assert np.all(zero[0] == 0) and np.all(zero[1] == 0)
    assert not np.array_equal(other[0], whole[0])


# ---- against ssde_path_stats --------------------------------------------------------------------------------------------------------
def test_eight_cells_are_eight_regions_of_path_stats():
    spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    ref = _ref(("const", "CTCRW", 2, "missing"), pb, spec["par"], seed=11, n_draws=5)
    grid, _ = make_grid(spec["obs"], ref, "CTCRW", 2, cells=(4, 2))
    assert clear_of_lines(ref, "CTCRW", 2, grid)
    xe = grid["x0"] + grid["dx"] * np.arange(5)
    ye = grid["y0"] + grid["dy"] * np.arange(3)
    # (an edge computed here may differ from the division's by an ulp: no reference position is within 1e-6 of one)
    regions = [[xe[ix], xe[ix + 1], ye[iy], ye[iy + 1]] for iy in range(2) for ix in range(4)]
    eng = capi.Engine(pb)
    occ, out = eng.path_occupancy(spec["par"], 5, grid, seed=11)
    stats = eng.path_stats(spec["par"], 5, seed=11, regions=regions)
    eng.close()
    assert np.array_equal(occ[0].ravel(), np.nansum(stats[:, :, 2:], axis=(0, 1)))   # whole numbers below 2^53 on both sides
    assert occ.sum() + out[0] == 5 * (pb.n - 70)


# ---- isolation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["const", "tv"])
def test_an_occupancy_call_leaves_every_other_result_as_it_was(layout, monkeypatch):
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
    ps = eng.path_stats(par, 5, seed=11, regions=reg, weight=w)
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.path_occupancy(par, 5, grid, seed=11, weight=w)
    eng.path_occupancy(par, 5, grid, seed=11, weight=w, group=np.arange(pb.n_seg) % 2, n_groups=2)
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
    ps2 = eng.path_stats(par, 5, seed=11, regions=reg, weight=w)
    eng.close()
    for k in ("mean", "cov", "resid"):
        assert np.array_equal(sm[k], sm2[k], equal_nan=True), k
    assert np.array_equal(dr, dr2, equal_nan=True) and np.array_equal(ps, ps2, equal_nan=True)
    for k in ("mean", "cov"):
        assert np.array_equal(pr[k], pr2[k], equal_nan=True), k


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_unserved_models_and_bad_arguments():
    g1, g2 = grid_of(0.0, 1.0, 4), grid_of(0.0, 1.0, 4, 0.0, 1.0, 3)
    for sp, g in ((make_spec("gp_ou", "OU", 1, seed=201, lengths=[9, 2, 14]), g1), (eseal_spec("gp_eseal", 211, [14, 9, 11]), g1),
                  (make_spec("gp_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70[:14], na_rows=(2, 19)), g2),
                  (make_spec("gp_coupled3", "CTCRW", 3, seed=33, lengths=LENGTHS70[:14], with_H=True, na_rows=(2, 19)), g2)):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.path_occupancy(sp["par"], 5, g)
        eng.close()
        assert ei.value.status == ERR_MODEL, sp["name"]
    spec = _const_spec("CTCRW", 2, "regular")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    ok = dict(n_draws=1, grid=g2)
    wbad = lambda v: np.r_[v, np.ones(pb.n - 1)]
    gbad = lambda v: np.r_[v, np.zeros(pb.n_seg - 1)].astype(np.int32)
    bad = [dict(n_draws=0), dict(draw0=-1), dict(n_draws=2, draw0=(1 << 28) - 2),
           dict(grid=dict(g2, nx=0)), dict(grid=dict(g2, nx=4097)), dict(grid=dict(g2, ny=0)), dict(grid=dict(g2, ny=4097)),
           dict(grid=dict(g2, dx=0.0)), dict(grid=dict(g2, dx=-1.0)), dict(grid=dict(g2, dx=np.inf)), dict(grid=dict(g2, dx=np.nan)),
           dict(grid=dict(g2, dy=0.0)), dict(grid=dict(g2, dy=np.nan)), dict(grid=dict(g2, x0=np.inf)), dict(grid=dict(g2, x0=np.nan)),
           dict(grid=dict(g2, y0=-np.inf)), dict(n_groups=0), dict(n_groups=2), dict(grid=dict(g2, nx=4096, ny=4096), group=gbad(0), n_groups=17),
           dict(group=gbad(-2), n_groups=1), dict(group=gbad(1), n_groups=1), dict(group=gbad(3), n_groups=3),
           dict(weight=wbad(-1e-300)), dict(weight=wbad(np.nan)), dict(weight=wbad(np.inf))]
    for kw in bad:
        with pytest.raises(capi.EngineError) as ei:
            eng.path_occupancy(spec["par"], **dict(ok, **kw))
        assert ei.value.status == ERR_ARG, kw
    assert eng.last_occupancy_form() == 0                                          # nothing ran
    # what the Python layer cannot send: NULL pointers, an unknown flag
    dp = C.POINTER(C.c_double)
    par = np.ascontiguousarray(spec["par"], dtype=np.float64)
    occ, out = np.zeros(12), np.zeros(1)
    G = capi.SsdeOccGrid(0.0, 1.0, 0.0, 1.0, 4, 3)
    P, O, U = par.ctypes.data_as(dp), occ.ctypes.data_as(dp), out.ctypes.data_as(dp)
    call = lambda h, p, g, o, u, flags: eng.lib.ssde_path_occupancy(h, p, eng.n_par_full, 0, 0, 1, g, None, None, 1, o, u, flags)
    assert call(None, P, C.byref(G), O, U, 0) == ERR_ARG and call(eng._h, None, C.byref(G), O, U, 0) == ERR_ARG
    assert call(eng._h, P, None, O, U, 0) == ERR_ARG and call(eng._h, P, C.byref(G), None, U, 0) == ERR_ARG
    assert call(eng._h, P, C.byref(G), O, U, 2) == ERR_ARG and call(eng._h, P, C.byref(G), O, U, 3) == ERR_ARG
    assert eng.lib.ssde_last_occupancy_form(None) == -1
    assert call(eng._h, P, C.byref(G), O, None, 0) == 0 and call(eng._h, P, C.byref(G), O, U, 1) == 0    # `outside` may be NULL
    state_rows = float(pb.n - 70)
    assert occ.sum() + out[0] == state_rows
    # a grid over the whole plane of the data counts every state row; one far from the data counts none
    everything = eng.path_occupancy(spec["par"], 1, grid_of(-1e6, 2e6, 1, -1e6, 2e6, 1), draw0=(1 << 28) - 2)
    nothing = eng.path_occupancy(spec["par"], 3, grid_of(1e7, 1.0, 5, 1e7, 1.0, 5))
    eng.close()
    assert everything[0][0, 0, 0] == state_rows and everything[1][0] == 0.0
    assert np.all(nothing[0] == 0.0) and nothing[1][0] == 3 * state_rows
    # one position column: ny must be 1, and y0 / dy are not read
    spec1 = _const_spec("OU_SSM", 1, "regular")
    eng = capi.Engine(problem_from_spec(spec1))
    with pytest.raises(capi.EngineError) as ei:
        eng.path_occupancy(spec1["par"], 1, dict(g1, ny=2))
    assert ei.value.status == ERR_ARG
    a = eng.path_occupancy(spec1["par"], 2, dict(g1, x0=2.0, y0=np.nan, dy=-1.0))
    b = eng.path_occupancy(spec1["par"], 2, dict(g1, x0=2.0))
    eng.close()
    _same(a, b, "d = 1 reads no y")


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_sde_utilisation_on_a_ctcrw_with_tau_smooth_in_x():
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
    ud = sde.utilisation(3, seed=2, cells=(16, 12))
    info = sde.engine_.info()
    _show("SDE tau ~ x", info)
    assert info["const_coeff"] == 0 and info["path"] == PATH_TV
    assert ud["density"].shape == (1, 12, 16) and ud["x_edges"].shape == (17,) and ud["y_edges"].shape == (13,)
    lo, hi = np.nanmin(obs, axis=0), np.nanmax(obs, axis=0)
    assert np.allclose([ud["x_edges"][0], ud["x_edges"][-1]], [lo[0] - 0.05 * (hi[0] - lo[0]), hi[0] + 0.05 * (hi[0] - lo[0])])
    assert np.allclose([ud["y_edges"][0], ud["y_edges"][-1]], [lo[1] - 0.05 * (hi[1] - lo[1]), hi[1] + 0.05 * (hi[1] - lo[1])])
    assert abs(ud["density"].sum() + ud["outside"][0] - 1.0) <= 1e-12
    # one grid per track: each sums to 1 (NaN for the tracks without weight), and their weighted sum is the pooled grid
    w = dt_weights(pb.seg_start, times)
    state_w = w.copy()
    state_w[pb.seg_start] = 0.0
    share = np.add.reduceat(state_w, pb.seg_start)
    by_id = sde.utilisation(3, seed=2, cells=(16, 12), by="ID")
    has = share > 0
    assert by_id["density"].shape == (70, 12, 16) and np.all(np.isnan(by_id["density"][~has]))
    assert np.allclose(by_id["density"][has].sum(axis=(1, 2)) + by_id["outside"][has], 1.0, rtol=0, atol=1e-12)
    mix = np.tensordot(share[has] / share.sum(), by_id["density"][has], axes=1)
    assert np.allclose(mix, ud["density"][0], rtol=0, atol=1e-12)
    labels = np.arange(70) % 3
    by_lab = sde.utilisation(3, seed=2, cells=(16, 12), by=labels)
    assert by_lab["density"].shape == (3, 12, 16)
    assert np.allclose(by_lab["density"].sum(axis=(1, 2)) + by_lab["outside"], 1.0, rtol=0, atol=1e-12)
    # against the definition on sample_states' draws of the same seed, on a grid clear of the reference draws
    ref = draws_ref(pb, par, seed=2, n_draws=3)
    grid, _ = make_grid(obs, ref, "CTCRW", 2)
    assert clear_of_lines(ref, "CTCRW", 2, grid)
    ext = (grid["x0"], grid["x0"] + 16 * grid["dx"], grid["y0"], grid["y0"] + 12 * grid["dy"])
    ud2 = sde.utilisation(3, seed=2, cells=(16, 12), extent=ext)
    g2 = grid_of(ext[0], (ext[1] - ext[0]) / 16, 16, ext[2], (ext[3] - ext[2]) / 12, 12)       # the grid utilisation() forms
    assert clear_of_lines(ref, "CTCRW", 2, g2)
    total = 3 * np.bincount(np.zeros(70, dtype=np.int64), weights=share)[0]        # summed as utilisation() sums it
    for draws in (sde.sample_states(3, seed=2), ref):
        occ, out = occ_ref(draws, pb.seg_start, "CTCRW", 2, g2, weight=w)
        assert np.array_equal(ud2["density"], occ / total) and np.array_equal(ud2["outside"], out / total)
    rows = sde.utilisation(3, seed=2, cells=(16, 12), extent=ext, weight=None)
    occ, out = occ_ref(ref, pb.seg_start, "CTCRW", 2, g2)
    assert np.array_equal(rows["density"], occ / (3.0 * (n - 70))) and np.array_equal(rows["outside"], out / (3.0 * (n - 70)))
    with pytest.raises(NotImplementedError):
        SDE(data={"ID": np.zeros(10), "time": np.arange(10.0), "z": np.exp(rng.standard_normal(10))}, type="CIR", response="z").utilisation(2)
