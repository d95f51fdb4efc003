"""CPU suite: the lane math of ssde_path_stats (csrc/ssde_path.hpp over csrc/ssde_draws.hpp), built with g++
(tests/hostsim/hostsim_path.cpp through tests/pathsim_lib.py), against the definition (tests/path_ref.py) on the reference draws
(tests/draws_ref.py).

Limit: 1e-9 (1 + max|ref|) per statistic, NaN patterns identical -- the limit §3.10 puts on the draws themselves; a length is a
sum of at most 43 differences of draws.  Every comparison first asserts that no reference position is within 1e-5 of a region
edge (path_cases.py), so that no count can flip on rounding."""
import numpy as np
import pytest

import pathsim_lib
from cases import make_spec, problem_from_spec
from draws_ref import draws_ref
from path_cases import clear_of_edges, compare, dt_weights, make_regions
from path_ref import path_ref

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS = [12, 25, 1, 40, 2, 7]
NA_ROWS = (4, 5, 11, 20, 60)                    # row 11 ends the first track


def _check(pb, par, obs, tag, seed, draw0=0, n_draws=5, n_regions=8):
    model, d = pb.model, pb.n_dim
    with np.errstate(invalid="ignore"):
        draws = draws_ref(pb, par, seed=seed, draw0=draw0, n_draws=n_draws)
    reg = make_regions(obs, d, n_regions)
    assert clear_of_edges(draws, model, d, reg), tag
    w = dt_weights(pb.seg_start, pb.times)
    ref = path_ref(draws, pb.seg_start, model, d, regions=reg, weight=w)
    got = pathsim_lib.path_stats(pb, par, seed=seed, draw0=draw0, n_draws=n_draws, regions=reg, weight=w)
    compare(got, ref, tag)
    return got, ref


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_constant_coefficients_with_na_rows(model, d):
    spec = make_spec(f"dh_{model}_{d}", model, d, seed=31 + d, lengths=LENGTHS, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    got, ref = _check(pb, spec["par"], spec["obs"], f"const {model} d={d}", seed=5, draw0=2)
    assert np.all(np.isnan(got[:, 2, :])) and np.all(got[:, 4, :2] == 0.0)         # the one-row and the two-row track
    assert np.all(np.isfinite(got[:, [0, 1, 3, 4, 5], :]))
    # the twin's own invariances, bitwise: draw numbering, weight = None as ones, no regions
    reg = make_regions(spec["obs"], d, 8)
    whole = pathsim_lib.path_stats(pb, spec["par"], seed=5, draw0=0, n_draws=8, regions=reg)
    part = pathsim_lib.path_stats(pb, spec["par"], seed=5, draw0=4, n_draws=4, regions=reg)
    ones = pathsim_lib.path_stats(pb, spec["par"], seed=5, draw0=4, n_draws=4, regions=reg, weight=np.ones(pb.n))
    assert np.array_equal(whole[4:], part, equal_nan=True) and np.array_equal(part, ones, equal_nan=True)
    bare = pathsim_lib.path_stats(pb, spec["par"], seed=5, draw0=4, n_draws=4)
    assert bare.shape == (4, 6, 2) and np.array_equal(bare, part[:, :, :2], equal_nan=True)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    spec = make_spec(f"dh_hp_{model}_{d}", model, d, seed=41 + d, lengths=LENGTHS, with_H=True, with_P0=True, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    _check(pb, spec["par"], spec["obs"], f"H P0 {model} d={d}", seed=9)


@pytest.mark.parametrize("model", MODELS)
def test_row_varying_parameters(model):
    spec = make_spec(f"dh_tv_{model}", model, 2, seed=51, lengths=[30, 18, 1, 44], variant="tv", na_rows=(3, 29, 50))
    pb = problem_from_spec(spec)
    _check(pb, spec["par"], spec["obs"], f"tv {model}", seed=3)


def test_negative_p0_follows_the_reference():
    # the det F <= 0 corner of §3.9, d = 1: whatever pivots fail, fail alike, and a path with one NaN position is NaN in every statistic
    from smoothsde_amd import capi
    from smoothsde_amd.synth import simulate
    seen = 0
    for model in MODELS:
        ID, times, obs = simulate(model, 5, 12, 1, seed=4)
        sdim = 2 if model == "CTCRW" else 1
        P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
        par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
        pb = capi.Problem(model, ID, times, obs, P0=P0)
        got, ref = _check(pb, par, obs, f"negative P0 {model}", seed=2, n_draws=4)
        nan = np.isnan(got)
        assert np.array_equal(nan.any(axis=2), nan.all(axis=2))                   # all of a (track, draw) or nothing
        seen += int(nan.any())
    assert seen > 0                                                               # the corner is met


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_rows_that_are_not_the_callers_take_part_in_nothing(model, d):
    """A lattice-padded handle walks its padded rows too: the twin runs the written-out tracks with those rows flagged, the reference
    is the definition on the caller's rows of the same draws, with the weights indexed by the caller's rows."""
    from test_gpu_draws import _written_out
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks(model, d, [40, 25, 1, 33, 2, 18], 0.5, 0.2, seed=8, na_frac=0.05)
    pb = capi_problem(model, ID, times, obs)
    par = _par(model, d, np.random.default_rng(2))
    ID2, t2, obs2, rows = _written_out(ID, times, obs, 0.5)
    pb2 = capi_problem(model, ID2, t2, obs2)
    assert pb2.n > pb.n and pb2.n_seg == pb.n_seg
    draws = draws_ref(pb2, par, seed=11, n_draws=5)
    reg = make_regions(obs, d, 8)
    assert clear_of_edges(draws[:, rows, :], model, d, reg)
    w = dt_weights(pb.seg_start, pb.times)
    ref = path_ref(draws[:, rows, :], pb.seg_start, model, d, regions=reg, weight=w)
    is_row = np.zeros(pb2.n, dtype=bool)
    is_row[rows] = True
    w2 = np.full(pb2.n, np.nan)                                      # a padded row's weight is never read into a sum
    w2[rows] = w
    got = pathsim_lib.path_stats(pb2, par, seed=11, n_draws=5, regions=reg, weight=w2, is_row=is_row)
    compare(got, ref, f"lattice-style {model} d={d}")
    # ... and they do change the numbers: every written-out row taken as a row of the data gives longer paths
    every = pathsim_lib.path_stats(pb2, par, seed=11, n_draws=5, regions=reg, weight=np.ones(pb2.n))
    assert np.nanmax(every[:, :, 0] - got[:, :, 0]) > 0


def capi_problem(model, ID, times, obs):
    from smoothsde_amd import capi
    return capi.Problem(model, ID, times, obs)
