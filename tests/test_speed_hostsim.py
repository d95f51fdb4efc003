"""CPU suite: the lane math of ssde_path_speed (csrc/ssde_speed.hpp over csrc/ssde_draws.hpp), built with g++
(tests/hostsim/hostsim_speed.cpp through tests/speedsim_lib.py), against the definition (tests/speed_ref.py) on the reference draws
(tests/draws_ref.py).

Limit: 1e-9 (1 + max|ref|) per statistic, NaN patterns identical -- the limit §3.10 puts on the draws themselves; a statistic is a
sum of at most 43 speeds or unit vectors of draws.  The row of the maximum and the per-row counts are exact: every comparison first
asserts that no reference speed is within 1e-5 (1 + thr) of a threshold and that the two largest speeds of every (track, draw) are
more than 1e-5 (1 + max) apart (speed_cases.py), so that neither can flip on rounding."""
import subprocess

import numpy as np
import pytest

import speedsim_lib
from cases import make_spec, problem_from_spec
from draws_ref import draws_ref
from speed_cases import clear_maxima, clear_of_thresholds, compare, dt_weights, make_thresholds
from speed_ref import speed_ref

LENGTHS = [12, 25, 1, 40, 2, 7]
NA_ROWS = (4, 5, 11, 20, 60)                    # row 11 ends the first track


def _check(pb, par, tag, seed, draw0=0, n_draws=5, n_thr=8):
    d = pb.n_dim
    with np.errstate(invalid="ignore"):
        draws = draws_ref(pb, par, seed=seed, draw0=draw0, n_draws=n_draws)
    thr = make_thresholds(draws, pb.seg_start, d, n_thr)
    assert clear_of_thresholds(draws, pb.seg_start, d, thr), tag
    assert clear_maxima(draws, pb.seg_start, d), tag
    w = dt_weights(pb.seg_start, pb.times)
    ref = speed_ref(draws, pb.seg_start, d, thresholds=thr, weight=w)
    got = speedsim_lib.path_speed(pb, par, seed=seed, draw0=draw0, n_draws=n_draws, thresholds=thr, weight=w)
    compare(got, ref, tag)
    return got, ref, thr


@pytest.mark.parametrize("d", [1, 2])
def test_constant_coefficients_with_na_rows(d):
    spec = make_spec(f"sp_CTCRW_{d}", "CTCRW", d, seed=31 + d, lengths=LENGTHS, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    (got, below), _, thr = _check(pb, spec["par"], f"const CTCRW d={d}", seed=5, draw0=2)
    assert np.all(np.isnan(got[:, 2, :])) and np.all(got[:, 4, 2] == float(pb.seg_start[4] + 1))   # the one-row and the two-row track
    assert np.all(np.isfinite(got[:, [0, 1, 3, 4, 5], :]))
    assert np.all(below[pb.seg_start] == 0) and below[:, 6].sum() == 5 * (pb.n - pb.n_seg)
    # the twin's own invariances, bitwise: draw numbering (counts adding up), weight = None as ones, thresholds as columns, the halves alone
    par = spec["par"]
    whole, wb = speedsim_lib.path_speed(pb, par, seed=5, draw0=0, n_draws=8, thresholds=thr)
    a, ab = speedsim_lib.path_speed(pb, par, seed=5, draw0=0, n_draws=4, thresholds=thr)
    b, bb = speedsim_lib.path_speed(pb, par, seed=5, draw0=4, n_draws=4, thresholds=thr)
    ones, ob = speedsim_lib.path_speed(pb, par, seed=5, draw0=4, n_draws=4, thresholds=thr, weight=np.ones(pb.n))
    assert np.array_equal(whole, np.concatenate([a, b]), equal_nan=True) and np.array_equal(wb, ab + bb)
    assert np.array_equal(b, ones, equal_nan=True) and np.array_equal(bb, ob)
    perm = np.random.default_rng(5).permutation(8)
    mixed, mb = speedsim_lib.path_speed(pb, par, seed=5, draw0=0, n_draws=8, thresholds=thr[perm])
    assert np.array_equal(mixed[:, :, :5], whole[:, :, :5], equal_nan=True)
    assert np.array_equal(mixed[:, :, 5:], whole[:, :, 5:][:, :, perm], equal_nan=True) and np.array_equal(mb, wb[:, perm])
    bare, none = speedsim_lib.path_speed(pb, par, seed=5, draw0=0, n_draws=8)
    assert none is None and bare.shape == (8, 6, 5) and np.array_equal(bare, whole[:, :, :5], equal_nan=True)
    only_s, _ = speedsim_lib.path_speed(pb, par, seed=5, draw0=0, n_draws=8, thresholds=thr, rows=False)
    _, only_b = speedsim_lib.path_speed(pb, par, seed=5, draw0=0, n_draws=8, thresholds=thr, stats=False)
    assert np.array_equal(only_s, whole, equal_nan=True) and np.array_equal(only_b, wb)


@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(d):
    spec = make_spec(f"sp_hp_CTCRW_{d}", "CTCRW", d, seed=41 + d, lengths=LENGTHS, with_H=True, with_P0=True, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    _check(pb, spec["par"], f"H P0 CTCRW d={d}", seed=9)


def test_row_varying_parameters():
    spec = make_spec("sp_tv_CTCRW", "CTCRW", 2, seed=51, lengths=[30, 18, 1, 44], variant="tv", na_rows=(3, 29, 50))
    pb = problem_from_spec(spec)
    _check(pb, spec["par"], "tv CTCRW", seed=3)


def test_negative_p0_follows_the_reference():
    # the det F <= 0 corner of §3.9, d = 1: whatever pivots fail, fail alike, and a path with one NaN velocity is NaN in every statistic
    from smoothsde_amd import capi
    from smoothsde_amd.synth import simulate
    ID, times, obs = simulate("CTCRW", 5, 12, 1, seed=4)
    pb = capi.Problem("CTCRW", ID, times, obs, P0=np.diag([-5.0, 1.0]))
    (got, below), _, _ = _check(pb, np.array([-2.0, 0.7, 0.3, 0.1]), "negative P0 CTCRW", seed=2, n_draws=4)
    nan = np.isnan(got)
    assert np.array_equal(nan.any(axis=2), nan.all(axis=2))                       # all of a (track, draw) or nothing
    assert nan.any()                                                              # the corner is met
    assert below[:, 6].max() <= 4 and below[:, 6].min() == 0


@pytest.mark.parametrize("d", [1, 2])
def test_rows_that_are_not_the_callers_take_part_in_nothing(d):
    """A lattice-padded handle walks its padded rows too: the twin runs the written-out tracks with those rows mapped to no caller's
    row, the reference is the definition on the caller's rows of the same draws; weights, counts and the row of the maximum are
    indexed by the caller's rows."""
    from smoothsde_amd import capi
    from test_gpu_draws import _written_out
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks("CTCRW", d, [40, 25, 1, 33, 2, 18], 0.5, 0.2, seed=8, na_frac=0.05)
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = _par("CTCRW", d, np.random.default_rng(2))
    ID2, t2, obs2, rows = _written_out(ID, times, obs, 0.5)
    pb2 = capi.Problem("CTCRW", ID2, t2, obs2)
    assert pb2.n > pb.n and pb2.n_seg == pb.n_seg
    draws = draws_ref(pb2, par, seed=11, n_draws=5)[:, rows, :]
    thr = make_thresholds(draws, pb.seg_start, d, 8)
    assert clear_of_thresholds(draws, pb.seg_start, d, thr) and clear_maxima(draws, pb.seg_start, d)
    w = dt_weights(pb.seg_start, pb.times)
    ref = speed_ref(draws, pb.seg_start, d, thresholds=thr, weight=w)
    crow = np.full(pb2.n, -1, dtype=np.int64)
    crow[rows] = np.arange(pb.n)
    got = speedsim_lib.path_speed(pb2, par, seed=11, n_draws=5, thresholds=thr, weight=w, crow=crow, n_out=pb.n)
    compare(got, ref, f"lattice-style CTCRW d={d}")
    # ... and they do change the numbers: every written-out row taken as a row of the data counts more rows below +inf
    every, eb = speedsim_lib.path_speed(pb2, par, seed=11, n_draws=5, thresholds=thr)
    assert eb[:, 6].sum() > got[1][:, 6].sum() and np.nanmax(every[:, :, 11] - speedsim_lib.path_speed(pb2, par, seed=11, n_draws=5, thresholds=thr, crow=crow, n_out=pb.n)[0][:, :, 11]) > 0


def test_the_sanitizer_program_runs_clean():
    """tests/hostsim/speed_san: the twin's walk on two small tracks (an NA row, a one-row track), built with -fsanitize=address,undefined,
    run as a program"""
    speedsim_lib.load()
    r = subprocess.run([speedsim_lib.SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "speed_san ok" in r.stdout, (r.stdout, r.stderr)
