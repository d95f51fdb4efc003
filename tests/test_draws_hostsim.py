"""CPU suite: the lane math of ssde_smooth_draws (csrc/ssde_draws.hpp: draw_factor_row, draw_step, the Philox deviates), built
with g++ (tests/hostsim/hostsim_draws.cpp through tests/drawsim_lib.py), against the numpy reference written from the definition
(tests/draws_ref.py, itself checked against the joint Gaussian in test_draws_host.py).

Limit: 1e-9 (1 + max|ref|), NaN patterns identical -- a draw is mean + factor z, so the limit is the smoother's covariance limit.
The header forms C as P_f - X X' (X = P_f T' Lp^-T, the algebraically equal form §3.10 allows), the reference as
sym(P_f - J P_{j+1} J')."""
import numpy as np
import pytest

import drawsim_lib
from cases import make_spec, problem_from_spec
from draws_ref import draws_ref

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS = [12, 25, 1, 40, 2, 7]
NA_ROWS = (4, 5, 11, 20, 60)                    # row 11 ends the first track


def _compare(got, ref, tag):
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
    ok = ~np.isnan(ref)
    gap = np.max(np.abs(got[ok] - ref[ok]), initial=0.0) / (1.0 + np.max(np.abs(ref[ok]), initial=0.0))
    print(f"GAP {tag}: {gap:.2e}")
    assert gap <= 1e-9, (tag, gap)
    return gap


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_constant_coefficients_with_na_rows(model, d):
    spec = make_spec(f"dh_{model}_{d}", model, d, seed=31 + d, lengths=LENGTHS, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    ref = draws_ref(pb, spec["par"], seed=5, draw0=2, n_draws=5)
    got = drawsim_lib.draws(pb, spec["par"], seed=5, draw0=2, n_draws=5)
    _compare(got, ref, f"const {model} d={d}")
    state = np.ones(pb.n, dtype=bool)
    state[pb.seg_start] = False
    assert np.all(np.isnan(got[:, ~state])) and np.all(np.isfinite(got[:, state]))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    spec = make_spec(f"dh_hp_{model}_{d}", model, d, seed=41 + d, lengths=LENGTHS, with_H=True, with_P0=True, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    ref = draws_ref(pb, spec["par"], seed=9, n_draws=5)
    _compare(drawsim_lib.draws(pb, spec["par"], seed=9, n_draws=5), ref, f"H P0 {model} d={d}")


@pytest.mark.parametrize("model", MODELS)
def test_row_varying_parameters(model):
    spec = make_spec(f"dh_tv_{model}", model, 2, seed=51, lengths=[30, 18, 1, 44], variant="tv", na_rows=(3, 29, 50))
    pb = problem_from_spec(spec)
    ref = draws_ref(pb, spec["par"], seed=3, n_draws=5)
    _compare(drawsim_lib.draws(pb, spec["par"], seed=3, n_draws=5), ref, f"tv {model}")


@pytest.mark.parametrize("model", MODELS)
def test_injected_deviates_and_draw_numbering(model):
    spec = make_spec(f"dh_inj_{model}", model, 2, seed=61, lengths=LENGTHS, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    z = np.random.default_rng(1).standard_normal((3, pb.n, pb.sdim))
    _compare(drawsim_lib.draws(pb, spec["par"], n_draws=3, normals=z), draws_ref(pb, spec["par"], n_draws=3, normals=z), f"injected {model}")
    whole = drawsim_lib.draws(pb, spec["par"], seed=7, draw0=0, n_draws=8)
    part = drawsim_lib.draws(pb, spec["par"], seed=7, draw0=4, n_draws=4)
    assert np.array_equal(whole[4:], part, equal_nan=True)


def test_negative_p0_follows_the_reference():
    # the det F <= 0 corner of §3.9, d = 1: CTCRW skips the update and carries an indefinite P; whatever pivots fail, fail alike
    from smoothsde_amd import capi
    from smoothsde_amd.synth import simulate
    for model in MODELS:
        ID, times, obs = simulate(model, 5, 12, 1, seed=4)
        sdim = 2 if model == "CTCRW" else 1
        P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
        par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
        pb = capi.Problem(model, ID, times, obs, P0=P0)
        ref = draws_ref(pb, par, seed=2, n_draws=4)
        _compare(drawsim_lib.draws(pb, par, seed=2, n_draws=4), ref, f"negative P0 {model}")


def test_factor_row_is_thirty_doubles_for_ctcrw_d2():
    assert drawsim_lib.fac_doubles("CTCRW", 2) == 30 and drawsim_lib.fac_doubles("OU_SSM", 1) == 3
