"""CPU suite: the lane math of ssde_predict_draws (csrc/ssde_bridge.hpp: bridge_side_row, bridge_deviates, bridge_step,
bridge_slot_walk over the draws' walk and the host plan's lists), built with g++ (tests/hostsim/hostsim_predict_draws.cpp through
tests/predictdrawsim_lib.py), against the numpy reference written from the definition (tests/bridge_ref.py, itself checked against the
joint Gaussian in test_predict_draws_host.py).  Limit: the twin's, 1e-9 (1 + max|ref|), NaN patterns identical."""
import numpy as np
import pytest

import drawsim_lib
import predictdrawsim_lib as twin
from bridge_ref import bridge_queries, compare_draws, predict_draws_ref
from predict_cases import MODELS, expected_nan, intervals, small_problem
from smoothsde_amd import capi

ND = 5


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("irregular", [False, True])
@pytest.mark.parametrize("log_sigma_obs", [-1.0, -6.0])
def test_constant_coefficients_with_na_rows(model, d, irregular, log_sigma_obs):
    pb, par = small_problem(model, d, irregular)
    par = par.copy(); par[0] = log_sigma_obs
    rows, offs = bridge_queries(pb, seed=5)
    got = twin.predict_draws(pb, par, rows, offs, seed=11, draw0=3, n_draws=ND)
    compare_draws(got, predict_draws_ref(pb, par, rows, offs, seed=11, draw0=3, n_draws=ND),
                  f"twin vs predict_draws_ref: {model} d={d} irregular={irregular} lso={log_sigma_obs}")
    assert np.array_equal(np.isnan(got[0, :, 0]), expected_nan(pb, rows, offs))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    pb, par = small_problem(model, d, with_HP=True)
    rows, offs = bridge_queries(pb, seed=6)
    compare_draws(twin.predict_draws(pb, par, rows, offs, seed=2, n_draws=ND), predict_draws_ref(pb, par, rows, offs, seed=2, n_draws=ND),
                  f"twin vs predict_draws_ref: H P0 {model} d={d}")


@pytest.mark.parametrize("model", MODELS)
def test_row_varying_parameters(model):
    pb, par = small_problem(model, 2, variant="tv")
    rows, offs = bridge_queries(pb, seed=7)
    compare_draws(twin.predict_draws(pb, par, rows, offs, seed=3, n_draws=ND), predict_draws_ref(pb, par, rows, offs, seed=3, n_draws=ND),
                  f"twin vs predict_draws_ref: tv {model}")


def test_negative_p0_follows_the_reference():
    # the det F <= 0 corner of §3.9, d = 1: CTCRW rejects the update (NaN for every query on such a row) and carries an indefinite P
    from smoothsde_amd.synth import simulate
    for model in MODELS:
        ID, times, obs = simulate(model, 5, 12, 1, seed=4)
        sdim = 2 if model == "CTCRW" else 1
        P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
        par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
        pb = capi.Problem(model, ID, times, obs, P0=P0)
        rows, offs = bridge_queries(pb, seed=9)
        ref = predict_draws_ref(pb, par, rows, offs, seed=4, n_draws=ND)
        compare_draws(twin.predict_draws(pb, par, rows, offs, seed=4, n_draws=ND), ref, f"twin vs predict_draws_ref: negative P0 {model}")
        if model == "CTCRW":
            assert np.isnan(ref[0, :, 0]).sum() > expected_nan(pb, rows, offs).sum()


@pytest.mark.parametrize("model", MODELS)
def test_the_twin_keeps_the_guarantees(model):
    pb, par = small_problem(model, 2)
    rows, offs = bridge_queries(pb, seed=8)
    first, last, dt = intervals(pb)
    whole = twin.predict_draws(pb, par, rows, offs, seed=7, n_draws=8)
    paths = drawsim_lib.draws(pb, par, seed=7, n_draws=8)
    z = np.flatnonzero((offs == 0.0) & ~first[rows])
    e = np.flatnonzero((offs == dt[rows]) & ~first[rows] & ~last[rows])
    assert np.array_equal(whole[:, z], paths[:, rows[z]]) and np.array_equal(whole[:, e], paths[:, rows[e] + 1])     # bitwise
    assert np.array_equal(whole[:4], twin.predict_draws(pb, par, rows, offs, seed=7, draw0=0, n_draws=4), equal_nan=True)
    assert np.array_equal(whole[4:], twin.predict_draws(pb, par, rows, offs, seed=7, draw0=4, n_draws=4), equal_nan=True)
    p = np.lexsort((offs, rows))
    assert np.array_equal(whole[:, p], twin.predict_draws(pb, par, rows[p], offs[p], seed=7, n_draws=8), equal_nan=True)
    j = int(np.flatnonzero(~first & ~last)[0])
    keep = rows != j
    more = twin.predict_draws(pb, par, np.r_[rows[keep], j, j], np.r_[offs[keep], 0.2 * dt[j], 0.7 * dt[j]], seed=7, n_draws=8)
    assert np.array_equal(more[:, :keep.sum()], whole[:, keep], equal_nan=True)


def test_one_step_against_the_conditional_by_plain_solves():
    from smooth_ref import _trans
    rng = np.random.default_rng(1)
    for model, d, par in (("CTCRW", 2, [0.3, -0.2, 0.4, 0.1]), ("OU_SSM", 1, [0.7, 0.3, -0.2]), ("BM_SSM", 2, [0.1, -0.3, 0.2])):
        sd = 2 * d if model == "CTCRW" else d
        pm = np.array([par])
        xp, an, z = rng.standard_normal(sd), rng.standard_normal(sd), rng.standard_normal(sd)
        T1, Q1, c1 = _trans(model, d, pm, np.array([0.4])); T2, Q2, c2 = _trans(model, d, pm, np.array([0.9]))
        m1 = T1[0] @ xp + c1[0]; S = T2[0] @ Q1[0] @ T2[0].T + Q2[0]; G = Q1[0] @ T2[0].T
        mean = m1 + G @ np.linalg.solve(S, an - (T2[0] @ m1 + c2[0]))
        C = Q1[0] - G @ np.linalg.solve(S, G.T)
        x = mean + np.linalg.cholesky(0.5 * (C + C.T)) @ z
        assert np.max(np.abs(twin.bridge_step(model, d, par, xp, an, 0.4, 0.9, False, z) - x)) < 1e-12
        xt = m1 + np.linalg.cholesky(Q1[0]) @ z
        assert np.max(np.abs(twin.bridge_step(model, d, par, xp, an, 0.4, 0.0, True, z) - xt)) < 1e-12


def test_the_seed_of_the_gpu_suite_s_statistical_check_passes_on_the_twin():
    # the GPU suite compares the mean of 4096 draws with ssde_predict's mean within 6 sqrt(V_ii / 4096); the draws are a fixed function
    # of the seed, so the same check on the twin's draws (and the predictor twin's moments) says beforehand whether that seed passes
    import predictsim_lib
    from bridge_ref import STAT_DRAWS, STAT_SEED, stat_problem, stat_ratio
    pb, par, rows, offs = stat_problem()
    assert len(rows) == 4 * (10 * 3 + 2)
    pred = predictsim_lib.predict(pb, par, rows, offs)
    draws = twin.predict_draws(pb, par, rows, offs, seed=STAT_SEED, n_draws=STAT_DRAWS)
    ratio = stat_ratio(draws, pred["mean"], pred["cov"])
    print(f"STAT largest ratio {ratio:.3f}")
    assert np.all(np.isfinite(draws)) and ratio <= 6.0
    # ... and the spread is the predictor's too: the variance of 4096 draws within 6 standard errors of V_ii (normal: sd V sqrt(2 / n))
    var = draws.var(axis=0, ddof=1)
    vii = np.einsum("kii->ki", pred["cov"])
    assert np.max(np.abs(var - vii) / (vii * np.sqrt(2.0 / STAT_DRAWS))) <= 6.0
