"""CPU suite: the lane math of ssde_predict (csrc/ssde_predict.hpp: predict_side_row, predict_packet_row, predict_query_row over
the records of ssde_smooth.hpp), built with g++ (tests/hostsim/hostsim_predict.cpp through tests/predictsim_lib.py), against the
numpy reference written from the definitions (tests/predict_ref.py, itself checked against the joint Gaussian in
test_predict_host.py).  Limits: the smoother's (mean 1e-10 (1 + max|ref|), covariance 1e-9 max|ref|), NaN patterns identical."""
import numpy as np
import pytest

import predictsim_lib
from predict_cases import MODELS, compare, expected_nan, query_set, small_problem
from predict_ref import augment, predict_ref
from smooth_ref import joint_track
from smoothsde_amd import capi


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("irregular", [False, True])
def test_constant_coefficients_with_na_rows(model, d, irregular):
    pb, par = small_problem(model, d, irregular)
    rows, offs = query_set(pb, seed=5)
    got = predictsim_lib.predict(pb, par, rows, offs)
    compare(got, predict_ref(pb, par, rows, offs), f"twin vs predict_ref: {model} d={d} irregular={irregular}")
    assert np.array_equal(np.isnan(got["mean"][:, 0]), expected_nan(pb, rows, offs))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    pb, par = small_problem(model, d, with_HP=True)
    rows, offs = query_set(pb, seed=6)
    compare(predictsim_lib.predict(pb, par, rows, offs), predict_ref(pb, par, rows, offs), f"twin vs predict_ref: H P0 {model} d={d}")


@pytest.mark.parametrize("model", MODELS)
def test_row_varying_parameters(model):
    pb, par = small_problem(model, 2, variant="tv")
    rows, offs = query_set(pb, seed=7)
    compare(predictsim_lib.predict(pb, par, rows, offs), predict_ref(pb, par, rows, offs), f"twin vs predict_ref: tv {model}")


@pytest.mark.parametrize("model", MODELS)
def test_the_twin_against_the_joint_gaussian_of_the_augmented_problem(model):
    pb, par = small_problem(model, 2)
    rows, offs = query_set(pb, seed=8)
    got = predictsim_lib.predict(pb, par, rows, offs)
    aug, index = augment(pb, rows, offs)
    bounds = list(aug.seg_start) + [aug.n]
    jm = np.full((aug.n, pb.sdim), np.nan); jc = np.full((aug.n, pb.sdim, pb.sdim), np.nan)
    for k in range(aug.n_seg):
        if bounds[k + 1] - bounds[k] >= 2:
            m_, c_, _ = joint_track(aug, par, k)
            jm[bounds[k] + 1:bounds[k + 1]] = m_; jc[bounds[k] + 1:bounds[k + 1]] = c_
    ok = index >= 0
    assert np.array_equal(~ok, np.isnan(got["mean"][:, 0]))
    compare({"mean": got["mean"][ok], "cov": got["cov"][ok]}, {"mean": jm[index[ok]], "cov": jc[index[ok]]},
            f"twin vs joint_track: {model}", mean_tol=1e-9, cov_tol=1e-9)


def test_negative_p0_follows_the_reference():
    # the det F <= 0 corner of §3.9, d = 1: CTCRW rejects the update (NaN for every query on such a row) and carries an indefinite P;
    # OU_SSM / BM_SSM update with a negative F
    from smoothsde_amd.synth import simulate
    for model in MODELS:
        ID, times, obs = simulate(model, 5, 12, 1, seed=4)
        sdim = 2 if model == "CTCRW" else 1
        P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
        par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
        pb = capi.Problem(model, ID, times, obs, P0=P0)
        rows, offs = query_set(pb, seed=9)
        ref = predict_ref(pb, par, rows, offs)
        got = predictsim_lib.predict(pb, par, rows, offs)
        compare(got, ref, f"twin vs predict_ref: negative P0 {model}")
        if model == "CTCRW":
            assert np.isnan(ref["mean"][:, 0]).sum() > expected_nan(pb, rows, offs).sum()      # rejected rows on top of the rest


def test_a_packet_is_thirty_three_doubles_for_ctcrw_d2():
    assert predictsim_lib.packet_doubles("CTCRW", 2) == 33 and predictsim_lib.packet_doubles("BM_SSM", 1) == 7
