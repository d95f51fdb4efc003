"""CPU suite: the numpy reference of ssde_predict (tests/predict_ref.py) is exact, not merely plausible.

A query (row j, offset) is the smoothed state of a NA row inserted at t_j + offset that carries row j's covariates.  So the
reference must agree with smooth_ref and with the dense joint Gaussian joint_track on the AUGMENTED problem (predict_ref.augment),
neither of which knows about queries.  Limits (§3.9's): mean 1e-10 (1 + max|ref|) and covariance 1e-9 max|ref| against smooth_ref,
1e-9 against joint_track, NaN patterns identical.  The gaps are printed (pytest -rA) and go into §3.11's table."""
import os
import re

import numpy as np
import pytest

from predict_cases import LENGTHS, MODELS, compare, expected_nan, intervals, query_set, small_problem
from predict_ref import augment, predict_ref
from smooth_ref import joint_track, smooth_ref
from smoothsde_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _against_the_augmented_problem(pb, par, tag):
    rows, offs = query_set(pb, seed=3)
    ref = predict_ref(pb, par, rows, offs)
    aug, index = augment(pb, rows, offs)
    assert aug.n == pb.n + int(np.sum(index >= 0)) and aug.n_seg == pb.n_seg
    nanq = expected_nan(pb, rows, offs)
    assert np.array_equal(index < 0, nanq)
    assert np.array_equal(np.isnan(ref["mean"][:, 0]), nanq) and np.array_equal(np.isnan(ref["cov"][:, 0, 0]), nanq)
    assert np.all(np.isfinite(ref["mean"][~nanq])) and np.all(np.isfinite(ref["cov"][~nanq]))
    sm = smooth_ref(aug, par)
    ok = index >= 0
    compare({"mean": ref["mean"][ok], "cov": ref["cov"][ok]}, {"mean": sm["mean"][index[ok]], "cov": sm["cov"][index[ok]]},
            f"predict_ref vs augmented smooth_ref: {tag}")
    # ... and against the dense joint Gaussian of every augmented track
    bounds = list(aug.seg_start) + [aug.n]
    jm = np.full((aug.n, pb.sdim), np.nan); jc = np.full((aug.n, pb.sdim, pb.sdim), np.nan)
    for k in range(aug.n_seg):
        if bounds[k + 1] - bounds[k] >= 2:
            m_, c_, _ = joint_track(aug, par, k)
            jm[bounds[k] + 1:bounds[k + 1]] = m_; jc[bounds[k] + 1:bounds[k + 1]] = c_
    compare({"mean": ref["mean"][ok], "cov": ref["cov"][ok]}, {"mean": jm[index[ok]], "cov": jc[index[ok]]},
            f"predict_ref vs joint_track: {tag}", mean_tol=1e-9, cov_tol=1e-9)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("irregular", [False, True])
def test_a_query_is_the_smoothed_state_of_an_inserted_na_row(model, d, irregular):
    pb, par = small_problem(model, d, irregular)
    _against_the_augmented_problem(pb, par, f"{model} d={d} irregular={irregular}")


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    pb, par = small_problem(model, d, with_HP=True)
    _against_the_augmented_problem(pb, par, f"H P0 {model} d={d}")


@pytest.mark.parametrize("model", MODELS)
def test_row_varying_parameters_use_row_j_on_both_sub_steps(model):
    # tau (sigma for BM_SSM) ~ 1 + x and a spline on the last parameter: the parameters differ from row j to row j + 1
    pb, par = small_problem(model, 2, variant="tv")
    _against_the_augmented_problem(pb, par, f"tv {model}")


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("variant", ["const", "tv"])
def test_offset_zero_and_the_whole_interval_are_the_smoother_at_the_rows(model, variant):
    pb, par = small_problem(model, 2, variant=variant)
    first, last, dt = intervals(pb)
    sm = smooth_ref(pb, par)
    at = np.flatnonzero(~first)
    got = predict_ref(pb, par, at, np.zeros(len(at)))
    compare(got, {"mean": sm["mean"][at], "cov": sm["cov"][at]}, f"predict_ref offset 0 vs smooth_ref: {model} {variant}")
    inner = np.flatnonzero(~first & ~last)
    got = predict_ref(pb, par, inner, dt[inner])
    compare(got, {"mean": sm["mean"][inner + 1], "cov": sm["cov"][inner + 1]}, f"predict_ref offset Delta vs smooth_ref: {model} {variant}")


@pytest.mark.parametrize("model", MODELS)
def test_a_forecast_is_the_forward_prediction_and_its_covariance_grows(model):
    pb, par = small_problem(model, 2)
    first, last, dt = intervals(pb)
    tails = np.flatnonzero(last & ~first)
    offs = np.array([0.0, 0.5, 1.0, 2.0, 4.0, 8.0])
    out = predict_ref(pb, par, np.repeat(tails, len(offs)), np.tile(offs, len(tails)))
    mean = out["mean"].reshape(len(tails), len(offs), -1); cov = out["cov"].reshape(len(tails), len(offs), pb.sdim, pb.sdim)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov))
    sm = smooth_ref(pb, par)
    assert np.allclose(mean[:, 0], sm["mean"][tails], rtol=0, atol=1e-10 * (1 + np.abs(sm["mean"][tails]).max()))
    pos = 0                                                      # the first state column: a position (CTCRW) or the state itself
    var = cov[:, :, pos, pos]
    if model == "OU_SSM":                                        # the stationary variance kappa is approached from one side
        kappa = np.exp(par[-1])
        assert np.all(np.diff(np.abs(var - kappa), axis=1) < 0)
    else:
        assert np.all(np.diff(var, axis=1) > 0)
    # two forecasts in a row compose: the state at 2 + 2 from the moments at 2, through the augmented problem
    aug, index = augment(pb, np.repeat(tails, 2), np.tile([2.0, 4.0], len(tails)))
    sa = smooth_ref(aug, par)
    k4 = np.arange(len(tails)) * len(offs) + 4
    compare({"mean": out["mean"][k4], "cov": out["cov"][k4]}, {"mean": sa["mean"][index[1::2]], "cov": sa["cov"][index[1::2]]},
            f"predict_ref forecast vs augmented smooth_ref: {model}")


@pytest.mark.parametrize("model", MODELS)
def test_nan_exactly_where_defined(model):
    pb, par = small_problem(model, 1)
    first, last, dt = intervals(pb)
    assert list(np.flatnonzero(first)) == [0, 9, 10, 12, 15] and LENGTHS[1] == 1
    rows = np.array([0, 9, 10, 12, 15, 3, 3, 3, 4, 8, 8, 11, 17])       # first rows (9: a one-row track); 4, 8, 17: NA rows
    offs = np.array([0.0, 0.0, 0.3, 0.0, 5.0, dt[3], dt[3] * (1 + 1e-12), dt[3] * 1.01, 0.2 * dt[4], 0.0, 9.0, 3.0, 0.5 * dt[17]])
    out = predict_ref(pb, par, rows, offs)
    want = np.array([True] * 5 + [False, False, True] + [False] * 5)
    assert np.array_equal(np.isnan(out["mean"]).all(axis=1), want) and np.array_equal(np.isnan(out["mean"]).any(axis=1), want)
    assert np.array_equal(np.isnan(out["cov"]).all(axis=(1, 2)), want) and np.array_equal(np.isnan(out["cov"]).any(axis=(1, 2)), want)


def test_a_rejected_update_serves_no_query():
    # the negative-P0 corner (det F <= 0): CTCRW skips the update on the first state rows and drops its drift there
    from smoothsde_amd.synth import simulate
    ID, times, obs = simulate("CTCRW", 3, 8, 1, seed=4)
    pb = capi.Problem("CTCRW", ID, times, obs, P0=np.diag([-5.0, 1.0]))
    par = np.array([-2.0, 0.7, 0.3, 0.1])
    rows = np.arange(pb.n); offs = np.full(pb.n, 0.25)
    out = predict_ref(pb, par, rows, offs)
    sm = smooth_ref(pb, par)
    rejected = np.isnan(sm["resid"][:, 0]) & np.isfinite(sm["mean"][:, 0])            # no NA rows here: no residual = no update
    assert rejected.sum() >= 3
    assert np.array_equal(np.isnan(out["mean"][:, 0]), rejected | np.isnan(sm["mean"][:, 0]))


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_ssde_predict_is_part_of_the_abi():
    text = open(os.path.join(ROOT, "include", "ssde.h")).read()
    assert re.search(r"int\s+ssde_predict\s*\(\s*ssde_handle\s*\*h,\s*const double\s*\*par,\s*int32_t n_par_full,\s*const int64_t\s*\*q_row,"
                     r"\s*const double\s*\*q_off,\s*int64_t n_query,\s*double\s*\*a_pred,\s*double\s*\*P_pred\)", text)
    assert re.search(r"\*\s+ssde_predict\s+<-", text)                   # the entry-point list
    assert "ssde_predict" in capi.EXPORTED_SYMBOLS and capi.ABI_VERSION == 12
    assert re.search(r"#define\s+SSDE_ABI_VERSION\s+12\b", text)
    assert hasattr(capi.Engine, "predict")
    from smoothsde_amd.sde import SDE
    assert hasattr(SDE, "predict_states")
