"""CPU suite: the numpy reference of ssde_smooth_draws (tests/draws_ref.py) is exact, not merely plausible.

A draw is an affine map of its deviates, path = mean + A z.  Injecting unit deviates recovers A column by column; A A' must be the
FULL cross-time posterior covariance of the dense joint Gaussian (draws_ref.joint_full: every block, not the row-wise ones the
smoother is checked on) and the zero-deviate path its mean.  Limits: 1e-9 max|cov| (the project's limit against joint_track) and
1e-10 (1 + max|mean|) at log sigma_obs = -1, where this reference measures 1.1e-14 and 1.4e-15; 1e-7 max|cov| at log sigma_obs = -6,
where it measures 1.3e-12 (the loss is in the filtered covariance: the plain and the Joseph form of C give the same gap)."""
import os
import re

import numpy as np
import pytest

from cases import make_spec, problem_from_spec
from draws_ref import draws_ref, joint_full
from smoothsde_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS = [9, 1, 2, 7]                       # rows 0-8, 9, 10-11, 12-18
NA_ROWS = (4, 15)


def _problem(model, d, irregular, log_sigma_obs):
    spec = make_spec(f"dr_{model}_{d}_{irregular}", model, d, seed=21 + d, lengths=LENGTHS, na_rows=NA_ROWS, irregular=irregular)
    par = np.array(spec["par"], dtype=np.float64)
    par[0] = log_sigma_obs
    return problem_from_spec(spec), par


def _affine_map(pb, par, k):
    """(mean, A) of track k: the zero-deviate path and the map from the track's deviates to its path, column by column"""
    sd = pb.sdim
    bounds = list(pb.seg_start) + [pb.n]
    rows = np.arange(bounds[k] + 1, bounds[k + 1])
    m = len(rows)
    normals = np.zeros((1 + m * sd, pb.n, sd))
    for j in range(m):
        for c in range(sd):
            normals[1 + j * sd + c, rows[j], c] = 1.0
    out = draws_ref(pb, par, n_draws=1 + m * sd, normals=normals)[:, rows, :]          # (1 + m sd, m, sd)
    mean = out[0]
    A = (out[1:] - mean[None]).reshape(m * sd, m * sd).T                                 # column q: the path's response to deviate q
    return mean, A


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("irregular", [False, True])
@pytest.mark.parametrize("log_sigma_obs,cov_tol", [(-1.0, 1e-9), (-6.0, 1e-7)])
def test_backward_sampling_has_the_joint_posterior_moments(model, d, irregular, log_sigma_obs, cov_tol):
    pb, par = _problem(model, d, irregular, log_sigma_obs)
    for k, L in enumerate(LENGTHS):
        if L < 2:
            continue
        mean, A = _affine_map(pb, par, k)
        jm, jcov = joint_full(pb, par, k)
        gap_c = np.max(np.abs(A @ A.T - jcov)) / np.max(np.abs(jcov))
        gap_m = np.max(np.abs(mean - jm)) / (1.0 + np.max(np.abs(jm)))
        print(f"GAP {model} d={d} irregular={irregular} lso={log_sigma_obs} track={k}: cov {gap_c:.2e} mean {gap_m:.2e}")
        assert gap_c <= cov_tol, (k, gap_c)
        assert gap_m <= 1e-10, (k, gap_m)


@pytest.mark.parametrize("model", MODELS)
def test_a_draw_is_a_pure_function_of_its_number(model):
    pb, par = _problem(model, 2, True, -1.0)
    whole = draws_ref(pb, par, seed=7, draw0=0, n_draws=8)
    part = draws_ref(pb, par, seed=7, draw0=4, n_draws=4)
    assert np.array_equal(whole[4:], part, equal_nan=True)
    assert not np.array_equal(whole[:4], part, equal_nan=True)
    other = draws_ref(pb, par, seed=8, draw0=0, n_draws=1)
    assert not np.array_equal(whole[0], other[0], equal_nan=True)


@pytest.mark.parametrize("model", MODELS)
def test_nan_exactly_on_rows_without_a_state(model):
    pb, par = _problem(model, 1, False, -1.0)
    out = draws_ref(pb, par, seed=1, n_draws=3)
    state = np.ones(pb.n, dtype=bool)
    state[pb.seg_start] = False                         # first rows; the one-row track (row 9) is its own first row
    assert out.shape == (3, pb.n, pb.sdim)
    assert np.all(np.isnan(out[:, ~state])) and np.all(np.isfinite(out[:, state]))
    assert not state[9] and state[11] and state[4] and state[15]          # NA rows carry states


def test_philox_deviates_are_standard_normal_and_keyed_by_column_pair():
    from draws_ref import philox_normals
    from sim_ref import normal_pair
    z = philox_normals(3, 5, 2, 11, 4000, 4)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    n1, n2 = normal_pair(3, np.uint64(11), np.uint64(17), np.uint64(6 * 8 + 1))        # draw 6 = draw0 + 1, columns 2 and 3
    assert z[1, 17, 2] == n1 and z[1, 17, 3] == n2


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_ssde_smooth_draws_is_part_of_the_abi():
    text = open(os.path.join(ROOT, "include", "ssde.h")).read()
    assert re.search(r"int\s+ssde_smooth_draws\s*\(\s*ssde_handle\s*\*h,\s*const double\s*\*par,\s*int32_t n_par_full,\s*uint64_t seed,"
                     r"\s*int64_t draw0,\s*int32_t n_draws,\s*double\s*\*draws,\s*uint32_t flags\)", text)
    assert re.search(r"#define\s+SSDE_DRAWS_DEVICE_OUT\s+1u", text)
    assert "ssde_smooth_draws" in capi.EXPORTED_SYMBOLS and capi.DRAWS_DEVICE_OUT == 1
    assert hasattr(capi.Engine, "smooth_draws")
    from smoothsde_amd.sde import SDE
    assert hasattr(SDE, "sample_states")
