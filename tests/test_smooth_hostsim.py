"""The smoother's lane math on the CPU: tests/hostsim compiles csrc/ssde_smooth.hpp over csrc/ssde_dense.hpp with
g++ and walks each track the way one lane does -- smooth_record_row into a plain per-row record, dense_step, then smooth_back_row
over the records (hostsim_lib.smooth).  That twin is compared with the numpy reference smoother (tests/smooth_ref.py) and, track by
track, with the dense joint Gaussian (joint_track: no recursion at all), for the three Kalman families at every width the engine
instantiates (d = 1 ... 8) and on the row-varying, a0 / P0, NA and detF <= 0 inputs.

Limits: twin against smooth_ref as the GPU suite's _compare (mean 1e-10 (1 + max|ref|), covariance 1e-9 max|ref|, residual 1e-9, NaN
patterns identical); twin and smooth_ref against joint_track 1e-9 (test_smooth_host.py's).  Largest gaps measured on these inputs:
smooth_ref against joint_track 3.4e-14 (mean, relative), 2.7e-13 (covariance, relative), 9.6e-13 (residual); the twin against joint_track
the same to two digits; the twin against smooth_ref 2.4e-15, 4.9e-14, 8.7e-14."""
import numpy as np
import pytest

import hostsim_lib
from cases import drift_spec, make_spec, problem_from_spec
from smooth_ref import joint_track, smooth_ref
from smoothsde_amd import capi
from smoothsde_amd.synth import simulate

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
GAPS = {}                                                     # the largest gaps seen, by comparison (printed by -s runs)


def _note(what, mean, cov, res):
    g = GAPS.setdefault(what, [0.0, 0.0, 0.0])
    g[0], g[1], g[2] = max(g[0], mean), max(g[1], cov), max(g[2], res)


def _twin_vs_ref(got, ref, resid=True):
    """The GPU suite's _compare (test_gpu_smooth.py), on the host twin."""
    gaps = []
    for key in ("mean", "cov", "resid"):
        g, r = got[key], ref[key]
        assert np.array_equal(np.isnan(g), np.isnan(r)), key
        ok = ~np.isnan(r)
        if not ok.any() or (key == "resid" and not resid):
            gaps.append(0.0)
            continue
        scale = {"mean": 1.0 + np.max(np.abs(r[ok])), "cov": np.max(np.abs(r[ok])), "resid": 1.0}[key]
        tol = {"mean": 1e-10, "cov": 1e-9, "resid": 1e-9}[key]
        err = np.max(np.abs(g[ok] - r[ok]))
        assert err <= tol * scale, (key, err, tol * scale)
        gaps.append(err / scale)
    _note("twin_vs_ref", *gaps)


def _vs_joint(what, out, pb, par, tol=1e-9):
    """test_smooth_host.py's _check_against_joint, for the reference's or the twin's output."""
    bounds = list(pb.seg_start) + [pb.n]
    for k in range(pb.n_seg):
        r0, r1 = bounds[k], bounds[k + 1]
        assert np.all(np.isnan(out["mean"][r0])) and np.all(np.isnan(out["cov"][r0])) and np.all(np.isnan(out["resid"][r0]))
        if r1 - r0 < 2:
            continue
        m, V, e = joint_track(pb, par, k)
        scale = 1.0 + np.max(np.abs(m))
        vscale = np.max(np.abs(V))
        em = np.max(np.abs(out["mean"][r0 + 1:r1] - m))
        ev = np.max(np.abs(out["cov"][r0 + 1:r1] - V))
        assert em <= tol * scale, (what, k, em)
        assert ev <= tol * vscale, (what, k, ev)
        assert np.array_equal(np.isnan(out["resid"][r0 + 1:r1]), np.isnan(e)), (what, k)
        ok = ~np.isnan(e)
        ee = np.max(np.abs(out["resid"][r0 + 1:r1][ok] - e[ok]), initial=0.0)
        assert ee <= tol * 10, (what, k, ee)
        _note(what + "_vs_joint", em / scale, ev / vscale, ee)


def _check(pb, par):
    ref = smooth_ref(pb, par)
    got = hostsim_lib.smooth(pb, par)
    _twin_vs_ref(got, ref)
    _vs_joint("ref", ref, pb, par)
    _vs_joint("twin", got, pb, par)
    return got, ref


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8])
def test_twin_every_model_and_width(model, d):
    # irregular times, a coupling per-row H_array, an NA row inside a track and one ending it (row 19), a one-row track;
    # a general P0 at d = 2, 5, 8
    spec = make_spec(f"hs_{model}_{d}", model, d, seed=40 + d, lengths=[20, 35, 1, 14], with_H=True, with_P0=d in (2, 5, 8),
                     na_rows=(2, 19))
    pb = problem_from_spec(spec)
    got, _ = _check(pb, spec["par"])
    assert np.all(np.isnan(got["resid"][[0, 2, 19, 20, 55, 56]])) and np.all(np.isfinite(got["mean"][[2, 19]]))
    assert np.all(np.isnan(got["mean"][55]))                  # the one-row track has no state row


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("variant", ["tv", "tv2"])
def test_twin_row_varying_parameters(model, d, variant):
    # tau (sigma for BM) with a slope, a smooth on the last parameter (mu_0 for BM); tv2: a second smooth (mu_0; sigma for BM)
    spec = make_spec(f"hs_{variant}_{model}_{d}", model, d, seed=5 + d, lengths=[30, 18, 1, 44], variant=variant, na_rows=(3, 29, 51))
    pb = problem_from_spec(spec)
    _check(pb, spec["par"])


def test_twin_two_smooths_with_r_na():
    # R's NA_real_ marks the missing rows (na_mode = 0), two smooths
    spec = make_spec("hs_tv2_rna", "CTCRW", 2, seed=171, lengths=[15, 9], variant="tv2", na_rows=(6, 7), na_mode=0)
    pb = problem_from_spec(spec)
    got, _ = _check(pb, spec["par"])
    assert np.all(np.isnan(got["resid"][[6, 7]])) and np.all(np.isfinite(got["mean"][[6, 7]]))


@pytest.mark.parametrize("case", ["OU_SSM_d1", "CTCRW_d2", "BM_SSM_d2_fixsig", "CTCRW_d1_fe"])
def test_twin_row_varying_drift(case):
    # the drift_spec cases of cases.py: mu smooth in a covariate (one and two smooths, a fixed-effect slope, a fixed sigma_obs)
    spec = {"OU_SSM_d1": lambda: drift_spec("OU_SSM_d1_drift", "OU_SSM", 1, seed=251),
            "CTCRW_d2": lambda: drift_spec("CTCRW_d2_drift", "CTCRW", 2, seed=252, smooth_dims=(0, 1)),
            "BM_SSM_d2_fixsig": lambda: drift_spec("BM_SSM_d2_drift_fixsig", "BM_SSM", 2, seed=253, smooth_dims=(1,), fix=(0,)),
            "CTCRW_d1_fe": lambda: drift_spec("CTCRW_d1_drift_fe", "CTCRW", 1, seed=254, fe_slope=True, smooth_dims=())}[case]()
    pb = problem_from_spec(spec)
    _check(pb, spec["par"])


@pytest.mark.parametrize("model", MODELS)
def test_twin_callers_a0_and_block_p0(model):
    # the construction of test_gpu_edge_cases.py::test_user_a0_and_block_identical_p0_stay_on_register_path, shortened
    M, T = 6, 25
    ID, times, obs = simulate(model, M, T, 2, seed=6)
    sd = 4 if model == "CTCRW" else 2
    a0 = np.zeros((M, sd))
    if model == "CTCRW":
        a0[:, 0] = obs[::T, 0] + 0.3; a0[:, 1] = 0.2; a0[:, 2] = obs[::T, 1]; a0[:, 3] = -0.1
        P0 = np.kron(np.eye(2), np.array([[2.0, 0.3], [0.3, 4.0]]))
        par = [-0.8, 0.05, -0.05, 0.4, 0.1]
    else:
        a0[:, 0] = obs[::T, 0] + 0.3; a0[:, 1] = obs[::T, 1] - 0.2
        P0 = 3.0 * np.eye(2)
        par = [-0.8, 0.05, -0.05, 0.4, 0.1][:4 if model == "BM_SSM" else 5]
    a0 += 0.01 * np.arange(M)[:, None]                         # every track its own: a wrong track index shows
    obs[7] = np.nan
    pb = capi.Problem(model, ID, times, obs, a0=a0, P0=P0)
    _check(pb, np.array(par))


@pytest.mark.parametrize("model", MODELS)
def test_twin_r_na_in_column_0_only(model):
    # na_mode = 0: the row is missing when obs(i, 0) is R's NA_real_, whatever column 1 holds (nllk_ctcrw.hpp:209) -- its residual
    # is NaN, its state a prediction, and column 1's finite value is not used
    spec = make_spec(f"hs_rna_{model}", model, 2, seed=17, lengths=[16, 1, 22], na_mode=0)
    for r in (5, 15, 30):                                     # row 15 ends the first track
        spec["obs"][r, 0] = capi.na_real()
    pb = problem_from_spec(spec)
    got, _ = _check(pb, spec["par"])
    assert np.all(np.isnan(got["resid"][[5, 15, 30]])) and np.all(np.isfinite(got["mean"][[5, 15, 30]]))
    spec2 = dict(spec, obs=spec["obs"].copy())
    spec2["obs"][[5, 15, 30], 1] += 100.0
    other = hostsim_lib.smooth(problem_from_spec(spec2), spec["par"])
    for k in got:
        assert np.array_equal(got[k], other[k], equal_nan=True), k


@pytest.mark.parametrize("model", MODELS)
def test_twin_plain_nan_is_data_under_r_na_semantics(model):
    # na_mode = 0: only R's NA_real_ marks a missing row; a plain NaN is an observation like any other and takes the update, so the
    # track's means are NaN from there on (and, through r, before it), the covariances -- which never see y -- stay finite, and
    # the row's residual is NaN from the NaN column on.  No Gaussian to condition on: the twin against smooth_ref only.
    spec = make_spec(f"hs_nan_{model}", model, 2, seed=17, lengths=[16, 1, 22], na_mode=0)
    spec["obs"][5, 0] = capi.na_real()
    spec["obs"][8, 0] = np.nan                                 # column 0, yet not missing
    spec["obs"][25, 1] = np.nan
    pb = problem_from_spec(spec)
    with np.errstate(invalid="ignore"):
        ref = smooth_ref(pb, spec["par"])
    got = hostsim_lib.smooth(pb, spec["par"])
    assert np.all(np.isnan(ref["mean"][1:16])) and np.all(np.isnan(ref["mean"][18:])) and np.all(np.isfinite(ref["cov"][18:]))
    assert np.isfinite(ref["resid"][25, 0]) and np.isnan(ref["resid"][25, 1]) and np.all(np.isfinite(ref["resid"][[6, 7]]))
    _twin_vs_ref(got, ref)


@pytest.mark.parametrize("model", MODELS)
def test_twin_nonpositive_innovation_variance_branch(model):
    """The negative-P0 construction of test_gpu_edge_cases.py::test_nonpositive_innovation_variance_branch (d = 1): CTCRW skips
    the update while det F <= 0 and then predicts without B mu; OU_SSM / BM_SSM update whenever |det F| > 0, with a negative
    F whose whitened innovation is NaN (no Cholesky factor).  An ordinary finite computation; there is no Gaussian with a
    negative variance, so the joint does not apply."""
    ID, times, obs = simulate(model, 5, 12, 1, seed=4)
    sdim = 2 if model == "CTCRW" else 1
    P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
    par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
    pb = capi.Problem(model, ID, times, obs, P0=P0)
    ref = smooth_ref(pb, par)
    got = hostsim_lib.smooth(pb, par)
    state = np.ones(pb.n, dtype=bool)
    state[pb.seg_start] = False
    assert np.all(np.isfinite(ref["mean"][state])) and np.all(np.isfinite(ref["cov"][state]))
    assert np.all(np.isnan(ref["resid"][pb.seg_start + 1]))      # the first state row of every track: F = P0 + h < 0
    assert np.any(np.isfinite(ref["resid"]))                     # ... and the filter recovers on later rows
    _twin_vs_ref(got, ref)


def _fuzz_cases():
    from test_gpu_smooth_layouts import FUZZ_SEEDS, FUZZ_WIDE_SEEDS
    return [(s, False) for s in FUZZ_SEEDS] + [(s, True) for s in FUZZ_WIDE_SEEDS]


@pytest.mark.parametrize("seed,wide", _fuzz_cases())
def test_fuzz_seeds_are_sound(seed, wide):
    """The seeds of test_gpu_smooth_layouts.py's fuzz: on every one smooth_ref is finite wherever a state exists and agrees with the
    joint Gaussian (a seed that does not is replaced there, the limits stay); the twin runs them as well."""
    from test_gpu_fuzz import random_problem
    pb, par = random_problem(seed, wide=wide)
    assert pb.model in MODELS
    _, ref = _check(pb, par)
    state = np.ones(pb.n, dtype=bool)
    state[pb.seg_start] = False
    assert np.all(np.isfinite(ref["mean"][state])) and np.all(np.isfinite(ref["cov"][state]))
