"""Leave-one-out residuals and predictive densities without a GPU: the numpy definition (tests/loo_ref.py: the
smoother's recursion with w_j, M_j added) against the dense joint Gaussian of each track with block j deleted (loo_joint: no
recursion), the identities that tie ssde_smooth_loo to ssde_smooth, and the C ABI / Python surface of the call.

Limits (loo_cases.py): mean 1e-10 (1 + max|ref|), covariance 1e-9 max|ref|, residual 1e-9 -- the smoother's; lpd and the statistics
k = 1, 2 at 1e-11 (1 + max|ref|), two decades above the largest gap measured on these inputs (loo_ref against loo_joint: lpd 9.5e-14,
sum of lpd 1.6e-14, largest q 9.8e-14, all relative to 1 + max|ref|; mean 8.3e-15, covariance 1.5e-13, residual 6.6e-13; w_j
9.0e-12 and M_j 8.6e-13 relative to their largest entry)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import loo_cases as LC
from loo_ref import loo_joint, loo_ref
from smooth_ref import _setup, smooth_ref
from smoothsde_amd import capi
from smoothsde_amd.capi import LOO_MAX_THR               # the feature itself: without it nothing below is worth running
from smoothsde_amd.sde import SDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = LC.host_cases()
_REF = {}


def _case(cid):
    """(pb, par, loo_ref with its midway thresholds, smooth_ref): computed once per case, shared, never changed"""
    if cid not in _REF:
        build = next(b for c, b, _, _ in CASES if c == cid)
        pb, par = build()
        with np.errstate(invalid="ignore"):
            thr = LC.midway_thresholds(loo_ref(pb, par)["q"])
            _REF[cid] = (pb, par, loo_ref(pb, par, thr), smooth_ref(pb, par), thr)
    return _REF[cid]


@pytest.mark.parametrize("cid", [c for c, _, joint, _ in CASES if joint])
def test_reference_is_the_joint_gaussian_with_the_block_deleted(cid):
    pb, par, ref, _, _ = _case(cid)
    bounds = list(pb.seg_start) + [pb.n]
    for k in range(pb.n_seg):
        r0, r1 = bounds[k], bounds[k + 1]
        for key in ("mean", "cov", "resid", "lpd"):
            assert np.all(np.isnan(ref[key][r0])), (key, k)               # a track's first row is never served
        if r1 - r0 < 2:
            assert np.array_equal(ref["stats"][k], [0, 0, np.nan, np.nan] + [0] * (ref["stats"].shape[1] - 4), equal_nan=True)
            continue
        m, V, z, lp, wj, Mj = loo_joint(pb, par, k)
        got = {key: ref[key][r0 + 1:r1] for key in ("mean", "cov", "resid", "lpd")}
        LC.compare(got, {"mean": m, "cov": V, "resid": z, "lpd": lp})
        # the recursion's w_j and M_j are the blocks of Sigma_yy^-1 (y - m) and of Sigma_yy^-1
        ok = ~np.isnan(lp)
        assert np.max(np.abs(ref["w"][r0 + 1:r1][ok] - wj[ok])) <= 1e-9 * np.max(np.abs(wj[ok]))
        assert np.max(np.abs(ref["M"][r0 + 1:r1][ok] - Mj[ok])) <= 1e-9 * np.max(np.abs(Mj[ok]))
        # the track's statistics from the joint's rows
        q = np.sum(z[ok] ** 2, axis=1)
        st = ref["stats"][k]
        assert st[0] == ok.sum()
        assert abs(st[1] - lp[ok].sum()) <= LC.LPD_TOL * (1.0 + abs(lp[ok].sum()))
        assert abs(st[2] - q.max()) <= LC.LPD_TOL * (1.0 + q.max())
        assert st[3] == r0 + 1 + np.nonzero(ok)[0][np.argmax(q)]


@pytest.mark.parametrize("cid", [c for c, _, _, _ in CASES])
def test_nan_pattern_is_the_smoothers_and_counts_follow_the_thresholds(cid):
    pb, par, ref, sm, thr = _case(cid)
    assert np.array_equal(ref["served"], ref["white"])                   # every M_j of these cases has both factors
    assert np.array_equal(np.isnan(ref["resid"]), np.isnan(sm["resid"]))
    assert np.array_equal(np.isnan(ref["lpd"]), np.isnan(sm["resid"][:, 0]))
    bounds = list(pb.seg_start) + [pb.n]
    for k in range(pb.n_seg):
        q = ref["q"][bounds[k]:bounds[k + 1]]
        q = q[np.isfinite(q)]
        assert np.array_equal(ref["stats"][k, 4:], [(q > t).sum() for t in thr])
    assert ref["stats"][:, 4].sum() < ref["stats"][:, 0].sum() and ref["stats"][:, 4:].max() > 0


@pytest.mark.parametrize("cid", [c for c, _, _, _ in CASES])
def test_leaving_out_the_last_fix_is_the_one_step_prediction(cid):
    """At a track's last state row, when it is served, loo_mean = obs - v and loo_resid = resid, to 1e-12 relative.  v comes from
    smooth_ref alone: v = C e with C the Cholesky factor of F = Z P_j Z' + H_j, P_j its predicted covariance, e its residual."""
    pb, par, ref, sm, _ = _case(cid)
    bounds = list(pb.seg_start) + [pb.n]
    d, obs = pb.n_dim, np.asarray(pb.obs, dtype=np.float64)
    _, _, Z, H, _, _, _, _ = _setup(pb, par)
    seen = 0
    for k in range(pb.n_seg):
        last = bounds[k + 1] - 1
        if last == bounds[k] or not ref["served"][last]:
            continue
        seen += 1
        assert np.max(np.abs(ref["resid"][last] - sm["resid"][last])) <= 1e-12 * (1.0 + np.max(np.abs(sm["resid"][last])))
        F = Z @ sm["pred_cov"][last] @ Z.T + H[last]
        pred = obs[last, :d] - np.linalg.cholesky(0.5 * (F + F.T)) @ sm["resid"][last]
        assert np.max(np.abs(ref["mean"][last] - pred)) <= 1e-12 * (1.0 + np.max(np.abs(pred)))
    assert seen >= 1


@pytest.mark.parametrize("cid", [c for c, _, joint, const_h in CASES if const_h and joint])
def test_smoothing_error_ties_the_call_to_the_smoother(cid):
    """obs - Z mean_smooth == H_j M_j (obs - loo_mean) on the constant-H cases: the left-hand side comes from smooth_ref"""
    pb, par, ref, sm, _ = _case(cid)
    d = pb.n_dim
    Zc = [2 * a if pb.model == "CTCRW" else a for a in range(d)]
    h = np.exp(par[0]) ** 2
    srv = ref["served"]
    lhs = np.asarray(pb.obs, dtype=np.float64)[srv][:, :d] - sm["mean"][srv][:, Zc]
    M = np.linalg.inv(ref["cov"][srv])
    rhs = h * np.einsum("mij,mj->mi", M, np.asarray(pb.obs, dtype=np.float64)[srv][:, :d] - ref["mean"][srv])
    assert srv.sum() > 10
    assert np.max(np.abs(lhs - rhs)) <= 1e-9 * (1.0 + np.max(np.abs(lhs)))


def test_a_track_without_a_served_row_and_the_shapes():
    pb, par, ref, _, thr = _case("CTCRW-d2")
    assert ref["stats"].shape == (4, 4 + len(thr)) and ref["lpd"].shape == (pb.n,) and ref["cov"].shape == (pb.n, 2, 2)
    assert np.array_equal(ref["stats"][2], [0, 0, np.nan, np.nan] + [0] * len(thr), equal_nan=True)      # the one-row track
    assert np.all(np.isnan(ref["lpd"][[0, 2, 19, 20, 55, 56]])) and np.isfinite(ref["lpd"][[1, 3, 18, 21]]).all()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_ssde_smooth_loo_is_part_of_the_abi():
    assert "ssde_smooth_loo" in capi.EXPORTED_SYMBOLS
    assert capi.ABI_VERSION == 12 and LOO_MAX_THR == 8
    hdr = open(os.path.join(ROOT, "include", "ssde.h")).read()
    assert re.search(r"^int ssde_smooth_loo\(ssde_handle \*h, const double \*par, int32_t n_par_full,\s*"
                     r"double \*loo_mean, double \*loo_cov, double \*loo_resid, double \*lpd,\s*"
                     r"const double \*thr, int32_t n_thr, double \*stats, uint32_t flags\);", hdr, re.M)
    assert re.search(r"^#define SSDE_LOO_MAX_THR 8$", hdr, re.M) and re.search(r"^#define SSDE_ABI_VERSION 12$", hdr, re.M)
    assert callable(getattr(capi.Engine, "smooth_loo", None))
    assert callable(getattr(SDE, "loo", None)) and callable(getattr(SDE, "outliers", None))


def test_the_built_library_exports_ssde_smooth_loo_and_refuses_no_handle():
    assert os.path.exists(capi.lib_path()), "libssde_hip.so not built"
    lib = capi.load_library()
    assert hasattr(lib, "ssde_smooth_loo")
    out = np.zeros(4)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ssde_smooth_loo(None, p, 4, p, None, None, None, None, 0, None, 0) == 1       # SSDE_ERR_ARG, nothing touched
    assert np.all(out == 0.0)


def test_models_without_a_latent_state_raise():
    rng = np.random.default_rng(1)
    data = {"ID": np.zeros(10), "time": np.arange(10.0), "z": np.exp(rng.standard_normal(10))}
    sde = SDE(data=data, type="CIR", response="z")
    with pytest.raises(NotImplementedError, match="no latent state in the model 'CIR'"):
        sde.loo()
    with pytest.raises(NotImplementedError, match="no latent state in the model 'CIR'"):
        sde.outliers()
