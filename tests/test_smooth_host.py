"""The fixed-interval smoother without a GPU: the numpy reference smoother (tests/smooth_ref.py) against the dense
joint Gaussian of each track, the direct families' residuals against a literal restatement of the reference's SDE$residuals()
(R/sde.R:1186-1228), and the C ABI / Python surface of ssde_smooth."""
import os
import re

import numpy as np
import pytest

from cases import make_spec, problem_from_spec
from smooth_ref import joint_track, smooth_ref
from smoothsde_amd import capi
from smoothsde_amd.sde import SDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_against_joint(pb, par, tol=1e-9):
    ref = smooth_ref(pb, par)
    bounds = list(pb.seg_start) + [pb.n]
    for k in range(pb.n_seg):
        r0, r1 = bounds[k], bounds[k + 1]
        assert np.all(np.isnan(ref["mean"][r0])) and np.all(np.isnan(ref["resid"][r0]))
        if r1 - r0 < 2:
            continue
        m, V, e = joint_track(pb, par, k)
        scale = 1.0 + np.max(np.abs(m))
        vscale = np.max(np.abs(V))
        assert np.max(np.abs(ref["mean"][r0 + 1:r1] - m)) <= tol * scale, k
        assert np.max(np.abs(ref["cov"][r0 + 1:r1] - V)) <= tol * vscale, k
        assert np.array_equal(np.isnan(ref["resid"][r0 + 1:r1]), np.isnan(e)), k
        ok = ~np.isnan(e)
        assert np.max(np.abs(ref["resid"][r0 + 1:r1][ok] - e[ok]), initial=0.0) <= tol * 10, k


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_reference_smoother_is_the_joint_gaussian_conditional(model, d):
    # irregular times, NA rows (one ending a track), a coupling per-row H_array and a general P0, plus a one-row track
    lengths = [12, 25, 1, 40, 7]
    spec = make_spec(f"sm_{model}_{d}", model, d, seed=11 + d, lengths=lengths, with_H=True, with_P0=True,
                     na_rows=(4, 5, 20, 36, 37 + 39))
    pb = problem_from_spec(spec)
    _check_against_joint(pb, spec["par"])


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
def test_reference_smoother_with_row_varying_parameters_and_isotropic_noise(model):
    spec = make_spec(f"sm_tv_{model}", model, 2, seed=5, lengths=[30, 18, 44], variant="tv", na_rows=(3, 29, 50))
    pb = problem_from_spec(spec)
    _check_against_joint(pb, spec["par"])


def test_last_row_without_fix_is_the_forward_prediction():
    spec = make_spec("sm_tail", "CTCRW", 2, seed=3, lengths=[20, 15], na_rows=(19, 33, 34))
    pb = problem_from_spec(spec)
    ref = smooth_ref(pb, spec["par"])
    m, V, _ = joint_track(pb, spec["par"], 0)
    assert np.allclose(ref["mean"][19], m[-1], rtol=0, atol=1e-10 * (1 + np.abs(m).max()))
    assert np.all(np.isnan(ref["resid"][[0, 19, 20, 33, 34]]))


# ---- direct families: R/sde.R:1186-1228, line by line ------------------------------------------------------------------------
def _residuals_literal(data, typ, response, par, df=None):
    ID, time = np.asarray(data["ID"]), np.asarray(data["time"], dtype=float)
    n = len(ID)
    break_ind = np.nonzero(ID[1:] != ID[:-1])[0] + 1          # which(ID[-1] != ID[-n]), 1-based
    start_ind = np.r_[1, break_ind + 1]
    end_ind = np.r_[break_ind, n]
    drop = lambda x, ind: np.delete(x, ind - 1, axis=0)      # x[-ind]
    dtimes = drop(time, start_ind) - drop(time, end_ind)
    Z = np.column_stack([np.asarray(data[r], dtype=float) for r in response])
    if typ in ("BM", "BM_t"):
        mean = drop(Z, end_ind) + drop(par["mu"], end_ind)[:, None] * dtimes[:, None]
        sd = (drop(par["sigma"], end_ind) * np.sqrt(dtimes))[:, None]
        if typ == "BM_t":
            sd = sd / np.sqrt(df / (df - 2))
    else:
        mu = np.column_stack([drop(par[k], end_ind) for k in par if k.startswith("mu")])
        tau, kappa = drop(par["tau"], end_ind)[:, None], drop(par["kappa"], end_ind)[:, None]
        mean = mu + np.exp(-dtimes[:, None] / tau) * (drop(Z, end_ind) - mu)
        sd = np.sqrt(kappa * (1 - np.exp(-2 * dtimes[:, None] / tau)))
    res = np.full((n, Z.shape[1]), np.nan)
    keep = np.delete(np.arange(n), end_ind - 1)
    res[keep] = (drop(Z, start_ind) - mean) / sd
    return res


@pytest.mark.parametrize("typ,d", [("BM", 1), ("BM_t", 1), ("OU", 1), ("OU", 2)])
def test_direct_family_residuals_follow_the_reference(typ, d):
    rng = np.random.default_rng(7)
    lengths = [9, 1, 14, 6]
    ID = np.repeat(np.arange(len(lengths), dtype=float), lengths)
    n = len(ID)
    time = np.concatenate([np.cumsum(rng.uniform(0.2, 1.5, L)) for L in lengths])
    x = rng.uniform(0, 1, n)
    data = {"ID": ID, "time": time, "x": x}
    resp = ["z%d" % a for a in range(d)]
    for r in resp:
        data[r] = rng.standard_normal(n).cumsum()
    names = (["mu"] if d == 1 else ["mu%d" % (a + 1) for a in range(d)]) + (["sigma"] if typ != "OU" else ["tau", "kappa"])
    formulas = {k: "~1" for k in names}
    formulas[names[-1]] = "~x"                                 # a row-varying parameter
    other = {"df": 6.0} if typ == "BM_t" else None
    sde = SDE(formulas=formulas, data=data, type=typ, response=resp if d > 1 else resp[0], other_data=other)
    sde.coeff_fe_ = rng.uniform(-0.5, 0.5, len(sde.coeff_fe_))
    got = sde.residuals()
    want = _residuals_literal(data, typ, resp, sde.par(), df=6.0)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.all(np.isnan(got[np.r_[8, 9, 23, 29]]))         # every track's last row (and the one-row track)
    np.testing.assert_allclose(got[~np.isnan(got)], want[~np.isnan(want)], rtol=1e-13, atol=0)


def test_models_without_residuals_raise():
    rng = np.random.default_rng(1)
    data = {"ID": np.zeros(10), "time": np.arange(10.0), "z": np.exp(rng.standard_normal(10))}
    with pytest.raises(NotImplementedError):
        SDE(data=data, type="CIR", response="z").residuals()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_ssde_smooth_is_part_of_the_abi():
    assert "ssde_smooth" in capi.EXPORTED_SYMBOLS
    assert capi.ABI_VERSION == 12 and capi.OPT_SMOOTH_BUDGET_MB == 3
    hdr = open(os.path.join(ROOT, "include", "ssde.h")).read()
    assert re.search(r"^int ssde_smooth\(ssde_handle \*h, const double \*par, int32_t n_par_full, double \*a_smooth, "
                     r"double \*P_smooth, double \*resid\);", hdr, re.M)
    assert re.search(r"SSDE_OPT_SMOOTH_BUDGET_MB = 3", hdr)
    assert callable(getattr(capi.Engine, "smooth", None))
    assert callable(getattr(SDE, "smooth_states", None)) and callable(getattr(SDE, "residuals", None))


def test_the_built_library_exports_ssde_smooth():
    if not os.path.exists(capi.lib_path()):
        pytest.skip("libssde_hip.so not built")
    lib = capi.load_library()
    assert hasattr(lib, "ssde_smooth")
