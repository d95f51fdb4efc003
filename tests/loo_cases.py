"""Cases, limits, thresholds and the comparison shared by the tests of ssde_smooth_loo (test infrastructure).

Limits.  Mean, covariance and residual take the smoother's: mean 1e-10 (1 + max|ref|), covariance 1e-9 max|ref|,
residual 1e-9.  lpd and the statistics k = 1 (the sum of lpd), k = 2 (the largest q) are compared at LPD_TOL (1 + max|ref|): two
decades above the largest gap measured on the CPU cases below, twin against loo_ref and loo_ref against loo_joint (the figures are
in DESIGN.md §3.20 and in test_loo_hostsim.py's docstring).  NaN patterns are compared exactly, and so are the statistics k = 0, 3
and the counts: the thresholds of a count test lie midway between neighbouring sorted reference q_j (midway_thresholds), and a
comparison asserts that the two largest q_j of a track are clear of each other before it compares the row of the maximum."""
import numpy as np

from cases import make_spec, problem_from_spec
from smoothsde_amd import capi
from smoothsde_amd.synth import simulate

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
MEAN_TOL, COV_TOL, RESID_TOL = 1e-10, 1e-9, 1e-9
LPD_TOL = 1e-11


def width_case(model, d):
    """irregular times, a coupling per-row H_array, an NA row inside a track and one ending it (row 19), a one-row track; a general
    P0 at d = 2, 5, 8 (test_smooth_hostsim.py's construction)"""
    spec = make_spec(f"loo_{model}_{d}", model, d, seed=40 + d, lengths=[20, 35, 1, 14], with_H=True, with_P0=d in (2, 5, 8),
                     na_rows=(2, 19))
    return problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)


def tv_case(model, d, variant):
    """tau (sigma for BM) with a slope, a smooth on the last parameter; tv2: a second smooth.  Isotropic sigma_obs^2 I noise."""
    spec = make_spec(f"loo_{variant}_{model}_{d}", model, d, seed=5 + d, lengths=[30, 18, 1, 44], variant=variant, na_rows=(3, 29, 51))
    return problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)


def a0_case(model):
    """a caller's a0 (every track its own) with a block P0"""
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
    a0 += 0.01 * np.arange(M)[:, None]
    obs[7] = np.nan
    return capi.Problem(model, ID, times, obs, a0=a0, P0=P0), np.array(par)


def rna_case(model):
    """na_mode = 0: a row is missing when obs(i, 0) is R's NA_real_, whatever column 1 holds; row 15 ends the first track"""
    spec = make_spec(f"loo_rna_{model}", model, 2, seed=17, lengths=[16, 1, 22], na_mode=0)
    for r in (5, 15, 30):
        spec["obs"][r, 0] = capi.na_real()
    return problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)


def negative_p0_case(model):
    """det F <= 0 on every track's first state rows (negative P0, d = 1): no Gaussian, so loo_ref only"""
    ID, times, obs = simulate(model, 5, 12, 1, seed=4)
    sdim = 2 if model == "CTCRW" else 1
    P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
    par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
    return capi.Problem(model, ID, times, obs, P0=P0), par


def host_cases():
    """(id, builder, has_joint, constant_H): every case the CPU suite runs"""
    out = []
    for model in MODELS:
        for d in range(1, 9):
            out.append((f"{model}-d{d}", (lambda m=model, k=d: width_case(m, k)), True, False))
        for d in (1, 2):
            for variant in ("tv", "tv2"):
                out.append((f"{model}-d{d}-{variant}", (lambda m=model, k=d, v=variant: tv_case(m, k, v)), True, True))
        out.append((f"{model}-a0", (lambda m=model: a0_case(m)), True, True))
        out.append((f"{model}-rna", (lambda m=model: rna_case(m)), True, True))
        out.append((f"{model}-negP0", (lambda m=model: negative_p0_case(m)), False, True))
    return out


def midway_thresholds(q, n_thr=8):
    """n_thr thresholds on the q scale, each midway between two neighbouring sorted finite reference q_j (spread over the order
    statistics), so no count hangs on rounding; the gap they sit in is asserted to be wide enough to hold a 1e-9 error"""
    s = np.sort(q[np.isfinite(q)])
    assert len(s) >= 2
    pos = np.unique(np.linspace(0, len(s) - 2, n_thr).round().astype(int))
    thr = 0.5 * (s[pos] + s[pos + 1])
    assert np.all(s[pos + 1] - s[pos] > 1e-7 * (1.0 + s[pos + 1])), "two reference q_j too close for a threshold between them"
    return thr


def clear_maxima(ref, bounds):
    """whether, in every track, the two largest reference q_j differ by more than 1e-7 (1 + max): the row of the maximum is then
    the same for any implementation within the limits"""
    for k in range(len(bounds) - 1):
        s = np.sort(ref["q"][bounds[k]:bounds[k + 1]][ref["white"][bounds[k]:bounds[k + 1]]])
        if len(s) >= 2 and not s[-1] - s[-2] > 1e-7 * (1.0 + s[-1]):
            return False
    return True


def compare(got, ref, bounds=None, gaps=None, lpd_tol=LPD_TOL):
    """`got` (the twin's or the engine's outputs) against loo_ref's: NaN patterns exactly, values at the limits above; the statistics
    where `got` carries them.  gaps: a dict that collects the largest relative gaps seen."""
    note = (lambda k, v: gaps.__setitem__(k, max(gaps.get(k, 0.0), v))) if gaps is not None else (lambda k, v: None)
    for key, tol, scale_of in (("mean", MEAN_TOL, lambda r: 1.0 + np.max(np.abs(r))), ("cov", COV_TOL, lambda r: np.max(np.abs(r))),
                               ("resid", RESID_TOL, lambda r: 1.0), ("lpd", lpd_tol, lambda r: 1.0 + np.max(np.abs(r)))):
        g, r = got.get(key), ref[key]
        if g is None:
            continue
        assert g.shape == r.shape, (key, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (key, np.nonzero(np.isnan(g) != np.isnan(r))[0][:8])
        ok = ~np.isnan(r)
        if not ok.any():
            continue
        scale = scale_of(r[ok])
        err = np.max(np.abs(g[ok] - r[ok]))
        note(key, err / scale)
        assert err <= tol * scale, (key, err, tol * scale)
    if got.get("stats") is None:
        return
    gs, rs = got["stats"], ref["stats"]
    assert gs.shape == rs.shape, (gs.shape, rs.shape)
    assert np.array_equal(gs[:, 0], rs[:, 0]), "served rows"
    assert np.array_equal(np.isnan(gs), np.isnan(rs))
    for k in (1, 2):
        ok = ~np.isnan(rs[:, k])
        if ok.any():
            scale = 1.0 + np.max(np.abs(rs[ok, k]))
            err = np.max(np.abs(gs[ok, k] - rs[ok, k]))
            note(f"stats{k}", err / scale)
            assert err <= lpd_tol * scale, (k, err, lpd_tol * scale)
    if bounds is not None:
        assert clear_maxima(ref, bounds), "two reference maxima too close: change the case, not the limit"
    assert np.array_equal(gs[:, 3], rs[:, 3], equal_nan=True), "row of the maximum"
    assert np.array_equal(gs[:, 4:], rs[:, 4:]), "counts"
