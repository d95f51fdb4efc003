"""Batches of tests/test_gpu_hess_windows.py and tests/test_oracle_hess_quad.py: the ragged state-space batch whose long tracks the
Hessian pass of the lane = direction path (csrc/ssde_hess.hip: hess_tv_device, k_tv_hess.hip) cuts into time windows, and the
direct-family batch of the 8 x 8 tiles (k_direct_hess.hip).  No GPU, no engine: problems and parameter vectors only."""
import numpy as np

from smoothsde_amd import capi
from smoothsde_amd.synth import bspline_basis, second_difference_penalty, simulate

RAGGED = (640, 1, 2, 3, 37, 290, 640)       # rows per track, the two long ones at the ends
K_SMOOTH = 5
_SIM = dict(CTCRW=dict(tau=1.0, nu=1.0), OU_SSM=dict(mu=2.0, tau=2.0, kappa=1.0, z0=2.0), BM_SSM=dict(sigma=0.7))


def _covariate(n):
    return np.clip(0.5 + 0.45 * np.sin(np.arange(n) * 0.013), 0.0, 1.0)


def ragged_problem(model, d, long_rows=640, lengths=None, full=None, na_first_column_only=False, missing=True, seed=5, flags=0,
                   smooth=True):
    """(problem, par).  Tracks of `lengths` rows (default RAGGED with its long tracks `long_rows` long), intervals uniform(0.5, 1.5),
    sigma_obs 0.05; the two variance parameters (BM_SSM: its one) get a 5-column B-spline smooth of a covariate, mu is an intercept;
    everything free.  smooth=False: constant coefficients.

    Missing rows, in STEPS of the first long track (step s of a track is its row s + 1: the first row starts the filter, k_tv_hess.hip
    row_of): every multiple of 16 in 160 .. 320 -- windows start at multiples of WIN_ALIGN = 16, so whatever the plan some window starts
    its warm-up and some window its scored rows on a missing row --, a run of 20 from 400; and the second row of the second long track.
    na_first_column_only: on every other such row (d = 2) only the FIRST response column is NaN -- the row is missing all the same
    (the likelihood looks at the first column alone, nllk_ctcrw.hpp:214) and its second column must not be used.

    full: None (isotropic lanes), "H" (per-row 2 x 2 error ellipses, test_gpu_colvar._with_h; log_sigma_obs is then not in the model)
    or "P0" (a general initial covariance)."""
    lengths = list(lengths) if lengths is not None else [long_rows if L == 640 else L for L in RAGGED]
    T = max(lengths)
    ID, _, obs = simulate(model, len(lengths), T, d, sigma_obs=0.05, seed=seed, **_SIM[model])
    keep = np.concatenate([np.arange(T) < L for L in lengths])
    ID, obs = ID[keep], obs[keep].copy()
    n = len(ID)
    times = np.cumsum(np.random.default_rng(seed + 1).uniform(0.5, 1.5, size=n))
    start = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    if missing:
        longs = [k for k, L in enumerate(lengths) if L == T]
        steps = [s for s in range(160, 321, 16)] + list(range(400, 420))
        rows = [start[longs[0]] + s + 1 for s in steps if s + 1 < T]
        if len(longs) > 1:
            rows.append(start[longs[-1]] + 1)
        for k, r in enumerate(rows):
            if na_first_column_only and d == 2 and k % 2 == 0:
                obs[r, 0] = np.nan
            else:
                obs[r, :] = np.nan
    q = capi.n_sde_par(model, d)
    X_re, S = [None] * q, []
    if smooth:
        x = _covariate(n)
        for j in range(d, q):
            X_re[j] = bspline_basis(x if j == d else np.clip(x ** 2, 0, 1), K_SMOOTH)
            S.append(second_difference_penalty(K_SMOOTH))
    kw = {}
    if full == "H":
        from test_gpu_colvar import _with_h
        proto = capi.Problem(model, ID, times, obs, X_re=X_re, S_list=S)
        kw["H"] = _with_h(proto, seed + 2)
    elif full == "P0":
        sd = 2 * d if model == "CTCRW" else d
        A = np.random.default_rng(seed + 3).standard_normal((sd, sd))
        kw["P0"] = A @ A.T + np.eye(sd)
    pb = capi.Problem(model, ID, times, obs, X_re=X_re, S_list=S, flags=flags, **kw)
    par = np.zeros(pb.n_par_full)
    k_re = 0
    for k, nm in enumerate(pb.par_names()):
        if nm == "log_sigma_obs":
            par[k] = np.log(0.05)
        elif nm.startswith("log_lambda"):
            par[k] = 0.2 - 0.1 * int(nm[11:-1])
        elif nm.startswith("coeff_re"):
            par[k] = 0.1 * np.sin(k_re)
            k_re += 1
        else:
            j = int(nm[9:nm.index("]")])
            par[k] = (2.0 if model == "OU_SSM" else 0.0) if j < d else (0.1 if j == d else -0.1)
    return pb, par


def free_entries(pb):
    return [k for k in range(pb.n_par_full) if not pb.par_fixed[k]]


def direction_entries(pb):
    """the free entries that are directions of the data term (everything but log_lambda)"""
    return [k for k in free_entries(pb) if not (pb.off_lambda <= k < pb.off_lambda + pb.n_smooth)]


# ---- the direct families' tiles -----------------------------------------------------------------------------------------------------
DIRECT_LENGTHS = (300, 1, 77)


def direct_problem(model, d, n_cols, seed=9):
    """(problem, par): BM / OU, tracks of 300, 1 and 77 rows with missing rows (the first of a track's, an isolated one, a pair), the
    first parameter (mu_1) with an intercept and `n_cols` spline columns -- with the other intercepts and log_lambda that is
    n_cols + q + 1 entries for ssde_hess, cut into 8 x 8 tiles."""
    T = max(DIRECT_LENGTHS)
    ID, _, obs = simulate(model, len(DIRECT_LENGTHS), T, d, seed=seed, **(dict(mu=1.0, tau=2.0, kappa=1.0) if model == "OU" else dict(mu=0.1, sigma=0.8)))
    keep = np.concatenate([np.arange(T) < L for L in DIRECT_LENGTHS])
    ID, obs = ID[keep], obs[keep].copy()
    n = len(ID)
    times = np.cumsum(np.random.default_rng(seed + 1).uniform(0.5, 1.5, size=n))
    for r in (0, 40, 41, 150, 299, 301 + 76):
        obs[r, :] = np.nan
    q = capi.n_sde_par(model, d)
    X_re = [None] * q
    X_re[0] = bspline_basis(_covariate(n), n_cols)
    pb = capi.Problem(model, ID, times, obs, X_re=X_re, S_list=[second_difference_penalty(n_cols)])
    par = np.zeros(pb.n_par_full)
    k_re = 0
    for k, nm in enumerate(pb.par_names()):
        if nm.startswith("log_lambda"):
            par[k] = 0.3
        elif nm.startswith("coeff_re"):
            par[k] = 0.1 * np.cos(k_re)
            k_re += 1
        else:
            j = int(nm[9:nm.index("]")])
            par[k] = (1.0 if model == "OU" else 0.1) if j < d else (0.5 if j == d else -0.2)
    return pb, par
