"""Cases of ssde_simulate_rows shared by the host-twin and the GPU tests -- test infrastructure.

A case names a model, the columns, the track lengths, the replicates, the coefficient rows (1, or one per replicate: the first row
plus 0.1 N(0, 1)), the design blocks (None = constant, "lin" = an intercept and a covariate in (-1, 1), "smooth" = an intercept
and a 9-column B-spline basis as random effects), sigma_obs (None, 0 or positive), the time grid and the thresholds.  The parameters
stay O(1) (log-link linear predictors within about +-1.5), so that |y| <= 1e3 on every case (asserted).  `reference(name)` computes
the numpy definition once per process and asserts that no reference step length lies within 1e-6 (1 + thr) of a threshold: the
counts can then be compared exactly and nothing is left out."""
import functools

import numpy as np

from simrows_ref import n_par, simrows_ref
from smoothsde_amd.synth import bspline_basis

EDGES = [0, 1, 2, 3, 31, 32, 33, 64, 65]     # the 32-row tile's edges

# name: (model, d, lengths, n_rep, rows_per_rep, blocks {parameter index: kind}, sigma_obs, grid, thresholds)
# parameter indices: 0 .. d - 1 the mu, d the first scale parameter (tau / sigma), d + 1 the second (nu / kappa)
CASES = {
    "ctcrw_smooth_d2": ("CTCRW", 2, [65, 0, 33], 65, True, {2: "smooth", 3: "lin"}, 0.05, "irregular", (0.4, 2.0, np.inf)),
    "ctcrw_wide_dt": ("CTCRW", 1, [65], 64, False, {}, None, "wide", (0.05, 1.0, 30.0)),
    "ctcrw_mu_smooth": ("CTCRW", 1, [32, 64, 1], 1, False, {0: "smooth", 2: "lin", 3: "smooth"}, None, "irregular", (0.6,)),
    "ou_const_d1": ("OU", 1, [64], 130, False, {}, None, "irregular", (0.3, 1.5)),
    "ou_ssm_smooth": ("OU_SSM", 2, [31, 32, 64], 63, True, {0: "smooth", 2: "lin", 3: "lin"}, 0.0, "irregular", (0.5, 2.5, np.inf)),
    "bm_d3": ("BM", 3, [3, 33, 2], 130, True, {1: "lin", 3: "smooth"}, None, "irregular", (0.7, 3.0)),
    "bm_ssm_70": ("BM_SSM", 2, [EDGES[k % 9] for k in range(70)], 1, False, {0: "lin"}, 0.1, "irregular", (0.5, 2.0, 0.0)),
    "ou_70_reps": ("OU", 1, [EDGES[(k + 4) % 9] for k in range(70)], 3, True, {1: "smooth"}, 0.2, "irregular", ()),
}


def make_case(model, d, lengths, n_rep, rows_per_rep, blocks, sigma_obs, grid, thr, seed):
    rng = np.random.default_rng(seed)
    row0 = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n, q = int(row0[-1]), n_par(model, d)
    if grid == "wide":                       # dt from 1e-6 tau to 1e3 tau (tau = 1), both ends present
        dt = 10.0 ** rng.uniform(-6.0, 3.0, size=n)
        dt[1], dt[2] = 1e-6, 1e3
    else:
        dt = rng.uniform(0.2, 1.8, size=n) * rng.choice([0.25, 1.0, 3.0], size=n)
    times = np.cumsum(dt)
    cov = np.sin(0.37 * np.arange(n) + rng.uniform(0, 6))
    X_fe, X_re, link, chat = [], [], [], []
    for j in range(q):
        kind = blocks.get(j)
        is_mu = j < d
        link.append(0 if is_mu else 1)
        icpt = rng.uniform(-1.0, 1.0) if is_mu else rng.uniform(-0.4, 0.4)
        if grid == "wide":                                  # tau = 1, nu = 1 / 2, a drift small enough for |y| <= 1e3 over 1e4 time units
            icpt = 0.02 * icpt if is_mu else (0.0 if j == d else np.log(0.5))
        if kind == "lin":
            X_fe.append(np.column_stack([np.ones(n), cov])); X_re.append(None)
            chat.append([icpt, rng.uniform(-0.5, 0.5)])
        elif kind == "smooth":
            X_fe.append(None); X_re.append(bspline_basis((np.sin(0.11 * np.arange(n) + 1.0) + 1.0) / 2.0, 9))
            chat.append(np.concatenate([[icpt], rng.uniform(-0.6, 0.6, size=9)]))
        else:
            X_fe.append(None); X_re.append(None)
            chat.append([icpt])
    chat = np.concatenate(chat)
    coeff = chat[None, :] + (np.r_[np.zeros((1, len(chat))), 0.1 * rng.standard_normal((n_rep - 1, len(chat)))] if rows_per_rep else 0.0)
    so = None if sigma_obs is None else np.full(coeff.shape[0], float(sigma_obs)) * (1.0 + 0.1 * np.arange(coeff.shape[0]) / max(coeff.shape[0], 1))
    return dict(model=model, n_dim=d, row0=row0, times=times, X_fe=X_fe, X_re=X_re, link=np.asarray(link, dtype=np.uint8), coeff=coeff,
                sigma_obs=so, z0=rng.uniform(-1.0, 1.0, size=d), seed=int(seed) * 7919 + 11, rep0=int(seed) % 5, n_rep=n_rep,
                thr=np.asarray(thr, dtype=np.float64), lengths=np.asarray(lengths))


@functools.lru_cache(maxsize=None)
def case(name):
    return make_case(*CASES[name], seed=sum(map(ord, name)))


def ref_kwargs(c, **over):
    kw = dict(sigma_obs=c["sigma_obs"], z0=c["z0"], seed=c["seed"], rep0=c["rep0"], n_rep=c["n_rep"])
    kw.update(over)
    return kw


def ref_args(c):
    return (c["model"], c["n_dim"], c["row0"], c["times"], c["X_fe"], c["X_re"], c["link"], c["coeff"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 definition of the case (computed once, shared, never written to): obs, stats, L"""
    c = case(name)
    ref = simrows_ref(*ref_args(c), thr=c["thr"], steps=True, **ref_kwargs(c))
    assert np.nanmax(np.abs(ref["obs"]), initial=0.0) <= 1e3, name
    L = ref["L"][np.isfinite(ref["L"])]
    for th in c["thr"]:
        if np.isfinite(th) and L.size:
            assert np.min(np.abs(L - th)) > 1e-6 * (1.0 + th), f"{name}: a step length within 1e-6 (1 + thr) of the threshold {th}"
    for v in ref.values():
        v.setflags(write=False)
    return ref


def limits(c, ref):
    """(obs limit, per-track limit of the sums): 1e-9 (1 + max|ref|), and that times the track's length"""
    big = float(np.nanmax(np.abs(ref["obs"]), initial=0.0))
    lim = 1e-9 * (1.0 + big)
    return lim, lim * np.maximum(c["lengths"], 1).astype(np.float64)


def compare(got, ref, c, tag, verbose=True):
    """`got` ({"obs", "stats"}, either may be missing) against the definition: obs within 1e-9 (1 + max|ref|) -- the bound
    tests/sim_ref.py records for device against numpy log / sincos on tracks of this length --, the sums of stats within that bound
    times the track length, max L within the obs bound, counts exact, NaN patterns identical.  Returns the largest gap over its
    limit of each group."""
    d, n_thr = c["n_dim"], len(c["thr"])
    lim, lim_t = limits(c, ref)
    worst = {}
    if "obs" in got:
        assert got["obs"].shape == ref["obs"].shape, (tag, got["obs"].shape, ref["obs"].shape)
        assert np.array_equal(np.isnan(got["obs"]), np.isnan(ref["obs"])), f"{tag}: NaN patterns of obs differ"
        gap = float(np.nanmax(np.abs(got["obs"] - ref["obs"]), initial=0.0))
        worst["obs"] = gap / lim
    if "stats" in got:
        gs, rs = got["stats"], ref["stats"]
        assert gs.shape == rs.shape, (tag, gs.shape, rs.shape)
        assert np.array_equal(np.isnan(gs), np.isnan(rs)), f"{tag}: NaN patterns of stats differ"
        with np.errstate(invalid="ignore"):
            gap = np.abs(gs - rs)
        sums = [3 * cc + k for cc in range(d) for k in range(3)] + [3 * d]
        worst["sums"] = float(np.nanmax(gap[:, :, sums] / lim_t[None, :, None], initial=0.0))
        worst["max"] = float(np.nanmax(gap[:, :, 3 * d + 1], initial=0.0)) / lim
        worst["counts"] = float(np.nanmax(gap[:, :, 3 * d + 2:], initial=0.0)) if n_thr else 0.0
    if verbose:
        print(f"simrows {tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + " (of the limit; counts: absolute)")
    for k, v in worst.items():
        assert v <= (0.0 if k == "counts" else 1.0), f"{tag} {k}: gap {v:.3g} of the limit"
    return worst
