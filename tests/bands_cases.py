"""Cases of ssde_par_bands shared by the host-twin and the GPU tests -- test infrastructure.

A case: per parameter a fixed-effect block (None = the intercept alone; else a column of ones and uniform(-1, 1) columns), a
random-effect block (None or uniform(0, 1) columns, like a spline basis), a link, and the coefficient table: the point estimate
c_hat with an intercept of size 1 .. 2 and the other entries in (-0.6, 0.6), the draws c_hat + spread * N(0, 1).  With spread = 0.25
the standard error of a linear predictor is about 0.25 sqrt(sum x^2), away from zero on every row, and S_i = max_k sum_c |x c| stays
below 100 at 64 columns (asserted by `row_scale`)."""
import statistics

import numpy as np

U = 2.0 ** -53


def make_case(n, n_post, cols, links, seed, spread=0.25, level=0.95, resp=True, shift=0.0):
    """cols: per parameter (ncol_fe, ncol_re); ncol_fe == 0 stands for the NULL block (the intercept alone).  `shift`: draw 1's
    intercepts are lowered and draw 2's raised by it -- with two draws and a small spread that, not chance, sets every row's se."""
    rng = np.random.default_rng(seed)
    X_fe, X_re, chat = [], [], []
    for kf, kr in cols:
        if kf == 0:
            X_fe.append(None)
            kf = 1
        else:
            X = rng.uniform(-1.0, 1.0, size=(n, kf))
            X[:, 0] = 1.0
            X_fe.append(X)
        X_re.append(rng.uniform(0.0, 1.0, size=(n, kr)) if kr else None)
        c = rng.uniform(-0.6, 0.6, size=kf + kr)
        c[0] = rng.choice([-1.0, 1.0]) * rng.uniform(1.0, 2.0)
        chat.append(c)
    chat = np.concatenate(chat)
    coeff = np.vstack([chat, chat + spread * rng.standard_normal((n_post, len(chat)))])
    icpt = np.cumsum([0] + [max(kf, 1) + kr for kf, kr in cols])[:-1]
    coeff[1, icpt] -= shift
    coeff[2, icpt] += shift
    return dict(X_fe=X_fe, X_re=X_re, link=np.asarray(links, dtype=np.uint8), coeff=coeff, level=level, resp=resp,
                z=statistics.NormalDist().inv_cdf((1.0 + level) / 2.0), n=n, n_post=n_post)


def ref_args(case):
    return (case["X_fe"], case["X_re"], case["link"], case["coeff"], case["level"], case["z"])


def row_scale(case):
    """(S, K): S[i, j] = max_k sum_c |X_j[i, c] coeff[k, off_j + c]|, K[j] the columns of parameter j; asserts S <= 100"""
    n, q = case["n"], len(case["X_fe"])
    S, K, off = np.zeros((n, q)), np.zeros(q, dtype=int), 0
    for j in range(q):
        cols = [np.ones((n, 1)) if case["X_fe"][j] is None else case["X_fe"][j]]
        if case["X_re"][j] is not None:
            cols.append(case["X_re"][j])
        X = np.concatenate(cols, axis=1)
        K[j] = X.shape[1]
        with np.errstate(invalid="ignore"):
            S[:, j] = np.nanmax(np.abs(X) @ np.abs(case["coeff"][:, off:off + K[j]]).T, axis=1)
        off += K[j]
    assert np.nanmax(S) <= 100.0, np.nanmax(S)
    return S, K


def same_nan(got, ref, tag):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{tag}: NaN patterns differ"


def compare(got, ref, ref_ld, case, tag, verbose=True):
    """`got` against the definition.  est, pw_* and se, max_dev: 4 (K + 4) u S_i per row -- relative to the value where the output is on
    the response scale of a log link, absolute on the link scale (max_dev: with the largest S of the parameter).  crit, sim_*: with g
    the largest gap between the float64 and the long double definition over these three, the inputs must give
    g <= 1e-11 (1 + max|ref|) and the limit is max(1e-12, 64 g) (1 + max|ref|).  Returns the largest gap over limit of each group."""
    S, K = row_scale(case)
    q = len(K)
    worst = {}
    for name in ("est", "pw_low", "pw_upp", "se"):
        if name not in got:
            continue
        same_nan(got[name], ref[name], f"{tag} {name}")
        for j in range(q):
            lim = 4.0 * (K[j] + 4) * U * S[:, j]
            if name != "se" and case["resp"] and case["link"][j] == 1:
                lim = lim * np.abs(ref[name][:, j])
            gap = np.abs(got[name][:, j] - ref[name][:, j])
            ok = ~np.isnan(ref[name][:, j])
            if ok.any():
                worst[name] = max(worst.get(name, 0.0), float(np.max(gap[ok] / lim[ok])))
            assert np.all(gap[ok] <= lim[ok]), f"{tag} {name}[:, {j}]: gap {np.max(gap[ok] / lim[ok]):.3g} of the limit"
    if "max_dev" in got:
        for j in range(q):
            lim = 4.0 * (K[j] + 4) * U * np.nanmax(S[:, j])
            gap = np.abs(got["max_dev"][j] - ref["max_dev"][j])
            gap[got["max_dev"][j] == ref["max_dev"][j]] = 0.0                 # inf == inf
            worst["max_dev"] = max(worst.get("max_dev", 0.0), float(np.max(gap) / lim))
            assert np.all(gap <= lim), f"{tag} max_dev[{j}]: gap {np.max(gap) / lim:.3g} of the limit"
    sim = [nm for nm in ("crit", "sim_low", "sim_upp") if nm in got]
    if sim:
        g, big = 0.0, 0.0
        for nm in ("crit", "sim_low", "sim_upp"):
            with np.errstate(invalid="ignore"):
                d = np.abs(ref[nm].astype(np.longdouble) - ref_ld[nm])
            g = max(g, float(np.nanmax(d)))
            big = max(big, float(np.nanmax(np.abs(ref[nm]))))
        assert g <= 1e-11 * (1.0 + big), f"{tag}: the inputs leave crit / sim_* open by {g:.3g}"
        lim = max(1e-12, 64.0 * g) * (1.0 + big)
        for nm in sim:
            if nm != "crit":
                same_nan(got[nm], ref[nm], f"{tag} {nm}")
            gap = float(np.nanmax(np.abs(got[nm] - ref[nm])))
            worst[nm] = max(worst.get(nm, 0.0), gap / lim)
            assert gap <= lim, f"{tag} {nm}: gap {gap:.3g}, limit {lim:.3g}"
        worst["g"] = g
    if verbose:
        print(f"bands {tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return worst


# (n, n_post, cols, links, level, resp): what the host twin and the GPU both run.  Rows around the wave's 64, draws around pass 2's
# blocks of 64, columns at 1 (the NULL block), 2, 9 + 10 and the cap 64, parameters 1, 4 and the cap 16, both links and scales.
CASES = {
    "one_row": (1, 63, [(0, 0)], [1], 0.95, True),
    "n63": (63, 64, [(2, 0), (0, 0), (9, 10), (1, 0)], [0, 1, 1, 0], 0.95, True),
    "n64_link": (64, 65, [(2, 0), (0, 0), (9, 10), (1, 0)], [1, 0, 0, 1], 0.95, False),
    "n65_two_draws": (65, 2, [(9, 10)], [1], 0.95, True),
    "n130_k64": (130, 63, [(32, 32), (64, 0), (1, 63)], [1, 0, 1], 0.95, True),
    "q16": (65, 64, [(0, 0), (2, 0), (1, 3), (3, 0)] * 4, [0, 1] * 8, 0.95, True),
    "level_half": (130, 40, [(2, 0), (9, 10)], [1, 1], 0.5, True),
    "n_post_1000": (65, 1000, [(2, 3), (0, 0)], [1, 0], 0.95, True),
}


def case(name, seed=None):
    n, n_post, cols, links, level, resp = CASES[name]
    two = n_post == 2                      # two draws: the spread comes from the intercepts, 0.5 below and above the estimate
    return make_case(n, n_post, cols, links, seed=sum(map(ord, name)) if seed is None else seed, level=level, resp=resp,
                     spread=0.02 if two else 0.25, shift=0.5 if two else 0.0)
