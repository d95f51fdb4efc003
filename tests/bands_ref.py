"""numpy definition of ssde_par_bands (include/ssde.h) -- test infrastructure.

It builds what the device never does: per parameter the n x (1 + n_post) matrix of linear predictors, sorted along the draws.  Any
float dtype (np.float64, np.longdouble): the GPU tests take the gap between the two as the measure of how well `crit` and the
simultaneous bands are determined by their inputs."""
import numpy as np


def quantile7(x_sorted, p):
    """R's type-7 quantile (the default of quantile()) along the last axis of sorted values: h = (m - 1) p, lo = floor(h),
    hi = min(lo + 1, m - 1), Q = x[lo] + (h - lo)(x[hi] - x[lo]); x[lo] as it is where x[hi] == x[lo] (as R does: no inf - inf)."""
    m = x_sorted.shape[-1]
    h = (m - 1) * p                                   # float64, as the C side forms it
    lo = min(max(int(np.floor(h)), 0), m - 1)
    hi = min(lo + 1, m - 1)
    frac = x_sorted.dtype.type(h - lo)
    a, b = x_sorted[..., lo], x_sorted[..., hi]
    with np.errstate(invalid="ignore"):
        return np.where((a == b) | (frac == 0), a, a + frac * (b - a))


def tail_sizes(n_post, level):
    """the order statistics the lower and the upper tail need: floor((n_post - 1) alpha) + 2 and its mirror"""
    alpha = (1.0 - level) / 2.0
    m_lo = int(np.floor((n_post - 1) * alpha)) + 2
    m_up = n_post - int(np.floor((n_post - 1) * (1.0 - alpha)))
    return m_lo, m_up


def bands_ref(X_fe, X_re, link, coeff, level, z, resp=True, dtype=np.float64):
    """X_fe[j]: (n, k) or None (a column of ones), X_re[j]: (n, k) or None; coeff (1 + n_post, n_coef).  Returns a dict of est,
    pw_low, pw_upp, se, sim_low, sim_upp (n, q), crit (q,), max_dev (q, n_post)."""
    q = len(X_fe)
    n = max([b.shape[0] for b in list(X_fe) + list(X_re) if b is not None], default=1)
    coeff = np.asarray(coeff, dtype=np.float64)
    n_post = coeff.shape[0] - 1
    alpha = (1.0 - level) / 2.0
    out = {k: np.full((n, q), np.nan, dtype=dtype) for k in ("est", "pw_low", "pw_upp", "se", "sim_low", "sim_upp")}
    out["crit"] = np.zeros(q, dtype=dtype)
    out["max_dev"] = np.zeros((q, n_post), dtype=dtype)
    off = 0
    for j in range(q):
        cols = [np.ones((n, 1)) if X_fe[j] is None else np.asarray(X_fe[j], dtype=np.float64)]
        if X_re[j] is not None:
            cols.append(np.asarray(X_re[j], dtype=np.float64))
        X = np.concatenate(cols, axis=1).astype(dtype)
        K = X.shape[1]
        cf = coeff[:, off:off + K].astype(dtype)
        off += K
        g = (lambda v: np.exp(v)) if (resp and link[j] == 1) else (lambda v: v)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            lp = X @ cf.T                                             # n x (1 + n_post)
            ok = np.isfinite(lp).all(axis=1)
            lp0 = lp[:, 0]
            srt = np.sort(lp[:, 1:], axis=1)
            q_lo = quantile7(srt, alpha)
            se = (lp0 - q_lo) / dtype(z)
            dev = X @ (cf[1:] - cf[0]).T                              # n x n_post
            a = np.abs(dev / se[:, None])
            a[np.isnan(a)] = 0.0
            a[~ok] = 0.0
            md = a.max(axis=0) if n else np.zeros(n_post, dtype=dtype)
            crit = quantile7(np.sort(md), level)
            crit = dtype(0.0) if np.isnan(crit) else crit
            res = dict(est=g(lp0), pw_low=quantile7(g(srt), alpha), pw_upp=quantile7(g(srt), 1.0 - alpha), se=se,
                       sim_low=g(lp0 - crit * se), sim_upp=g(lp0 + crit * se))
        for k, v in res.items():
            out[k][ok, j] = v[ok]
        out["crit"][j] = crit
        out["max_dev"][j] = md
    return out
