"""numpy restatements of the leave-one-out residuals and predictive densities (ssde_smooth_loo) for the tests (test
infrastructure).

* loo_ref: the forward loop and the de Jong / Durbin-Koopman backward recursion of tests/smooth_ref.py with the smoothing error
  w_j = F_j^-1 v_j - K_j'r and its precision M_j = F_j^-1 + K_j'N K_j added (r, N the values BEFORE row j is folded in), then the
  outputs of the call: D_j = M_j^-1, delta_j = D_j w_j, the whitened z_j, lpd_j and the per-track statistics.  Vectorised over the
  tracks, a loop over rows.
* loo_joint: the ground truth for one short track -- the dense joint Gaussian of its observations with block j deleted, conditioned
  with numpy.linalg; no recursion at all.
"""
from __future__ import annotations

import math

import numpy as np

from smooth_ref import _forward, _setup, _trans, _whiten

LOG_2PI = math.log(2.0 * math.pi)


def _chol(S):
    """(C, ok): the lower Cholesky factors of S (m x d x d, symmetric) and whether every pivot is > 0 and finite (the rule of
    csrc/ssde_loo.hpp: loo_cholesky); C means nothing where ok is False."""
    m, d, _ = S.shape
    C = np.zeros((m, d, d)); ok = np.ones(m, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(d):
            s = S[:, j, j] - np.einsum("mk,mk->m", C[:, j, :j], C[:, j, :j])
            ok &= (s > 0) & np.isfinite(s)
            C[:, j, j] = np.sqrt(s)
            for i in range(j + 1, d):
                C[:, i, j] = (S[:, i, j] - np.einsum("mk,mk->m", C[:, i, :j], C[:, j, :j])) / C[:, j, j]
    return C, ok


def _stats(n_seg, bounds, q, lpd, white, thresholds, crow=None):
    """The per-track statistics, folded in the walk's order (a track's last row first): the served rows, the sum of lpd, the largest
    q and the caller's row attaining it (the smallest of a tie), the rows with q above each threshold."""
    thr = np.zeros(0) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    st = np.zeros((n_seg, 4 + len(thr)))
    st[:, 2:4] = np.nan
    for k in range(n_seg):
        rows, lsum, qmax, qrow, over = 0, 0.0, 0.0, 0.0, np.zeros(len(thr))
        for i in range(bounds[k + 1] - 1, bounds[k], -1):
            if not white[i] or (crow is not None and crow[i] < 0):
                continue
            lsum += lpd[i]
            if rows == 0 or q[i] >= qmax:
                qmax, qrow = q[i], float(i if crow is None else crow[i])
            rows += 1
            over += q[i] > thr
        st[k, 0], st[k, 1] = rows, lsum
        if rows:
            st[k, 2], st[k, 3] = qmax, qrow
        st[k, 4:] = over
    return st


def loo_ref(pb, par, thresholds=None):
    """{"mean": n x d, "cov": n x d x d, "resid": n x d, "lpd": n, "q": n, "stats": n_seg x (4 + n_thr), "w": n x d, "M": n x d x d,
    "served": n, "white": n}, NaN where the definitions say so (w, M: on rows without a state)."""
    d, sd, n, model = pb.n_dim, pb.sdim, pb.n, pb.model
    pm, dt, Z, H, P0, bounds, a0s, na = _setup(pb, par)
    obs = np.asarray(pb.obs, dtype=np.float64)
    mean = np.full((n, d), np.nan); cov = np.full((n, d, d), np.nan); res = np.full((n, d), np.nan)
    lpd = np.full(n, np.nan); qq = np.full(n, np.nan); wout = np.full((n, d), np.nan); Mout = np.full((n, d, d), np.nan)
    served = np.zeros(n, dtype=bool); white = np.zeros(n, dtype=bool)
    starts = np.array(bounds[:-1]); lens = np.array(bounds[1:]) - starts
    trk = np.nonzero(lens >= 2)[0]

    def result():
        return {"mean": mean, "cov": cov, "resid": res, "lpd": lpd, "q": qq, "w": wout, "M": Mout, "served": served, "white": white,
                "stats": _stats(pb.n_seg, bounds, qq, lpd, white, thresholds)}
    if len(trk) == 0:
        return result()
    ns = lens[trk] - 1
    M_, S = len(trk), int(ns.max())
    a = a0s[trk].copy()
    P = np.repeat(P0[None], M_, 0)
    rec = []                                                           # per step: rows, active, Z a + v, v, Fi, K, T, resid
    for s in range(S):                                                 # (smooth_ref's forward loop)
        act = s < ns
        rows = np.where(act, starts[trk] + 1 + s, 0)
        T, Q, c = _trans(model, d, pm[rows], dt[rows])
        y = obs[rows]
        F = Z @ P @ Z.T + H[rows]
        det = np.linalg.det(F) if d > 2 else (F[:, 0, 0] if d == 1 else F[:, 0, 0] * F[:, 1, 1] - F[:, 1, 0] * F[:, 0, 1])
        if d > 2:
            det = np.abs(det)
        upd = ~na[rows] & ((det > 0) if model == "CTCRW" else (np.abs(det) > 0))
        Fs = np.where(upd[:, None, None], F, np.eye(d)[None])
        Fi = np.where(upd[:, None, None], np.linalg.inv(Fs), 0.0)
        v = np.where(upd[:, None], y - a @ Z.T, 0.0)
        TP = T @ P
        K = TP @ Z.T @ Fi
        Fi = 0.5 * (Fi + Fi.transpose(0, 2, 1))                        # (the record keeps the symmetric part of F^-1, K the product)
        keep_drift = na[rows] | (model != "CTCRW")
        a_new = np.einsum("mij,mj->mi", T, a) + np.einsum("mij,mj->mi", K, v) + np.where((upd | keep_drift)[:, None], c, 0.0)
        P_new = TP @ T.transpose(0, 2, 1) + Q - TP @ Z.T @ K.transpose(0, 2, 1)
        if d > 1:
            P_new = 0.5 * (P_new + P_new.transpose(0, 2, 1))
        with np.errstate(invalid="ignore"):
            e = _whiten(np.where(upd[:, None, None], 0.5 * (Fs + Fs.transpose(0, 2, 1)), np.eye(d)[None]), v)
        e = np.where(upd[:, None], e, np.nan)
        rec.append((rows, act, a @ Z.T + v, v, Fi, K, T, e))
        a = np.where(act[:, None], a_new, a)
        P = np.where(act[:, None, None], P_new, P)
    r = np.zeros((M_, sd)); N = np.zeros((M_, sd, sd))
    for s in range(S - 1, -1, -1):
        rows, act, zav, v, Fi, K, T, e = rec[s]
        tail = (s == ns - 1)[:, None]
        # the deletion quantities from the incoming r, N (a tail row: r = N = 0)
        u = np.einsum("mij,mj->mi", Fi, v)
        w = u - np.where(tail, 0.0, np.einsum("mai,ma->mi", K, r))
        Mj = Fi + np.where(tail[:, :, None], 0.0, K.transpose(0, 2, 1) @ N @ K)
        Mj = 0.5 * (Mj + Mj.transpose(0, 2, 1))
        _, pd = _chol(Mj)
        srv = act & pd & ~np.any(np.isnan(e), axis=1)
        Ms = np.where(srv[:, None, None], Mj, np.eye(d)[None])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            Dj = np.linalg.inv(Ms)
            Dj = 0.5 * (Dj + Dj.transpose(0, 2, 1))
            dl = np.einsum("mij,mj->mi", Dj, w)
            C, okc = _chol(Dj)
            wh = srv & okc
            Cs = np.where(wh[:, None, None], C, np.eye(d)[None])
            z = _forward(Cs, dl)
            q = np.einsum("mi,mi->m", z, z)
            ld = 2.0 * np.sum(np.log(np.einsum("mii->mi", Cs)), axis=1)
        lp = -0.5 * (d * LOG_2PI + ld + q)
        wout[rows[act]] = w[act]; Mout[rows[act]] = Mj[act]
        mean[rows[srv]] = (zav - dl)[srv]; cov[rows[srv]] = Dj[srv]
        res[rows[wh]] = z[wh]; lpd[rows[wh]] = lp[wh]; qq[rows[wh]] = q[wh]
        served[rows[srv]] = True; white[rows[wh]] = True
        # smooth_ref's backward step
        L = T - K @ Z
        r_new = np.einsum("ij,mj->mi", Z.T, u) + np.where(tail, 0.0, np.einsum("mji,mj->mi", L, r))
        N_new = Z.T @ Fi @ Z + np.where(tail[:, :, None], 0.0, L.transpose(0, 2, 1) @ N @ L)
        N_new = 0.5 * (N_new + N_new.transpose(0, 2, 1))
        r = np.where(act[:, None], r_new, r); N = np.where(act[:, None, None], N_new, N)
    return result()


def loo_joint(pb, par, k):
    """Track k's leave-one-out outputs from the dense joint Gaussian of its observations (rows r0+1 .. r1-1) with block j deleted:
    (mean m x d, cov m x d x d, resid m x d, lpd m, w m x d, M m x d x d), NaN on NA rows; w and M are the blocks of
    Sigma_yy^-1 (y - m) and of Sigma_yy^-1."""
    d, sd, model = pb.n_dim, pb.sdim, pb.model
    pm, dt, Z, H, P0, bounds, a0s, na = _setup(pb, par)
    r0, r1 = bounds[k], bounds[k + 1]
    rows = np.arange(r0 + 1, r1)
    m_ = len(rows)
    T, Q, c = _trans(model, d, pm[rows], dt[rows])
    mu = np.zeros((m_, sd))
    Sig = np.zeros((m_ * sd, m_ * sd))
    mu[0] = a0s[k]
    Vm = [P0]
    for j in range(1, m_):
        mu[j] = T[j - 1] @ mu[j - 1] + c[j - 1]
        Vm.append(T[j - 1] @ Vm[j - 1] @ T[j - 1].T + Q[j - 1])
    for t in range(m_):                                               # Cov(s_u, s_t) = Phi(u, t) V_t, u >= t
        Cc = Vm[t]
        for u in range(t, m_):
            Sig[u * sd:(u + 1) * sd, t * sd:(t + 1) * sd] = Cc
            Sig[t * sd:(t + 1) * sd, u * sd:(u + 1) * sd] = Cc.T
            if u + 1 < m_:
                Cc = T[u] @ Cc
    mean = np.full((m_, d), np.nan); cov = np.full((m_, d, d), np.nan); res = np.full((m_, d), np.nan); lpd = np.full(m_, np.nan)
    wj = np.full((m_, d), np.nan); Mj = np.full((m_, d, d), np.nan)
    obs_t = [j for j in range(m_) if not na[rows[j]]]
    if not obs_t:
        return mean, cov, res, lpd, wj, Mj
    nb = len(obs_t)
    G = np.zeros((nb * d, m_ * sd)); Hb = np.zeros((nb * d, nb * d)); y = np.zeros(nb * d)
    for q, j in enumerate(obs_t):
        G[q * d:(q + 1) * d, j * sd:(j + 1) * sd] = Z
        Hb[q * d:(q + 1) * d, q * d:(q + 1) * d] = H[rows[j]]
        y[q * d:(q + 1) * d] = pb.obs[rows[j]]
    Syy = G @ Sig @ G.T + Hb
    Syy = 0.5 * (Syy + Syy.T)
    my = G @ mu.reshape(-1)
    Pi = np.linalg.inv(Syy)
    pw = Pi @ (y - my)
    for q, j in enumerate(obs_t):
        b = np.arange(q * d, (q + 1) * d)
        o = np.setdiff1d(np.arange(nb * d), b)
        if len(o):
            W = np.linalg.solve(Syy[np.ix_(o, o)], np.c_[y[o] - my[o], Syy[np.ix_(o, b)]])
            cm = my[b] + Syy[np.ix_(b, o)] @ W[:, 0]
            cv = Syy[np.ix_(b, b)] - Syy[np.ix_(b, o)] @ W[:, 1:]
        else:
            cm, cv = my[b], Syy[np.ix_(b, b)]
        cv = 0.5 * (cv + cv.T)
        Lc = np.linalg.cholesky(cv)
        z = np.linalg.solve(Lc, y[b] - cm)
        mean[j], cov[j], res[j] = cm, cv, z
        lpd[j] = -0.5 * (d * LOG_2PI + 2.0 * np.sum(np.log(np.diag(Lc))) + z @ z)
        wj[j] = pw[b]; Mj[j] = Pi[np.ix_(b, b)]
    return mean, cov, res, lpd, wj, Mj
