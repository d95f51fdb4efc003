"""numpy restatements of the fixed-interval smoother for the tests (test infrastructure).

* smooth_ref: the reference's forward loop (nllk_ctcrw.hpp:180-247 and its OU / BM twins, with the engine's symmetric covariance
  update) keeping a_j, P_j, v_j, F_j, K_j, then the de Jong / Durbin-Koopman backward recursion.  Vectorised over the
  tracks, a loop over rows.
* joint_track: the ground truth for one short track -- the dense joint Gaussian of (states, observations), conditioned with
  numpy.linalg; no recursion at all.  Whitened innovations from the lower Cholesky factor of the observations' covariance.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from refimpl import _is_na, linear_predictor


def _trans(model, d, pm, dt):
    """T (m x s x s), Q, c (m x s) for rows with linear predictors pm (m x q) and intervals dt (m)."""
    m = pm.shape[0]
    if model == "CTCRW":
        sd = 2 * d
        tau, nu = np.exp(pm[:, d]), np.exp(pm[:, d + 1])
        beta = 1 / tau
        sig = 2 * nu / np.sqrt(math.pi * tau)
        e = np.exp(-beta * dt)
        e2 = np.exp(-2 * beta * dt)
        t12 = (1 - e) / beta
        q11 = (sig / beta) ** 2 * (dt - 2 / beta * (1 - e) + 1 / (2 * beta) * (1 - e2))
        q12 = sig ** 2 / (2 * beta ** 2) * (1 - 2 * e + e2)
        q22 = sig ** 2 / (2 * beta) * (1 - e2)
        T = np.zeros((m, sd, sd)); Q = np.zeros((m, sd, sd)); c = np.zeros((m, sd))
        for a in range(d):
            p, v = 2 * a, 2 * a + 1
            T[:, p, p] = 1; T[:, p, v] = t12; T[:, v, v] = e
            Q[:, p, p] = q11; Q[:, p, v] = q12; Q[:, v, p] = q12; Q[:, v, v] = q22
            c[:, p] = (dt - t12) * pm[:, a]; c[:, v] = (1 - e) * pm[:, a]
        return T, Q, c
    eye = np.eye(d)[None]
    if model == "OU_SSM":
        tau, kappa = np.exp(pm[:, d]), np.exp(pm[:, d + 1])
        e = np.exp(-dt / tau)
        return e[:, None, None] * eye, (kappa * (1 - np.exp(-2 * dt / tau)))[:, None, None] * eye, (1 - e)[:, None] * pm[:, :d]
    sig = np.exp(pm[:, d])
    return np.repeat(eye, m, 0), (sig ** 2 * dt)[:, None, None] * eye, pm[:, :d] * dt[:, None]


def _setup(pb, par):
    d, sd, n = pb.n_dim, pb.sdim, pb.n
    pm = linear_predictor(pb, torch.as_tensor(np.asarray(par, dtype=np.float64))).detach().numpy()
    t = np.asarray(pb.times, dtype=np.float64)
    dt = np.r_[t[1:] - t[:-1], 1.0]                                   # dtimes(n-1) = 1
    Z = np.zeros((d, sd))
    for a in range(d):
        Z[a, 2 * a if pb.model == "CTCRW" else a] = 1.0
    if pb.H is not None:
        H = np.moveaxis(np.asarray(pb.H, dtype=np.float64), 2, 0)       # n x d x d
    else:
        H = np.repeat((math.exp(par[0]) ** 2 * np.eye(d))[None], n, 0)
    if pb.P0 is not None:
        P0 = np.asarray(pb.P0, dtype=np.float64)
    elif pb.model == "CTCRW":
        P0 = np.diag([1.0, 10.0] * d)
    else:
        P0 = 10.0 * np.eye(d)
    bounds = list(pb.seg_start) + [n]
    a0 = []
    for k in range(pb.n_seg):
        if pb.a0 is not None:
            a0.append(np.asarray(pb.a0[k], dtype=np.float64))
        else:
            m = np.zeros(sd)
            for a in range(d):
                m[2 * a if pb.model == "CTCRW" else a] = pb.obs[bounds[k], a]
            a0.append(m)
    na = np.array([_is_na(pb.obs[i, 0], pb.na_mode) for i in range(n)])
    return pm, dt, Z, H, P0, bounds, np.array(a0), na


def _forward(C, v):
    """C^-1 v by forward substitution (m x d x d lower triangular, m x d): component i reads v[: i + 1] only, as the kernel's does."""
    e = np.zeros(v.shape)
    for i in range(v.shape[1]):
        e[:, i] = (v[:, i] - np.einsum("mk,mk->m", C[:, i, :i], e[:, :i])) / C[:, i, i]
    return e


def _whiten(F, v):
    """C^-1 v per row, C the lower Cholesky factor of F (m x d x d); NaN on a row whose F has none (OU_SSM / BM_SSM update
    whenever |det F| > 0, so a negative F reaches here: the kernel's sqrt gives NaN there)."""
    try:
        return _forward(np.linalg.cholesky(F), v)
    except np.linalg.LinAlgError:
        e = np.full(v.shape, np.nan)
        for k in range(F.shape[0]):
            try:
                e[k] = _forward(np.linalg.cholesky(F[k:k + 1]), v[k:k + 1])[0]
            except np.linalg.LinAlgError:
                pass
        return e


def smooth_ref(pb, par):
    """{"mean": n x sdim, "cov": n x sdim x sdim, "resid": n x d, "pred_cov": the filter's P_j}, NaN where the definitions say so."""
    d, sd, n, model = pb.n_dim, pb.sdim, pb.n, pb.model
    pm, dt, Z, H, P0, bounds, a0s, na = _setup(pb, par)
    obs = np.asarray(pb.obs, dtype=np.float64)
    mean = np.full((n, sd), np.nan); cov = np.full((n, sd, sd), np.nan); res = np.full((n, d), np.nan)
    pred = np.full((n, sd, sd), np.nan)
    starts = np.array(bounds[:-1]); lens = np.array(bounds[1:]) - starts
    trk = np.nonzero(lens >= 2)[0]
    if len(trk) == 0:
        return {"mean": mean, "cov": cov, "resid": res, "pred_cov": pred}
    ns = lens[trk] - 1
    M, S = len(trk), int(ns.max())
    a = a0s[trk].copy()
    P = np.repeat(P0[None], M, 0)
    rec = []                                                           # per step: rows, active, a, P, v, Fi, K, T
    for s in range(S):
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
        keep_drift = na[rows] | (model != "CTCRW")
        a_new = np.einsum("mij,mj->mi", T, a) + np.einsum("mij,mj->mi", K, v) + np.where((upd | keep_drift)[:, None], c, 0.0)
        P_new = TP @ T.transpose(0, 2, 1) + Q - TP @ Z.T @ K.transpose(0, 2, 1)
        if d > 1:
            P_new = 0.5 * (P_new + P_new.transpose(0, 2, 1))
        e = _whiten(np.where(upd[:, None, None], 0.5 * (Fs + Fs.transpose(0, 2, 1)), np.eye(d)[None]), v)
        rec.append((rows, act, a.copy(), P.copy(), v, Fi, K, T))
        res[rows[act & upd]] = e[act & upd]
        pred[rows[act]] = P[act]
        a = np.where(act[:, None], a_new, a)
        P = np.where(act[:, None, None], P_new, P)
    r = np.zeros((M, sd)); N = np.zeros((M, sd, sd))
    for s in range(S - 1, -1, -1):
        rows, act, a_s, P_s, v, Fi, K, T = rec[s]
        tail = (s == ns - 1)[:, None]
        L = T - K @ Z
        r_new = np.einsum("ij,mjk,mk->mi", Z.T, Fi, v) + np.where(tail, 0.0, np.einsum("mji,mj->mi", L, r))
        N_new = Z.T @ Fi @ Z + np.where(tail[:, :, None], 0.0, L.transpose(0, 2, 1) @ N @ L)
        N_new = 0.5 * (N_new + N_new.transpose(0, 2, 1))
        r = np.where(act[:, None], r_new, r); N = np.where(act[:, None, None], N_new, N)
        am = a_s + np.einsum("mij,mj->mi", P_s, r)
        V = P_s - P_s @ N @ P_s
        V = 0.5 * (V + V.transpose(0, 2, 1))
        mean[rows[act]] = am[act]; cov[rows[act]] = V[act]
    return {"mean": mean, "cov": cov, "resid": res, "pred_cov": pred}


def joint_track(pb, par, k):
    """E[states | y], Cov[states | y] and the whitened innovations of track k from the dense joint Gaussian (rows r0+1 .. r1-1)."""
    d, sd, model = pb.n_dim, pb.sdim, pb.model
    pm, dt, Z, H, P0, bounds, a0s, na = _setup(pb, par)
    r0, r1 = bounds[k], bounds[k + 1]
    rows = np.arange(r0 + 1, r1)
    m_ = len(rows)
    T, Q, c = _trans(model, d, pm[rows], dt[rows])
    mu = np.zeros((m_, sd)); Phi = [None] * m_
    Sig = np.zeros((m_ * sd, m_ * sd))
    mu[0] = a0s[k]
    Vm = [P0]
    for j in range(1, m_):
        mu[j] = T[j - 1] @ mu[j - 1] + c[j - 1]
        Vm.append(T[j - 1] @ Vm[j - 1] @ T[j - 1].T + Q[j - 1])
    for t in range(m_):                                               # Cov(s_u, s_t) = Phi(u, t) V_t, u >= t
        C = Vm[t]
        for u in range(t, m_):
            Sig[u * sd:(u + 1) * sd, t * sd:(t + 1) * sd] = C
            Sig[t * sd:(t + 1) * sd, u * sd:(u + 1) * sd] = C.T
            if u + 1 < m_:
                C = T[u] @ C
    obs_t = [j for j in range(m_) if not na[rows[j]]]
    if not obs_t:
        return mu, Sig.reshape(m_, sd, m_, sd)[np.arange(m_), :, np.arange(m_), :], np.full((m_, d), np.nan)
    G = np.zeros((len(obs_t) * d, m_ * sd))
    Hb = np.zeros((len(obs_t) * d, len(obs_t) * d))
    y = np.zeros(len(obs_t) * d)
    for q, j in enumerate(obs_t):
        G[q * d:(q + 1) * d, j * sd:(j + 1) * sd] = Z
        Hb[q * d:(q + 1) * d, q * d:(q + 1) * d] = H[rows[j]]
        y[q * d:(q + 1) * d] = pb.obs[rows[j]]
    Syy = G @ Sig @ G.T + Hb
    Say = Sig @ G.T
    resid_y = y - G @ mu.reshape(-1)
    W = np.linalg.solve(Syy, np.c_[resid_y, Say.T])
    mean = mu.reshape(-1) + Say @ W[:, 0]
    covf = Sig - Say @ W[:, 1:]
    covf = 0.5 * (covf + covf.T)
    Lc = np.linalg.cholesky(0.5 * (Syy + Syy.T))
    e = np.linalg.solve(Lc, resid_y)
    res = np.full((m_, d), np.nan)
    for q, j in enumerate(obs_t):
        res[j] = e[q * d:(q + 1) * d]
    cov = np.stack([covf[j * sd:(j + 1) * sd, j * sd:(j + 1) * sd] for j in range(m_)])
    return mean.reshape(m_, sd), cov, res
