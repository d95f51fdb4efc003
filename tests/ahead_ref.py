"""The definition of ssde_forecast_scores in plain numpy (test infrastructure): a Kalman filter written from the
model definitions with dense T, Q, Z, H per family (the transition and noise formulas are tests/refimpl.py's: _ctcrw_blocks,
_step_matrices), which forecasts row t from the data through row t - k by LITERALLY setting rows t - k + 1 .. t - 1 to missing and
filtering the track again from its first row, once per target and horizon.  Nothing here is shared with the twin or the kernels.

The filter is the reference's (nllk_ctcrw.hpp:195-247 and its OU_SSM / BM_SSM twins): the state enters a track's second row as
a0, P0; a row is stepped through by a <- T a + c, P <- T P T' + Q when it is missing, with the Kalman update in front when it is
not and det F passes the family's test (CTCRW drops the drift c where it fails)."""
import math

import numpy as np
import torch

from refimpl import _is_na, linear_predictor


def _matrices(model, d, pm, dt):
    """T, Q, c of one row with linear predictors pm over the interval dt"""
    if model == "CTCRW":
        sd = 2 * d
        tau, nu = math.exp(pm[d]), math.exp(pm[d + 1])
        beta = 1.0 / tau
        sigma = 2.0 * nu / math.sqrt(math.pi * tau)
        e, e2 = math.exp(-beta * dt), math.exp(-2.0 * beta * dt)
        qvv = sigma ** 2 / (2 * beta) * (1 - e2)
        qzz = (sigma / beta) ** 2 * (dt + (1 - e2) / (2 * beta) - 2 * (1 - e) / beta)
        qvz = sigma ** 2 / (2 * beta ** 2) * (1 - 2 * e + e2)
        T, Q, c = np.zeros((sd, sd)), np.zeros((sd, sd)), np.zeros(sd)
        for a in range(d):
            p, v = 2 * a, 2 * a + 1
            T[p, p], T[p, v], T[v, v] = 1.0, (1 - e) / beta, e
            Q[p, p], Q[p, v], Q[v, p], Q[v, v] = qzz, qvz, qvz, qvv
            c[p], c[v] = (dt - (1 - e) / beta) * pm[a], (1 - e) * pm[a]
        return T, Q, c
    if model == "OU_SSM":
        tau, kappa = math.exp(pm[d]), math.exp(pm[d + 1])
        e = math.exp(-dt / tau)
        return e * np.eye(d), kappa * (1 - math.exp(-2 * dt / tau)) * np.eye(d), (1 - e) * pm[:d]
    sigma = math.exp(pm[d])
    return np.eye(d), sigma ** 2 * dt * np.eye(d), pm[:d] * dt


def _predict_row(pb, pm, dt, Z, H, a0, P0, na, r0, t, blank_from):
    """(a_t, P_t): the filter of the track starting at row r0 run up to row t with rows blank_from .. t - 1 set to missing"""
    d, model = pb.n_dim, pb.model
    obs = np.asarray(pb.obs, dtype=np.float64)
    a, P = a0.copy(), P0.copy()
    for i in range(r0 + 1, t):
        T, Q, c = _matrices(model, d, pm[i], dt[i])
        upd = not (na[i] or i >= blank_from)
        if upd:
            F = Z @ P @ Z.T + H[i]
            det = np.linalg.det(F)
            upd = det > 0 if model == "CTCRW" else abs(det) > 0
            if not upd and model == "CTCRW":
                c = np.zeros_like(c)                                     # (Q3: the drift is dropped where det F <= 0)
        if upd:
            K = T @ P @ Z.T @ np.linalg.inv(F)
            a_new = T @ a + K @ (obs[i, :d] - Z @ a) + c
            P = T @ P @ (T - K @ Z).T + Q
            P = 0.5 * (P + P.T)
            a = a_new
        else:
            a = T @ a + c
            P = T @ P @ T.T + Q
    return a, P


def ahead_ref(pb, par, horizons, thresholds=None):
    """{"z": n x n_h x d, "lpd": n x n_h, "q": n x n_h, "lead": n x n_h, "stats": n_seg x n_h x (5 + n_thr)}; NaN where a target
    is not scored, zero statistics for a track without a scored target"""
    d, sd, n, model = pb.n_dim, pb.sdim, pb.n, pb.model
    par = np.asarray(par, dtype=np.float64)
    hz = [int(k) for k in horizons]
    thr = np.zeros(0) if thresholds is None else np.asarray(thresholds, dtype=np.float64).ravel()
    pm = linear_predictor(pb, torch.as_tensor(par)).detach().numpy()
    tm = np.asarray(pb.times, dtype=np.float64)
    dt = np.r_[tm[1:] - tm[:-1], 1.0]
    obs = np.asarray(pb.obs, dtype=np.float64)
    Z = np.zeros((d, sd))
    for a in range(d):
        Z[a, 2 * a if model == "CTCRW" else a] = 1.0
    H = np.moveaxis(np.asarray(pb.H, dtype=np.float64), 2, 0) if pb.H is not None else np.repeat((math.exp(par[0]) ** 2 * np.eye(d))[None], n, 0)
    P0 = np.asarray(pb.P0, dtype=np.float64) if pb.P0 is not None else (np.diag([1.0, 10.0] * d) if model == "CTCRW" else 10.0 * np.eye(d))
    na = np.array([_is_na(pb.obs[i, 0], pb.na_mode) for i in range(n)])
    bounds = list(pb.seg_start) + [n]
    nh = len(hz)
    z, lpd, q, lead = np.full((n, nh, d), np.nan), np.full((n, nh), np.nan), np.full((n, nh), np.nan), np.full((n, nh), np.nan)
    stats = np.zeros((pb.n_seg, nh, 5 + len(thr)))
    for k in range(pb.n_seg):
        r0, r1 = bounds[k], bounds[k + 1]
        if pb.a0 is not None:
            a0 = np.asarray(pb.a0[k], dtype=np.float64)
        else:
            a0 = np.zeros(sd)
            for a in range(d):
                a0[2 * a if model == "CTCRW" else a] = obs[r0, a]
        for j, kk in enumerate(hz):
            for t in range(r0 + kk, r1):
                if na[t]:
                    continue
                a, P = _predict_row(pb, pm, dt, Z, H, a0, P0, na, r0, t, t - kk + 1)
                m = Z @ a
                S = Z @ P @ Z.T + H[t]
                S = 0.5 * (S + S.T)
                if not (np.all(np.isfinite(m)) and np.all(np.isfinite(S))):
                    continue
                try:
                    C = np.linalg.cholesky(S)
                except np.linalg.LinAlgError:
                    continue
                if not np.all(np.isfinite(C)) or np.any(np.diag(C) <= 0):
                    continue
                e = obs[t, :d] - m
                zt = np.linalg.solve(C, e)
                qt = float(zt @ zt)
                lt = -0.5 * (d * math.log(2 * math.pi) + 2 * np.sum(np.log(np.diag(C))) + qt)
                z[t, j], q[t, j], lpd[t, j], lead[t, j] = zt, qt, lt, np.sum(dt[t - kk:t])
                stats[k, j, :5] += [1.0, lt, qt, float(e @ e), lead[t, j]]
                stats[k, j, 5:] += qt > thr
    return {"z": z, "lpd": lpd, "q": q, "lead": lead, "stats": stats}
