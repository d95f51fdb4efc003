"""numpy restatement of ssde_predict for the tests (test infrastructure).

* predict_ref: written from the definitions -- a forward loop of its own keeping a_j, P_j, v_j, F_j^-1, K_j, T_j and the filtered
  moments per row, a backward loop keeping the r and N the recursion holds BEFORE each row is processed (r+, N+ of the interval the
  row starts), then one prediction step over the offset with row j's parameters and the correction by T2 = T(Delta_j - delta).
  One track after the other, one row after the other: nothing here is shared with smooth_ref but the transition formulas.
* augment: the problem with NA rows inserted at the query times (covariate rows and H copied from row j, forecast rows appended
  to their track).  smooth_ref and joint_track run on it unchanged: a query IS the smoothed state of such a row.
"""
from __future__ import annotations

import numpy as np

from smooth_ref import _setup, _trans
from smoothsde_amd import capi

DT_RTOL = 1e-9            # "delta > Delta_j by more than rounding" (csrc/ssde_predict.hpp: PREDICT_DT_RTOL)


def _sym(A):
    return 0.5 * (A + A.T)


def predict_ref(pb, par, rows, offs):
    """{"mean": m x sdim, "cov": m x sdim x sdim} of the queries (rows[k], offs[k]); NaN where the definitions say so."""
    d, sd, n, model = pb.n_dim, pb.sdim, pb.n, pb.model
    pm, dt, Z, H, P0, bounds, a0s, na = _setup(pb, par)
    obs = np.asarray(pb.obs, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int64).ravel()
    offs = np.asarray(offs, dtype=np.float64).ravel()
    T, Q, c = _trans(model, d, pm, dt)
    af = np.full((n, sd), np.nan); Pf = np.full((n, sd, sd), np.nan)
    rp = np.zeros((n, sd)); Np = np.zeros((n, sd, sd))
    state = np.zeros(n, dtype=bool); rejected = np.zeros(n, dtype=bool); tail = np.zeros(n, dtype=bool)
    for k in range(pb.n_seg):
        r0, r1 = bounds[k], bounds[k + 1]
        if r1 - r0 < 2:
            continue
        a, P = a0s[k].copy(), P0.copy()
        fw = {}
        for i in range(r0 + 1, r1):
            F = Z @ P @ Z.T + H[i]
            det = abs(np.linalg.det(F)) if d > 2 else (F[0, 0] if d == 1 else F[0, 0] * F[1, 1] - F[1, 0] * F[0, 1])
            upd = (not na[i]) and ((det > 0) if model == "CTCRW" else (abs(det) > 0))
            rejected[i] = (not na[i]) and not upd
            Fi = np.linalg.inv(F) if upd else np.zeros((d, d))
            v = (obs[i] - Z @ a) if upd else np.zeros(d)
            K = T[i] @ P @ Z.T @ Fi
            fw[i] = (v, Fi, K)
            state[i] = True
            af[i] = a + P @ Z.T @ Fi @ v
            Pf[i] = _sym(P - P @ Z.T @ Fi @ Z @ P)
            keep_drift = na[i] or model != "CTCRW"
            a = T[i] @ a + K @ v + (c[i] if (upd or keep_drift) else 0.0)
            P = T[i] @ P @ T[i].T + Q[i] - T[i] @ P @ Z.T @ K.T
            if d > 1:
                P = _sym(P)
        tail[r1 - 1] = True
        r, N = np.zeros(sd), np.zeros((sd, sd))
        for i in range(r1 - 1, r0, -1):
            rp[i], Np[i] = r, N                                       # what the recursion holds before row i: r+, N+ of (t_i, t_{i+1}]
            v, Fi, K = fw[i]
            if tail[i]:
                r, N = Z.T @ Fi @ v, Z.T @ Fi @ Z
            else:
                L = T[i] - K @ Z
                r, N = Z.T @ Fi @ v + L.T @ r, _sym(Z.T @ Fi @ Z + L.T @ N @ L)
    m = len(rows)
    mean = np.full((m, sd), np.nan); cov = np.full((m, sd, sd), np.nan)
    for k in range(m):
        j, delta = int(rows[k]), float(offs[k])
        if not state[j] or rejected[j]:
            continue
        if not tail[j] and delta > dt[j] * (1.0 + DT_RTOL):
            continue
        T1, Q1, c1 = _trans(model, d, pm[j:j + 1], np.array([delta]))
        a_t = T1[0] @ af[j] + c1[0]
        P_t = T1[0] @ Pf[j] @ T1[0].T + Q1[0]
        if tail[j]:
            mean[k], cov[k] = a_t, _sym(P_t)
            continue
        T2 = _trans(model, d, pm[j:j + 1], np.array([max(dt[j] - delta, 0.0)]))[0][0]
        mean[k] = a_t + P_t @ T2.T @ rp[j]
        cov[k] = _sym(P_t - P_t @ T2.T @ Np[j] @ T2 @ P_t)
    return {"mean": mean, "cov": cov}


def augment(pb, rows, offs):
    """(problem, index): `pb` with one NA row per query inserted at time[row] + off, carrying row `row`'s covariate rows and H; a
    query on a track's last row is appended to the track.  index[k] is query k's row in the new problem.  Queries of one interval
    go in by offset (ties in the order given); the caller's rows keep their order.  A query the definitions answer with NaN
    whatever the data (on a track's first row -- a row inserted there would move the prior --, or past the next fix) inserts nothing:
    index[k] = -1."""
    rows = np.asarray(rows, dtype=np.int64).ravel()
    offs = np.asarray(offs, dtype=np.float64).ravel()
    n, m = pb.n, len(rows)
    t_ = np.asarray(pb.times, dtype=np.float64)
    first = np.zeros(n, dtype=bool); first[pb.seg_start] = True
    last = np.zeros(n, dtype=bool); last[np.r_[pb.seg_start[1:] - 1, n - 1]] = True
    served = [not first[rows[k]] and (last[rows[k]] or offs[k] <= (t_[rows[k] + 1] - t_[rows[k]]) * (1.0 + DT_RTOL)) for k in range(m)]
    # the new order: every old row i at key (i, -1, .), query k at key (rows[k], offs[k], k)
    keys = [(i, -1.0, -1, i) for i in range(n)] + [(int(rows[k]), float(offs[k]), k, int(rows[k])) for k in range(m) if served[k]]
    keys.sort(key=lambda t: t[:3])
    src = np.array([t[3] for t in keys])                                # the old row every new row copies
    is_q = np.array([t[2] >= 0 for t in keys])
    index = np.full(m, -1, dtype=np.int64)
    for pos, t in enumerate(keys):
        if t[2] >= 0:
            index[t[2]] = pos
    times = np.asarray(pb.times)[src].copy()
    times[is_q] += np.array([t[1] for t in keys])[is_q]
    obs = np.asarray(pb.obs)[src].copy()
    if pb.na_mode == 0:
        obs[is_q, 0] = capi.na_real()
    else:
        obs[is_q] = np.nan
    take = lambda X: None if X is None else np.asarray(X)[src]
    X_fe = [take(x) for x in pb.X_fe]
    X_re = [take(x) for x in pb.X_re]
    H = None if pb.H is None else np.asarray(pb.H)[:, :, src]
    out = capi.Problem(pb.model, np.asarray(pb.id)[src], times, obs, X_fe=X_fe if any(x is not None for x in X_fe) else None,
                       X_re=X_re if any(x is not None for x in X_re) else None, S_list=pb.S_list or None, a0=pb.a0, P0=pb.P0, H=H,
                       par_fixed=pb.par_fixed, include_penalty=pb.include_penalty, na_mode=pb.na_mode)
    return out, index
