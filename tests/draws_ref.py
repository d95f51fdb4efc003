"""numpy restatement of ssde_smooth_draws for the tests (test infrastructure), written from the definition.

* draws_ref: the filter's forward loop keeping a_j, P_j, v_j, F_j^-1 and T_j per state row (the update rule of smooth_ref), then
  backward sampling: alpha_last = a_f + chol(P_f) z, alpha_j = a_f + J (alpha_{j+1} - a_{j+1}) + chol(C) z with
  J = P_f T_j' P_{j+1}^-1 and C = sym(P_f - J P_{j+1} J').  One track after the other, vectorised over the draws.
* joint_full: the ground truth for one short track -- mean and the FULL cross-time covariance of the states given the observations,
  from the dense joint Gaussian (smooth_ref.joint_track keeps the diagonal blocks only).
* Deviates: sim_ref.normal_pair(seed, track, s, draw * 8 + (c >> 1))[c & 1] -- track the ID segment's ordinal, s the state row's
  position in the track, c the state column -- or `normals` (n_draws x n x sdim, indexed by the row) in their place.
"""
from __future__ import annotations

import numpy as np

from sim_ref import normal_pair
from smooth_ref import _setup, _trans


def chol_zero(S):
    """lower Cholesky factor in state order; a pivot <= 0 gives a zero column"""
    m = S.shape[0]
    L = np.zeros((m, m))
    for j in range(m):
        s = S[j, j] - L[j, :j] @ L[j, :j]
        if s <= 0.0:
            continue
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, m):
            L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def chol_nan(S):
    """lower Cholesky factor; a pivot <= 0 gives NaN through the square root"""
    m = S.shape[0]
    L = np.zeros((m, m))
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(m):
            L[j, j] = np.sqrt(S[j, j] - L[j, :j] @ L[j, :j])
            for i in range(j + 1, m):
                L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def philox_normals(seed, draw0, n_draws, track, n_rows, sd):
    """(n_draws, n_rows, sd) deviates of one track's state rows s = 0 ... n_rows - 1"""
    z = np.empty((n_draws, n_rows, sd))
    s = np.arange(n_rows, dtype=np.uint64)[None, :]
    draw = (draw0 + np.arange(n_draws, dtype=np.uint64))[:, None]
    for p in range(0, sd, 2):
        n1, n2 = normal_pair(seed, np.uint64(track), s, draw * np.uint64(8) + np.uint64(p >> 1))
        z[:, :, p] = n1
        if p + 1 < sd:
            z[:, :, p + 1] = n2
    return z


def draws_ref(pb, par, seed=0, draw0=0, n_draws=1, normals=None):
    """(n_draws, n, sdim): joint posterior draws of the state path, NaN on rows without a state."""
    d, sd, n, model = pb.n_dim, pb.sdim, pb.n, pb.model
    pm, dt, Z, H, P0, bounds, a0s, na = _setup(pb, par)
    obs = np.asarray(pb.obs, dtype=np.float64)
    Ta, Qa, ca = _trans(model, d, pm, dt)
    out = np.full((n_draws, n, sd), np.nan)
    for k in range(pb.n_seg):
        r0, r1 = bounds[k], bounds[k + 1]
        rows = np.arange(r0 + 1, r1)
        m = len(rows)
        if m == 0:
            continue
        # ---- forward: the records ----
        a, P = np.array(a0s[k], dtype=np.float64), P0.copy()
        rec = []
        for i in rows:
            T, Q, c = Ta[i], Qa[i], ca[i]
            F = Z @ P @ Z.T + H[i]
            det = F[0, 0] if d == 1 else (F[0, 0] * F[1, 1] - F[1, 0] * F[0, 1] if d == 2 else abs(np.linalg.det(F)))
            upd = (not na[i]) and ((det > 0) if model == "CTCRW" else (abs(det) > 0))
            if upd:
                Fi = np.linalg.inv(F)
                Fi = 0.5 * (Fi + Fi.T)
                v = obs[i] - Z @ a
            else:
                Fi, v = np.zeros((d, d)), np.zeros(d)
            rec.append((a, P, v, Fi, T))
            TP = T @ P
            K = TP @ Z.T @ Fi
            drift = upd or na[i] or model != "CTCRW"
            a = T @ a + K @ v + (c if drift else 0.0)
            P = TP @ T.T + Q - TP @ Z.T @ K.T
            if d > 1:
                P = 0.5 * (P + P.T)
        # ---- backward: the draws ----
        z = normals[:, rows, :] if normals is not None else philox_normals(seed, draw0, n_draws, k, m, sd)
        alpha = None
        for s in range(m - 1, -1, -1):
            a, P, v, Fi, T = rec[s]
            G = P @ Z.T @ Fi
            af = a + G @ v
            Pf = P - G @ Z @ P
            Pf = 0.5 * (Pf + Pf.T)
            if s == m - 1:
                mean = np.repeat(af[None], n_draws, 0)
                C = Pf
            else:
                an, Pn = rec[s + 1][0], rec[s + 1][1]
                Lp = chol_nan(Pn)
                with np.errstate(invalid="ignore", divide="ignore"):
                    Li = np.linalg.inv(Lp) if np.all(np.isfinite(Lp)) else np.full((sd, sd), np.nan)
                    J = Pf @ T.T @ Li.T @ Li
                    C = Pf - J @ Pn @ J.T
                    C = 0.5 * (C + C.T)
                    mean = af[None] + (alpha - an[None]) @ J.T
            with np.errstate(invalid="ignore"):
                alpha = mean + z[:, s, :] @ chol_zero(C).T
            out[:, rows[s], :] = alpha
    return out


def joint_full(pb, par, k):
    """(mean m x sd, cov (m sd) x (m sd)) of track k's states given its observations, from the dense joint Gaussian
    (state rows r0 + 1 ... r1 - 1, m of them; the construction of smooth_ref.joint_track with every block kept)"""
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
        C = Vm[t]
        for u in range(t, m_):
            Sig[u * sd:(u + 1) * sd, t * sd:(t + 1) * sd] = C
            Sig[t * sd:(t + 1) * sd, u * sd:(u + 1) * sd] = C.T
            if u + 1 < m_:
                C = T[u] @ C
    obs_t = [j for j in range(m_) if not na[rows[j]]]
    if not obs_t:
        return mu, Sig
    G = np.zeros((len(obs_t) * d, m_ * sd))
    Hb = np.zeros((len(obs_t) * d, len(obs_t) * d))
    y = np.zeros(len(obs_t) * d)
    for q, j in enumerate(obs_t):
        G[q * d:(q + 1) * d, j * sd:(j + 1) * sd] = Z
        Hb[q * d:(q + 1) * d, q * d:(q + 1) * d] = H[rows[j]]
        y[q * d:(q + 1) * d] = pb.obs[rows[j]]
    Syy = G @ Sig @ G.T + Hb
    Say = Sig @ G.T
    W = np.linalg.solve(Syy, np.c_[y - G @ mu.reshape(-1), Say.T])
    mean = mu.reshape(-1) + Say @ W[:, 0]
    covf = Sig - Say @ W[:, 1:]
    return mean.reshape(m_, sd), 0.5 * (covf + covf.T)
