"""numpy restatement of ssde_predict_draws for the tests (test infrastructure), written from the definition.

* predict_draws_ref: the draw's states at the rows from draws_ref.draws_ref; then, per row with queries, the distinct offsets in
  ascending order, each drawn from the conditional of x_t given both ends -- the last answer below it (or the row's state) and the
  draw's state at the next row -- through plain np.linalg solves: mean m1 + G S^-1 (alpha_next - m2), covariance Q1 - G S^-1 G' with
  G = Q1 T2'.  Past a track's last row: a plain simulation step.  One row after the other, vectorised over the draws.
* Deviates: sim_ref.normal_pair with the counter words (s, track ordinal, rank, 2^31 | (draw * 8 + (c >> 1))), element c & 1 -- or
  `normals` = (row deviates (n_draws x n x sdim), bridge deviates (n_draws x n_query x sdim): an offset takes those of the first
  query that carries it) in their place.
* bridge_queries: the query sets of the CPU suites, over every rule of the definition.
"""
from __future__ import annotations

import numpy as np

from draws_ref import chol_nan, chol_zero, draws_ref
from predict_ref import DT_RTOL, predict_ref
from sim_ref import normal_pair
from smooth_ref import _setup, _trans


def bridge_normals(seed, draw0, n_draws, track, s, rank, sd, col0=0):
    """(n_draws, sd) deviates of rank `rank` of the slot at state row s of track `track`"""
    z = np.empty((n_draws, sd))
    draw = draw0 + np.arange(n_draws, dtype=np.uint64)
    trk = np.uint64((int(track) & 0xFFFFFFFF) | (int(rank) << 32))
    for p in range(0, sd, 2):
        n1, n2 = normal_pair(seed, trk, np.uint64(s), np.uint64(1 << 31) | (draw * np.uint64(8) + np.uint64((col0 + p) >> 1)))
        z[:, p] = n1
        if p + 1 < sd:
            z[:, p + 1] = n2
    return z


def predict_draws_ref(pb, par, rows, offs, seed=0, draw0=0, n_draws=1, normals=None):
    """(n_draws, n_query, sdim): the draws' states at the queries (rows[k], offs[k]); NaN where the definition says so."""
    d, sd, n, model = pb.n_dim, pb.sdim, pb.n, pb.model
    rows = np.asarray(rows, dtype=np.int64).ravel()
    offs = np.asarray(offs, dtype=np.float64).ravel()
    m = len(rows)
    pm, dt, Z, H, P0, bounds, a0s, na = _setup(pb, par)
    paths = draws_ref(pb, par, seed=seed, draw0=draw0, n_draws=n_draws, normals=None if normals is None else normals[0])
    served = ~np.isnan(predict_ref(pb, par, rows, np.zeros(m))["mean"][:, 0])     # the row has a state and did not reject its update
    seg_of = np.searchsorted(np.asarray(bounds), np.arange(n), side="right") - 1
    out = np.full((n_draws, m, sd), np.nan)
    for j in np.unique(rows[served]):
        j = int(j)
        k = int(seg_of[j])
        last = j == bounds[k + 1] - 1
        s = j - bounds[k] - 1
        mine = np.flatnonzero(rows == j)
        uniq = np.unique(offs[mine])                                    # ascending; +0.0 and -0.0 are one offset
        t_prev, x_prev = 0.0, paths[:, j, :]
        for rank, delta in enumerate(uniq):
            who = mine[offs[mine] == delta]
            if delta == 0.0:
                out[:, who, :] = paths[:, j, None, :]
                continue
            if not last and delta > dt[j] * (1.0 + DT_RTOL):
                break
            if not last and delta >= dt[j]:
                out[:, who, :] = paths[:, j + 1, None, :]
                continue
            T1, Q1, c1 = _trans(model, d, pm[j:j + 1], np.array([delta - t_prev]))
            m1 = x_prev @ T1[0].T + c1[0]
            if last:
                mean, C = m1, Q1[0]
            else:
                T2, Q2, c2 = _trans(model, d, pm[j:j + 1], np.array([dt[j] - delta]))
                S = T2[0] @ Q1[0] @ T2[0].T + Q2[0]
                S = 0.5 * (S + S.T)
                m2 = m1 @ T2[0].T + c2[0]
                G = Q1[0] @ T2[0].T
                if np.all(np.isfinite(chol_nan(S))):
                    W = np.linalg.solve(S, np.c_[(paths[:, j + 1, :] - m2).T, G.T])
                    mean = m1 + (G @ W[:, :n_draws]).T
                    C = Q1[0] - G @ W[:, n_draws:]
                    C = 0.5 * (C + C.T)
                else:
                    mean, C = np.full_like(m1, np.nan), np.zeros((sd, sd))
            z = normals[1][:, who[0], :] if normals is not None else bridge_normals(seed, draw0, n_draws, k, s, rank, sd)
            with np.errstate(invalid="ignore"):
                x = mean + z @ chol_zero(C).T
            out[:, who, :] = x[:, None, :]
            t_prev, x_prev = float(delta), x
    return out


def bridge_queries(pb, seed=0, shuffle=True, frac=1.0):
    """Queries over every rule: on the interior state rows, in turn, 1, 2 and 5 distinct offsets inside the interval, then 0, Delta and
    a duplicate pair inside; past every track's last row 0 and a chain of three forecasts; a query on every first row and one past
    the next fix (both NaN); in no particular order.  frac < 1: only that share of the interior rows and of the tracks' ends is asked."""
    from predict_cases import intervals
    rng = np.random.default_rng(seed)
    first, last, dt = intervals(pb)
    pats = [[0.5], [0.3, 0.8], [0.1, 0.25, 0.5, 0.75, 0.9], [0.0, 1.0, 0.4, 0.4]]
    rows, offs, turn = [], [], 0
    for j in range(pb.n):
        if first[j]:
            rows += [j]; offs += [0.05]
        elif frac < 1.0 and rng.uniform() >= frac:
            continue
        elif last[j]:
            rows += [j] * 4; offs += [0.0, 0.25, 1.7, 6.0]
        else:
            f = pats[turn % len(pats)]; turn += 1
            rows += [j] * len(f); offs += [dt[j] if x == 1.0 else x * dt[j] for x in f]
    inner = np.flatnonzero(~first & ~last)
    if len(inner):
        j = int(inner[len(inner) // 2])
        rows += [j]; offs += [1.5 * dt[j]]
    rows, offs = np.array(rows, dtype=np.int64), np.array(offs, dtype=np.float64)
    if shuffle:
        p = rng.permutation(len(rows))
        rows, offs = rows[p], offs[p]
    return rows, offs


def compare_draws(got, ref, tag, tol=1e-9):
    """the twin's limit (§3.9 / §3.11): 1e-9 (1 + max|ref|), NaN patterns identical.  Returns the gap."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
    ok = ~np.isnan(ref)
    gap = np.max(np.abs(got[ok] - ref[ok]), initial=0.0) / (1.0 + np.max(np.abs(ref[ok]), initial=0.0))
    print(f"GAP {tag}: {gap:.2e}")
    assert gap <= tol, (tag, gap)
    return gap


# ---- the statistical check of the GPU suite, confirmed on the CPU by the host twin (test_predict_draws_hostsim.py) ----
def stat_problem():
    """4 tracks x 12 rows; 3 interior offsets per interval and 2 forecasts per track"""
    from predict_cases import intervals
    from smoothsde_amd import capi
    from smoothsde_amd.synth import simulate
    ID, times, obs = simulate("CTCRW", 4, 12, 2, seed=21)
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = np.array([-1.0, 0.05, -0.05, 0.4, 0.1])
    first, last, dt = intervals(pb)
    rows, offs = [], []
    for j in range(pb.n):
        if last[j]:
            rows += [j, j]; offs += [0.8, 2.5]
        elif not first[j]:
            rows += [j] * 3; offs += [0.2 * dt[j], 0.5 * dt[j], 0.85 * dt[j]]
    return pb, par, np.array(rows, dtype=np.int64), np.array(offs)


STAT_SEED, STAT_DRAWS = 5, 4096


def stat_ratio(draws, mean, cov):
    """max over queries and columns of |mean of the draws - mean| / sqrt(V_ii / n_draws)"""
    sdv = np.sqrt(np.einsum("kii->ki", cov) / draws.shape[0])
    return float(np.max(np.abs(draws.mean(axis=0) - mean) / sdv))
