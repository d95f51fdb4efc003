"""numpy restatement of ssde_path_occupancy_fine for the tests (test infrastructure): the definition and nothing
else.  The quantum rule, the m rule and the split of a row's quanta over its points are part of the definition, so the result is
comparable BITWISE.

* fine_plan: per state row i of the problem's rows (the RESIDENT rows: a written-out lattice with `is_row` flagging the caller's
  rows stands for a lattice-padded handle) that is not its track's last, Delta_i = times[i + 1] - times[i] and
  m_i = min(64, max(1, ceil(Delta_i / max_step))) (np.ceil of an IEEE quotient); a track's last state row has m = 1.  The inner
  points of row i are the queries (i, (k * Delta_i) / m_i), k = 1 .. m_i - 1.  A caller's state row j owns the points of the rows
  from j up to, not including, the next caller's row; N_j is their number.
* occ_fine_counts: on ANY provider's draws at the rows (n_draws, n, sdim) and at the plan's queries (n_draws, n_query, sdim) -- the
  reference's (draws_ref.draws_ref and bridge_ref.predict_draws_ref), the host twin's or a GPU's own smooth_draws + predict_draws.
  Row j's W_j quanta: every one of its N_j points gets W_j // N_j, its own point W_j % N_j more; a point goes to the cell of its
  position by occ_ref.cells_of, a point with a non-finite coordinate outside.
* occ_fine_ref: the same on the reference draws.
"""
from __future__ import annotations

import numpy as np

from occ_ref import cells_of, quantise, quantum_exp
from path_ref import position_columns

MAX_SUB = 64


def substeps(dt, max_step, max_sub=MAX_SUB):
    """(m, capped) of intervals dt: an interval that is NaN or <= 0 has one sub-step"""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.ceil(np.asarray(dt, dtype=np.float64) / float(max_step))
    capped = c > max_sub
    m = np.where(c >= 1.0, np.minimum(c, max_sub), 1.0)
    return m.astype(np.int64), capped


def fine_plan(times, seg_start, max_step, is_row=None, group=None, max_sub=MAX_SUB):
    """m [n] (0 on the rows without a state), the queries of the inner points (q_rows, q_offs) with row i's at q_ptr[i] .. q_ptr[i + 1],
    owner [n] (the caller's state row that owns row i's points, -1: none), caller [n] (the row is a row of the caller's data), n_points
    and n_capped over the tracks that take part"""
    times = np.asarray(times, dtype=np.float64)
    n = len(times)
    bounds = np.r_[np.asarray(seg_start, dtype=np.int64), n]
    m = np.zeros(n, dtype=np.int64)
    owner = np.full(n, -1, dtype=np.int64)
    n_capped = 0
    for t in range(len(bounds) - 1):
        first, last = int(bounds[t]), int(bounds[t + 1]) - 1
        takes_part = group is None or int(group[t]) >= 0
        if last > first:
            inner = np.arange(first + 1, last)
            mm, capped = substeps(times[inner + 1] - times[inner], max_step, max_sub)
            m[inner], m[last] = mm, 1
            n_capped += int(capped.sum()) if takes_part else 0
        own = -1
        for i in range(first + 1, last + 1):
            if is_row is None or is_row[i]:
                own = i
            owner[i] = own
    q_ptr = np.r_[0, np.cumsum(np.maximum(m - 1, 0))]
    q_rows = np.repeat(np.arange(n), np.maximum(m - 1, 0))
    k = np.arange(len(q_rows)) - q_ptr[q_rows] + 1
    dt = np.r_[np.diff(times), 1.0]
    q_offs = (k * dt[q_rows]) / m[q_rows]
    seg_of = np.searchsorted(bounds, np.arange(n), side="right") - 1
    part = np.ones(n, dtype=bool) if group is None else np.asarray(group)[seg_of] >= 0
    n_points = int(m[(owner >= 0) & part].sum())
    caller = np.ones(n, dtype=bool) if is_row is None else np.asarray(is_row, dtype=bool)
    return dict(m=m, q_rows=q_rows, q_offs=q_offs, q_ptr=q_ptr, owner=owner, caller=caller, n_points=n_points, n_capped=n_capped)


def occ_fine_counts(row_draws, inner_draws, plan, seg_start, model, d, grid, weight=None, group=None, n_groups=1, n_rows=None):
    """(counts (n_groups, ny, nx) uint64, outside counts (n_groups,) uint64, e); weight is indexed by the rows of row_draws (read at
    the caller's rows only), n_rows the rows of the caller's data (which set the quantum)"""
    row_draws = np.asarray(row_draws, dtype=np.float64)
    inner_draws = np.asarray(inner_draws, dtype=np.float64)
    nd, n, _ = row_draws.shape
    m, owner, q_ptr, q_rows = plan["m"], plan["owner"], plan["q_ptr"], plan["q_rows"]
    callers = np.flatnonzero(owner == np.arange(n))
    n_rows = (n if n_rows is None else n_rows)
    cols = position_columns(model, d)
    nx, ny = grid["nx"], (grid["ny"] if d == 2 else 1)
    w = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64)
    e = quantum_exp(1.0 if weight is None else np.max(w[plan["caller"]], initial=0.0), n_rows, nd)      # wmax: over ALL the caller's rows
    W = np.zeros(n, dtype=np.uint64)
    W[callers] = quantise(w[callers], e)
    N = np.zeros(n, dtype=np.uint64)
    np.add.at(N, owner[owner >= 0], m[owner >= 0].astype(np.uint64))
    share = np.zeros(n, dtype=np.uint64)                                 # per resident row: the quanta of each of its points ...
    has = owner >= 0
    share[has] = W[owner[has]] // N[owner[has]]
    own = share.copy()                                                    # ... and of its own point
    own[callers] += W[callers] % N[callers]
    bounds = np.r_[np.asarray(seg_start, dtype=np.int64), n]
    seg_of = np.searchsorted(bounds, np.arange(n), side="right") - 1
    grp = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)[seg_of]
    occ = np.zeros((n_groups, nx * ny), dtype=np.uint64)
    out = np.zeros(n_groups, dtype=np.uint64)
    for pos, wt, g in ((row_draws[:, :, cols], own, grp), (inner_draws[:, :, cols], share[q_rows], grp[q_rows])):
        keep = (wt > 0) & (g >= 0)
        if not np.any(keep):
            continue
        cell = cells_of(pos[:, keep], grid, d)                            # n_draws x points
        wts = np.broadcast_to(wt[keep][None, :], cell.shape)
        gs = np.broadcast_to(g[keep][None, :], cell.shape)
        inside = cell >= 0
        np.add.at(occ, (gs[inside], cell[inside]), wts[inside])
        np.add.at(out, gs[~inside], wts[~inside])
    return occ.reshape(n_groups, ny, nx), out, e


def to_float(occ, out, e):
    assert max(int(occ.max(initial=0)), int(out.max(initial=0))) < 2 ** 52
    return np.ldexp(occ.astype(np.float64), e), np.ldexp(out.astype(np.float64), e)


def reference_draws(pb, par, plan, seed=0, draw0=0, n_draws=1):
    """(draws at the rows, draws at the plan's queries) by the reference (draws_ref, predict_draws_ref)"""
    from bridge_ref import predict_draws_ref
    from draws_ref import draws_ref
    with np.errstate(invalid="ignore"):
        rows = draws_ref(pb, par, seed=seed, draw0=draw0, n_draws=n_draws)
        if len(plan["q_rows"]):
            inner = predict_draws_ref(pb, par, plan["q_rows"], plan["q_offs"], seed=seed, draw0=draw0, n_draws=n_draws)
        else:
            inner = np.zeros((n_draws, 0, rows.shape[2]))
    return rows, inner


def occ_fine_ref(pb, par, grid, max_step, seed=0, draw0=0, n_draws=1, weight=None, group=None, n_groups=1, is_row=None, n_rows=None,
                 draws=None):
    """(occ (n_groups, ny, nx), outside (n_groups,)) as ssde_path_occupancy_fine returns them on a handle whose resident rows are pb's;
    draws: reference_draws' pair, where the caller has it already"""
    plan = fine_plan(pb.times, pb.seg_start, max_step, is_row=is_row, group=group)
    rows, inner = draws if draws is not None else reference_draws(pb, par, plan, seed=seed, draw0=draw0, n_draws=n_draws)
    return to_float(*occ_fine_counts(rows, inner, plan, pb.seg_start, pb.model, pb.n_dim, grid, weight=weight, group=group,
                                     n_groups=n_groups, n_rows=n_rows))


def all_points(rows, inner):
    """every point's draw as one (n_draws, n + n_query, sdim) array: what occ_cases.make_grid / clear_of_lines take"""
    return np.concatenate([rows, inner], axis=1)
