"""CPU suite: the definition of ssde_path_occupancy_fine (tests/occ_fine_ref.py) against a per-draw, per-track,
per-point loop in Python integers, and the definition's own properties: exact conservation, m = 1 is ssde_path_occupancy's
definition bit for bit, a weight below the point count stays on the row's own point, the cap, a NaN inner point moves exactly its
share outside, the last state row has one point, draw ranges."""
import math

import numpy as np
import pytest

from cases import make_spec, problem_from_spec
from occ_cases import clear_of_lines, make_grid
from occ_fine_ref import MAX_SUB, all_points, fine_plan, occ_fine_counts, occ_fine_ref, reference_draws, substeps
from occ_ref import occ_counts, occ_ref, quantise, quantum_exp
from path_cases import dt_weights
from path_ref import position_columns

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS = [9, 1, 2, 7]
GROUPINGS = [(None, 1), ([1, 0, -1, 1], 2), ([0, 1, 2, 3], 4)]                 # pooled / two groups with a -1 / a group per track
_CASE = {}


def _case(model, d, irregular=True, n_draws=8, seed=5):
    key = (model, d, irregular, n_draws, seed)
    if key not in _CASE:
        spec = make_spec(f"of_{model}_{d}", model, d, seed=71 + d, lengths=LENGTHS, na_rows=(3, 15), irregular=irregular)
        pb = problem_from_spec(spec)
        b = np.r_[pb.seg_start, pb.n]
        inner = np.concatenate([np.arange(b[t] + 1, b[t + 1] - 1) for t in range(len(b) - 1)])
        max_step = 0.4 * float(np.median(np.diff(pb.times)[inner]))
        plan = fine_plan(pb.times, pb.seg_start, max_step)
        rows, inner_d = reference_draws(pb, spec["par"], plan, seed=seed, n_draws=n_draws)
        grid, _ = make_grid(spec["obs"], all_points(rows, inner_d), model, d, cells=(7, 5))
        rows.setflags(write=False); inner_d.setflags(write=False)
        _CASE[key] = (spec, pb, max_step, plan, rows, inner_d, grid)
    return _CASE[key]


def _loop(pb, rows, inner, max_step, grid, w, group, n_groups):
    """the definition one point at a time, in Python integers: {(group, cell or 'out'): quanta}, and e"""
    model, d, n = pb.model, pb.n_dim, pb.n
    nd = rows.shape[0]
    cols = position_columns(model, d)
    e = quantum_exp(max(w) if len(w) else 0.0, n, nd)
    b = list(pb.seg_start) + [n]
    acc = {}

    def place(g, x, quanta):
        p = [x[c] for c in cols]
        cell = "out"
        if all(math.isfinite(v) for v in p):
            ix = math.floor((p[0] - grid["x0"]) / grid["dx"])
            iy = math.floor((p[1] - grid["y0"]) / grid["dy"]) if d == 2 else 0
            if 0 <= ix < grid["nx"] and 0 <= iy < (grid["ny"] if d == 2 else 1):
                cell = ix + grid["nx"] * iy
        acc[(g, cell)] = acc.get((g, cell), 0) + quanta

    qi = 0
    for t in range(len(b) - 1):
        g = 0 if group is None else group[t]
        for j in range(b[t] + 1, b[t + 1]):
            last = j == b[t + 1] - 1
            m = 1
            if not last:
                c = math.ceil((pb.times[j + 1] - pb.times[j]) / max_step)
                m = min(MAX_SUB, max(1, c))
            W = int(np.rint(np.ldexp(w[j], -e)))
            if g >= 0:
                for q in range(nd):
                    place(g, rows[q, j], W // m + W % m)
                    for k in range(1, m):
                        place(g, inner[q, qi + k - 1], W // m)
            qi += m - 1
    assert qi == inner.shape[1]
    return acc, e


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_the_reference_is_the_point_by_point_loop(model, d):
    spec, pb, max_step, plan, rows, inner, grid = _case(model, d)
    pts = all_points(rows, inner)
    assert clear_of_lines(pts, model, d, grid)
    assert plan["m"].max() >= 4 and len(plan["q_rows"]) == plan["n_points"] - (pb.n - pb.n_seg)
    w = dt_weights(pb.seg_start, pb.times)
    state = np.ones(pb.n, dtype=bool)
    state[pb.seg_start] = False
    seg_of = np.searchsorted(np.r_[pb.seg_start, pb.n], np.arange(pb.n), side="right") - 1
    for group, ng in GROUPINGS:
        occ, out, e = occ_fine_counts(rows, inner, plan, pb.seg_start, model, d, grid, weight=w, group=group, n_groups=ng)
        acc, e2 = _loop(pb, rows, inner, max_step, grid, list(w), group, ng)
        assert e == e2
        flat = occ.reshape(ng, -1)
        for g in range(ng):
            for cell in range(flat.shape[1]):
                assert int(flat[g, cell]) == acc.get((g, cell), 0), (g, cell)
            assert int(out[g]) == acc.get((g, "out"), 0)
            # conservation, exact: n_draws times the group's quanta
            mine = state & ((np.zeros(pb.n, dtype=int) if group is None else np.asarray(group)[seg_of]) == g)
            assert int(flat[g].sum()) + int(out[g]) == rows.shape[0] * int(quantise(w, e)[mine].sum(dtype=np.uint64))
        assert sum(acc.values()) == int(flat.sum()) + int(out.sum())
        assert fine_plan(pb.times, pb.seg_start, max_step, group=group)["n_points"] == \
            sum(int(plan["m"][j]) for j in np.flatnonzero(state) if group is None or group[seg_of[j]] >= 0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("irregular", [True, False])
def test_every_m_one_is_the_definition_of_path_occupancy(model, d, irregular):
    spec, pb, _, _, rows, _, grid = _case(model, d, irregular)
    w = dt_weights(pb.seg_start, pb.times)
    for group, ng in GROUPINGS:
        for ms in (np.inf, 1e6):
            fine = occ_fine_ref(pb, spec["par"], grid, ms, seed=5, n_draws=8, weight=w, group=group, n_groups=ng)
            old = occ_ref(rows, pb.seg_start, model, d, grid, weight=w, group=group, n_groups=ng)
            assert np.array_equal(fine[0], old[0]) and np.array_equal(fine[1], old[1])
    plan = fine_plan(pb.times, pb.seg_start, np.inf)
    assert len(plan["q_rows"]) == 0 and plan["n_points"] == pb.n - pb.n_seg and plan["n_capped"] == 0


def test_a_weight_below_the_point_count_stays_on_the_rows_own_point():
    spec, pb, max_step, plan, rows, inner, grid = _case("CTCRW", 2)
    j = int(np.flatnonzero(plan["m"] >= 3)[0])
    # quanta of 2^e with e set by wmax = 1: row j gets 2 quanta, fewer than its m >= 3 points
    e = quantum_exp(1.0, pb.n, 8)
    w = np.zeros(pb.n)
    w[j] = np.ldexp(2.0, e)
    w[int(np.flatnonzero(plan["m"] == 1)[0])] = 1.0
    occ, out, e2 = occ_fine_counts(rows, inner, plan, pb.seg_start, "CTCRW", 2, grid, weight=w)
    ref_old, out_old, _ = occ_counts(rows, pb.seg_start, "CTCRW", 2, grid, weight=w, n_rows=pb.n)
    assert e2 == e and np.array_equal(occ, ref_old) and np.array_equal(out, out_old)       # nothing reached an inner point


def test_the_cap():
    times = np.r_[0.0, 1.0, 2.0, 102.0, 103.0, 200.0, 201.0]
    plan = fine_plan(times, [0, 5], 1.0)
    assert list(plan["m"]) == [0, 1, 64, 1, 1, 0, 1] and plan["n_capped"] == 1 and plan["n_points"] == 68
    assert substeps(100.0, 1.0) == (64, True) and substeps(64.0, 1.0) == (64, False) and substeps(np.nan, 1.0) == (1, False)
    k = np.arange(1, 64)
    assert np.array_equal(plan["q_offs"], (k * 100.0) / 64) and np.all(plan["q_rows"] == 2)
    assert fine_plan(times, [0, 5], 1.0, group=[-1, 0])["n_capped"] == 0


def test_an_injected_nan_inner_point_moves_exactly_its_share_outside():
    spec, pb, max_step, plan, rows, inner, grid = _case("OU_SSM", 2)
    w = dt_weights(pb.seg_start, pb.times)
    occ, out, e = occ_fine_counts(rows, inner, plan, pb.seg_start, "OU_SSM", 2, grid, weight=w)
    cells = occ.reshape(-1)
    k = next(k for k in range(inner.shape[1]) if np.all(np.isfinite(inner[2, k])))
    from occ_ref import cells_of
    cell = int(cells_of(inner[2, k][None, [0, 1]], grid, 2)[0])
    assert cell >= 0
    j = int(plan["q_rows"][k])
    share = int(quantise(w, e)[j]) // int(plan["m"][j])
    bad = inner.copy()
    bad[2, k, 1] = np.nan
    occ2, out2, _ = occ_fine_counts(rows, bad, plan, pb.seg_start, "OU_SSM", 2, grid, weight=w)
    diff = occ.reshape(-1).astype(np.int64) - occ2.reshape(-1).astype(np.int64)
    assert share > 0 and diff[cell] == share and np.count_nonzero(diff) == 1 and int(out2[0]) - int(out[0]) == share
    # a NaN in a velocity column changes nothing
    spec_c, pb_c, _, plan_c, rows_c, inner_c, grid_c = _case("CTCRW", 2)
    inner_v = inner_c.copy(); inner_v[:, :, 1] = np.nan
    a = occ_fine_counts(rows_c, inner_c, plan_c, pb_c.seg_start, "CTCRW", 2, grid_c)
    b = occ_fine_counts(rows_c, inner_v, plan_c, pb_c.seg_start, "CTCRW", 2, grid_c)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_last_state_row_has_one_point():
    spec, pb, max_step, plan, rows, inner, grid = _case("BM_SSM", 1)
    last = np.r_[pb.seg_start[1:], pb.n] - 1
    has_state = last > np.asarray(pb.seg_start)
    assert np.all(plan["m"][last[has_state]] == 1) and np.all(plan["m"][pb.seg_start] == 0)
    assert not np.any(np.isin(plan["q_rows"], last))
    # whatever the interval to the next track's first row is
    assert np.all(np.diff(pb.times)[last[:-1]] > max_step)


@pytest.mark.parametrize("model", MODELS)
def test_draw_ranges_add_up(model):
    spec, pb, max_step, plan, rows, inner, grid = _case(model, 2)
    first = (rows[:4], inner[:4])
    second = (rows[4:], inner[4:])
    # bitwise where every point's share is a whole number of both calls' quanta: w_j = N_j (on an unpadded handle N_j = m_j)
    wn = plan["m"].astype(np.float64)
    whole = occ_fine_ref(pb, spec["par"], grid, max_step, weight=wn, draws=(rows, inner))
    a = occ_fine_ref(pb, spec["par"], grid, max_step, weight=wn, draws=first)
    b = occ_fine_ref(pb, spec["par"], grid, max_step, weight=wn, draws=second)
    assert np.array_equal(whole[0], a[0] + b[0]) and np.array_equal(whole[1], a[1] + b[1])
    assert whole[0].sum() + whole[1].sum() == 8 * plan["n_points"]
    # the second range drawn on its own is the same numbers
    rows2, inner2 = reference_draws(pb, spec["par"], plan, seed=5, draw0=4, n_draws=4)
    assert np.array_equal(rows2, rows[4:], equal_nan=True) and np.array_equal(inner2, inner[4:], equal_nan=True)
    # otherwise a point's quanta are floors of quotients in two different quanta, 2^e of the whole call and 2^(e - 1) or 2^e of the
    # parts.  W_j is w_j to half a quantum and a share W_j div N_j to one more, so an inner point's amounts differ by less than
    # 2.25 x 2^e between the calls; the row's own point holds W_j less the N_j - 1 shares: less than 3 N_j x 2^e.  Per cell: hits x
    # 3 N_max x 2^e, hits the points of all eight draws in the cell.
    from occ_ref import cells_of
    w = dt_weights(pb.seg_start, pb.times)
    whole = occ_fine_ref(pb, spec["par"], grid, max_step, weight=w, draws=(rows, inner))
    a = occ_fine_ref(pb, spec["par"], grid, max_step, weight=w, draws=first)
    b = occ_fine_ref(pb, spec["par"], grid, max_step, weight=w, draws=second)
    e = quantum_exp(w.max(), pb.n, 8)
    cell = cells_of(all_points(rows, inner)[:, :, position_columns(model, 2)], grid, 2)
    hits = np.bincount(cell[cell >= 0], minlength=grid["nx"] * grid["ny"]).reshape(grid["ny"], grid["nx"])
    gap = np.abs(whole[0][0] - (a[0][0] + b[0][0]))
    print(f"draw ranges {model}: largest gap {gap.max():.3e}, its bound {(hits * 3 * plan['m'].max() * np.ldexp(1.0, e)).max():.3e}")
    assert np.all(gap <= hits * 3 * plan["m"].max() * np.ldexp(1.0, e))
