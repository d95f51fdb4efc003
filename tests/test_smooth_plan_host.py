"""The host-side plans of the smoother's consumers (csrc/ssde_smooth_plan.hpp) through the hostsim_predict library: where
ssde_predict's queries land (DESIGN.md §3.11's rules, not the C++), how the groups are cut into chunks, how many draws go into a
batch.

On the caller's own rows the plan holds no time stamps: it places every query whose row carries a state, and a query past the next
fix is turned away by the query kernel's rule (delta > Delta_j (1 + 1e-9), predict_query_row: tests/test_predict_hostsim.py).  So
there the planned set is checked as "has a state", and the planned queries that rule accepts as ~expected_nan; on a lattice handle
the plan itself drops the queries past the next fix and the planned set is ~expected_nan exactly."""
from types import SimpleNamespace

import numpy as np
import pytest

import predictsim_lib
from predict_cases import LENGTHS, expected_nan, intervals, query_set, small_problem

DT_RTOL = 1e-9                # PREDICT_DT_RTOL
DRAW_CH = 4
WAVE = 2                      # lanes per group here: five tracks make three groups, so the chunk ranges have something to cut


def _natural():
    pb, _ = small_problem("CTCRW", 2)
    rows, offs = query_set(pb, seed=3)
    seg = np.asarray(pb.seg_start, dtype=np.int64)
    nrows = np.diff(np.append(seg, pb.n))
    return dict(pb=pb, rows=rows, offs=offs, row0=seg, ns=nrows - 1, pad_row=None, step=0.0,
                t_of=lambda lane_row: np.asarray(pb.times)[lane_row])


def _lattice():
    """LENGTHS on a lattice of 0.5 with gaps of one to four steps, laid out the way a lattice-padded handle keeps them: every
    track on consecutive lattice rows, the absent fixes as rows of their own"""
    step, rng = 0.5, np.random.default_rng(12)
    times, seg, pad_row, row0, ns, t_lat = [], [], [], [], [], []
    t0, p0 = 3.0, 0
    for T in LENGTHS:
        inc = np.r_[0, rng.permutation(np.resize([1, 2, 3, 4, 1, 2, 3, 4], T - 1))] if T > 1 else np.zeros(1, dtype=int)
        idx = np.cumsum(inc)
        seg.append(len(times))
        times += list(t0 + step * idx)                      # (multiples of 0.5: exact)
        pad_row += list(p0 + idx)
        row0.append(p0); ns.append(int(idx[-1]))
        t_lat += list(t0 + step * np.arange(idx[-1] + 1))
        p0 += int(idx[-1]) + 1
        t0 = times[-1] + 7.25
    pb = SimpleNamespace(n=len(times), seg_start=np.array(seg), times=np.array(times))
    first, last, dt = intervals(pb)
    rows, offs = query_set(pb, seed=17, per_row=False)
    gaps = np.flatnonzero(~first & ~last & (dt > 0.75))     # intervals of two to four lattice steps
    assert len(gaps) >= 8 and {1.0, 1.5, 2.0} <= set(dt[gaps])
    # in every such gap: on a lattice point, just before and after one, in the last step, at the gap's end
    rows = np.r_[rows, np.repeat(gaps, 5)]
    offs = np.r_[offs, np.c_[np.full(len(gaps), 0.5), np.full(len(gaps), 0.49), np.full(len(gaps), 0.61), dt[gaps] - 0.2, dt[gaps]].ravel()]
    t_lat = np.array(t_lat)
    return dict(pb=pb, rows=rows, offs=offs, row0=np.array(row0, dtype=np.int64), ns=np.array(ns), pad_row=np.array(pad_row, dtype=np.int64),
                step=step, t_of=lambda lane_row: t_lat[lane_row])


CASES = {"natural": _natural, "lattice": _lattice}


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_query_plan(case, reverse):
    c = CASES[case]()
    pb, rows, offs = c["pb"], c["rows"], c["offs"]
    row0, ns = (c["row0"][::-1], c["ns"][::-1]) if reverse else (c["row0"], c["ns"])   # (the TV route's lanes are not sorted by row)
    nl, nq = len(row0), len(rows)
    n_groups = (nl + WAVE - 1) // WAVE
    P = predictsim_lib.plan_queries(row0, ns, rows, offs, pad_row=c["pad_row"], pad_step=c["step"], cuts=np.arange(n_groups + 1), wave=WAVE)
    order, q_slot, off, want_off, want_step = P["order"], P["q_slot"], P["off"], P["want_off"], P["want_step"]
    first, last, dt = intervals(pb)
    times = np.asarray(pb.times, dtype=np.float64)

    # ---- which queries are planned
    one_row = np.isin(rows, np.asarray(pb.seg_start)[np.array(LENGTHS) == 1])
    wanted = ~expected_nan(pb, rows, offs) & ~one_row
    planned = np.zeros(nq, dtype=bool); planned[order] = True
    assert len(set(order)) == len(order)
    if case == "lattice":
        assert np.array_equal(planned, wanted)
    else:
        assert np.array_equal(planned, ~first[rows])                                    # every row that carries a state
        accepted = planned & (last[rows] | ~(offs > dt[rows] * (1.0 + DT_RTOL)))         # ... the query kernel's rule on the rest
        assert np.array_equal(accepted, wanted)
    assert wanted.sum() > nq // 2 and (~wanted).sum() >= len(LENGTHS)

    # ---- every planned query: its lane, its step, its residual
    assert len(want_off) == nl + 1 and want_off[0] == 0 and want_off[-1] == len(want_step)
    lane_of_slot = np.repeat(np.arange(nl), np.diff(want_off))                          # want_off is the prefix count of the lists
    tol = DT_RTOL * (c["step"] if case == "lattice" else 1.0)
    for i, k in enumerate(order):
        l, st = lane_of_slot[q_slot[i]], want_step[q_slot[i]]
        assert 0 <= st < ns[l]
        # the lane is the query's track
        p = rows[k] if c["pad_row"] is None else c["pad_row"][rows[k]]
        assert row0[l] < p <= row0[l] + ns[l]
        assert off[i] >= 0.0
        assert abs(c["t_of"](row0[l] + 1 + st) + off[i] - (times[rows[k]] + offs[k])) <= tol, (k, l, st, off[i])
    for l in range(nl):
        assert np.all(np.diff(want_step[want_off[l]:want_off[l + 1]]) > 0)              # strictly ascending per lane
    assert np.all(np.diff(want_off) >= 0)
    assert np.all(np.diff(q_slot) >= 0) and set(q_slot) == set(range(len(want_step)))   # every slot is wanted by a query
    # stable: queries of one slot keep the caller's order
    assert all(order[i] < order[i + 1] for i in range(len(order) - 1) if q_slot[i] == q_slot[i + 1])
    dup = [i for i in range(len(order) - 1) if q_slot[i] == q_slot[i + 1] and off[i] == off[i + 1]]
    assert dup                                                                          # (query_set's duplicate pair is among them)

    # ---- the chunks: consecutive, and they cover everything
    r = P["ranges"]
    assert r.shape == (n_groups, 4)
    assert r[0, 0] == 0 and r[0, 2] == 0 and r[-1, 1] == len(want_step) and r[-1, 3] == len(order)
    assert np.array_equal(r[1:, 0], r[:-1, 1]) and np.array_equal(r[1:, 2], r[:-1, 3])
    for g in range(n_groups):
        s0, s1, q0, q1 = r[g]
        assert s0 == want_off[min(g * WAVE, nl)] and s1 == want_off[min((g + 1) * WAVE, nl)]
        assert np.all((q_slot[q0:q1] >= s0) & (q_slot[q0:q1] < s1))


def test_chunk_groups():
    rng = np.random.default_rng(4)
    for G in (1, 2, 7, 40):
        goff = np.r_[0, np.cumsum(rng.integers(1, 50, size=G) * 31 * 64)]
        sizes = np.diff(goff)
        for budget in (1, int(sizes.max()), int(sizes.max()) * 3 + 5, int(goff[-1]), int(goff[-1]) * 2):
            cut = predictsim_lib.chunk_groups(goff, budget)
            assert cut[0] == 0 and cut[-1] == G and np.all(np.diff(cut) > 0)
            for a, b in zip(cut[:-1], cut[1:]):
                assert goff[b] - goff[a] <= budget or b - a == 1
            if budget == 1:
                assert np.array_equal(cut, np.arange(G + 1))
            if budget >= goff[-1]:
                assert len(cut) == 2


def test_batch_caps():
    for budget in (0, 1, 999, 10**6, 10**12):
        for per_draw in (0, 1, 37, 10**5):
            for n_draws in (1, 3, 4, 5, 1000, 2**27):
                a = predictsim_lib.batch_cap(budget, per_draw, 1, DRAW_CH, n_draws)       # ssde_smooth_draws
                assert 1 <= a <= n_draws and a <= DRAW_CH << 15
                if per_draw > 0:
                    b = predictsim_lib.batch_cap(budget, per_draw, DRAW_CH, DRAW_CH, n_draws)   # ssde_path_stats
                    assert 1 <= b <= n_draws and b <= DRAW_CH << 15
                    assert b % DRAW_CH == 0 or b == n_draws
                    if a > 1:
                        assert a * per_draw <= budget                                   # beyond the one that always goes, a batch fits


# ---- a parent of several engines: the deal of the queries and the placement of the engines' outputs --------------------------------
# Two track shards of 3 and 4 rows crossed with two column pairs: the parent has sd = 4 from engines of sd = 2, shard k = 2 * track
# shard + pair, as the engine orders them.
ROWS = [(0, 3), (3, 4)]
N, SD, sd = 7, 4, 2


def _engines():
    return [(lo, m, 2 * pair) for lo, m in ROWS for pair in (0, 1)]


def test_deal_queries():
    q_row = np.array([4, 6, 3, 5, 4], dtype=np.int64)                    # five queries, none of them on the first shard's rows
    q_off = np.array([0.5, 0.0, 1.25, 0.5, 0.75])
    got = [predictsim_lib.deal_queries(lo, m, q_row, q_off) for lo, m in ROWS]
    assert all(len(v) == 0 for v in got[0])
    idx, rows, offs = got[1]
    assert np.array_equal(idx, np.arange(5)) and np.array_equal(rows, q_row - 3) and np.array_equal(offs, q_off)
    # ... and one on each side of the boundary, in the caller's order
    q_row[[1, 3]] = [2, 0]
    for lo, m in ROWS:
        idx, rows, offs = predictsim_lib.deal_queries(lo, m, q_row, q_off)
        mine = np.flatnonzero((q_row >= lo) & (q_row < lo + m))
        assert np.array_equal(idx, mine) and np.array_equal(rows, q_row[mine] - lo) and np.array_equal(offs, q_off[mine])


def test_place_columns_by_rows_and_by_queries():
    rng = np.random.default_rng(1)
    dst, ref = np.full((N, SD), np.nan, order="F"), np.full((N, SD), np.nan)
    for lo, m, c0 in _engines():
        src = np.asfortranarray(rng.standard_normal((m, sd)))
        predictsim_lib.place_columns(dst, c0, src, lo=lo)
        ref[lo:lo + m, c0:c0 + sd] = src
    assert np.array_equal(dst, ref) and not np.isnan(dst).any()
    # the dealt queries: five of them, the first shard gets none (so its rows of the output keep the preset)
    q_row = np.array([4, 6, 3, 5, 4], dtype=np.int64)
    dst, ref = np.full((5, SD), np.nan, order="F"), np.full((5, SD), np.nan)
    for lo, m, c0 in _engines():
        idx = np.flatnonzero((q_row >= lo) & (q_row < lo + m))
        src = np.asfortranarray(rng.standard_normal((len(idx), sd)))
        predictsim_lib.place_columns(dst, c0, src, idx=idx)
        ref[idx, c0:c0 + sd] = src
    assert np.array_equal(dst, ref) and not np.isnan(dst).any()


@pytest.mark.parametrize("by_query", [False, True])
def test_place_cov_block_and_the_all_nan_rule(by_query):
    """Row 1 of the second track shard is NaN in the first pair only, row 2 of it in both.  The rule runs engine by engine, as the
    engine runs it: a NaN block blanks the parent's whole row, and a pair placed later writes its own block over that."""
    rng = np.random.default_rng(2)
    dst, ref = np.zeros((N, SD, SD), order="F"), np.zeros((N, SD, SD))
    perm = rng.permutation(N)                                             # by_query: row i of an engine is the parent's row perm[lo + i]
    for lo, m, c0 in _engines():
        src = np.asfortranarray(rng.standard_normal((m, sd, sd)))
        if lo == 3:
            src[2] = np.nan
            if c0 == 0:
                src[1] = np.nan
        at = perm[lo:lo + m] if by_query else np.arange(lo, lo + m)
        predictsim_lib.place_block(dst, c0, src, lo=0 if by_query else lo, idx=at if by_query else None)
        ref[at, c0:c0 + sd, c0:c0 + sd] = src
        ref[at[np.isnan(src[:, 0, 0])]] = np.nan
    assert np.array_equal(dst, ref, equal_nan=True)
    one, both, full = (perm[4], perm[5], perm[0]) if by_query else (4, 5, 0)
    assert np.isnan(dst[both]).all()
    assert np.isnan(dst[one]).sum() == SD * SD - sd * sd and not np.isnan(dst[one, 2:, 2:]).any()     # the later pair's block stands
    assert np.all(dst[full, :2, 2:] == 0.0) and np.all(dst[full, 2:, :2] == 0.0) and not np.isnan(dst[full]).any()   # cross-pair blocks
    # without the rule (ssde_smooth_loo's placement): the blocks alone
    dst2 = np.zeros((N, SD, SD), order="F")
    src = np.asfortranarray(np.full((4, sd, sd), np.nan))
    predictsim_lib.place_block(dst2, 2, src, lo=3, nan_rule=False)
    assert np.isnan(dst2[3:, 2:, 2:]).all() and np.isnan(dst2).sum() == 4 * sd * sd


def test_place_track_stats_moves_the_row_of_a_maximum():
    """track shards of 2 and 3 tracks whose rows start at 0 and 40; statistic 2 of 4 is the row of a maximum, NaN for one track"""
    rng = np.random.default_rng(3)
    NT, n_stat, n_rep = 5, 4, 3
    dst, ref = np.full((NT, n_stat, n_rep), np.nan, order="F"), np.full((NT, n_stat, n_rep), np.nan)
    for track0, mt, lo in ((0, 2, 0), (2, 3, 40)):
        src = np.asfortranarray(rng.integers(0, 30, size=(mt, n_stat, n_rep)).astype(np.float64))
        src[mt - 1, 2, 1] = np.nan
        predictsim_lib.place_track_stats(dst, track0, src, 2, lo)
        ref[track0:track0 + mt] = src
        ref[track0:track0 + mt, 2] += lo
    assert np.array_equal(dst, ref, equal_nan=True) and np.isnan(dst).sum() == 2 and np.all(dst[2:, 2, 0] >= 40)
    plain = np.full((NT, n_stat, 1), np.nan, order="F")
    src = np.asfortranarray(rng.standard_normal((3, n_stat, 1)))
    predictsim_lib.place_track_stats(plain, 2, src, -1, 40)                            # ssde_path_stats: no row among the statistics
    assert np.array_equal(plain[2:], src) and np.isnan(plain[:2]).all()


def test_max_distinct_offsets_against_limits():
    """rows with runs of 1, 2 and 3 distinct offsets (duplicates and the queries' order do not count); a slot holds at most one more
    than its row's, and the entry points refuse where that reaches the limit (2^32 there, 3 and 4 here)"""
    runs = {1: ([7, 7, 7], [0.5, 0.5, 0.5]), 2: ([3, 9, 3, 3], [0.25, 0.1, 0.0, 0.25]), 3: ([5, 2, 5, 5, 5, 2], [0.3, 0.0, 0.1, 0.2, 0.3, 0.0])}
    for want, (rows, offs) in runs.items():
        got = predictsim_lib.max_distinct_offsets(rows, offs)
        assert got == want == max(len(set(o for r, o in zip(rows, offs) if r == row)) for row in set(rows))
        assert (got + 1 >= 3) == (want >= 2) and (got + 1 >= 4) == (want >= 3)
    assert predictsim_lib.max_distinct_offsets([], []) == 0
    assert predictsim_lib.max_distinct_offsets([1, 1], [0.0, -0.0]) == 1                # +0.0 and -0.0 are one offset
