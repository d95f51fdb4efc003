"""CPU suite: the host plans of ssde_path_occupancy_fine (csrc/ssde_smooth_plan.hpp: plan_all_slots, plan_fine_weights, the m rule and
occ_fine_batch_cap through the small entry points of tests/hostsim/hostsim_occ_fine.cpp) against a numpy restatement, exact."""
import numpy as np

import occfinesim_lib as twin

DRAW_CH, MAX_SUB = 4, 64


def _slots(ns, lane_grp):
    """(lane, step) of every slot, lane-major: the lanes that take part and have a state row"""
    return [(l, s) for l in range(len(ns)) if lane_grp[l] >= 0 and ns[l] > 0 for s in range(ns[l])]


def _restate(ns, lane_grp, row0, slot_dt, max_step, row_map, wq, unit):
    """m, own, share per slot, n_points, n_capped in Python integers"""
    slots = _slots(ns, lane_grp)
    m, own, share = [1] * len(slots), [0] * len(slots), [0] * len(slots)
    n_points = n_capped = 0
    for i, (l, s) in enumerate(slots):
        if s < ns[l] - 1:
            c = np.ceil(np.float64(slot_dt[i]) / np.float64(max_step))
            m[i] = int(min(MAX_SUB, c)) if c >= 1 else 1
            n_capped += int(c > MAX_SUB)
    i = 0
    while i < len(slots):
        l, s = slots[i]
        crow = row0[l] + 1 + s if row_map is None else row_map[row0[l] + 1 + s]
        j = i + 1
        while row_map is not None and j < len(slots) and slots[j][0] == l and row_map[row0[l] + 1 + slots[j][1]] < 0:
            j += 1
        if crow >= 0:
            N = sum(m[i:j])
            W = int(unit if wq is None else wq[crow])
            for k in range(i, j):
                own[k] = share[k] = W // N
            own[i] += W % N
            n_points += N
        i = j
    return m, own, share, n_points, n_capped


def _check(ns, lane_grp, row0, slot_dt, max_step, row_map=None, wq=None, unit=1):
    got = twin.plan_fine_weights(ns, lane_grp, row0, slot_dt, max_step, row_map=row_map, wq=wq, unit=unit)
    ref = _restate(ns, lane_grp, row0, slot_dt, max_step, row_map, wq, unit)
    assert [int(v) for v in got[0]] == ref[0] and [int(v) for v in got[1]] == ref[1] and [int(v) for v in got[2]] == ref[2]
    assert got[3:] == ref[3:]
    return got


def test_all_slots_are_written_arithmetically():
    ns = [8, 0, 1, 6, -1, 3, 2]
    grp = [0, 0, 2, -1, 0, 1, 1]
    want_off, want_step = twin.plan_all_slots(ns, grp)
    slots = _slots(ns, grp)
    assert list(want_off) == [0, 8, 8, 9, 9, 9, 12, 14]                 # lanes without a state row, and group -1, want nothing
    assert list(want_step) == [s for _, s in slots]
    none_off, none_step = twin.plan_all_slots([0, 0], [0, 0])
    assert list(none_off) == [0, 0, 0] and len(none_step) == 0
    e_off, e_step = twin.plan_all_slots([], [])
    assert list(e_off) == [0] and len(e_step) == 0


def test_the_m_rule_is_numpys_ceil_of_the_ieee_quotient():
    rng = np.random.default_rng(3)
    dt = np.r_[rng.uniform(0.01, 9.0, 400), [1.0, 2.0, 0.3 * 3, 0.1 * 7, 64.0, 64.0000001, 100.0, 1e300, 0.0, -1.0, np.nan, np.inf, 5e-324]]
    for max_step in (1.0, 0.3, 0.1, 0.7, np.inf, 1e-300):
        for v in dt:
            with np.errstate(invalid="ignore", over="ignore"):
                c = np.ceil(np.float64(v) / np.float64(max_step))
            want = int(min(MAX_SUB, c)) if c >= 1 else 1
            assert twin.substeps(v, max_step) == want, (v, max_step)
    assert twin.substeps(100.0, 1.0) == 64 and twin.substeps(3.0, np.inf) == 1 and twin.substeps(0.3 * 3, 0.3) == int(np.ceil(0.3 * 3 / 0.3))


def test_the_remainder_rule_and_weights_below_the_point_count():
    ns, grp, row0 = [5, 3], [0, 0], [0, 6]
    slots = _slots(ns, grp)
    dt = np.array([0.5, 1.5, 2.5, 3.5, 9.0, 100.0, 1.0, 9.0])        # the last step of a lane is not read
    wq = np.zeros(10, dtype=np.uint64)
    wq[1:6] = [10, 11, 2, 7, 5]
    wq[7:10] = [1000, 3, 9]
    m, own, share, n_points, n_capped = _check(ns, grp, row0, dt, 1.0, wq=wq)
    assert list(m) == [1, 2, 3, 4, 1, 64, 1, 1] and n_capped == 1 and n_points == 1 + 2 + 3 + 4 + 1 + 64 + 1 + 1
    assert list(own) == [10, 6, 2, 1 + 3, 5, 15 + 40, 3, 9] and list(share[1:4]) == [5, 0, 1] and share[5] == 15
    # W_j < N_j: everything on the row's own point (row 3: 2 quanta, 3 points)
    assert own[2] == 2 and share[2] == 0
    for i in range(len(slots)):
        assert int(own[i]) + int(share[i]) * (int(m[i]) - 1) == int(wq[row0[slots[i][0]] + 1 + slots[i][1]])      # nothing lost
    # every m = 1: own is the weight, as ssde_path_occupancy places it
    m1, own1, _, np1, cap1 = _check(ns, grp, row0, dt, np.inf, wq=wq)
    assert list(m1) == [1] * 8 and list(own1) == [10, 11, 2, 7, 5, 1000, 3, 9] and np1 == 8 and cap1 == 0
    # unit weights
    _, own_u, share_u, _, _ = _check(ns, grp, row0, dt, 1.0, unit=1 << 40)
    assert own_u[5] == (1 << 40) // 64 + (1 << 40) % 64 and share_u[5] == (1 << 40) // 64


def test_lattice_spans_share_a_callers_weight_among_the_padded_rows():
    # one lane of 9 lattice steps (rows 1 .. 9 of the layout); the caller's rows sit at lattice rows 1, 2, 5, 6, 9
    ns, grp, row0 = [9, 2], [0, 0], [0, 10]
    row_map = np.full(13, -1, dtype=np.int64)
    row_map[[0, 1, 2, 5, 6, 9]] = np.arange(6)
    row_map[[10, 11, 12]] = [6, 7, 8]
    wq = np.array([999, 10, 20, 30, 40, 50, 999, 7, 8], dtype=np.uint64)
    dt = np.full(11, 0.5)
    m, own, share, n_points, n_capped = _check(ns, grp, row0, dt, 0.2, row_map=row_map, wq=wq)
    assert list(m) == [3, 3, 3, 3, 3, 3, 3, 3, 1, 3, 1]
    # caller row 2 (lattice row 2) owns lattice rows 2, 3, 4: N = 9 points, 20 quanta: 2 each and 2 more on its own point
    assert list(own[1:4]) == [4, 2, 2] and list(share[1:4]) == [2, 2, 2]
    # caller row 4 (lattice row 6) owns rows 6, 7, 8: 40 = 9 * 4 + 4
    assert list(own[5:8]) == [8, 4, 4] and list(share[5:8]) == [4, 4, 4]
    assert n_points == 3 + 9 + 3 + 9 + 1 + 3 + 1 and n_capped == 0
    tot = sum(int(own[i]) + int(share[i]) * (int(m[i]) - 1) for i in range(11))
    assert tot == 10 + 20 + 30 + 40 + 50 + 7 + 8
    # a padded row before the lane's first caller row belongs to no state row: nothing is placed there
    rm2 = row_map.copy()
    rm2[1] = -1
    m2, own2, share2, np2, _ = _check(ns, grp, row0, dt, 0.2, row_map=rm2, wq=wq)
    assert own2[0] == 0 and share2[0] == 0 and np2 == n_points - 3
    # a lane left out contributes neither points nor capped intervals
    got = _check(ns, [0, -1], row0, np.full(9, 100.0), 0.2, row_map=row_map, wq=wq)
    assert got[4] == 8 and len(got[0]) == 9


def test_random_plans():
    rng = np.random.default_rng(11)
    for trial in range(30):
        nl = int(rng.integers(1, 9))
        ns = rng.integers(-1, 12, nl)
        grp = rng.integers(-1, 3, nl)
        row0 = np.r_[0, np.cumsum(np.maximum(ns, 0) + 1)][:nl]
        n = int(np.sum(np.maximum(ns, 0) + 1))
        n_slots = len(_slots(ns, grp))
        dt = rng.choice([0.25, 0.5, 1.0, 3.0, 70.0], n_slots) * rng.uniform(0.9, 1.1, n_slots)
        row_map = None
        if trial % 2:
            keep = rng.random(n) < 0.6
            keep[row0] = True
            row_map = np.where(keep, np.cumsum(keep) - 1, -1)
        wq = rng.integers(0, 1 << 45, n).astype(np.uint64)
        _check(ns, grp, row0, dt, float(rng.choice([0.3, 1.0, np.inf])), row_map=row_map, wq=wq if trial % 3 else None, unit=12345)


def test_the_batch_rule_counts_the_ends_of_every_slot():
    for n_draws in (1, 5, 32, 1 << 20):
        assert twin.batch_cap(0, 1000, 8, DRAW_CH, n_draws) == 1                                  # one draw always goes
        assert twin.batch_cap(1 << 50, 1000, 8, DRAW_CH, n_draws) == min(n_draws, DRAW_CH << 15)   # one launch's second dimension
        assert twin.batch_cap(8000 * 7 + 5, 1000, 8, DRAW_CH, n_draws) == min(n_draws, 7)          # slots x EZ doubles a draw
    assert twin.batch_cap(1 << 20, 0, 8, DRAW_CH, 9) == 9
