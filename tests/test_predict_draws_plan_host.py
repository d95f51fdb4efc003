"""CPU suite: the host plan of ssde_predict_draws (csrc/ssde_smooth_plan.hpp: plan_slot_offsets over plan_queries' slot-ordered
queries, and the draws-per-batch rule through batch_cap), against a numpy restatement."""
import numpy as np

import predictdrawsim_lib as twin
import predictsim_lib

DRAW_CH = 4


def _restate(row0, ns, q_row, q_off):
    """slots (lane, step) of every planned query (the rows ARE the caller's), then per slot np.unique of its offsets"""
    row0, ns = np.asarray(row0), np.asarray(ns)
    slots = {}
    for k, (r, o) in enumerate(zip(q_row, q_off)):
        for l in range(len(row0)):
            if ns[l] > 0 and row0[l] < r <= row0[l] + ns[l]:
                slots.setdefault((l, int(r - row0[l] - 1)), []).append((o, k))
    return slots


def _check(row0, ns, q_row, q_off, pad_row=None, pad_step=0.0):
    q_row, q_off = np.asarray(q_row, dtype=np.int64), np.asarray(q_off, dtype=np.float64)
    S = twin.plan_slot_offsets(row0, ns, q_row, q_off, pad_row, pad_step)
    base = predictsim_lib.plan_queries(row0, ns, q_row, q_off, pad_row, pad_step)
    assert np.array_equal(S["order"], base["order"]) and np.array_equal(S["q_slot"], base["q_slot"])      # plan_queries is untouched
    n_slots = len(base["want_step"])
    assert len(S["off_ptr"]) == n_slots + 1 and S["off_ptr"][0] == 0 and S["off_ptr"][-1] == len(S["off_val"])
    assert len(S["q_ptr"]) == len(S["off_val"]) + 1 and S["q_ptr"][0] == 0 and S["q_ptr"][-1] == len(S["order"])
    seen = np.zeros(len(q_row), dtype=int)
    for i in range(n_slots):
        mine = np.flatnonzero(base["q_slot"] == i)
        lst = S["off_val"][S["off_ptr"][i]:S["off_ptr"][i + 1]]
        uniq = np.unique(base["off"][mine])
        assert np.array_equal(lst, uniq) and np.all(np.diff(lst) > 0)                 # distinct, ascending (-0.0 == 0.0: one entry)
        assert np.array_equal(lst[S["q_rank"][mine]], base["off"][mine])              # every query's rank names its own offset
        for r in range(len(lst)):
            g = S["off_ptr"][i] + r
            dest = S["q_dest"][S["q_ptr"][g]:S["q_ptr"][g + 1]]
            assert sorted(dest) == sorted(base["order"][mine][base["off"][mine] == lst[r]])
            seen[dest] += 1
    assert np.all(seen[base["order"]] == 1) and seen.sum() == len(base["order"])      # every planned query is answered exactly once
    assert S["most"] == max(np.diff(S["off_ptr"]), default=0)
    return S, base


def test_ranks_duplicates_and_signed_zeros():
    row0, ns = [0, 10, 11, 13], [8, 0, 1, 6]
    q_row = [3, 3, 3, 3, 3, 5, 5, 12, 0, 10, 3, 5]
    q_off = [0.5, 0.25, 0.5, 0.0, -0.0, 0.1, 0.1, 2.0, 0.3, 0.2, 0.75, 0.0]
    S, base = _check(row0, ns, q_row, q_off)
    slots = _restate(row0, ns, q_row, q_off)
    assert len(slots) == len(base["want_step"]) == 3
    mine = np.flatnonzero(np.asarray(q_row)[base["order"]] == 3)
    assert list(S["q_rank"][mine]) == [2, 1, 2, 0, 0, 3]                               # in the caller's order (the plan's sort is stable)
    assert S["most"] == 4


def test_offsets_one_ulp_apart_are_two_ranks():
    a = 0.3
    b = np.nextafter(a, 1.0)
    S, _ = _check([0], [5], [2, 2, 2, 2], [b, a, b, a])
    assert list(S["off_val"]) == [a, b] and list(S["q_rank"]) == [1, 0, 1, 0]


def test_a_slot_with_257_offsets():
    rng = np.random.default_rng(0)
    offs = rng.permutation(np.r_[np.linspace(0.0, 1.0, 257), np.linspace(0.0, 1.0, 257)[::3]])
    S, _ = _check([0, 20], [10, 10], np.r_[np.full(len(offs), 4), 25], np.r_[offs, 0.5])
    assert S["most"] == 257 and list(np.diff(S["off_ptr"])) == [257, 1]


def test_lattice_residuals_share_slots():
    # a lattice handle: caller rows 0..4 of one track at lattice rows 0, 1, 4, 5, 9 (step 0.5): an offset spanning whole lattice steps
    # moves the slot and leaves a residual; two callers' offsets that land on one lattice step share its slot and rank by residual
    pad_row = np.array([0, 1, 4, 5, 9])
    q_row = [1, 1, 1, 1, 3, 3, 1]
    q_off = [0.2, 0.7, 1.2, 0.7, 1.6, 0.1, 1.5]
    S, base = _check([0], [9], q_row, q_off, pad_row=pad_row, pad_step=0.5)
    assert list(base["want_step"]) == [0, 1, 2, 3, 4, 7]
    assert S["most"] == 1 and len(S["off_val"]) == 6                                   # (1, 0.7) twice: one answer
    np.testing.assert_allclose(S["off_val"], [0.2, 0.2, 0.2, 0.0, 0.1, 0.1], atol=1e-12)


def test_groups_without_queries():
    row0 = np.arange(200) * 6
    ns = np.full(200, 5)
    q_row = [row0[3] + 2, row0[3] + 2, row0[150] + 5, row0[150] + 5]
    S, base = _check(row0, ns, q_row, [0.1, 0.2, 1.0, 3.0])
    assert list(np.diff(base["want_off"]).nonzero()[0]) == [3, 150] and S["most"] == 2
    none = twin.plan_slot_offsets(row0, ns, [row0[7]], [0.5])                          # a first row: nothing planned
    assert len(none["off_val"]) == 0 and list(none["q_ptr"]) == [0] and none["most"] == 0


def test_the_batch_rule_always_gives_a_draw_and_batches_cover_every_draw_once():
    for budget in (0, 1, 100, 10 ** 4, 10 ** 9, 2 ** 62):
        for n_slots, sd, nq in ((1, 1, 1), (100, 4, 257), (10 ** 5, 2, 10 ** 5), (10 ** 7, 4, 10 ** 8)):
            for n_draws in (1, 4, 5, 32, 1000, 131072, 131073, (1 << 28) - 1):
                cap = twin.batch_cap(budget, n_slots, sd, nq, DRAW_CH, n_draws)
                per = n_slots * 2 * sd + nq * sd
                assert 1 <= cap <= n_draws and cap <= DRAW_CH << 15
                assert cap == predictsim_lib.batch_cap(budget, per, 1, DRAW_CH, n_draws)
                assert cap == 1 or cap * per <= budget or cap == n_draws and cap * per <= max(budget, per)
                starts = list(range(0, n_draws, cap)) if n_draws // cap < 10 ** 4 else None
                if starts is not None:
                    covered = sum(min(cap, n_draws - k0) for k0 in starts)
                    assert covered == n_draws
