"""CPU suite: the item plan and the retry rule of the Hessian pass of the lane = direction path (csrc/ssde_windows.hpp:
hess_first_warmup, hess_item_plan, hess_next_warmup -- what ssde_hess.hip's hess_tv_device launches k_tv_hess.hip with), compiled
for the host by tests/hostsim.  The windows are window_bounds(L, nc, W, 0, c) of ssde_device.hpp, mirrored in
test_head_plan_host.py as the kernels deal them."""
import os
import re

import numpy as np
import pytest

import hostsim_lib
from test_head_plan_host import window_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "smoothsde_amd", "csrc", "ssde_device.hpp")) as _f:
    WIN_ALIGN = int(re.search(r"constexpr int WIN_ALIGN = (\d+);", _f.read()).group(1))
WARMUPS = (48, 80, 144)


def _lengths(W):
    return [0, 1, 2, 15, 16, 17, 31, 32, 33, 2 * W - 1, 2 * W, 2 * W + 1, 640, 3000]


@pytest.mark.parametrize("waves", [1, 64, 2048])
@pytest.mark.parametrize("n_pb", [1, 2])
@pytest.mark.parametrize("W", WARMUPS)
def test_every_step_is_scored_once_and_the_items_are_in_hand_over_order(W, n_pb, waves):
    L = _lengths(W)
    items = hostsim_lib.hess_item_plan(L, n_pb, W, waves, WIN_ALIGN)
    # (track, pair block, window) order, every (track, pair block) with all its windows: an item's successor in the list is the next
    # window of the same (track, pair block) -- what hess_finish_kernel reads at item + 1
    expect = []
    for t, ns in enumerate(L):
        nc = {int(it[2]) for it in items if it[0] == t}
        assert len(nc) == 1
        nc = nc.pop()
        assert nc >= 1 and (nc == 1 or ns >= 2 * W)                 # only tracks of two warm-ups are cut
        expect += [(t, c, nc, b) for b in range(n_pb) for c in range(nc)]
    assert [tuple(int(v) for v in it) for it in items] == expect
    for k, (t, c, nc, b) in enumerate(expect):
        if c + 1 < nc:
            assert expect[k + 1] == (t, c + 1, nc, b)
    # the budget: no more windows per track than keep `waves` waves busy (at least one)
    cap = max(1, -(-waves // (len(L) * n_pb)))
    assert max(e[2] for e in expect) <= cap
    if waves == 2048:
        assert max(e[2] for e in expect) > 1
    for t, ns in enumerate(L):
        nc = next(e[2] for e in expect if e[0] == t)
        scored = np.zeros(ns, dtype=int)
        prev_end = 0
        for c in range(nc):
            s_begin, s_acc, s_end = window_bounds(ns, nc, W, 0, c, -1)
            assert 0 <= s_begin <= s_acc <= s_end <= ns             # the warm-up stays inside the track
            assert s_acc == prev_end                                # windows are neighbours
            assert s_acc - s_begin == (min(W, s_acc) if nc > 1 else 0)
            if nc > 1:
                assert s_end > s_acc, (ns, nc, c)                   # no window of several is empty
                assert s_acc % WIN_ALIGN == 0
            scored[s_acc:s_end] += 1
            prev_end = s_end
        assert prev_end == ns and np.all(scored == 1)


def test_one_window_plans_and_the_wave_budget():
    L = [640, 3000]
    assert [tuple(it) for it in hostsim_lib.hess_item_plan(L, 1, 0, 2048, WIN_ALIGN)] == [(0, 0, 1, 0), (1, 0, 1, 0)]      # W = 0: sequential
    assert [tuple(it) for it in hostsim_lib.hess_item_plan(L, 1, 400, 2048, WIN_ALIGN)] == [(0, 0, 1, 0)] + [(1, c, 94, 0) for c in range(94)]
    # each window at least two alignment units of scored rows: ceil(3000 / 32) = 94, ceil(640 / 32) = 20
    nc = {int(it[0]): int(it[2]) for it in hostsim_lib.hess_item_plan(L, 1, 48, 2048, WIN_ALIGN)}
    assert nc == {0: 20, 1: 94}
    nc = {int(it[0]): int(it[2]) for it in hostsim_lib.hess_item_plan(L, 2, 48, 40, WIN_ALIGN)}
    assert nc == {0: 10, 1: 10}                                      # 40 waves over 2 tracks x 2 pair blocks


def test_the_first_warm_up():
    assert hostsim_lib.hess_first_warmup(32, None, WIN_ALIGN) == 2 * 32 + WIN_ALIGN
    assert hostsim_lib.hess_first_warmup(64, None, WIN_ALIGN) == 2 * 64 + WIN_ALIGN
    assert hostsim_lib.hess_first_warmup(32, 16, WIN_ALIGN) == 16                 # SSDE_HESS_WINDOW replaces it
    assert hostsim_lib.hess_first_warmup(0, None, WIN_ALIGN) == 0                 # the evaluation has no warm-up: sequential
    assert hostsim_lib.hess_first_warmup(0, 16, WIN_ALIGN) == 16                  # ... also where the evaluation runs one window


@pytest.mark.parametrize("glen_max", [0, 95, 96, 640, 3000, 10 ** 6])
@pytest.mark.parametrize("W0", [16] + list(WARMUPS))
def test_the_retry_sequence_quadruples_and_ends_in_one_sequential_window(W0, glen_max):
    seq, W = [W0], W0
    for attempt in range(10):
        W = hostsim_lib.hess_next_warmup(W, attempt, glen_max)
        seq.append(W)
        if W == 0:
            break
    assert seq[-1] == 0 and len(seq) - 1 <= 4                       # at most four widenings, the last one to 0
    for a, b in zip(seq, seq[1:-1]):
        assert b == 4 * a and 2 * b <= glen_max                     # a warm-up that a track holds twice, or none
    if len(seq) - 1 < 4:
        assert 2 * 4 * seq[-2] > glen_max
    else:
        assert seq[:4] == [W0, 4 * W0, 16 * W0, 64 * W0]
