"""CPU suite: the numpy statement of ssde_path_stats (tests/path_ref.py) on the draws of tests/draws_ref.py,
against a per-track, per-draw, per-row loop written here from the definition, and the rules the definition implies: NaN for a
track without a state row and for a (track, draw) with a non-finite position, length and displacement 0 for a single state row,
and -- bitwise -- the independence of the draw batching, weight = None as ones, and regions as independent columns.

Limit against the loop: 1e-13 (1 + max|ref|).  Both sides add the same at most 8 terms per statistic, in different orders; each
addition rounds by 1.1e-16 relative, so the two sums differ by ~1e-15 relative at the most."""
import math

import numpy as np
import pytest

from cases import make_spec, problem_from_spec
from draws_ref import draws_ref
from path_cases import clear_of_edges, dt_weights, make_regions
from path_ref import path_ref, position_columns

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS = [9, 1, 2, 7]                           # rows 0-8 | 9 | 10-11 | 12-18
NA_ROWS = (3, 15)
_CASE = {}


def _case(model, d):
    """problem, eight reference draws, regions and weights of a (model, d), computed once"""
    if (model, d) not in _CASE:
        spec = make_spec(f"ph_{model}_{d}", model, d, seed=71 + d, lengths=LENGTHS, na_rows=NA_ROWS)
        pb = problem_from_spec(spec)
        draws = draws_ref(pb, spec["par"], seed=13, n_draws=8)
        draws.setflags(write=False)
        reg = make_regions(spec["obs"], d, 8)
        w = dt_weights(pb.seg_start, pb.times)
        _CASE[(model, d)] = (spec, pb, draws, reg, w)
    return _CASE[(model, d)]


def _brute(draws, seg_start, model, d, regions, weight):
    nd, n, _ = draws.shape
    cols = position_columns(model, d)
    bounds = list(seg_start) + [n]
    out = np.full((nd, len(bounds) - 1, 2 + len(regions)), np.nan)
    for q in range(nd):
        for k in range(len(bounds) - 1):
            first, last = bounds[k], bounds[k + 1] - 1
            if last < first + 1:
                continue
            pos = [[float(draws[q, j, c]) for c in cols] for j in range(first + 1, last + 1)]
            if any(not math.isfinite(v) for p in pos for v in p):
                continue
            length = 0.0
            for a, b in zip(pos[:-1], pos[1:]):
                length += math.sqrt(sum((x - y) ** 2 for x, y in zip(a, b))) if d > 1 else abs(a[0] - b[0])
            net = math.sqrt(sum((x - y) ** 2 for x, y in zip(pos[-1], pos[0]))) if d > 1 else abs(pos[-1][0] - pos[0][0])
            out[q, k, 0], out[q, k, 1] = length, net
            for r, box in enumerate(regions):
                s = 0.0
                for j, p in zip(range(first + 1, last + 1), pos):
                    if all(box[2 * c] <= p[c] < box[2 * c + 1] for c in range(d)):
                        s += weight[j]
                out[q, k, 2 + r] = s
    return out


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_path_ref_is_the_definition(model, d):
    spec, pb, draws, reg, w = _case(model, d)
    assert clear_of_edges(draws, model, d, reg)
    got = path_ref(draws, pb.seg_start, model, d, regions=reg, weight=w)
    ref = _brute(draws, pb.seg_start, model, d, reg, w)
    assert got.shape == (8, 4, 10)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    for k in range(10):
        gap = np.nanmax(np.abs(got[:, :, k] - ref[:, :, k])) / (1.0 + np.nanmax(np.abs(ref[:, :, k])))
        print(f"GAP ref-loop {model} d={d} stat {k}: {gap:.2e}")
        assert gap <= 1e-13, (k, gap)
    inside = got[:, :, 2:][~np.isnan(got[:, :, 2:])]
    assert np.any(inside > 0) and np.any(inside == 0)               # both branches of the indicator


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_nan_rules_and_single_state_rows(model, d):
    spec, pb, draws, reg, w = _case(model, d)
    got = path_ref(draws, pb.seg_start, model, d, regions=reg, weight=w)
    assert np.all(np.isnan(got[:, 1, :]))                           # the one-row track
    assert np.all(got[:, 2, 0] == 0.0) and np.all(got[:, 2, 1] == 0.0)   # two rows: one state row
    assert np.all(np.isfinite(got[:, [0, 2, 3], :]))
    bad = np.array(draws)
    bad[1, 14, position_columns(model, d)[-1]] = np.nan              # one position of (track 3, draw 1)
    hit = path_ref(bad, pb.seg_start, model, d, regions=reg, weight=w)
    assert np.all(np.isnan(hit[1, 3, :]))
    hit[1, 3, :] = got[1, 3, :]
    assert np.array_equal(hit, got, equal_nan=True)                 # ... and nothing else
    inf = np.array(draws)
    inf[2, 5, position_columns(model, d)[0]] = np.inf                # +-inf is not finite either
    assert np.all(np.isnan(path_ref(inf, pb.seg_start, model, d, regions=reg, weight=w)[2, 0, :]))
    if model == "CTCRW":                                             # a velocity column is no position
        vel = np.array(draws)
        vel[:, :, 1] = np.nan
        assert np.array_equal(path_ref(vel, pb.seg_start, model, d, regions=reg, weight=w), got, equal_nan=True)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_batching_weights_and_regions_bitwise(model, d):
    spec, pb, draws, reg, w = _case(model, d)
    whole = path_ref(draws, pb.seg_start, model, d, regions=reg, weight=w)
    a = path_ref(draws_ref(pb, spec["par"], seed=13, draw0=0, n_draws=4), pb.seg_start, model, d, regions=reg, weight=w)
    b = path_ref(draws_ref(pb, spec["par"], seed=13, draw0=4, n_draws=4), pb.seg_start, model, d, regions=reg, weight=w)
    assert np.array_equal(whole, np.concatenate([a, b]), equal_nan=True)          # [0, 8) = [0, 4) + [4, 8)
    none = path_ref(draws, pb.seg_start, model, d, regions=reg, weight=None)
    ones = path_ref(draws, pb.seg_start, model, d, regions=reg, weight=np.ones(pb.n))
    assert np.array_equal(none, ones, equal_nan=True)
    assert not np.array_equal(none, whole, equal_nan=True)
    perm = np.random.default_rng(5).permutation(8)
    mixed = path_ref(draws, pb.seg_start, model, d, regions=reg[perm], weight=w)
    assert np.array_equal(mixed[:, :, :2], whole[:, :, :2], equal_nan=True)
    assert np.array_equal(mixed[:, :, 2:], whole[:, :, 2:][:, :, perm], equal_nan=True)
    assert path_ref(draws, pb.seg_start, model, d).shape == (8, 4, 2)             # no regions
    # a non-finite weight enters the sums it is added to and no other
    wn = w.copy()
    wn[5] = np.nan
    nanw = path_ref(draws, pb.seg_start, model, d, regions=reg, weight=wn)
    assert np.array_equal(nanw[:, 1:], whole[:, 1:], equal_nan=True) and np.array_equal(nanw[:, :, :2], whole[:, :, :2], equal_nan=True)
    p5 = draws[:, 5, position_columns(model, d)]
    for r in range(8):
        inside = np.all((reg[r, 0:2 * d:2] <= p5) & (p5 < reg[r, 1:2 * d:2]), axis=1)
        assert np.array_equal(np.isnan(nanw[:, 0, 2 + r]), inside)
