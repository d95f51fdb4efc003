"""CPU suite: the tile plan of ssde_path_proximity (plan_prox_tiles of csrc/ssde_prox.hpp through tests/proxsim_lib.py): pairs of 0, 1,
255, 256, 257 and 600 points in one list."""
import numpy as np
import pytest

import proxsim_lib as twin
from prox_cases import EDGE_SIZES

TILE = 256


def _ptr(sizes):
    return np.r_[0, np.cumsum(sizes)].astype(np.int64)


def test_the_tables_of_the_edge_sizes():
    pp = _ptr(EDGE_SIZES)                                # 0, 0, 1, 256, 512, 769, 1369
    P = twin.plan(pp)
    assert P["n_tiles"] == 0 + 1 + 1 + 1 + 2 + 3 and P["tiles_max"] == 3
    assert P["pair_tile"].tolist() == [0, 0, 1, 2, 3, 5, 8]
    assert P["tile_pair"].tolist() == [1, 2, 3, 4, 4, 5, 5, 5]
    assert P["tile_first"].tolist() == [0, 1, 256, 512, 768, 769, 1025, 1281]
    assert P["tile_idx0"].tolist() == [0, 0, 0, 0, 256, 0, 256, 512]
    assert P["tile_count"].tolist() == [1, 255, 256, 256, 1, 256, 256, 88]


@pytest.mark.parametrize("sizes", [EDGE_SIZES, EDGE_SIZES[::-1], [0, 0, 3, 0], [1], [1024, 0, 1023, 1025], [0, 0, 0, 7]])
def test_no_tile_spans_a_pair_and_the_counts_add_up(sizes):
    pp = _ptr(sizes)
    P = twin.plan(pp)
    want = [-(-s // TILE) for s in sizes]
    assert P["n_tiles"] == sum(want) and P["tiles_max"] == max(want)
    assert np.array_equal(np.diff(P["pair_tile"]), want) and P["pair_tile"][0] == 0
    covered = np.zeros(int(pp[-1]), dtype=np.int64)
    for i in range(P["n_tiles"]):
        p, f, c = int(P["tile_pair"][i]), int(P["tile_first"][i]), int(P["tile_count"][i])
        assert 1 <= c <= TILE and pp[p] <= f and f + c <= pp[p + 1]                       # inside its pair
        assert P["tile_idx0"][i] == f - pp[p]
        assert P["pair_tile"][p] <= i < P["pair_tile"][p + 1]
        if i + 1 < P["pair_tile"][p + 1]:
            assert c == TILE                                                             # only a pair's last tile is partly filled
        covered[f:f + c] += 1
    assert np.all(covered == 1)                                                          # every point in exactly one tile
    assert int(P["tile_count"].sum()) == int(pp[-1])


def test_another_tile_size_and_the_quantum():
    P = twin.plan(_ptr([5, 0, 4]), tile=2)
    assert P["tile_count"].tolist() == [2, 2, 1, 2, 2] and P["pair_tile"].tolist() == [0, 3, 3, 5] and P["tiles_max"] == 3
    from prox_ref import quantum_exp
    for wmax, n in ((1.0, 1), (1.0, 1369), (1e-300, 7), (1e300, 1 << 20), (0.0, 5), (3.7, 255), (4.0, 256)):
        assert twin.quantum_exp(wmax, n) == quantum_exp(wmax, n), (wmax, n)
