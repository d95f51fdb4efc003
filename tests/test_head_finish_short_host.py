"""CPU suite: the finish of an evaluation whose head came from its Gram statistics (run_once, ssde_reduce_host.hpp:
reduce_host_head through ssde_reduce_host_head).  Nothing was launched, so every record but group 0's is zero: the result is formed
from that record and the by-value lag entry alone, and must equal -- by ==, the check slot included -- what ssde_reduce_host gives on
the full array with its zeros.

Group counts: 1 (every live entry on a thread of its own), 157 (the headline's: the lag entry in the first 1024-block), 1563 (live
entries in later blocks), 256 and 1024 (live entries that share a virtual thread: as terms of one four-term sum, and block after
block).  Windows 1 and 4; accumulators 5 and 6 (d = 1, 2); add[] and map[] as fill_reduce_args sets them: slot 0 and the three
covariance directions for add, a map that leaves a fixed parameter's slot unfed."""
import numpy as np
import pytest

from smoothsde_amd import capi


def _case(rng, W, nacc, lag, with_add, fixed, kind):
    sums0 = rng.standard_normal((W, nacc)) * 10.0 ** rng.integers(-6, 7, size=(W, nacc))
    if kind == "zeros":
        sums0[:] = 0.0
    elif kind == "negative zeros":
        sums0[:] = -0.0
    elif kind == "some zeros":
        sums0[rng.random((W, nacc)) < 0.4] = -0.0
    n_out = 1 + (nacc - 1) + 3                                    # three further parameters nothing feeds
    map_ = np.array(rng.permutation(np.arange(1, n_out))[:nacc - 1], dtype=np.int16)
    if fixed:
        map_[rng.integers(0, nacc - 1)] = -1
    lag_acc = rng.standard_normal(nacc) * 1e3 if lag else None
    if lag and kind == "negative zeros":
        lag_acc[:] = -0.0
    add = rng.standard_normal(4) * 1e2 if with_add else np.zeros(4)
    add_slot = np.array([0, int(map_[0]), int(map_[-2]), int(map_[-1])], dtype=np.int16) if with_add else np.full(4, -1, dtype=np.int16)
    return dict(sums0=sums0, chk0=float(abs(rng.standard_normal()) * 1e-13), n_out=n_out, map_=map_, lag_acc=lag_acc, lag_chk=3e-14,
                add=add, add_slot=add_slot)


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("G", [1, 157, 256, 1024, 1563])
def test_the_short_finish_equals_reduce_host_on_the_array_of_zeros(G, W):
    rng = np.random.default_rng(100 * G + W)
    n = 0
    for nacc in (5, 6):
        for kind in ("random", "some zeros", "zeros", "negative zeros"):
            for lag in (False, True):
                for with_add in (False, True):
                    for fixed in (False, True):
                        c = _case(rng, W, nacc, lag, with_add, fixed, kind)
                        full = np.zeros((G, W, nacc))
                        full[0] = c["sums0"]
                        chk = np.zeros(G)
                        chk[0] = c["chk0"]
                        want = capi.reduce_host(full, chk, c["n_out"], c["map_"], lag_acc=c["lag_acc"], lag_chk=c["lag_chk"],
                                                add=c["add"], add_slot=c["add_slot"])
                        got = capi.reduce_host_head(c["sums0"], c["chk0"], G, c["n_out"], c["map_"], lag_acc=c["lag_acc"],
                                                    lag_chk=c["lag_chk"], add=c["add"], add_slot=c["add_slot"])
                        assert got.shape == want.shape and np.all(got == want), (G, W, nacc, kind, lag, with_add, fixed, got, want)
                        assert got[c["n_out"]] == (max(c["chk0"], c["lag_chk"]) if lag else c["chk0"])
                        n += 1
    assert n == 64


def test_the_check_slot_takes_not_a_number_as_infinity():
    sums0 = np.ones((1, 5))
    map_ = np.array([1, 2, 3, 4], dtype=np.int16)
    for chk0, lag_chk, want in ((np.nan, 1e-14, np.inf), (1e-13, np.nan, np.inf), (2e-13, 7e-13, 7e-13), (0.0, 0.0, 0.0)):
        full = np.zeros((157, 1, 5))
        full[0] = sums0
        chk = np.zeros(157)
        chk[0] = chk0
        a = capi.reduce_host(full, chk, 5, map_, lag_acc=np.zeros(5), lag_chk=lag_chk)
        b = capi.reduce_host_head(sums0, chk0, 157, 5, map_, lag_acc=np.zeros(5), lag_chk=lag_chk)
        assert a[5] == want and b[5] == want and np.all(a == b)


def test_arguments_out_of_range_are_refused():
    map_ = np.array([1, 2, 3, 4], dtype=np.int16)
    with pytest.raises(ValueError):
        capi.reduce_host_head(np.ones((64, 5)), 0.0, 10, 5, map_)                  # more windows than the short form serves
    with pytest.raises(ValueError):
        capi.reduce_host_head(np.ones((1, 5)), 0.0, 0, 5, map_)
    with pytest.raises(ValueError):
        capi.reduce_host_head(np.ones((1, 5)), 0.0, 10, 3, map_)                   # a slot past n_out
