"""CPU suite: the head of the lag-statistics path finished on the host.

1. ssde_reduce_host (smoothsde_amd/csrc/ssde_reduce_host.hpp) against a numpy mirror of reduce_slot's order (ssde_device.hpp), bitwise:
   entries i = c G + g with the by-value lag entry after the last one, 256 virtual threads with stride 1024 and the
   (v0 + v1) + (v2 + v3) grouping, the 128 .. 1 tree, then add[] and map[]; the check slot is the largest of the groups' checks and
   the forms' check as bit patterns, not-a-number counting as infinity.
2. The plan (ssde_windows.hpp: head_latency_plan, through hostsim_lib.window_geometry): the bench's head gets exactly one workgroup's
   worth of windows with the transient window on a wave of its own; more groups than wave slots and a forced window count keep what
   they had."""
import numpy as np
import pytest

from hostsim_lib import window_geometry
from smoothsde_amd import capi
from test_head_plan_host import BENCH, CONSTS, LAG_A, T0_COST, _align, _bench_par, _const, _parent_head, wave_rows

WG_WAVES = _const("ssde_device.hpp", r"constexpr int WG_WAVES = (\d+);")


def reduce_slot_mirror(sums, chk, n_out, map_, lag_acc, lag_chk, add, add_slot):
    """reduce_slot, one output slot after the other, as its 256 threads form it"""
    G, W, nacc = sums.shape
    out = np.zeros(n_out + 1)
    for slot in range(n_out):
        acc = np.zeros(256)
        for k in ([0] if slot == 0 else [k for k in range(1, nacc) if map_[k - 1] == slot]):
            flat = [float(sums[g, c, k]) for c in range(W) for g in range(G)]           # entry i = c G + g
            if lag_acc is not None:
                flat.append(float(lag_acc[k]))
            n = len(flat)
            for tid in range(256):
                a = float(acc[tid])
                for i0 in range(tid, n, 1024):
                    v = [flat[i0 + 256 * u] if i0 + 256 * u < n else 0.0 for u in range(4)]
                    a += (v[0] + v[1]) + (v[2] + v[3])
                acc[tid] = a
        o = 128
        while o > 0:
            acc[:o] = acc[:o] + acc[o:2 * o]
            o >>= 1
        r = float(acc[0])
        for i in range(4):
            if add_slot[i] == slot:
                r += float(add[i])
        out[slot] = r
    vals = [np.inf if np.isnan(v) else abs(float(v)) for v in chk]
    if lag_acc is not None:
        vals.append(np.inf if np.isnan(lag_chk) else abs(float(lag_chk)))
    out[n_out] = np.array(vals, dtype=np.float64).view(np.uint64).max().view(np.float64) if vals else 0.0
    return out


def _case(rng, G, nacc, lag, with_add, fixed):
    """sums of mixed sign over twelve decades (so that the order of the additions shows in the last bits), a map that leaves the
    slots of fixed parameters unfed"""
    sums = rng.standard_normal((G, WG_WAVES, nacc)) * 10.0 ** rng.integers(-6, 7, size=(G, WG_WAVES, nacc))
    n_out = 1 + (nacc - 1) + 3                                    # three further parameters nothing feeds
    slots = rng.permutation(np.arange(1, n_out))[:nacc - 1]
    map_ = np.array(slots, dtype=np.int16)
    if fixed:
        map_[rng.integers(0, nacc - 1)] = -1
    lag_acc = rng.standard_normal(nacc) * 1e3 if lag else None
    add = rng.standard_normal(4) * 1e2 if with_add else np.zeros(4)
    add_slot = np.array([0, int(map_[0]), -1, int(map_[-1])], dtype=np.int16) if with_add else np.full(4, -1, dtype=np.int16)
    chk = np.abs(rng.standard_normal(G)) * 1e-13
    return dict(sums=sums, chk=chk, n_out=n_out, map_=map_, lag_acc=lag_acc, lag_chk=3e-14, add=add, add_slot=add_slot)


@pytest.mark.parametrize("nacc", [5, 6])
@pytest.mark.parametrize("G", [1, 4, 157, 300])
def test_reduce_host_is_reduce_slot_bitwise(G, nacc):
    """G x 4 windows: entry counts below 256 (1, 4 groups), between 256 and 1024 (157) and above 1024 (300)"""
    rng = np.random.default_rng(1000 * G + nacc)
    for lag in (False, True):
        for with_add in (False, True):
            for fixed in (False, True):
                c = _case(rng, G, nacc, lag, with_add, fixed)
                got = capi.reduce_host(c["sums"], c["chk"], c["n_out"], c["map_"], lag_acc=c["lag_acc"], lag_chk=c["lag_chk"],
                                       add=c["add"], add_slot=c["add_slot"])
                want = reduce_slot_mirror(**c)
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (G, nacc, lag, with_add, fixed, got, want)
                unfed = [s for s in range(1, c["n_out"]) if s not in c["map_"] and s not in c["add_slot"]]
                assert unfed and all(got[s] == 0.0 for s in unfed)
                assert any(got[s] != 0.0 for s in range(c["n_out"]))


def test_the_sums_depend_on_the_order():
    """the mirror is a check of the ORDER: the same entries summed group-major differ in the last bits"""
    rng = np.random.default_rng(7)
    c = _case(rng, 157, 6, True, False, False)
    got = capi.reduce_host(c["sums"], c["chk"], c["n_out"], c["map_"], lag_acc=c["lag_acc"], lag_chk=c["lag_chk"])
    naive = float(np.sum(c["sums"][:, :, 0].reshape(-1))) + float(c["lag_acc"][0])
    assert got[0] != naive and abs(got[0] - naive) <= 1e-9 * np.sum(np.abs(c["sums"][:, :, 0]))


def test_the_check_slot():
    sums = np.zeros((5, WG_WAVES, 5))
    map_ = np.array([1, 2, 3, 4], dtype=np.int16)
    chk = np.array([0.0, 2e-13, 1e-13, 0.0, 5e-14])
    assert capi.reduce_host(sums, chk, 5, map_)[5] == 2e-13
    assert capi.reduce_host(sums, chk, 5, map_, lag_acc=np.zeros(5), lag_chk=7e-13)[5] == 7e-13
    assert capi.reduce_host(sums, chk, 5, map_, lag_acc=np.zeros(5), lag_chk=1e-14)[5] == 2e-13
    assert capi.reduce_host(sums, chk, 5, map_, lag_chk=7e-13)[5] == 2e-13                      # no lag entry: its check is not read
    assert capi.reduce_host(sums, np.zeros(5), 5, map_)[5] == 0.0
    chk[3] = np.nan
    assert capi.reduce_host(sums, chk, 5, map_)[5] == np.inf
    assert capi.reduce_host(sums, np.zeros(5), 5, map_, lag_acc=np.zeros(5), lag_chk=np.nan)[5] == np.inf
    # the order of non-negative doubles is the order of their bit patterns: denormals and huge values included
    chk = np.array([5e-324, 1e-300, 0.0, 1e300, 1.0])
    assert capi.reduce_host(sums, chk, 5, map_)[5] == 1e300
    assert capi.reduce_host(sums, chk[:2].repeat(3)[:5], 5, map_)[5] == 1e-300
    with pytest.raises(ValueError):
        capi.reduce_host(sums, chk, 3, map_)                                                    # a slot past n_out


def test_the_bench_head_is_one_workgroup_of_windows():
    for k in (-6, 0, 7, 50, 99):
        par = _bench_par(k)
        for gain_last in range(20, 33):
            g = window_geometry(CONSTS, par, ev=dict(gain_last=gain_last), **BENCH)
            assert g["lag_K"] > 0 and g["t0"] > 0 and g["t0_delta"] == 0 and g["n_chunks"] == WG_WAVES, (k, gain_last, g)
            rows = wave_rows(g)
            assert len(rows) == WG_WAVES and rows[0] == g["t0"] and min(rows) > 0
            assert max(rows) < max(wave_rows(_parent_head(g)))


def test_more_groups_than_wave_slots_and_a_forced_count_keep_what_they_had():
    par = _bench_par(0)
    c4 = dict(BENCH, n_groups=1563, max_chunks=2, want_chunks=1)
    for gain_last in (12, 20, 32):
        g = window_geometry(CONSTS, par, ev=dict(gain_last=gain_last), **c4)
        W = g["plan"]["warmup"]
        assert g["lag_K"] == W > 0 and g["n_chunks"] == 2 and g["t0"] == _align(g["s_stat"] + W)
        assert g["t0_delta"] == _align(int(T0_COST * g["t0"])) > 0 and wave_rows(g) == [LAG_A + W]
        forced = window_geometry(CONSTS, par, ev=dict(gain_last=gain_last), **dict(BENCH, chunks_forced=1))
        parent = _parent_head(forced)
        assert {k_: forced[k_] for k_ in parent} == parent, (forced, parent)
