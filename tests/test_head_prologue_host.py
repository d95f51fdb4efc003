"""Host tests of what create and the launch prepare for the lag-path head's own prologue (k_iso_shared_cut.hip):
the per-group ns_min array that replaces the lanes' six shuffles (head_ns_min), the leading groups whose offset the wave computes
instead of loading it (head_lead_groups), and the hot argument block filled from the IsoArgs of the launch (head_args_fill), field
by field.  The three are plain host functions of ssde_device.hpp; tests/hostsim/hostsim_headargs.cpp builds them without a device."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_ip = C.POINTER(C.c_int32)
_lib = None
WAVE = 64
TILE_U = 4
INT32_MAX = 2 ** 31 - 1
RAGGED = (40, 63, 64, 65, 256, 257, 300, 2000)       # tests/test_gpu_head_cut.py's ragged batch: 100 tracks of these lengths
LAG_CUTS = tuple(range(32, 129, 16))


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(os.path.join(_DIR, "libhostsim_headargs.so")):
            subprocess.run(["make", "-s", "-C", _DIR, "-f", "headargs.mk"], check=True)
        lib = C.CDLL(os.path.join(_DIR, "libhostsim_headargs.so"))
        lib.hostsim_head_ns_min.argtypes = [_ip, C.c_int, _ip]
        lib.hostsim_head_ns_min.restype = None
        lib.hostsim_head_lead_groups.argtypes = [_ip, C.c_int]
        lib.hostsim_head_args_check.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int]
        lib.hostsim_head_args_check.restype = C.c_ulonglong
        _lib = lib
    return _lib


def _groups(lengths):
    """the engine's grouping: tracks sorted by length (longest first), 64 to a group; lane_nsteps = rows - 1, 0 = no track"""
    steps = np.sort(np.asarray(lengths, dtype=np.int32) - 1)[::-1]
    G = (len(steps) + WAVE - 1) // WAVE
    ns = np.zeros(G * WAVE, dtype=np.int32)
    ns[:len(steps)] = steps
    glen = (ns.reshape(G, WAVE).max(axis=1) + TILE_U - 1) // TILE_U * TILE_U
    return ns, glen.astype(np.int32)


def _ns_min(ns):
    ns = np.ascontiguousarray(ns, dtype=np.int32)
    G = ns.size // WAVE
    out = np.empty(G, dtype=np.int32)
    _load().hostsim_head_ns_min(ns.ctypes.data_as(_ip), G, out.ctypes.data_as(_ip))
    return out


def test_ns_min_of_the_ragged_batch_is_the_min_over_the_lanes_with_a_track():
    ns, _ = _groups(np.resize(np.array(RAGGED), 100))
    assert ns.size == 2 * WAVE and np.count_nonzero(ns) == 100
    for cut in LAG_CUTS + (256,):
        capped = np.minimum(ns, cut)                                # lag_cut_ns: lane_nsteps capped at the cut
        want = np.array([row[row > 0].min() if (row > 0).any() else INT32_MAX for row in capped.reshape(-1, WAVE)], dtype=np.int32)
        got = _ns_min(capped)
        assert np.array_equal(got, want), (cut, got, want)
        # group 0 holds the long tracks (capped: the cut itself); group 1 ends with 28 empty lanes, which do not count
        assert got[0] == min(cut, ns[:WAVE].min()) and got[1] == min(cut, 39), (cut, got)


def test_ns_min_edges():
    ns = np.zeros(3 * WAVE, dtype=np.int32)
    ns[5] = 17                                                      # one track in group 0, none in group 1, a full group 2
    ns[2 * WAVE:] = np.arange(100, 100 + WAVE)
    assert _ns_min(ns).tolist() == [17, INT32_MAX, 100]


def test_lead_groups_are_those_whose_offset_is_a_multiple_of_the_first_groups_size():
    lib = _load()
    rng = np.random.default_rng(3)
    cases = [np.full(130, 2000), np.resize(np.array(RAGGED), 100), np.full(1, 2000), np.r_[np.full(64 * 5, 900), rng.integers(40, 900, 200)],
             rng.integers(40, 2000, 300)]
    for lengths in cases:
        ns, glen = _groups(lengths)
        G = glen.size
        n = lib.hostsim_head_lead_groups(glen.ctypes.data_as(_ip), G)
        off = np.r_[0, np.cumsum(glen.astype(np.int64))][:G]        # group_off in rows (the engine's, over C * 64 doubles per row)
        assert 1 <= n <= G
        assert np.array_equal(off[:n], np.arange(n, dtype=np.int64) * glen[0]), (n, off[:n + 1], glen[:n + 1])
        if n < G:                                                   # ... and it is the longest such prefix
            assert off[n] != n * int(glen[0]), (n, off[:n + 2])
    # tests/test_gpu_head_prologue.py's four-group batch: two leading groups, two whose offset the wave loads
    ns, glen = _groups(np.resize(np.array(RAGGED), 200))
    assert glen.tolist() == [2000, 256, 64, 40] and lib.hostsim_head_lead_groups(glen.ctypes.data_as(_ip), 4) == 2


def test_the_hot_block_is_the_iso_args_field_by_field():
    lib = _load()
    assert lib.hostsim_head_args_bytes() <= 9 * 64 and lib.hostsim_head_args_bytes() % 8 == 0
    assert lib.hostsim_iso_args_bytes() + 8 + 17 * 13 * 8 <= 4096     # (IsoArgs keeps its size: the wg entry's by-value table keeps its 17 rows)
    assert lib.hostsim_head_statc() >= 25                             # CTCRW's stationary constants: statc[0 .. 25)
    for gain_rows, lead_n, stride, with_ns in ((0, 0, 0, 1), (17, 157, 10000 * 2 * 64, 1), (3, 2, 40 * 2 * 64, 1), (5, 9, 1234, 0)):
        bad = lib.hostsim_head_args_check(gain_rows, lead_n, stride, with_ns)
        assert bad == 0, "fields (bits, in the struct's order) that did not arrive: %s" % bin(bad)
