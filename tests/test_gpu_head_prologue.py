"""GPU suite: the lag-path head's own prologue (k_iso_shared_cut.hip).  The direction-part entry takes a hot
argument block instead of IsoArgs and issues ONE round of loads before its first row -- the group's length and ns_min from an array
built at create, the lane's nsteps and a0, the first two row blocks (at an offset computed from the block for the leading groups of
one length, loaded for the others) and the first gain slab.  No floating-point operation changes, so every comparison here is
BITWISE: the default form (the parts, finished on the host) against the single wave per group of iso_shared_kernel on the same
window (SSDE_FUSED_FINALIZE=0), the synchronous call against ssde_eval_device through the finalize launch, a handle with a history
against fresh ones.

Every case is CTCRW with two response coordinates, the path forced on small batches with SSDE_LAGSTATS=2 and the early cuts built by
set_option(OPT_LAG_EARLY, 1).  Batches: 1, 64, 65 and 130 tracks of 2000 rows (padding workgroups; a last group with empty lanes,
which ns_min must not count), 100 tracks whose lengths cycle through (40, 63, 64, 65, 256, 257, 300, 2000): two groups of
different lengths -- the second one's offset is still the first one's size --, tracks shorter than the cut, so ns_min < the cut and
the predicated rows run; and 200 tracks over the same lengths: FOUR groups of four different lengths (25 tracks of each length,
sorted longest first, 64 to a group: the groups' longest tracks have 2000, 257, 64 and 40 rows), so only the
first two are leading groups and the last two load group_off[g] before their first rows -- the branch of run_lane_cut that every
batch with three or more group lengths takes.  Direction masks through par_fixed: 15 (everything free), 13 (log sigma_obs, log
tau, log nu: the benchmark's), 1 (log sigma_obs alone) and 0 (nothing free: one part, the value chain alone), and an order-0 call.  The masks are [bit 0 sigma_obs | bit 1 mu | bit 2 par d | bit 3 par d + 1] (ssde_device.hpp: DIR_*)."""
import subprocess

import numpy as np
import pytest

from smoothsde_amd import capi
from test_gain_feed_host import build_gainfeed

pytestmark = pytest.mark.gpu
T = 2000
D = 2
HEAD_GAIN_ROWS = 17
RAGGED = (40, 63, 64, 65, 256, 257, 300, 2000)
SHAPES = [dict(M=1), dict(M=64), dict(M=65), dict(M=130), dict(M=100, ragged=True), dict(M=200, ragged=True)]
N_GROUPS = {1: 1, 64: 1, 65: 2, 130: 3, 100: 2, 200: 4}
# par = [log sigma_obs, mu_1, mu_2, log tau, log nu]; 1 = fixed
MASKS = {15: (0, 0, 0, 0, 0), 13: (0, 1, 1, 0, 0), 1: (0, 1, 1, 1, 1), 0: (1, 1, 1, 1, 1)}
LOG_TAU, LOG_NU = float(np.log(2.0)), 0.0


def _data(M, ragged=False):
    import torch
    lengths = np.resize(np.array(RAGGED, dtype=np.int64), M) if ragged else None
    return capi.simulate_device("CTCRW", M, T, D, mu=0.0, tau=2.0, nu=1.0, kappa=1.0, sigma=1.0, sigma_obs=0.1, seed=171 + M,
                                track0=0, lengths=lengths, device=torch.device("cuda:0"))


@pytest.fixture(scope="module")
def batches():
    """the five batches, simulated once"""
    cache = {}

    def get(M, ragged=False):
        if (M, ragged) not in cache:
            cache[(M, ragged)] = _data(M, ragged)
        return cache[(M, ragged)]
    return get


def _engine(data, mask, monkeypatch, fused=None):
    ID, times, obs = data
    with monkeypatch.context() as m:
        for name in ("SSDE_CHUNKS", "SSDE_FUSED_FINALIZE", "SSDE_WINDOW", "SSDE_PUBLISH", "SSDE_WAVE_CLOCK"):
            m.delenv(name, raising=False)
        m.setenv("SSDE_LAGSTATS", "2")
        if fused is not None:
            m.setenv("SSDE_FUSED_FINALIZE", str(fused))
        eng = capi.Engine(capi.Problem.from_torch("CTCRW", ID, times, obs, par_fixed=np.array(MASKS[mask], dtype=np.uint8)))
    eng.set_option(capi.OPT_KERNEL_STAMPS, 0)
    eng.set_option(capi.OPT_LAG_EARLY, 1)
    return eng


def _theta(k, log_sigma_obs=np.log(0.1)):
    th = np.zeros(3 + D)
    th[0], th[1 + D], th[2 + D] = log_sigma_obs, LOG_TAU, LOG_NU
    return th + 0.01 * np.sin(np.arange(th.size) + 0.7 * k)


def _run(eng, th, order=1):
    if order == 0:
        return eng.eval(th, order=0), None, eng.info()["window_check"]
    v, g = eng.eval(th)
    return v, g, eng.info()["window_check"]


def _same(a, b):
    return a[0] == b[0] and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])) and a[2] == b[2]


def _is_parts(eng, mask):
    inf = eng.info()
    g8 = (inf["n_groups"] + 7) // 8 * 8
    parts = max(1, bin(mask & 0b1101).count("1"))                      # one part per covariance direction; mu rides along
    return (eng.last_lag_cut() in capi.LAG_CUTS and eng.last_finish_form() == 2 and inf["n_kernel_blocks"] == g8
            and inf["lanes_per_track"] == parts and inf["window_retries"] == 0)


def _shape_id(s):
    return "M%d%s" % (s["M"], "_ragged" if s.get("ragged") else "")


@pytest.mark.parametrize("mask", [15, 13, 1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_the_parts_are_the_single_wave_and_the_finalize_launch_bitwise(shape, mask, batches, monkeypatch):
    import torch
    data = batches(**shape)
    eng, ref = _engine(data, mask, monkeypatch), _engine(data, mask, monkeypatch, fused=0)
    try:
        n = eng.n_par_full
        for k in range(2):
            th = _theta(k)
            got, want = _run(eng, th), _run(ref, th)
            assert _is_parts(eng, mask), (eng.last_lag_cut(), eng.last_finish_form(), eng.info())
            assert eng.info()["n_groups"] == N_GROUPS[shape["M"]]           # (M200: past the leading groups, the loaded offset)
            assert ref.last_lag_cut() == eng.last_lag_cut() and ref.last_finish_form() == 0 and ref.info()["lanes_per_track"] == 1
            assert eng.last_gain_feed() == 1 and 0 < eng.last_gain_rows() <= HEAD_GAIN_ROWS        # (the by-value slab, fetched with the first round)
            assert np.isfinite(got[0]) and got[2] == 0.0
            assert _same(got, want), (k, got, want)
            free = np.array(MASKS[mask]) == 0
            assert np.all(got[1][~free] == 0.0) and np.all(got[1][free] != 0.0)
            # an order-0 call (the engine may let the gradient ride along: what is pinned is the value's bits and the way out)
            g0, w0 = _run(eng, th, order=0), _run(ref, th, order=0)
            assert eng.last_finish_form() == 2 and eng.last_lag_cut() == ref.last_lag_cut()
            assert _same(g0, w0) and g0[0] == got[0], (g0, w0, got[0])
            # the other way out of the same kernel: partials and a finalize launch
            out = torch.zeros(2 + n, dtype=torch.float64, device="cuda:0")
            s = torch.cuda.Stream()
            eng.eval_device(th, out.data_ptr(), order=1, stream=s.cuda_stream)
            s.synchronize()
            assert eng.last_finish_form() == 0 and eng.last_lag_cut() == ref.last_lag_cut()
            r = out.cpu().numpy()
            assert _same((r[0], r[1:-1], r[-1]), got), (k, r, got)
    finally:
        eng.close(); ref.close()


@pytest.fixture(scope="module")
def long_table_theta(tmp_path_factory):
    """a log sigma_obs whose CTCRW gain table (tau = 2, nu = 1, dt = 1, the default P0) is a few rows longer than the by-value capacity:
    found on the host (tests/gainfeed/gainfeed_host.cpp, the engine's own stationarity test)"""
    exe = build_gainfeed(tmp_path_factory.mktemp("gainfeed"))
    r = subprocess.run([exe, "rows", str(D), "1.0", repr(LOG_TAU), repr(LOG_NU), "341", "-2.4", "-0.7", "1", "0", "10"],
                       capture_output=True, text=True, check=True)
    for line in r.stdout.strip().splitlines():
        a, b = line.split()
        if HEAD_GAIN_ROWS + 1 <= int(b) <= HEAD_GAIN_ROWS + 6:
            th = np.zeros(3 + D)
            th[0], th[1 + D], th[2 + D] = float(a), LOG_TAU, LOG_NU
            return th, int(b)
    pytest.fail("no log sigma_obs on the grid gives a table of 18 .. 23 rows")


@pytest.mark.parametrize("shape", [dict(M=65), dict(M=100, ragged=True), dict(M=200, ragged=True)], ids=_shape_id)
def test_a_table_longer_than_the_block_is_staged_from_its_copy(shape, batches, long_table_theta, monkeypatch):
    th, rows = long_table_theta
    data = batches(**shape)
    eng, ref = _engine(data, 13, monkeypatch), _engine(data, 13, monkeypatch, fused=0)
    try:
        got, want = _run(eng, th), _run(ref, th)
        assert eng.last_gain_rows() == rows == ref.last_gain_rows() and rows > HEAD_GAIN_ROWS
        assert eng.last_gain_feed() == 0 and _is_parts(eng, 13), (eng.last_lag_cut(), eng.info())
        assert _same(got, want), (got, want)
    finally:
        eng.close(); ref.close()


def test_fifty_evaluations_alternating_between_two_cuts_equal_fresh_handles(batches, monkeypatch):
    data = batches(200, True)                                         # (both offset paths: two leading groups, two loaded)
    eng = _engine(data, 13, monkeypatch)
    others = []
    try:
        scratch = _engine(data, 13, monkeypatch)
        others.append(scratch)
        by_cut = {}
        for ls in np.linspace(np.log(0.05), np.log(1.0), 16):
            th = _theta(2, log_sigma_obs=ls)
            scratch.eval(th)
            if scratch.last_lag_cut() in capi.LAG_CUTS and scratch.last_finish_form() == 2:
                by_cut.setdefault(scratch.last_lag_cut(), th)
        assert len(by_cut) >= 2, by_cut
        cuts = sorted(by_cut)[:2]
        thetas = [by_cut[c] for c in cuts]
        want = []
        for th in thetas:
            e = _engine(data, 13, monkeypatch)
            others.append(e)
            want.append(_run(e, th))
        assert not _same(want[0], want[1])
        for i in range(50):
            got = _run(eng, thetas[i & 1])
            assert eng.last_lag_cut() == cuts[i & 1] and eng.last_finish_form() == 2
            assert _same(got, want[i & 1]), (i, got, want[i & 1])
        assert eng.info()["window_retries"] == 0
    finally:
        for e in [eng] + others:
            e.close()
