"""GPU suite: how the head of the lag-statistics path gets its gain table and its groups' numbers (k_iso_shared.inc:
iso_shared_wg_kernel, ssde_gain_feed.hpp).

A table of at most HEAD_GAIN_ROWS rows rides BY VALUE in the launch's argument block (ssde_last_gain_feed 1: no copy, no ring slot, no
event), a longer one goes through the pinned ring and a copy as before (0).  That may not change a bit: the form that still copies --
SSDE_FUSED_FINALIZE=0, iso_shared_kernel -- is the reference, bitwise, for value, gradient and hand-over check.

The parameters are chosen on the CPU by the length of the table they give: tests/gainfeed/gainfeed_host.cpp runs the covariance
recursion (host code, the engine's own header) over a grid of log sigma_obs and the tests pick the first grid point with the wanted
row count -- fewer than the capacity, exactly the capacity, one more, many more.

Shapes of tests/test_gpu_head_finish.py: 320 rows, 64 tracks (one full group) and 130 (two full groups and a last group of two
tracks); the path forced with SSDE_LAGSTATS=2, plain launches."""
import os
import subprocess

import numpy as np
import pytest

from smoothsde_amd import capi
from test_gain_feed_host import build_gainfeed

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 8)
T = 320
HEAD_GAIN_ROWS = 17          # (4096 - sizeof(IsoArgs) - 8) / (13 * 8): asserted through the feed the engine reports at 17 and at 18 rows
PAR_RING = 8
LOG_TAU, LOG_NU = float(np.log(2.0)), 0.0
SIM = dict(CTCRW=dict(mu=0.0, tau=2.0, nu=1.0, sigma_obs=0.1), OU_SSM=dict(mu=1.0, tau=2.0, kappa=1.0, sigma_obs=0.1),
           BM_SSM=dict(mu=0.2, sigma=1.0, sigma_obs=0.1))


@pytest.fixture(scope="module")
def table_rows(tmp_path_factory):
    """d -> (grid of log sigma_obs, rows of the CTCRW table at each), tau = 2, nu = 1, dt = 1, the default P0 (R/sde.R:584); computed once"""
    exe = build_gainfeed(tmp_path_factory.mktemp("gainfeed"))
    cache = {}

    def rows(d):
        if d not in cache:
            ls, n = [], []
            for lo, hi, cnt in ((-2.4, -0.7, 341), (0.8, 1.5, 15)):
                r = subprocess.run([exe, "rows", str(d), "1.0", repr(LOG_TAU), repr(LOG_NU), str(cnt), repr(lo), repr(hi), "1", "0", "10"],
                                   capture_output=True, text=True, check=True)
                for line in r.stdout.strip().splitlines():
                    a, b = line.split()
                    ls.append(float(a)); n.append(int(b))
            cache[d] = (np.array(ls), np.array(n))
        return cache[d]
    return rows


def _pick(table_rows, d, want, count=1):
    """the first `count` grid points whose table has a row count in `want`"""
    ls, n = table_rows(d)
    idx = [i for i in range(len(ls)) if n[i] in want][:count]
    assert len(idx) == count, (want, sorted(set(n.tolist())))
    return [(_ctcrw_theta(d, ls[i]), int(n[i])) for i in idx]


def _ctcrw_theta(d, log_sigma_obs):
    th = np.zeros(3 + d)
    th[0], th[1 + d], th[2 + d] = log_sigma_obs, LOG_TAU, LOG_NU
    return th


def _other_theta(model, d, k):
    if model == "OU_SSM":
        th = np.array([np.log(0.1)] + [1.0] * d + [np.log(2.0), 0.0])
    else:
        th = np.array([np.log(0.1)] + [0.2] * d + [0.0])
    return th + 0.01 * np.sin(np.arange(th.size) + 0.7 * k)


def _batch(model, M, d, lengths=None):
    import torch
    ID, times, obs = capi.simulate_device(model, M, T, d, seed=53 + M + d, track0=0, lengths=lengths, device=torch.device("cuda:0"), **SIM[model])
    fixed = np.zeros(1 + capi.n_sde_par(model, d), dtype=np.uint8)
    host = capi.Problem(model, ID.cpu().numpy(), times.cpu().numpy(), obs.cpu().numpy(), par_fixed=fixed)
    assert np.all(np.diff(host.times)[np.diff(host.id) == 0] == 1.0)           # (the grid the row counts were computed for)
    return host, (model, ID, times, obs, fixed)


def _engine(dd, monkeypatch, fused=None, host=None, devices=None):
    model, ID, times, obs, fixed = dd
    with monkeypatch.context() as m:
        m.setenv("SSDE_LAGSTATS", "2")
        m.delenv("SSDE_CHUNKS", raising=False)
        m.delenv("SSDE_PUBLISH", raising=False)
        if fused is None:
            m.delenv("SSDE_FUSED_FINALIZE", raising=False)
        else:
            m.setenv("SSDE_FUSED_FINALIZE", str(fused))
        eng = capi.Engine(host, devices=devices) if host is not None else capi.Engine(capi.Problem.from_torch(model, ID, times, obs, par_fixed=fixed))
    eng.set_option(capi.OPT_KERNEL_STAMPS, 0)
    return eng


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _run(eng, th):
    v, g = eng.eval(th)
    return v, g, eng.info()["window_check"]


@pytest.mark.parametrize("M", [64, 130])
@pytest.mark.parametrize("d", [2, 1])
def test_same_bits_as_the_form_that_still_copies(M, d, table_rows, monkeypatch):
    """tables shorter than the capacity, exactly at it, one row past it and far past it: by value, by value, copied, copied -- and
    every one the bits of the two-launch form, which copies whatever the length; against the oracle at tests/test_gpu_lag_models.py's
    tolerance (1e-10 / 1e-8)"""
    from oracle_lib import oracle_eval
    cases = [_pick(table_rows, d, range(2, HEAD_GAIN_ROWS))[0] + (1,), _pick(table_rows, d, [HEAD_GAIN_ROWS])[0] + (1,),
             _pick(table_rows, d, [HEAD_GAIN_ROWS + 1])[0] + (0,), _pick(table_rows, d, range(40, 300))[0] + (0,)]
    host, dd = _batch("CTCRW", M, d)
    eng, ref = _engine(dd, monkeypatch), _engine(dd, monkeypatch, fused=0)
    try:
        for th, rows, feed in cases:
            got, want = _run(eng, th), _run(ref, th)
            inf = eng.info()
            print("d=%d M=%d log sigma_obs %.4f: rows %d (engine %d) feed %d form %d lag rows %d" %
                  (d, M, th[0], rows, eng.last_gain_rows(), eng.last_gain_feed(), eng.last_finish_form(), inf["lagstat_rows"]))
            assert eng.last_gain_rows() == rows and ref.last_gain_rows() == rows
            assert eng.last_gain_feed() == feed and ref.last_gain_feed() == 0
            if rows <= HEAD_GAIN_ROWS + 1:                      # (the far longer table may leave the path: it streams, and copies)
                assert inf["lagstat_rows"] > 0 and eng.last_finish_form() == 2 and inf["window_retries"] == 0, inf
            assert ref.last_finish_form() == 0
            assert _same(got, want), (rows, got, want)
            ov, og = oracle_eval(host, th, order=1, threads=THREADS)
            print("    value %.3e gradient %.3e check %.3e" % (abs(got[0] - ov) / abs(ov), np.max(np.abs(got[1] - og)) / np.max(np.abs(og)), got[2]))
            assert got[2] <= capi.WINDOW_TOL
            assert abs(got[0] - ov) <= 1e-10 * abs(ov), (got[0], ov)
            assert np.max(np.abs(got[1] - og)) <= 1e-8 * np.max(np.abs(og)), (got[1], og)
    finally:
        eng.close(); ref.close()


@pytest.mark.parametrize("model", ["OU_SSM", "BM_SSM"])
def test_the_scalar_family_takes_its_table_by_value_too(model, monkeypatch):
    """d = 2, 130 tracks: the scalar column set (four of the thirteen packed columns are zero); by value exactly when the rows fit"""
    from oracle_lib import oracle_eval
    host, dd = _batch(model, 130, 2)
    eng, ref = _engine(dd, monkeypatch), _engine(dd, monkeypatch, fused=0)
    try:
        fed = 0
        for k in range(4):
            th = _other_theta(model, 2, k)
            got, want = _run(eng, th), _run(ref, th)
            rows = eng.last_gain_rows()
            print("%s k=%d: rows %d feed %d" % (model, k, rows, eng.last_gain_feed()))
            assert eng.info()["lagstat_rows"] > 0 and eng.last_finish_form() == 2
            assert eng.last_gain_feed() == (1 if rows <= HEAD_GAIN_ROWS else 0) and ref.last_gain_feed() == 0 and ref.last_gain_rows() == rows
            fed += eng.last_gain_feed()
            assert _same(got, want), (k, got, want)
            ov, og = oracle_eval(host, th, order=1, threads=THREADS)
            assert abs(got[0] - ov) <= 1e-10 * abs(ov), (got[0], ov)
            assert np.max(np.abs(got[1] - og)) <= 1e-8 * np.max(np.abs(og)), (got[1], og)
        print("%s: %d of 4 tables by value" % (model, fed))
    finally:
        eng.close(); ref.close()


def test_fifty_alternating_evaluations_never_see_a_stale_table(table_rows, monkeypatch):
    """a short table (by value) and a long one (the ring) in turn on one handle: each result the bits of a fresh handle's at that theta"""
    (short, _), (long_, _) = _pick(table_rows, 2, range(2, HEAD_GAIN_ROWS))[0], _pick(table_rows, 2, [HEAD_GAIN_ROWS + 1])[0]
    host, dd = _batch("CTCRW", 130, 2)
    want = []
    for th in (short, long_):
        fresh = _engine(dd, monkeypatch)
        try:
            want.append(_run(fresh, th))
        finally:
            fresh.close()
    assert not _same(want[0], want[1])
    eng = _engine(dd, monkeypatch)
    try:
        for i in range(50):
            got = _run(eng, (short, long_)[i & 1])
            assert eng.last_gain_feed() == 1 - (i & 1) and eng.last_finish_form() == 2
            assert _same(got, want[i & 1]), (i, got, want[i & 1])
    finally:
        eng.close()


@pytest.mark.parametrize("table", ["short", "long"])
def test_evaluations_in_flight_keep_their_own_table(table, table_rows, monkeypatch):
    """PAR_RING + 1 distinct thetas queued back to back on one stream through ssde_eval_device, one synchronisation at the end: every
    result the synchronous one's bits -- by value nothing is shared between launches, a long table takes a ring slot and waits for the
    slot's earlier copy; then a two-shard handle and a one-rank communicator, as tests/test_gpu_head_finish.py runs them"""
    import torch
    want_rows = range(2, HEAD_GAIN_ROWS) if table == "short" else range(HEAD_GAIN_ROWS + 1, HEAD_GAIN_ROWS + 6)
    feed = 1 if table == "short" else 0
    thetas = [th for th, _ in _pick(table_rows, 2, want_rows, PAR_RING + 1)]
    host, dd = _batch("CTCRW", 130, 2)
    eng = _engine(dd, monkeypatch)
    sh = _engine(dd, monkeypatch, host=host, devices=[0, 0])
    cm = _engine(dd, monkeypatch)
    try:
        sync = [_run(eng, th) for th in thetas]
        assert eng.last_finish_form() == 2 and eng.last_gain_feed() == feed
        assert all(not _same(sync[0], s) for s in sync[1:])
        n = eng.n_par_full
        outs = torch.zeros((len(thetas), 2 + n), dtype=torch.float64, device="cuda:0")
        s = torch.cuda.Stream()
        for k, th in enumerate(thetas):
            eng.eval_device(th, outs[k].data_ptr(), order=1, stream=s.cuda_stream)
        s.synchronize()
        assert eng.last_finish_form() == 0 and eng.last_gain_feed() == feed and eng.info()["lagstat_rows"] > 0
        res = outs.cpu().numpy()
        for k in range(len(thetas)):
            assert _same((res[k, 0], res[k, 1:-1], res[k, -1]), sync[k]), (k, res[k], sync[k])
        again = _run(eng, thetas[0])
        assert eng.last_finish_form() == 2 and _same(again, sync[0])
        cm.comm_init(1, 0, capi.comm_unique_id())
        for k, th in enumerate(thetas[:2]):
            vs, gs = sh.eval(th)
            assert sh.info()["n_devices"] == 2 and sh.info()["lagstat_rows"] > 0 and sh.last_finish_form() == 0 and sh.last_gain_feed() == feed
            assert abs(vs - sync[k][0]) <= 1e-12 * abs(sync[k][0]) and np.max(np.abs(gs - sync[k][1])) <= 1e-12 * np.max(np.abs(sync[k][1]))
            vc, gc = cm.eval(th)
            assert cm.info()["lagstat_rows"] > 0 and cm.last_finish_form() == 0 and cm.last_gain_feed() == feed
            assert abs(vc - sync[k][0]) <= 1e-12 * abs(sync[k][0]) and np.max(np.abs(gc - sync[k][1])) <= 1e-12 * np.max(np.abs(sync[k][1]))
    finally:
        for e in (eng, sh, cm):
            e.close()


GROUP_CASES = {
    "all_full": None,                                       # two full groups and a last group of two tracks
    "short_track_in_group_0": (5, 200),                     # a lane of the first group ends inside the head
    "short_track_in_group_1": (64 + 5, 200),                # ... of the second
    "ragged": "ragged",                                     # lanes that end inside the transient window, tile offsets of every stride
}


@pytest.mark.parametrize("case", sorted(GROUP_CASES))
@pytest.mark.parametrize("model,d", [("CTCRW", 2), ("CTCRW", 1), ("OU_SSM", 2), ("BM_SSM", 2)])
def test_every_group_layout_by_value(model, d, case, monkeypatch):
    """130 tracks, full, short and ragged groups: the table by value gives the bits of the two-launch form, which copies it"""
    M = 130
    spec = GROUP_CASES[case]
    lengths = None
    if spec == "ragged":
        lengths = np.resize(np.array([40, 256, 257, 300, 320], dtype=np.int64), M)
    elif spec is not None:
        lengths = np.full(M, T, dtype=np.int64)
        lengths[spec[0]] = spec[1]
    host, dd = _batch(model, M, d, lengths=lengths)
    eng, ref = _engine(dd, monkeypatch), _engine(dd, monkeypatch, fused=0)
    try:
        for k in range(2):
            th = _ctcrw_theta(d, np.log(0.1)) + 0.01 * np.sin(np.arange(3 + d) + 0.7 * k) if model == "CTCRW" else _other_theta(model, d, k)
            got, want = _run(eng, th), _run(ref, th)
            assert eng.info()["lagstat_rows"] > 0 and eng.last_finish_form() == 2 and ref.last_finish_form() == 0
            assert got[2] <= capi.WINDOW_TOL and np.all(got[1] != 0.0)
            assert _same(got, want), (case, k, got, want)
    finally:
        eng.close(); ref.close()
