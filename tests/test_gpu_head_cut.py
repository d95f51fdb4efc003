"""GPU suite: the bulk of the lag-statistics path cut at the end of the covariance transient (ssde_windows.hpp:
head_early_cut, SSDE_OPT_LAG_EARLY).  The streamed head is then the transient window alone -- one window per track, capped at the
cut --, the rows past it come from statistics built for that cut (k_lagstats.hip: the late statistics plus the head rows' own
contribution).  By default the head's launch is one workgroup per track group whose waves are the DIRECTION PARTS of that window
(k_iso_shared_cut.hip); SSDE_FUSED_FINALIZE=0 / =1 run it as one wave per group on iso_shared_kernel.  All three are the same bits.

Setup: the path forced with SSDE_LAGSTATS=2 (these batches are far below the size where the dispatch rule builds anything), then
set_option(OPT_LAG_EARLY, 1), which builds the early cuts.  Batches: 1, 64, 65 and 130 tracks of 2000 rows and 100 tracks whose
lengths cycle through (40, 63, 64, 65, 256, 257, 300, 2000) -- a track's first row initialises its state, so these are 39 .. 1999
steps: tracks that end before the cut, at it, one step past it, at and around row 256; d = 1, 2, and once with mu free.

Tolerances: the project's for this path against streaming (value 1e-12 relative, gradient 1e-10 of its max-norm) and against the
oracle (1e-10 / 1e-8); the device statistics against the host reference 1e-12 of the largest entry.

A handle of two shards splits the tracks over two engines and adds their sums: its bits are not a single engine's (nor were they
before: tests/test_gpu_head_finish.py), so it is held to 1e-12 against the single engine and bitwise against a second two-shard
handle in the other finalising form."""
import os

import numpy as np
import pytest

from smoothsde_amd import capi

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 8)
T = 2000
LAG_A = 256
RAGGED = (40, 63, 64, 65, 256, 257, 300, 2000)
SHAPES = [dict(M=1), dict(M=64), dict(M=65), dict(M=130), dict(M=100, ragged=True)]
CASES = [dict(s, d=d) for d in (2, 1) for s in SHAPES] + [dict(M=130, d=2, free_mu=True), dict(M=100, d=2, ragged=True, free_mu=True)]


def _batch(M, d, ragged=False, free_mu=False):
    import torch
    lengths = np.resize(np.array(RAGGED, dtype=np.int64), M) if ragged else None
    ID, times, obs = capi.simulate_device("CTCRW", M, T, d, mu=0.0, tau=2.0, nu=1.0, kappa=1.0, sigma=1.0, sigma_obs=0.1, seed=71 + M + d,
                                          track0=0, lengths=lengths, device=torch.device("cuda:0"))
    fixed = np.zeros(1 + capi.n_sde_par("CTCRW", d), dtype=np.uint8)
    if not free_mu:
        fixed[1:1 + d] = 1
    host = capi.Problem("CTCRW", ID.cpu().numpy(), times.cpu().numpy(), obs.cpu().numpy(), par_fixed=fixed)
    steps = (lengths if ragged else np.full(M, T, dtype=np.int64)) - 1
    return host, (ID, times, obs, fixed), steps


def _engine(dd, monkeypatch, early=1, lagstats=2, fused=None, host=None, devices=None):
    ID, times, obs, fixed = dd
    with monkeypatch.context() as m:
        for name in ("SSDE_CHUNKS", "SSDE_FUSED_FINALIZE", "SSDE_WINDOW", "SSDE_PUBLISH"):
            m.delenv(name, raising=False)
        m.setenv("SSDE_LAGSTATS", str(lagstats))
        if fused is not None:
            m.setenv("SSDE_FUSED_FINALIZE", str(fused))
        eng = capi.Engine(host, devices=devices) if host is not None else capi.Engine(capi.Problem.from_torch("CTCRW", ID, times, obs, par_fixed=fixed))
    eng.set_option(capi.OPT_KERNEL_STAMPS, 0)
    if early is not None:
        eng.set_option(capi.OPT_LAG_EARLY, early)
    return eng


def _theta(npar, d, k, log_sigma_obs=np.log(0.1)):
    th = np.zeros(npar)
    th[0] = log_sigma_obs
    th[1 + d] = np.log(2.0)
    return th + 0.01 * np.sin(np.arange(npar) + 0.7 * k)


def _run(eng, th):
    v, g = eng.eval(th)
    return v, g, eng.info()["window_check"]


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _tracks(dd):
    ID, _, obs, _ = dd
    idh, yh = ID.cpu().numpy(), obs.cpu().numpy()
    starts = np.flatnonzero(np.r_[True, idh[1:] != idh[:-1]])
    ends = np.r_[starts[1:], len(idh)]
    return [yh[a + 1:b] for a, b in zip(starts, ends)]              # tiled row t of a track = its row t + 1 (the scored rows)


def _case_id(c):
    return "M%d_d%d%s%s" % (c["M"], c["d"], "_ragged" if c.get("ragged") else "", "_mu" if c.get("free_mu") else "")


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_the_early_cut_against_the_late_cut_streaming_and_the_oracle(case, monkeypatch):
    """(a), (c), (g): the same handle with the option off, SSDE_LAGSTATS=0 and the oracle; the three finalising forms; the rows"""
    from oracle_lib import oracle_eval
    d = case["d"]
    host, dd, steps = _batch(**case)
    eng = _engine(dd, monkeypatch)
    forms = dict(two_launch=_engine(dd, monkeypatch, fused=0), fused=_engine(dd, monkeypatch, fused=1))
    stream = _engine(dd, monkeypatch, early=None, lagstats=0)
    try:
        for k in range(2):
            th = _theta(eng.n_par_full, d, k)
            res = _run(eng, th)
            v, g, chk = res
            inf = eng.info()
            cut = eng.last_lag_cut()
            assert cut in capi.LAG_CUTS and inf["window_retries"] == 0 and chk <= capi.WINDOW_TOL, (cut, inf)
            assert inf["lagstat_rows"] == int(np.sum(np.maximum(steps - cut, 0))) > 0, (cut, inf)
            assert inf["main_kernel_rows"] + inf["lagstat_rows"] == inf["n_steps"], inf
            # what ran: the direction parts of window 0 (sigma_obs, tau, nu; mu rides with nu) on the waves of one workgroup per padded
            # group, finished on the host
            g8 = (inf["n_groups"] + 7) // 8 * 8
            # (d = 1: the single wave per group and a finalize launch -- the parts' value was not that wave's bits there: DESIGN.md §3.3d)
            if d == 2:
                assert inf["lanes_per_track"] == 3 and inf["n_kernel_blocks"] == g8 and eng.last_finish_form() == 2, inf
            else:
                assert inf["lanes_per_track"] == 1 and inf["n_kernel_blocks"] == (g8 + 3) // 4 and eng.last_finish_form() == 0, inf
            for name, e in forms.items():
                other = _run(e, th)
                oi = e.info()
                # ... against the single wave per group on the same window (iso_shared_kernel), finalize launch or fused: the same bits
                assert e.last_lag_cut() == cut and e.last_finish_form() == (1 if name == "fused" else 0)
                assert oi["lanes_per_track"] == 1 and oi["n_kernel_blocks"] == (g8 + 3) // 4, oi
                assert oi["lagstat_rows"] == inf["lagstat_rows"] and oi["main_kernel_rows"] == inf["main_kernel_rows"]
                assert _same(res, other), (name, res, other)
            # a value-only evaluation: one part, the same value
            assert eng.eval(th, order=0) == v
            # the same handle with the option off: the late cut
            eng.set_option(capi.OPT_LAG_EARLY, 0)
            vl, gl = eng.eval(th)
            il = eng.info()
            assert eng.last_lag_cut() == LAG_A and il["lagstat_rows"] == int(np.sum(np.maximum(steps - LAG_A, 0))), il
            assert il["main_kernel_rows"] + il["lagstat_rows"] == il["n_steps"] and il["lanes_per_track"] > 3, il
            eng.set_option(capi.OPT_LAG_EARLY, 1)
            vs, gs = stream.eval(th)
            assert stream.info()["lagstat_rows"] == 0 and stream.last_lag_cut() == 0
            ov, og = oracle_eval(host, th, order=1, threads=THREADS)
            print("%s k=%d cut %d: value %.2e (late) %.2e (stream) %.2e (oracle), gradient %.2e %.2e %.2e, check %.2e" % (
                _case_id(case), k, cut, abs(v - vl) / abs(vl), abs(v - vs) / abs(vs), abs(v - ov) / abs(ov),
                np.max(np.abs(g - gl)) / np.max(np.abs(gl)), np.max(np.abs(g - gs)) / np.max(np.abs(gs)), np.max(np.abs(g - og)) / np.max(np.abs(og)), chk))
            for vr, gr in ((vl, gl), (vs, gs)):
                assert abs(v - vr) <= 1e-12 * abs(vr), (v, vr)
                assert np.max(np.abs(g - gr)) <= 1e-10 * np.max(np.abs(gr)), (g, gr)
            assert abs(v - ov) <= 1e-10 * abs(ov), (v, ov)
            assert np.max(np.abs(g - og)) <= 1e-8 * np.max(np.abs(og)), (g, og)
            fixed = host.par_fixed != 0
            assert np.all(g[fixed] == 0.0) and np.all(g[~fixed] != 0.0)
    finally:
        for e in [eng, stream] + list(forms.values()):
            e.close()


@pytest.mark.parametrize("case", [dict(M=100, d=2, ragged=True), dict(M=100, d=1, ragged=True), dict(M=130, d=2)], ids=_case_id)
def test_the_device_statistics_against_the_host_reference(case, monkeypatch):
    """(b): every early cut, and two builds give the same bits"""
    host, dd, steps = _batch(**case)
    a, b = _engine(dd, monkeypatch), _engine(dd, monkeypatch)
    off = _engine(dd, monkeypatch, early=None)
    try:
        with pytest.raises(capi.EngineError):
            off.lagstats_cut(64)                                       # SSDE_LAGSTATS=2 alone builds the late statistics only
        assert off.lagstats() is not None
        off.eval(_theta(off.n_par_full, case["d"], 0))
        assert off.last_lag_cut() == LAG_A
        tracks = _tracks(dd)
        late = a.lagstats()
        for cut in capi.LAG_CUTS:
            Md, sd, nd = a.lagstats_cut(cut)
            Mh, sh, nh = capi.lagstats_host_cut(tracks, cut)
            assert nd == nh == float(np.sum(np.maximum(steps - cut, 0)))
            print("cut %d: M %.2e s %.2e" % (cut, np.max(np.abs(Md - Mh)) / np.max(np.abs(Mh)), np.max(np.abs(sd - sh)) / np.max(np.abs(sh))))
            assert np.max(np.abs(Md - Mh)) <= 1e-12 * np.max(np.abs(Mh))
            assert np.max(np.abs(sd - sh)) <= 1e-12 * np.max(np.abs(sh))
            assert not Md[cut:, :].any() and not Md[:, cut:].any() and not sd[:, cut:].any()
            Mb, sb, nb = b.lagstats_cut(cut)
            assert np.array_equal(Md, Mb) and np.array_equal(sd, sb) and nd == nb
        again = a.lagstats_cut(LAG_A)                                  # the late statistics are what they were
        assert np.array_equal(again[0], late[0]) and np.array_equal(again[1], late[1]) and again[2] == late[2]
    finally:
        for e in (a, b, off):
            e.close()


def test_the_other_callers_get_the_same_bits_through_the_finalize_launch(monkeypatch):
    """(d): ssde_eval_device queued on one stream and a one-rank communicator -- bitwise the synchronous call; a handle of two shards"""
    import torch
    d = 2
    host, dd, steps = _batch(130, d, free_mu=True)
    eng, cm = _engine(dd, monkeypatch), _engine(dd, monkeypatch)
    sh = _engine(dd, monkeypatch, host=host, devices=[0, 0])
    sh0 = _engine(dd, monkeypatch, host=host, devices=[0, 0], fused=0)
    try:
        thetas = [_theta(eng.n_par_full, d, k) for k in range(4)]
        sync = [_run(eng, th) for th in thetas]
        cut = eng.last_lag_cut()
        assert cut in capi.LAG_CUTS and eng.last_finish_form() == 2
        n = eng.n_par_full
        outs = torch.zeros((4, 2 + n), dtype=torch.float64, device="cuda:0")
        s = torch.cuda.Stream()
        for k, th in enumerate(thetas):
            eng.eval_device(th, outs[k].data_ptr(), order=1, stream=s.cuda_stream)
        s.synchronize()
        assert eng.last_lag_cut() == cut and eng.last_finish_form() == 0
        res = outs.cpu().numpy()
        for k, th in enumerate(thetas):
            pv, pg = eng.penalty(th)
            assert pv == 0.0 and not np.any(pg)
            assert _same((res[k, 0], res[k, 1:-1], res[k, -1]), sync[k]), (k, res[k], sync[k])
        cm.comm_init(1, 0, capi.comm_unique_id())
        for k, th in enumerate(thetas[:2]):
            got = _run(cm, th)
            assert cm.last_lag_cut() == cut and cm.last_finish_form() == 0 and cm.info()["lagstat_rows"] == sum(np.maximum(steps - cut, 0))
            assert _same(got, sync[k]), (k, got, sync[k])
            vs, gs = sh.eval(th)
            inf = sh.info()
            assert inf["n_devices"] == 2 and sh.last_lag_cut() == cut and inf["lagstat_rows"] == sum(np.maximum(steps - cut, 0)), inf
            assert abs(vs - sync[k][0]) <= 1e-12 * abs(sync[k][0]) and np.max(np.abs(gs - sync[k][1])) <= 1e-12 * np.max(np.abs(sync[k][1]))
            v0, g0 = sh0.eval(th)
            assert sh0.last_lag_cut() == cut and v0 == vs and np.array_equal(g0, gs)
    finally:
        for e in (eng, cm, sh, sh0):
            e.close()


def test_a_cut_off_the_list_runs_the_late_cut(monkeypatch):
    """(e): noisier fixes forget more slowly -- the first log sigma_obs on a grid whose transient window ends past the last early cut
    still takes its bulk from the statistics, at row 256, and computes the bits of the option off"""
    d = 2
    host, dd, steps = _batch(130, d, free_mu=True)
    on, off = _engine(dd, monkeypatch), _engine(dd, monkeypatch, early=0)
    try:
        seen_early = False
        for ls in np.linspace(np.log(0.1), np.log(3.0), 24):           # (both engines walk the same thetas: the same window policy history)
            th = _theta(on.n_par_full, d, 1, log_sigma_obs=ls)
            a, b = _run(on, th), _run(off, th)
            cut = on.last_lag_cut()
            assert off.last_lag_cut() in (0, LAG_A)
            if cut in capi.LAG_CUTS:
                seen_early = True
                continue
            if cut == LAG_A:
                break
        else:
            pytest.fail("no sigma_obs on the grid puts the transient window past the last early cut with the bulk still on the statistics")
        assert seen_early and off.last_lag_cut() == LAG_A
        assert on.info()["lagstat_rows"] == off.info()["lagstat_rows"] == sum(np.maximum(steps - LAG_A, 0))
        assert _same(a, b), (a, b)
    finally:
        on.close(); off.close()


def test_fifty_evaluations_alternating_between_two_cuts_equal_fresh_handles(monkeypatch):
    """(f): nothing of an evaluation at one cut is left for the next one at another"""
    d = 2
    host, dd, steps = _batch(130, d, free_mu=True)
    eng = _engine(dd, monkeypatch)
    fresh = []
    try:
        # two thetas with different early cuts, found on a scratch handle
        scratch = _engine(dd, monkeypatch)
        by_cut = {}
        for ls in np.linspace(np.log(0.05), np.log(1.0), 16):
            th = _theta(eng.n_par_full, d, 2, log_sigma_obs=ls)
            scratch.eval(th)
            if scratch.last_lag_cut() in capi.LAG_CUTS:
                by_cut.setdefault(scratch.last_lag_cut(), th)
        scratch.close()
        assert len(by_cut) >= 2, by_cut
        cuts = sorted(by_cut)[:2]
        thetas = [by_cut[c] for c in cuts]
        want = []
        for th in thetas:
            e = _engine(dd, monkeypatch)
            fresh.append(e)
            want.append(_run(e, th))
        assert not _same(want[0], want[1])
        for i in range(50):
            got = _run(eng, thetas[i & 1])
            assert eng.last_lag_cut() == cuts[i & 1] and eng.info()["lagstat_rows"] == sum(np.maximum(steps - cuts[i & 1], 0))
            assert _same(got, want[i & 1]), (i, got, want[i & 1])
        assert eng.info()["window_retries"] == 0
    finally:
        for e in [eng] + fresh:
            e.close()


@pytest.mark.parametrize("d,M,rows", [(2, 1000, 5000), (1, 1300, 4000)], ids=["d2", "d1"])
def test_the_default_where_the_dispatch_rule_builds_the_statistics(d, M, rows, monkeypatch):
    """Batches just past the size at which create builds the lag statistics by its own rule (no SSDE_LAGSTATS, no option set): with two
    response coordinates the early cuts are built with them and the option is on -- the direction parts, finished on the host; with one
    coordinate nothing early is built, the option is off and the evaluation is the late cut's one-workgroup head, as before"""
    import torch
    ID, times, obs = capi.simulate_device("CTCRW", M, rows, d, mu=0.0, tau=2.0, nu=1.0, kappa=1.0, sigma=1.0, sigma_obs=0.1, seed=5 + d,
                                          track0=0, device=torch.device("cuda:0"))
    fixed = np.zeros(1 + capi.n_sde_par("CTCRW", d), dtype=np.uint8)
    fixed[1:1 + d] = 1
    with monkeypatch.context() as m:
        for name in ("SSDE_LAGSTATS", "SSDE_CHUNKS", "SSDE_FUSED_FINALIZE", "SSDE_WINDOW", "SSDE_PUBLISH"):
            m.delenv(name, raising=False)
        eng = capi.Engine(capi.Problem.from_torch("CTCRW", ID, times, obs, par_fixed=fixed))
    try:
        eng.set_option(capi.OPT_KERNEL_STAMPS, 0)
        assert eng.lagstats() is not None
        v, g = eng.eval(_theta(eng.n_par_full, d, 0))
        inf = eng.info()
        g8 = (inf["n_groups"] + 7) // 8 * 8
        assert inf["window_check"] <= capi.WINDOW_TOL and inf["window_retries"] == 0, inf
        assert inf["main_kernel_rows"] + inf["lagstat_rows"] == inf["n_steps"], inf
        if d == 2:
            cut = eng.last_lag_cut()
            assert cut in capi.LAG_CUTS and inf["lanes_per_track"] == 3 and inf["lagstat_rows"] == M * (rows - 1 - cut), (cut, inf)
            assert inf["n_kernel_blocks"] == g8 and eng.last_finish_form() == 2, inf
            assert eng.lagstats_cut(cut)[2] == inf["lagstat_rows"]
            eng.set_option(capi.OPT_LAG_EARLY, 0)
            vl, gl = eng.eval(_theta(eng.n_par_full, d, 0))
            assert eng.last_lag_cut() == LAG_A and eng.info()["lanes_per_track"] > 3
            assert abs(v - vl) <= 1e-12 * abs(vl) and np.max(np.abs(g - gl)) <= 1e-10 * np.max(np.abs(gl))
        else:
            # (the late cut's head: more than three windows, each on a wave of its own; four are one workgroup, finished on the host)
            assert eng.last_lag_cut() == LAG_A and inf["lanes_per_track"] > 3 and inf["lagstat_rows"] == M * (rows - 1 - LAG_A), inf
            assert (eng.last_finish_form() == 2) == (inf["lanes_per_track"] == 4), inf
            with pytest.raises(capi.EngineError):
                eng.lagstats_cut(64)
    finally:
        eng.close()
