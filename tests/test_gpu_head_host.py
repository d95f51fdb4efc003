"""GPU suite: the head of the lag-statistics path from Gram statistics built at create (ssde_headforms.hpp,
k_lagstats.hip: head_gram_kernel, SSDE_OPT_LAG_HEAD_HOST).  A synchronous single-device ssde_eval whose bulk is cut early then forms the
head's accumulators on the host and launches nothing; every other caller keeps the launch.

Setup: the path forced with SSDE_LAGSTATS=2 (these batches are far below the size where the dispatch rule builds anything), then
set_option(OPT_LAG_EARLY, 1) and set_option(OPT_LAG_HEAD_HOST, 1), which build the early cuts and the head's statistics.  Batches: 1, 64,
65 and 130 tracks of 2000 rows, d = 2 (padding workgroups; a last group with empty lanes).

Tolerances: the host head against the same handle with the option off -- value 1e-12 relative, gradient 1e-10 of its max-norm,
window_check <= WINDOW_TOL: what test_gpu_head_cut.py holds the early cut to against the late one; the device statistics against the
host reference 1e-12 of the largest entry, as the lag statistics' tests."""
import numpy as np
import pytest

from smoothsde_amd import capi

pytestmark = pytest.mark.gpu
T = 2000
SIZES = (1, 64, 65, 130)


def _batch(M, ragged=None, free_mu=True):
    import torch
    lengths = None if ragged is None else np.resize(np.array(ragged, dtype=np.int64), M)
    ID, times, obs = capi.simulate_device("CTCRW", M, T, 2, mu=0.0, tau=2.0, nu=1.0, kappa=1.0, sigma=1.0, sigma_obs=0.1, seed=171 + M,
                                          track0=0, lengths=lengths, device=torch.device("cuda:0"))
    fixed = np.zeros(1 + capi.n_sde_par("CTCRW", 2), dtype=np.uint8)
    if not free_mu:
        fixed[1:3] = 1
    return ID, times, obs, fixed


def _engine(dd, monkeypatch, head=1):
    ID, times, obs, fixed = dd
    with monkeypatch.context() as m:
        for name in ("SSDE_CHUNKS", "SSDE_FUSED_FINALIZE", "SSDE_WINDOW", "SSDE_PUBLISH"):
            m.delenv(name, raising=False)
        m.setenv("SSDE_LAGSTATS", "2")
        eng = capi.Engine(capi.Problem.from_torch("CTCRW", ID, times, obs, par_fixed=fixed))
    eng.set_option(capi.OPT_KERNEL_STAMPS, 0)
    eng.set_option(capi.OPT_LAG_EARLY, 1)
    if head is not None:
        eng.set_option(capi.OPT_LAG_HEAD_HOST, head)
    return eng


def _theta(npar, k, log_sigma_obs=np.log(0.1)):
    th = np.zeros(npar)
    th[0] = log_sigma_obs
    th[3] = np.log(2.0)
    return th + 0.01 * np.sin(np.arange(npar) + 0.7 * k)


def _run(eng, th):
    v, g = eng.eval(th)
    return v, g, eng.info()["window_check"]


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _close(a, b):
    return abs(a[0] - b[0]) <= 1e-12 * abs(b[0]) and np.max(np.abs(a[1] - b[1])) <= 1e-10 * np.max(np.abs(b[1])) and a[2] <= capi.WINDOW_TOL


def _tracks_a0(dd):
    ID, _, obs, _ = dd
    idh, yh = ID.cpu().numpy(), obs.cpu().numpy()
    starts = np.flatnonzero(np.r_[True, idh[1:] != idh[:-1]])
    ends = np.r_[starts[1:], len(idh)]
    # tiled row t of a track = its row t + 1; the first row is the initial state (the default a0: the first fix, velocity 0)
    tracks = [yh[a + 1:b] for a, b in zip(starts, ends)]
    a0 = np.stack([np.array([yh[a, 0], 0.0, yh[a, 1], 0.0]) for a in starts])
    return tracks, a0


@pytest.mark.parametrize("M", SIZES)
def test_the_host_head_against_the_kernel_on_the_same_handle(M, monkeypatch):
    dd = _batch(M)
    eng, other = _engine(dd, monkeypatch), _engine(dd, monkeypatch)
    try:
        # the device statistics against the host reference, entry by entry; two builds give the same bits
        Gd, sd, nd = eng.headstats()
        Gh, sh, nh = capi.headstats_host(*_tracks_a0(dd))
        print("M %d statistics: G %.2e s %.2e" % (M, np.max(np.abs(Gd - Gh)) / np.max(np.abs(Gh)), np.max(np.abs(sd - sh)) / np.max(np.abs(sh))))
        assert nd == nh == M
        assert np.all(np.abs(Gd - Gh) <= 1e-12 * np.max(np.abs(Gh))) and np.all(np.abs(sd - sh) <= 1e-12 * np.max(np.abs(sh)))
        Gb, sb, nb = other.headstats()
        assert np.array_equal(Gd, Gb) and np.array_equal(sd, sb) and nd == nb
        for k in range(2):
            th = _theta(eng.n_par_full, k)
            res = _run(eng, th)
            inf, cut = eng.info(), eng.last_lag_cut()
            assert eng.last_head_form() == 1 and cut in capi.LAG_CUTS and inf["window_retries"] == 0, (cut, inf)
            # the fields describe the head launch of this plan, which every other caller of the handle runs
            g8 = (inf["n_groups"] + 7) // 8 * 8
            assert inf["lanes_per_track"] == 3 and inf["n_kernel_blocks"] == g8 and eng.last_finish_form() == 2, inf
            assert inf["lagstat_rows"] == M * (T - 1 - cut) and inf["main_kernel_rows"] + inf["lagstat_rows"] == inf["n_steps"], inf
            v0 = eng.eval(th, order=0)
            assert eng.last_head_form() == 1
            eng.set_option(capi.OPT_LAG_HEAD_HOST, 0)
            ref = _run(eng, th)
            ri = eng.info()
            assert eng.last_head_form() == 0 and eng.last_lag_cut() == cut and eng.last_finish_form() == 2
            for key in ("lanes_per_track", "n_kernel_blocks", "lagstat_rows", "main_kernel_rows", "n_steps", "window"):
                assert ri[key] == inf[key], (key, ri, inf)
            v0k = eng.eval(th, order=0)
            eng.set_option(capi.OPT_LAG_HEAD_HOST, 1)
            print("M %d k %d cut %d: value %.2e gradient %.2e check %.2e" % (M, k, cut, abs(res[0] - ref[0]) / abs(ref[0]),
                                                                         np.max(np.abs(res[1] - ref[1])) / np.max(np.abs(ref[1])), res[2]))
            assert _close(res, ref), (res, ref)
            assert abs(v0 - v0k) <= 1e-12 * abs(v0k) and abs(v0 - res[0]) <= 1e-12 * abs(v0k)
            fixed = dd[3] != 0
            assert np.all(res[1][fixed] == 0.0) and np.all(res[1][~fixed] != 0.0)
            assert _same(_run(other, th), res)                   # a second handle: the same bits
    finally:
        eng.close(); other.close()


def test_fifty_evaluations_alternating_between_two_cuts_equal_fresh_handles(monkeypatch):
    dd = _batch(130)
    eng = _engine(dd, monkeypatch)
    fresh = []
    try:
        scratch = _engine(dd, monkeypatch)
        by_cut = {}
        for ls in np.linspace(np.log(0.05), np.log(1.0), 16):
            th = _theta(eng.n_par_full, 2, log_sigma_obs=ls)
            scratch.eval(th)
            if scratch.last_lag_cut() in capi.LAG_CUTS and scratch.last_head_form() == 1:
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
            assert eng.last_lag_cut() == cuts[i & 1] and eng.last_head_form() == 1
            assert _same(got, want[i & 1]), (i, got, want[i & 1])
        assert eng.info()["window_retries"] == 0
    finally:
        for e in [eng] + fresh:
            e.close()


def test_eval_device_on_the_same_handle_still_launches_and_agrees(monkeypatch):
    import torch
    dd = _batch(130)
    eng = _engine(dd, monkeypatch)
    try:
        thetas = [_theta(eng.n_par_full, k) for k in range(3)]
        sync = [_run(eng, th) for th in thetas]
        assert eng.last_head_form() == 1
        n = eng.n_par_full
        outs = torch.zeros((3, 2 + n), dtype=torch.float64, device="cuda:0")
        s = torch.cuda.Stream()
        for k, th in enumerate(thetas):
            eng.eval_device(th, outs[k].data_ptr(), order=1, stream=s.cuda_stream)
        s.synchronize()
        assert eng.last_head_form() == 0 and eng.last_finish_form() == 0
        res = outs.cpu().numpy()
        for k in range(3):
            assert _close((res[k, 0], res[k, 1:-1], res[k, -1]), sync[k]), (k, res[k], sync[k])
        # ... and the synchronous call after it takes the statistics again, to the bits it had
        assert _same(_run(eng, thetas[0]), sync[0]) and eng.last_head_form() == 1
    finally:
        eng.close()


def test_a_ragged_batch_with_a_short_track_keeps_the_kernel(monkeypatch):
    dd = _batch(70, ragged=(2000, 40, 2000, 300))
    eng, off = _engine(dd, monkeypatch), _engine(dd, monkeypatch, head=None)
    try:
        with pytest.raises(capi.EngineError):
            eng.headstats()                                            # the option returned without building
        th = _theta(eng.n_par_full, 0)
        a, b = _run(eng, th), _run(off, th)
        assert eng.last_head_form() == 0 and eng.last_lag_cut() in capi.LAG_CUTS and eng.last_finish_form() == 2
        assert _same(a, b), (a, b)
    finally:
        eng.close(); off.close()


def test_the_default_where_the_dispatch_rule_builds_the_statistics(monkeypatch):
    """1000 tracks x 5000 rows, nothing set: create builds the head's statistics with the early cuts, and the option's default is what
    the measurement of DESIGN.md §3.3d left it at"""
    import torch
    M, rows = 1000, 5000
    ID, times, obs = capi.simulate_device("CTCRW", M, rows, 2, mu=0.0, tau=2.0, nu=1.0, kappa=1.0, sigma=1.0, sigma_obs=0.1, seed=7,
                                          track0=0, device=torch.device("cuda:0"))
    fixed = np.zeros(1 + capi.n_sde_par("CTCRW", 2), dtype=np.uint8)
    fixed[1:3] = 1
    with monkeypatch.context() as m:
        for name in ("SSDE_LAGSTATS", "SSDE_CHUNKS", "SSDE_FUSED_FINALIZE", "SSDE_WINDOW", "SSDE_PUBLISH"):
            m.delenv(name, raising=False)
        eng = capi.Engine(capi.Problem.from_torch("CTCRW", ID, times, obs, par_fixed=fixed))
    try:
        eng.set_option(capi.OPT_KERNEL_STAMPS, 0)
        assert eng.headstats()[2] == M
        th = _theta(eng.n_par_full, 0)
        res = _run(eng, th)
        assert eng.last_lag_cut() in capi.LAG_CUTS and eng.last_finish_form() == 2
        assert eng.last_head_form() == HEAD_HOST_DEFAULT
        eng.set_option(capi.OPT_LAG_HEAD_HOST, 1 - HEAD_HOST_DEFAULT)
        ref = _run(eng, th)
        assert eng.last_head_form() == 1 - HEAD_HOST_DEFAULT
        assert _close(res, ref) and _close(ref, res), (res, ref)
    finally:
        eng.close()


HEAD_HOST_DEFAULT = 1      # (the A/B of DESIGN.md §3.3d: on)
