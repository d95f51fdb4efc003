"""GPU suite: the head of the lag-statistics path with one workgroup per track group -- the hand-overs checked in LDS -- and, for the
synchronous single-device call, finished on the host (k_iso_shared.inc: iso_shared_wg_kernel, ssde_reduce_host.hpp).

Three engines per batch: SSDE_FUSED_FINALIZE unset (the new form: 2, the host), = 0 (the two-launch form on iso_shared_kernel: 0) and
= 1 (the finalising work fused into that kernel: 1).  Value, gradient and the hand-over check must be the same bits in all three, and in
the form every other caller gets (the records in device memory and a finalize launch without check workgroups: stamped evaluations,
ssde_eval_device, shards, a communicator).  The synchronous engines run with plain launches (SSDE_OPT_KERNEL_STAMPS off, as the
timed steps of bench.py do): a stamped evaluation is one of the other callers.

Batches of tests/test_gpu_head_plan.py's size, the path forced with SSDE_LAGSTATS=2: 320 rows (barely longer than LAG_A), one group, a
full group, a one-lane last group, three groups, and ragged lengths whose lanes end inside the transient window, inside the last
window and at row 256; d = 1, 2; CTCRW, OU_SSM and BM_SSM with mu free, so that every accumulator is fed."""
import os

import numpy as np
import pytest

from smoothsde_amd import capi

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 8)
T = 320
WG_WAVES = 4
SIM = dict(CTCRW=dict(mu=0.0, tau=2.0, nu=1.0, sigma_obs=0.1), OU_SSM=dict(mu=1.0, tau=2.0, kappa=1.0, sigma_obs=0.1),
           BM_SSM=dict(mu=0.2, sigma=1.0, sigma_obs=0.1))
SHAPES = [dict(M=1), dict(M=64), dict(M=65), dict(M=130), dict(M=100, ragged=True)]
FORMS = {"host": None, "two_launch": 0, "fused": 1}        # SSDE_FUSED_FINALIZE -> ssde_last_finish_form 2 / 0 / 1
FORM_ID = {"host": 2, "two_launch": 0, "fused": 1}


def _batch(model, M, d, ragged=False):
    import torch
    lengths = np.resize(np.array([40, 256, 257, 300, 320], dtype=np.int64), M) if ragged else None
    ID, times, obs = capi.simulate_device(model, M, T, d, seed=53 + M + d, track0=0, lengths=lengths, device=torch.device("cuda:0"),
                                          **SIM[model])
    fixed = np.zeros(1 + capi.n_sde_par(model, d), dtype=np.uint8)
    host = capi.Problem(model, ID.cpu().numpy(), times.cpu().numpy(), obs.cpu().numpy(), par_fixed=fixed)
    return host, (model, ID, times, obs, fixed)


def _engine(dd, monkeypatch, fused=None, stamps=0, host=None, devices=None):
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
    eng.set_option(capi.OPT_KERNEL_STAMPS, stamps)
    return eng


def _theta(model, d, k):
    if model == "CTCRW":
        th = np.zeros(3 + d)
        th[0] = np.log(0.1)
        th[1 + d] = np.log(2.0)
    elif model == "OU_SSM":
        th = np.array([np.log(0.1)] + [1.0] * d + [np.log(2.0), 0.0])
    else:
        th = np.array([np.log(0.1)] + [0.2] * d + [0.0])
    return th + 0.01 * np.sin(np.arange(th.size) + 0.7 * k)


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _run(eng, th):
    v, g = eng.eval(th)
    return v, g, eng.info()["window_check"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d%s" % (s["M"], "_ragged" if s.get("ragged") else ""))
@pytest.mark.parametrize("d", [2, 1])
@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
def test_the_three_forms_are_the_same_bits(model, d, shape, monkeypatch):
    from oracle_lib import oracle_eval
    host, dd = _batch(model, d=d, **shape)
    engines = {name: _engine(dd, monkeypatch, fused=f) for name, f in FORMS.items()}
    engines["stamped"] = _engine(dd, monkeypatch, stamps=1)               # one of the other callers: the records in device memory
    try:
        for k in range(4):
            th = _theta(model, d, k)
            res = {name: _run(e, th) for name, e in engines.items()}
            for name, e in engines.items():
                inf = e.info()
                assert e.last_finish_form() == FORM_ID.get(name, 0), (name, e.last_finish_form(), inf)
                assert inf["lagstat_rows"] > 0 and inf["window_retries"] == 0, (name, inf)
            inf = engines["host"].info()
            assert inf["lanes_per_track"] == WG_WAVES and inf["n_kernel_blocks"] == (inf["n_groups"] + 7) // 8 * 8, inf
            for name in ("two_launch", "fused", "stamped"):
                assert _same(res["host"], res[name]), (name, res["host"], res[name])
            v, g, chk = res["host"]
            assert chk <= capi.WINDOW_TOL
            assert np.all(g != 0.0)
            ov, og = oracle_eval(host, th, order=1, threads=THREADS)
            print("%s d=%d k=%d: value %.3e gradient %.3e check %.3e" % (model, d, k, abs(v - ov) / abs(ov), np.max(np.abs(g - og)) / np.max(np.abs(og)), chk))
            assert abs(v - ov) <= 1e-10 * abs(ov), (v, ov)
            assert np.max(np.abs(g - og)) <= 1e-8 * np.max(np.abs(og)), (g, og)
    finally:
        for e in engines.values():
            e.close()


def test_fifty_evaluations_on_one_handle_never_read_a_stale_record(monkeypatch):
    """alternating two parameter vectors: a sequence word or a record left over from the evaluation before would show at once"""
    host, dd = _batch("CTCRW", 130, 2)
    eng, ref = _engine(dd, monkeypatch), _engine(dd, monkeypatch, fused=0)
    try:
        thetas = [_theta("CTCRW", 2, 0), _theta("CTCRW", 2, 5)]
        want = [_run(ref, th) for th in thetas]
        assert ref.last_finish_form() == 0 and not _same(want[0], want[1])
        for i in range(50):
            got = _run(eng, thetas[i & 1])
            assert eng.last_finish_form() == 2
            assert _same(got, want[i & 1]), (i, got, want[i & 1])
        # ... and a value-only evaluation takes the same route (the gradient rides along on this path)
        assert eng.eval(thetas[0], order=0) == want[0][0] and eng.last_finish_form() == 2
    finally:
        eng.close(); ref.close()


def test_the_other_callers_get_the_records_in_device_memory(monkeypatch):
    """ssde_eval_device queued four deep on one stream, a two-shard handle and a one-rank communicator: a finalize launch (form 0), the
    synchronous results -- bitwise where nothing is added to them (no penalty, one engine), within tests/test_gpu_lag_models.py's
    limits for the shards"""
    import torch
    host, dd = _batch("CTCRW", 130, 2)
    eng = _engine(dd, monkeypatch)
    sh = _engine(dd, monkeypatch, host=host, devices=[0, 0])
    cm = _engine(dd, monkeypatch)
    try:
        thetas = [_theta("CTCRW", 2, k) for k in range(4)]
        sync = [_run(eng, th) for th in thetas]
        assert eng.last_finish_form() == 2
        n = eng.n_par_full
        outs = torch.zeros((4, 2 + n), dtype=torch.float64, device="cuda:0")
        s = torch.cuda.Stream()
        for k, th in enumerate(thetas):
            eng.eval_device(th, outs[k].data_ptr(), order=1, stream=s.cuda_stream)
        s.synchronize()
        assert eng.last_finish_form() == 0
        res = outs.cpu().numpy()
        for k, th in enumerate(thetas):
            pv, pg = eng.penalty(th)
            assert pv == 0.0 and not np.any(pg)
            assert _same((res[k, 0], res[k, 1:-1], res[k, -1]), sync[k]), (k, res[k], sync[k])
        again = _run(eng, thetas[0])                                 # the synchronous call after them is back on the host
        assert eng.last_finish_form() == 2 and _same(again, sync[0])
        cm.comm_init(1, 0, capi.comm_unique_id())
        for k, th in enumerate(thetas[:2]):
            vs, gs = sh.eval(th)
            inf = sh.info()
            assert inf["n_devices"] == 2 and inf["lagstat_rows"] > 0 and sh.last_finish_form() == 0, inf
            assert abs(vs - sync[k][0]) <= 1e-12 * abs(sync[k][0]) and np.max(np.abs(gs - sync[k][1])) <= 1e-12 * np.max(np.abs(sync[k][1]))
            vc, gc = cm.eval(th)
            assert cm.info()["lagstat_rows"] > 0 and cm.last_finish_form() == 0
            assert abs(vc - sync[k][0]) <= 1e-12 * abs(sync[k][0]) and np.max(np.abs(gc - sync[k][1])) <= 1e-12 * np.max(np.abs(sync[k][1]))
    finally:
        for e in (eng, sh, cm):
            e.close()
