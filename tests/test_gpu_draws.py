"""GPU suite (-m gpu): ssde_smooth_draws on every handle layout it serves, against the numpy reference of
tests/draws_ref.py (itself, and the host twin of the lane math, checked on the CPU: test_draws_host.py, test_draws_hostsim.py).

Every case runs a few thousand rows at most and five draws, asserts the layout it ran on (info()) and compares at
1e-9 (1 + max|ref|) with identical NaN patterns -- a draw is mean + factor z, so the limit is the smoother's covariance limit.
Shapes as test_gpu_smooth_layouts.py: 70 ragged tracks (two groups, the second partly filled), a one-row and a two-row track, an NA
row ending a track, log sigma_obs in [-1.5, 0]."""
import numpy as np
import pytest

from cases import _tracks, eseal_spec, make_spec, problem_from_spec
from draws_ref import draws_ref
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS70 = [20, 35, 1, 14, 2, 27, 9] * 10
N70 = sum(LENGTHS70)
ERR_ARG, ERR_MODEL = 1, 2
_REF = {}


def _ref(key, pb, par, **kw):
    """the reference of a case, computed once"""
    if key not in _REF:
        with np.errstate(invalid="ignore"):
            _REF[key] = draws_ref(pb, par, **kw)
    return _REF[key]


def _show(tag, info, **more):
    keys = ("path", "kernel_id", "const_coeff", "uniform_dt", "n_rows", "n_rows_tiled", "n_groups", "n_devices", "n_tracks", "sdim")
    print("LAYOUT", tag, {k: info[k] for k in keys}, more)


def _compare(got, ref, tag):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
    ok = ~np.isnan(ref)
    gap = np.max(np.abs(got[ok] - ref[ok]), initial=0.0) / (1.0 + np.max(np.abs(ref[ok]), initial=0.0))
    print(f"GAP {tag}: {gap:.2e}")
    assert gap <= 1e-9, (tag, gap)


def _run(pb, par, n_draws=5, seed=11, draw0=0, **kw):
    eng = capi.Engine(pb, **kw)
    try:
        return eng.smooth_draws(par, n_draws, seed=seed, draw0=draw0), eng.info(), eng
    except Exception:
        eng.close()
        raise


def _const_spec(model, d, what, seed=3):
    na = (5, 19, 40, 41, N70 - 1) if what == "missing" else ()
    return make_spec(f"gd_{model}_{d}_{what}", model, d, seed=seed + d, lengths=LENGTHS70, irregular=(what == "irregular"), na_rows=na)


# ---- path 1: constant coefficients ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("what", ["regular", "irregular", "missing"])
def test_constant_coefficients(model, d, what):
    spec = _const_spec(model, d, what)
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    _show(f"const {model} d={d} {what}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_groups"] == 2
    assert info["n_tracks"] == 70
    _compare(got, _ref(("const", model, d, what), pb, spec["par"], seed=11, n_draws=5), f"const {model} d={d} {what}")
    state = np.ones(pb.n, dtype=bool)
    state[pb.seg_start] = False
    assert np.all(np.isnan(got[:, ~state])) and np.all(np.isfinite(got[:, state]))


# ---- a lattice handle -----------------------------------------------------------------------------------------------------------
def _written_out(ID, times, obs, step):
    """the same tracks with the absent fixes written out as NA rows; rows[i] = the written-out row of caller row i.  A track's first
    interval is no step of the filter (the initial state IS the prediction for the second row, whenever that row is), so it is not on
    the lattice and nothing is written out inside it: rows between the first two would be prediction steps the model does not take."""
    out_id, out_t, out_obs, rows = [], [], [], []
    n_out = 0
    for k in np.unique(ID):
        sel = np.flatnonzero(ID == k)
        t = times[sel]
        pos = np.zeros(len(sel), dtype=int)
        pos[1:] = 1 + np.rint((t[1:] - t[1:2]) / step).astype(int)
        m = pos[-1] + 1
        o = np.full((m, obs.shape[1]), np.nan)
        o[pos] = obs[sel]
        out_id += [k] * m
        out_t += list(np.r_[t[0], t[1:2] + step * np.arange(m - 1)])
        out_obs.append(o)
        rows += list(n_out + pos)
        n_out += m
    return np.array(out_id), np.array(out_t), np.vstack(out_obs), np.array(rows)


@pytest.mark.parametrize("model", MODELS)
def test_a_lattice_handle_samples_the_padded_rows_too(model):
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks(model, 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
    pb = capi.Problem(model, ID, times, obs)
    par = _par(model, 2, np.random.default_rng(2))
    got, info, eng = _run(pb, par)
    eng.close()
    _show(f"lattice {model}", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] > pb.n
    ID2, t2, obs2, rows = _written_out(ID, times, obs, 0.5)
    pb2 = capi.Problem(model, ID2, t2, obs2)
    assert pb2.n == info["n_rows_tiled"] and pb2.n_seg == pb.n_seg                 # the written-out rows ARE the handle's lattice
    ref = _ref(("lattice", model), pb2, par, seed=11, n_draws=5)
    _compare(got, ref[:, rows, :], f"lattice {model}")


# ---- path 2, per-row H, a general P0 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_force_dense(model):
    spec = _const_spec(model, 2, "missing")
    pb = problem_from_spec(spec, flags=capi.FLAG_FORCE_DENSE)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    _show(f"dense {model}", info)
    assert info["path"] == PATH_DENSE and info["n_groups"] == 2
    _compare(got, _ref(("const", model, 2, "missing"), pb, spec["par"], seed=11, n_draws=5), f"dense {model}")


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    spec = make_spec(f"gd_hp_{model}_{d}", model, d, seed=21, lengths=LENGTHS70, with_H=True, with_P0=True, na_rows=(3, 19, 40, 41))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    _show(f"H P0 {model} d={d}", info)
    # with H_array a batch of eight tracks or more sits on the tiles of the full-covariance lane = track kernels (reported as path 1);
    # the records come from dense_kernel on those tiles, per-row H and the general P0 included
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n and info["n_tracks"] == 70
    _compare(got, _ref(("hp", model, d), pb, spec["par"], seed=11, n_draws=5), f"H P0 {model} d={d}")


# ---- path 3: row-varying coefficients, 150 tracks ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_tv_route_with_150_tracks(model, monkeypatch):
    from test_gpu_smooth_layouts import _tv_many
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = _tv_many(model, seed=29)
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    _show(f"tv {model}", info)
    assert info["path"] == PATH_TV and info["n_tracks"] == 150 and info["const_coeff"] == 0
    # three groups of lanes by length: 1 MiB of records makes each group of the CTCRW its own chunk (test_gpu_smooth_layouts.py)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.smooth_draws(spec["par"], 5, seed=11)
    eng.close()
    assert np.array_equal(got, many, equal_nan=True)
    _compare(got, _ref(("tv", model), pb, spec["par"], seed=11, n_draws=5), f"tv {model}")


# ---- column pairs and shards ------------------------------------------------------------------------------------------------------
def test_uncoupled_ctcrw_d4_runs_as_column_pairs_with_global_state_columns():
    spec = make_spec("gd_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70, na_rows=(2, 19))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    _show("pairs", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == 2 * pb.n and info["sdim"] == 8
    _compare(got, _ref("pairs", pb, spec["par"], seed=11, n_draws=5), "pairs")
    assert not np.array_equal(got[:, :, :4], got[:, :, 4:], equal_nan=True)      # the second pair has streams of its own
    # the pairs of one device leave their draws in HBM too
    import torch
    out = torch.zeros((5, 8, pb.n), dtype=torch.float64, device="cuda:0")
    dev = eng.smooth_draws(spec["par"], 5, seed=11, out=out)
    torch.cuda.synchronize()
    eng.close()
    assert np.array_equal(dev.cpu().numpy(), got, equal_nan=True)


@pytest.mark.parametrize("layout", ["const", "pairs", "tv"])
def test_two_shards_are_bitwise_the_single_device_handle(layout, monkeypatch):
    if layout == "tv":
        from test_gpu_smooth_layouts import _tv_many
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = _tv_many("OU_SSM", seed=37)
    elif layout == "pairs":
        spec = make_spec("gd_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70, na_rows=(2, 19))
    else:
        spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    one, info1, e1 = _run(pb, spec["par"])
    e1.close()
    two, info2, e2 = _run(pb, spec["par"], devices=[0, 0])
    _show(f"shards {layout}", info2)
    assert info2["n_devices"] == 2 and info1["n_devices"] <= 1
    assert np.array_equal(one, two, equal_nan=True)
    import torch
    out = torch.zeros((5, pb.sdim, pb.n), dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.EngineError) as ei:                                   # DEVICE_OUT on a multi-device parent
        e2.smooth_draws(spec["par"], 5, seed=11, out=out)
    e2.close()
    assert ei.value.status == ERR_ARG


# ---- invariance, all bitwise ------------------------------------------------------------------------------------------------------
def test_budget_chunks_on_six_ragged_groups_and_draw_batches_are_bitwise():
    # the batch of test_gpu_smooth_layouts.py::test_chunks_on_ragged_tiled_groups_are_bitwise: 1 MiB = 131072 doubles cuts the
    # records into three chunks and, at ~10^4 rows x 4 columns, the five draws into batches of three and two
    rng = np.random.default_rng(31)
    lengths = np.r_[rng.integers(71, 90, 64), rng.integers(45, 61, 63), [60], rng.integers(10, 16, 64), rng.integers(3, 8, 64),
                    rng.integers(2, 4, 64), [1, 2, 5, 1, 3]]
    lengths = [int(v) for v in rng.permutation(lengths)]
    starts = np.r_[0, np.cumsum(lengths)]
    k5 = next(k for k, L in enumerate(lengths) if L >= 5)
    spec = make_spec("gd_chunks", "CTCRW", 2, seed=31, lengths=lengths, irregular=True,
                     na_rows=(int(starts[k5]) + 2, int(starts[k5]) + 3, int(starts[k5 + 1]) - 1))
    pb = problem_from_spec(spec)
    one, info, eng = _run(pb, spec["par"])
    _show("chunks ragged", info)
    assert info["path"] == PATH_ISO and info["n_groups"] == 6 and 131072 // (4 * pb.n) in (1, 2, 3, 4)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.smooth_draws(spec["par"], 5, seed=11)
    import torch
    out = torch.zeros((5, 4, pb.n), dtype=torch.float64, device="cuda:0")          # ... and the batches written in place in HBM
    dev = eng.smooth_draws(spec["par"], 5, seed=11, out=out)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):                                                # eight-byte elements that are no doubles
        eng.smooth_draws(spec["par"], 5, seed=11, out=torch.zeros((5, 4, pb.n), dtype=torch.int64, device="cuda:0"))
    eng.close()
    assert np.array_equal(one, many, equal_nan=True) and np.array_equal(dev.cpu().numpy(), one, equal_nan=True)
    _compare(one, _ref("chunks", pb, spec["par"], seed=11, n_draws=5), "chunks ragged")


@pytest.mark.parametrize("model", MODELS)
def test_draw_numbering_device_output_and_repeatability(model):
    import torch
    spec = _const_spec(model, 2, "missing")
    pb = problem_from_spec(spec)
    whole, info, eng = _run(pb, spec["par"], n_draws=8, seed=5)
    a = eng.smooth_draws(spec["par"], 4, seed=5, draw0=0)
    b = eng.smooth_draws(spec["par"], 4, seed=5, draw0=4)
    assert np.array_equal(whole, np.concatenate([a, b]), equal_nan=True)           # [0, 8) = [0, 4) + [4, 8)
    again = eng.smooth_draws(spec["par"], 8, seed=5)
    assert np.array_equal(whole, again, equal_nan=True)                            # two identical calls
    out = torch.zeros((8, pb.sdim, pb.n), dtype=torch.float64, device="cuda:0")
    dev = eng.smooth_draws(spec["par"], 8, seed=5, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), whole, equal_nan=True)                # DEVICE_OUT copied back
    other = eng.smooth_draws(spec["par"], 1, seed=6)
    eng.close()
    assert not np.array_equal(other[0], whole[0], equal_nan=True)
    # draws 5 ... 7 sit in a second chunk of the grid's second dimension: against the reference too
    _compare(whole[5:], _ref(("numbering", model), pb, spec["par"], seed=5, draw0=5, n_draws=3), f"numbering {model}")


def test_a_lattice_handle_leaves_its_draws_in_hbm_on_the_callers_rows():
    import torch
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks("CTCRW", 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = _par("CTCRW", 2, np.random.default_rng(2))
    host, info, eng = _run(pb, par)
    assert info["n_rows_tiled"] > pb.n
    out = torch.zeros((5, 4, pb.n), dtype=torch.float64, device="cuda:0")
    dev = eng.smooth_draws(par, 5, seed=11, out=out)
    torch.cuda.synchronize()
    eng.close()
    assert np.array_equal(dev.cpu().numpy(), host, equal_nan=True)


def test_the_column_pairs_of_a_lattice_handle_gather_into_the_parents_matrices():
    import torch
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks("CTCRW", 4, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = _par("CTCRW", 4, np.random.default_rng(2))
    host, info, eng = _run(pb, par)
    _show("lattice pairs", info)
    assert info["path"] == PATH_ISO and info["sdim"] == 8 and info["n_rows_tiled"] > 2 * pb.n     # two pairs, each on the lattice
    out = torch.zeros((5, 8, pb.n), dtype=torch.float64, device="cuda:0")
    dev = eng.smooth_draws(par, 5, seed=11, out=out)
    torch.cuda.synchronize()
    eng.close()
    assert np.array_equal(dev.cpu().numpy(), host, equal_nan=True)
    ID2, t2, obs2, rows = _written_out(ID, times, obs, 0.5)
    pb2 = capi.Problem("CTCRW", ID2, t2, obs2)
    assert 2 * pb2.n == info["n_rows_tiled"]
    _compare(host, _ref("lattice pairs", pb2, par, seed=11, n_draws=5)[:, rows, :], "lattice pairs")


# ---- isolation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["const", "tv"])
def test_a_draws_call_leaves_eval_and_smooth_as_they_were(layout, monkeypatch):
    if layout == "tv":
        from test_gpu_smooth_layouts import _tv_many
        monkeypatch.setenv("SSDE_NO_COLVAR", "1")
        monkeypatch.setenv("SSDE_NO_DRIFT", "1")
        spec = _tv_many("CTCRW", seed=29)
    else:
        spec = _const_spec("CTCRW", 2, "missing")
    pb = problem_from_spec(spec)
    par = np.array(spec["par"], dtype=np.float64)
    par_b = par.copy(); par_b[1] += 0.01
    eng = capi.Engine(pb)
    va, ga = eng.eval(par, order=1)
    sm = eng.smooth(par)
    vb, gb = eng.eval(par_b, order=1)                                              # the memo now holds par_b
    before = eng.info()
    eng.smooth_draws(par, 5, seed=11)
    after = eng.info()
    assert after["n_evals"] == before["n_evals"] and after["n_memo_hits"] == before["n_memo_hits"]
    vb2, gb2 = eng.eval(par_b, order=1)                                            # still the memo's: a hit, as after ssde_smooth
    assert eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1 and vb2 == vb and np.array_equal(gb2, gb)
    va2, ga2 = eng.eval(par, order=1)                                              # evaluated afresh
    assert eng.info()["n_evals"] > before["n_evals"] and eng.info()["n_memo_hits"] == before["n_memo_hits"] + 1
    assert va2 == va and np.array_equal(ga2, ga)
    sm2 = eng.smooth(par)
    eng.close()
    for k in ("mean", "cov", "resid"):
        assert np.array_equal(sm[k], sm2[k], equal_nan=True), k


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_unserved_models_and_bad_arguments():
    for sp in (make_spec("gd_ou", "OU", 1, seed=201, lengths=[9, 2, 14]), make_spec("gd_cir", "CIR", 1, seed=221, lengths=[9, 2, 14]),
               eseal_spec("gd_eseal", 211, [14, 9, 11]),
               make_spec("gd_coupled3", "CTCRW", 3, seed=33, lengths=LENGTHS70[:14], with_H=True, na_rows=(2, 19))):
        eng = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            eng.smooth_draws(sp["par"], 5)
        eng.close()
        assert ei.value.status == ERR_MODEL, sp["name"]
    spec = _const_spec("CTCRW", 2, "regular")
    eng = capi.Engine(problem_from_spec(spec))
    for kw in (dict(n_draws=0), dict(n_draws=1, draw0=-1), dict(n_draws=2, draw0=(1 << 28) - 2)):
        with pytest.raises(capi.EngineError) as ei:
            eng.smooth_draws(spec["par"], **kw)
        assert ei.value.status == ERR_ARG, kw
    last = eng.smooth_draws(spec["par"], 1, draw0=(1 << 28) - 2)                  # the last draw number there is
    eng.close()
    assert np.isfinite(last[0, 1]).all()


# ---- the det F <= 0 corner ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_negative_p0_follows_the_reference(model):
    from smoothsde_amd.synth import simulate
    ID, times, obs = simulate(model, 70, 12, 1, seed=4)
    keep = np.ones(len(ID), dtype=bool)
    keep[2 * 12 + 1:3 * 12] = False; keep[4 * 12 + 2:5 * 12] = False
    ID, times, obs = ID[keep], times[keep], obs[keep]
    obs[11] = np.nan
    sdim = 2 if model == "CTCRW" else 1
    P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
    par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
    pb = capi.Problem(model, ID, times, obs, P0=P0)
    got, info, eng = _run(pb, par)
    eng.close()
    _show(f"negative P0 {model}", info)
    assert info["path"] == PATH_ISO
    _compare(got, _ref(("negp0", model), pb, par, seed=11, n_draws=5), f"negative P0 {model}")


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_sde_sample_states_on_a_ctcrw_with_tau_smooth_in_x():
    from smoothsde_amd.sde import SDE
    rng = np.random.default_rng(61)
    ID, times, obs = _tracks(rng, "CTCRW", 2, LENGTHS70, irregular=True)
    n = len(ID)
    obs[[5, 19]] = np.nan
    data = {"ID": ID, "time": times, "x": np.clip((np.sin(np.linspace(0, 7, n)) + 1) / 2, 0, 1), "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~x", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.05, -0.05, 0.3, 0.4, 0.1])
    sde.setup()
    got = sde.sample_states(3)
    par = sde._current_par_full()
    direct = sde.engine_.smooth_draws(par, 3)
    info = sde.engine_.info()
    _show("SDE tau ~ x", info)
    assert got.shape == (3, n, 4) and np.array_equal(got, direct, equal_nan=True)
    assert info["const_coeff"] == 0 and info["path"] == PATH_TV
    _compare(got, draws_ref(sde.problem_, par, seed=0, n_draws=3), "SDE tau ~ x")
    with pytest.raises(NotImplementedError):
        SDE(data={"ID": np.zeros(10), "time": np.arange(10.0), "z": np.exp(rng.standard_normal(10))}, type="CIR", response="z").sample_states(2)


# ---- one statistical check ------------------------------------------------------------------------------------------------------------
def test_the_mean_over_4096_draws_is_the_smoothed_mean():
    """Each coordinate's mean over K = 4096 independent draws has standard deviation sqrt(V_ii / K), V the smoothed covariance:
    6 of them bound it (a 6 sigma event over 4 x 11 x 4 coordinates has probability ~ 3.5e-7; the seed is fixed, so the outcome is
    deterministic anyway)."""
    spec = make_spec("gd_stat", "CTCRW", 2, seed=71, lengths=[12] * 4, na_rows=(5,))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    K = 4096
    draws = eng.smooth_draws(spec["par"], K, seed=123)
    sm = eng.smooth(spec["par"])
    eng.close()
    state = np.ones(pb.n, dtype=bool)
    state[pb.seg_start] = False
    m = draws[:, state, :].mean(axis=0)
    sd = np.sqrt(np.einsum("ncc->nc", sm["cov"][state]) / K)
    z = np.abs(m - sm["mean"][state]) / sd
    print("STAT max z", z.max())
    assert np.all(z <= 6.0), z.max()
