"""CPU suite: the numpy definition of ssde_simulate_rows (tests/simrows_ref.py) against ssde_simulate's restatement
(tests/sim_ref.py) where the two describe the same batch, one fixed-seed distribution check of its transitions, every SSDE_ERR_ARG
case of the C call through the library -- none of them needs a device --, and SDE.check_post's pooling against numpy."""
import ctypes as C

import numpy as np
import pytest

from sim_ref import simulate_ref
from simrows_ref import n_par, simrows_ref
from smoothsde_amd import capi
from smoothsde_amd.sde import SDE


def _const_blocks(model, d, mu, p1, p2=None):
    q = n_par(model, d)
    coeff = list(np.broadcast_to(np.asarray(mu, dtype=np.float64), (d,))) + [np.log(p1)] + ([np.log(p2)] if q == d + 2 else [])
    return [None] * q, [None] * q, np.array([0] * d + [1] * (q - d), dtype=np.uint8), np.array([coeff])


@pytest.mark.parametrize("model", ["CTCRW", "OU", "OU_SSM", "BM", "BM_SSM"])
def test_replicate_zero_on_a_regular_grid_is_ssde_simulate(model):
    """constant parameters, one dt, replicate number 0: the counter (row, track, 0, stream) is ssde_simulate's, so the two
    restatements give the same batch up to the rounding of the factors' forms (expm1 against 1 - exp)"""
    M, T, d, dt = 5, 40, 2, 0.7
    kw = dict(mu=[0.3, -0.2], tau=1.5, nu=0.8, kappa=0.6, sigma=0.9, sigma_obs=0.1, dt=dt, z0=[0.5, -1.0], seed=12345)
    _, obs, n = simulate_ref(model, M, T, d, **kw)
    p1, p2 = {"CTCRW": (1.5, 0.8), "OU": (1.5, 0.6), "OU_SSM": (1.5, 0.6), "BM": (0.9, None), "BM_SSM": (0.9, None)}[model]
    X_fe, X_re, link, coeff = _const_blocks(model, d, kw["mu"], p1, p2)
    times = np.tile(dt * np.arange(1, T + 1), M)
    with_error = model in ("CTCRW", "OU_SSM", "BM_SSM")
    out = simrows_ref(model, d, np.arange(M + 1) * T, times, X_fe, X_re, link, coeff, sigma_obs=0.1 if with_error else None,
                      z0=kw["z0"], seed=kw["seed"], rep0=0, n_rep=1)
    gap = np.max(np.abs(out["obs"][0] - obs))
    print(f"simrows_ref against sim_ref, {model}: {gap:.3g}")
    assert gap <= 1e-12 * (1.0 + np.max(np.abs(obs)))
    # and another replicate number is another batch
    other = simrows_ref(model, d, np.arange(M + 1) * T, times, X_fe, X_re, link, coeff, z0=kw["z0"], seed=kw["seed"], rep0=1, n_rep=1)
    assert np.max(np.abs(other["obs"][0] - obs)) > 0.1


def test_one_step_moments_of_ou_and_ctcrw():
    """4096 one-step transitions (4096 replicates of a two-row track) from a fixed seed: sample mean and variance within 5 standard
    errors of the exact moments -- se(mean) = sd / sqrt(N), se(var) = var sqrt(2 / (N - 1)) for a normal sample"""
    N, dt, z0 = 4096, 0.8, 1.3
    for model, p1, p2, mu in (("OU", 1.5, 0.6, 0.4), ("CTCRW", 1.5, 0.8, 0.4)):
        X_fe, X_re, link, coeff = _const_blocks(model, 1, [mu], p1, p2)
        y = simrows_ref(model, 1, [0, 2], [1.0, 1.0 + dt], X_fe, X_re, link, coeff, z0=z0, seed=2024, n_rep=N)["obs"][:, 1, 0]
        e = np.exp(-dt / p1)
        if model == "OU":
            mean, var = e * z0 + (1 - e) * mu, p2 * (1 - e * e)
        else:
            beta, sigma = 1 / p1, 2 * p2 / np.sqrt(np.pi * p1)
            mean = z0 + mu * dt + (0.0 - mu) / beta * (1 - e)
            var = (sigma / beta) ** 2 * (dt + (1 - e * e) / (2 * beta) - 2 * (1 - e) / beta)
        assert abs(np.mean(y) - mean) <= 5 * np.sqrt(var / N), (model, np.mean(y), mean)
        assert abs(np.var(y, ddof=1) - var) <= 5 * var * np.sqrt(2.0 / (N - 1)), (model, np.var(y, ddof=1), var)


# ---- SSDE_ERR_ARG: every check precedes the device ---------------------------------------------------------------------------------
class _Desc:
    """a valid OU descriptor (one column, two tracks of 3 and 2 rows, mu on two fixed columns, tau on one random column) and what keeps it alive"""

    def __init__(self):
        self.row0 = np.array([0, 3, 5], dtype=np.int64)
        self.times = np.array([0.5, 1.0, 2.0, 0.1, 0.4])
        self.x_mu = np.asfortranarray(np.column_stack([np.ones(5), np.linspace(-1, 1, 5)]))
        self.x_tau = np.asfortranarray(np.linspace(0, 1, 5)[:, None])
        self.kf = np.array([2, 1, 1], dtype=np.int32)
        self.kr = np.array([0, 1, 0], dtype=np.int32)
        self.xf = (C.c_void_p * 3)(self.x_mu.ctypes.data, None, None)
        self.xr = (C.c_void_p * 3)(None, self.x_tau.ctypes.data, None)
        self.link = np.array([0, 1, 1], dtype=np.uint8)
        self.coeff = np.array([[0.1, 0.2, 0.0, 0.3, -0.2], [0.0, 0.1, 0.1, 0.2, -0.1]])
        self.so = np.array([0.1, 0.0])
        self.thr = np.array([0.5, np.inf])
        d = capi.SsdeSimrowsDesc()
        d.abi_version, d.device, d.model, d.n_dim, d.n_par, d.n, d.n_tracks = capi.ABI_VERSION, -1, capi.MODEL_CODES["OU"], 1, 3, 5, 2
        d.row0 = self.row0.ctypes.data_as(C.POINTER(C.c_int64))
        d.times = self.times.ctypes.data_as(C.POINTER(C.c_double))
        d.ncol_fe, d.x_fe = self.kf.ctypes.data_as(C.POINTER(C.c_int32)), self.xf
        d.ncol_re, d.x_re = self.kr.ctypes.data_as(C.POINTER(C.c_int32)), self.xr
        d.link, d.coeff = self.link.ctypes.data_as(C.POINTER(C.c_uint8)), self.coeff.ctypes.data_as(C.POINTER(C.c_double))
        d.n_coeff_rows, d.n_coef = 2, 5
        d.sigma_obs = self.so.ctypes.data_as(C.POINTER(C.c_double))
        d.seed, d.rep0, d.n_rep = 7, 0, 2
        d.thr, d.n_thr = self.thr.ctypes.data_as(C.POINTER(C.c_double)), 2
        self.d = d
        self.obs, self.stats = np.zeros(5 * 1 * 2), np.zeros(2 * 7 * 2)

    def call(self, obs=True, stats=True, null_desc=False):
        lib = capi.load_library()
        st = lib.ssde_simulate_rows(None if null_desc else C.byref(self.d), self.obs.ctypes.data if obs else None,
                                    self.stats.ctypes.data if stats else None)
        msg = lib.ssde_last_error(None)
        return st, (msg.decode() if msg else "")


def _null(ptr_type):
    return C.cast(None, ptr_type)


def _set(field, value):
    def f(D):
        setattr(D.d, field, value)
    return f


def _arr(name, index, value):
    def f(D):
        getattr(D, name)[index] = value
    return f


def _k64(D):
    D.big = np.asfortranarray(np.ones((5, 64)))
    D.kf[:] = [64, 64, 64]
    D.kr[:] = 0
    D.xf[0] = D.xf[1] = D.xf[2] = D.big.ctypes.data
    D.xr[1] = None
    D.big_coeff = np.zeros((2, 192))
    D.d.coeff, D.d.n_coef = D.big_coeff.ctypes.data_as(C.POINTER(C.c_double)), 192


ARG_CASES = {
    "wrong abi_version": _set("abi_version", capi.ABI_VERSION + 1),
    "unknown flag": _set("flags", 4),
    "n_dim 0": _set("n_dim", 0),
    "n_dim 9": _set("n_dim", 9),
    "n_par of another model": _set("n_par", 2),
    "n negative": _set("n", -1),
    "n_tracks negative": _set("n_tracks", -1),
    "n_tracks 2^32": _set("n_tracks", 1 << 32),
    "NULL row0": _set("row0", _null(C.POINTER(C.c_int64))),
    "NULL times": _set("times", _null(C.POINTER(C.c_double))),
    "NULL ncol_fe": _set("ncol_fe", _null(C.POINTER(C.c_int32))),
    "NULL ncol_re": _set("ncol_re", _null(C.POINTER(C.c_int32))),
    "NULL x_fe": _set("x_fe", _null(C.POINTER(C.c_void_p))),
    "NULL x_re": _set("x_re", _null(C.POINTER(C.c_void_p))),
    "NULL link": _set("link", _null(C.POINTER(C.c_uint8))),
    "NULL coeff": _set("coeff", _null(C.POINTER(C.c_double))),
    "row0[0] != 0": _arr("row0", 0, 1),
    "row0[n_tracks] != n": _arr("row0", 2, 4),
    "row0 decreases": _arr("row0", 1, 6),
    "dt zero": _arr("times", 1, 0.5),
    "dt negative": _arr("times", 4, 0.05),
    "dt NaN": _arr("times", 1, np.nan),
    "dt inf": _arr("times", 2, np.inf),
    "ncol_fe 0": _arr("kf", 1, 0),
    "ncol_re negative": _arr("kr", 0, -1),
    "K over the cap": _arr("kr", 1, 65),
    "NULL fixed block with two columns": _arr("kf", 1, 2),
    "NULL random block with a column": _arr("kr", 2, 1),
    "link 2": _arr("link", 1, 2),
    "n_coef not the blocks' sum": _set("n_coef", 6),
    "n_coef over SSDE_SIMROWS_MAX_COEF": _k64,
    "rep0 negative": _set("rep0", -1),
    "n_rep 0": _set("n_rep", 0),
    "rep0 + n_rep = 2^28": _set("rep0", (1 << 28) - 2),
    "n_coeff_rows neither 1 nor n_rep": _set("n_rep", 3),
    "coeff NaN": _arr("coeff", (1, 2), np.nan),
    "coeff inf": _arr("coeff", (0, 0), np.inf),
    "sigma_obs negative": _arr("so", 1, -0.1),
    "sigma_obs NaN": _arr("so", 0, np.nan),
    "sigma_obs inf": _arr("so", 0, np.inf),
    "n_thr 9": _set("n_thr", 9),
    "n_thr negative": _set("n_thr", -1),
    "thr NULL with n_thr > 0": _set("thr", _null(C.POINTER(C.c_double))),
    "thr negative": _arr("thr", 0, -1.0),
    "thr NaN": _arr("thr", 1, np.nan),
}


@pytest.mark.parametrize("name", sorted(ARG_CASES))
def test_err_arg_before_the_device(name):
    D = _Desc()
    ARG_CASES[name](D)
    st, msg = D.call()
    assert st == 1 and msg.startswith("ssde_simulate_rows: "), (name, st, msg)


def test_err_arg_null_descriptor_outputs_and_z0():
    D = _Desc()
    assert D.call(null_desc=True)[0] == 1
    st, msg = D.call(obs=False, stats=False)
    assert st == 1 and "both outputs" in msg
    D.d.z0[0] = np.inf
    assert D.call()[0] == 1


@pytest.mark.parametrize("model", ["CIR", "BM_t", "ESEAL_SSM"])
def test_other_models_are_refused_with_the_references_message(model):
    D = _Desc()
    D.d.model = capi.MODEL_CODES[model]
    st, msg = D.call()
    assert st == 2 and "Simulation not implemented yet" in msg, (st, msg)


def test_a_valid_descriptor_passes_the_checks():
    """... and then needs a device: status 0 with one, SSDE_ERR_NODEVICE (4) without -- never a CPU fallback"""
    import torch
    D = _Desc()
    st, msg = D.call()
    assert st == (0 if torch.cuda.is_available() else 4), (st, msg)
    D2 = _Desc()
    D2.d.n_tracks, D2.d.n = 0, 0
    D2.row0[:] = 0
    assert D2.call()[0] == 0                             # no track: nothing to do, and nothing touched


def test_the_binding_raises_with_the_status():
    with pytest.raises(capi.EngineError) as e:
        capi.simulate_rows("OU", 1, [0, 2], [1.0, 1.0], [None] * 3, [None] * 3, [0, 1, 1], np.zeros((1, 3)))
    assert e.value.status == 1 and "time step" in str(e.value)
    with pytest.raises(capi.EngineError) as e:
        capi.simulate_rows("CIR", 1, [0, 2], [1.0, 2.0], [None] * 3, [None] * 3, [1, 1, 1], np.zeros((1, 3)))
    assert e.value.status == 2


# ---- SDE.check_post's pooling ---------------------------------------------------------------------------------------------------
def test_check_post_pooling_against_numpy():
    """the per-track sums of three replicate data sets (numpy) pooled by SDE._pool_check_stats against the statistics computed
    directly from the increments of all tracks put together"""
    rng = np.random.default_rng(3)
    row0 = np.array([0, 40, 41, 41, 90, 120])            # a one-row and an empty track among them
    d, thr = 2, np.array([0.8, 2.0])
    reps = [np.cumsum(rng.standard_normal((120, d)) * [1.0, 0.5] + [0.1, -0.2], axis=0) for _ in range(3)]
    st = np.stack([SDE._track_check_sums(y, row0, thr) for y in reps])
    pooled = SDE._pool_check_stats(st, row0, d, len(thr))
    assert pooled.shape == (3 * d + 2 + 2, 3) and SDE._check_names(d, 2)[:3] == ["mean_incr1", "sd_incr1", "acf1_incr1"]
    for k, y in enumerate(reps):
        D = [np.diff(y[row0[t]:row0[t + 1]], axis=0) for t in range(5) if row0[t + 1] - row0[t] >= 2]
        allD = np.concatenate(D)
        L = np.sqrt(np.sum(allD ** 2, axis=1))
        N, N2 = len(allD), sum(len(x) - 1 for x in D)
        for c in range(d):
            m, var = allD[:, c].mean(), allD[:, c].var(ddof=1)
            cross = sum(np.sum(x[1:, c] * x[:-1, c]) for x in D)
            assert abs(pooled[3 * c, k] - m) <= 1e-13 and abs(pooled[3 * c + 1, k] - np.sqrt(var)) <= 1e-13
            assert abs(pooled[3 * c + 2, k] - (cross / N2 - m * m) / (var * (N - 1) / N)) <= 1e-12
            assert abs(pooled[3 * c + 2, k]) < 0.3                   # independent increments: no autocorrelation to speak of
        assert abs(pooled[3 * d, k] - L.mean()) <= 1e-13 and pooled[3 * d + 1, k] == L.max()
        assert np.array_equal(pooled[3 * d + 2:, k], [np.mean(L <= r) for r in thr])
    # a NaN track makes its replicate NaN, and no other
    st[1, 0, :] = np.nan
    pooled = SDE._pool_check_stats(st, row0, d, len(thr))
    assert np.isnan(pooled[:, 1]).all() and not np.isnan(pooled[:, [0, 2]]).any()
