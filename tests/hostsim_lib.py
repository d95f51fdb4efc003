"""ctypes loader of the test-only host build of the kernel arithmetic (tests/hostsim)."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
_LIB = None
_dp = C.POINTER(C.c_double)
_lp = C.POINTER(C.c_int64)
# the twins' common arguments (tests/hostsim/hostsim_records.hpp: TWIN_PARAMS), after model and d
TWIN_ARGTYPES = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _lp, _lp, _dp, _dp, _dp, _dp, C.c_double, _dp, _dp]


_LIBS = {}


def load_lib(name, protos=None):
    """tests/hostsim/<name>, after `make` there (which compiles nothing in a built tree), loaded once; protos: {function: (restype,
    argtypes)}"""
    if name not in _LIBS:
        alt = os.environ.get("SSDE_ORACLE_LIBDIR") if name == "libhostsim.so" else None      # tools/sanitize_cpu.sh: the sanitizer build
        if not alt:
            subprocess.run(["make", "-s", "-C", _DIR, name], check=True)
        lib = C.CDLL(os.path.join(alt or _DIR, name))
        for f, (res, args) in (protos or {}).items():
            getattr(lib, f).restype, getattr(lib, f).argtypes = res, args
        _LIBS[name] = lib
    return _LIBS[name]


def ptr(a, t=None):
    """the ctypes pointer of an array (None stays NULL)"""
    return None if a is None else a.ctypes.data_as(t or (_lp if a.dtype == np.int64 else _dp))


def twin_args(pb, par):
    """A problem as the twins take it: (arguments in TWIN_ARGTYPES' order, the arrays they point to -- keep them alive over the
    call).  The linear predictors are formed here (refimpl.linear_predictor), a0 and P0 default as the engine's create path sets
    them."""
    import torch
    from refimpl import linear_predictor
    from smoothsde_amd.capi import MODEL_CODES
    d, sd, n = pb.n_dim, pb.sdim, pb.n
    par = np.asarray(par, dtype=np.float64)
    parmat = np.ascontiguousarray(linear_predictor(pb, torch.as_tensor(par)).detach().numpy())          # n x q
    row0 = np.ascontiguousarray(pb.seg_start, dtype=np.int64)
    nrows = np.diff(np.append(pb.seg_start, n)).astype(np.int64)
    z = (lambda a: 2 * a) if pb.model == "CTCRW" else (lambda a: a)
    if pb.P0 is None:
        P0 = np.diag([1.0, 10.0] * d) if pb.model == "CTCRW" else 10.0 * np.eye(d)
    else:
        P0 = np.asarray(pb.P0, dtype=np.float64)
    p0f = np.ascontiguousarray(P0.ravel(order="F"))
    if pb.a0 is None:
        a0 = np.zeros((pb.n_seg, sd))
        for a in range(d):
            a0[:, z(a)] = pb.obs[row0, a]
    else:
        a0 = np.ascontiguousarray(pb.a0, dtype=np.float64)
    harr = None if pb.H is None else np.ascontiguousarray(np.moveaxis(np.asarray(pb.H, dtype=np.float64), 2, 0))   # n x d x d
    keep = (parmat, row0, nrows, p0f, a0, harr)
    return [MODEL_CODES[pb.model], d, int(pb.na_mode == 1), n, pb.n_seg, ptr(row0), ptr(nrows), ptr(pb.times), ptr(pb.obs),
            ptr(parmat), ptr(harr), float(np.exp(par[0]) ** 2), ptr(p0f), ptr(a0)], keep


def load():
    global _LIB
    if _LIB is None:
        lib = load_lib("libhostsim.so")
        lib.hostsim_kalman_iso.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _lp, _lp,
                                           _dp, _dp, _dp, _dp, _dp]
        lib.hostsim_kalman_iso.restype = C.c_int
        lib.hostsim_direct.argtypes = [C.c_int] + [C.c_double] * 6 + [_dp]
        lib.hostsim_direct.restype = C.c_double
        _ipt = C.POINTER(C.c_int)
        lib.hostsim_kalman_tv.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _lp, _lp, _dp, _dp, _dp,
                                          C.c_int, C.c_int, _ipt, _ipt, _dp, C.c_double, _dp, _dp, _dp]
        lib.hostsim_kalman_tv.restype = C.c_int
        lib.hostsim_kalman_adj.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, _lp, _lp, _dp, _dp, _dp,
                                           C.c_int, C.c_double, _dp, _dp, _dp, _dp]
        lib.hostsim_kalman_adj.restype = C.c_int
        lib.hostsim_kalman_adj_full.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int64, _lp, _lp, _dp, _dp, _dp,
                                                C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp]
        lib.hostsim_kalman_adj_full.restype = C.c_int
        lib.hostsim_smooth.argtypes = TWIN_ARGTYPES + [_dp, _dp, _dp]
        lib.hostsim_smooth.restype = C.c_int
        lib.hostsim_knobs.argtypes = [C.c_int, C.c_char_p, C.c_int]
        lib.hostsim_knobs.restype = C.c_int
        _ip = C.POINTER(C.c_int)
        lib.hostsim_closed_loop_rho.argtypes = [C.c_int] + [C.c_double] * 4 + [_dp]
        lib.hostsim_closed_loop_rho.restype = C.c_double
        lib.hostsim_window_params.argtypes = [C.c_int] + [C.c_double] * 3 + [_dp, _dp]
        lib.hostsim_window_plan.argtypes = [_dp, _ip, _dp, C.c_int, _dp]
        lib.hostsim_window_geometry.argtypes = [_dp, _ip, _dp, C.c_int, C.c_int, _dp, _dp]
        lib.hostsim_warmup.argtypes = [C.c_double] + [C.c_int] * 4
        lib.hostsim_warmup.restype = C.c_int64
        lib.hostsim_balanced_window0.argtypes = [C.c_int] * 5
        lib.hostsim_balanced_window0.restype = C.c_int
        lib.hostsim_hess_first_warmup.argtypes = [C.c_int] * 3
        lib.hostsim_hess_next_warmup.argtypes = [C.c_int] * 3
        _i32 = C.POINTER(C.c_int32)
        lib.hostsim_hess_item_plan.argtypes = [_i32, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _i32, C.c_int64]
        lib.hostsim_hess_item_plan.restype = C.c_int64
        lib.hostsim_adj_row_bytes.argtypes = [C.c_int]
        lib.hostsim_adj_row_offset.argtypes = lib.hostsim_adj_window_span.argtypes = [C.c_int, C.c_int]
        lib.hostsim_adj_row_bytes.restype = lib.hostsim_adj_row_offset.restype = lib.hostsim_adj_window_span.restype = C.c_int64
        lib.hostsim_policy_new.argtypes = [C.c_int, C.c_int]
        lib.hostsim_policy_new.restype = C.c_void_p
        lib.hostsim_policy_free.argtypes = [C.c_void_p]
        lib.hostsim_policy_begin.argtypes = [C.c_void_p]
        lib.hostsim_policy_attempt.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.hostsim_policy_attempt.restype = C.c_int
        lib.hostsim_policy_end.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.hostsim_policy_end.restype = C.c_int
        lib.hostsim_policy_widen.argtypes = [C.c_void_p, C.c_int]
        lib.hostsim_policy_relax.argtypes = [C.c_void_p]
        lib.hostsim_policy_state.argtypes = [C.c_void_p, _dp]
        _LIB = lib
    return _LIB


def knobs(win_align):
    """The engine's knobs as the current environment sets them (csrc/ssde_knobs.hpp: knobs_from_env): {"SSDE_X": text}."""
    buf = C.create_string_buffer(1 << 14)
    n = load().hostsim_knobs(win_align, buf, len(buf))
    assert 0 < n < len(buf)
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


# ---- the window policy (csrc/ssde_windows.hpp) ----------------------------------------------------------------------------------
# WindowFacts, in the order hostsim.cpp reads them; window = -1: SSDE_WINDOW unset
WINDOW_FACTS = dict(model=4, uniform_dt=1, dt_uniform=1.0, dt_min=1.0, dt_max=1.0, max_chunks=9, want_chunks=8, want_chunks_d=0,
                    glen_max=4000, n_groups=16, use_shared=0, drift=0, cv_adj=0, cv_one_wave=0, chunks_forced=0, window=-1,
                    eta_lo0=0.0, eta_lo1=0.0, eta_hi0=0.0, eta_hi1=0.0, any_dirty=0, quiet_ok=0, lag_ready=0, quiet_window=0,
                    block_rows=4)
WINDOW_EVAL = dict(n_parts=1, can_derive=1, hess_req=0, gain_last=40, gain_usable=1)
GEOMETRY_OUT = ("n_chunks", "window", "t0", "t0_delta", "dual", "n_chunks_d", "t0_d", "lag_K", "s_stat", "quiet_window", "quiet_w",
                "quiet_b0")
POLICY_STATE = ("window_boost", "gave_up", "calm", "cooldown", "probe_from", "probing", "check_floor", "check_max", "last_check",
                "n_retries", "attempt", "max_chunks", "want_chunks", "saved_max_chunks", "saved_want_chunks")
CHUNK_ACTIONS = ("none", "sequential_saving", "sequential", "restore")


def _vec(defaults, over):
    unknown = set(over) - set(defaults)
    assert not unknown, unknown
    return np.array([float(over.get(k, v)) for k, v in defaults.items()])


def closed_loop_rho(model, dt, p1, p2, hobs, p0):
    p0 = np.asarray(p0, dtype=np.float64)
    return load().hostsim_closed_loop_rho(model, dt, p1, p2, hobs, p0.ctypes.data_as(_dp))


def window_params(model, p1, p2, hobs, p0):
    """[tau, beta, sigma, h, p0[3]] at working-scale par[d] = p1, par[d + 1] = p2, decoded as an evaluation decodes them."""
    p0 = np.asarray(p0, dtype=np.float64)
    out = np.zeros(7)
    load().hostsim_window_params(model, p1, p2, hobs, p0.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    return out


def _plan_dict(v):
    return dict(n_chunks=int(v[0]), window=int(v[1]), warmup=int(v[2]), rho=float(v[3]))


def window_plan(consts, params, boost=1, **facts):
    """plan_windows: consts = (WIN_ALIGN, SHARED_U, LAG_A, LAG_KMAX)"""
    f, c, out = _vec(WINDOW_FACTS, facts), np.asarray(consts, dtype=np.int32), np.zeros(4)
    load().hostsim_window_plan(f.ctypes.data_as(_dp), c.ctypes.data_as(C.POINTER(C.c_int)), params.ctypes.data_as(_dp), boost,
                               out.ctypes.data_as(_dp))
    return _plan_dict(out)


def window_geometry(consts, params, boost=1, gave_up=False, ev=None, **facts):
    """plan_windows, then window_geometry: the geometry's fields, with `first` (the plan) and `plan` (the plan in force)"""
    f, c, out = _vec(WINDOW_FACTS, facts), np.asarray(consts, dtype=np.int32), np.zeros(20)
    e = _vec(WINDOW_EVAL, ev or {})
    load().hostsim_window_geometry(f.ctypes.data_as(_dp), c.ctypes.data_as(C.POINTER(C.c_int)), params.ctypes.data_as(_dp), boost,
                                   int(gave_up), e.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    g = {k: int(v) for k, v in zip(GEOMETRY_OUT, out[8:])}
    g["first"], g["plan"] = _plan_dict(out[:4]), _plan_dict(out[4:8])
    return g


# ---- the Hessian pass's plan (csrc/ssde_windows.hpp: hess_first_warmup, hess_item_plan, hess_next_warmup) -------------------------
def hess_first_warmup(tv_window, knob, win_align):
    """knob: SSDE_HESS_WINDOW as knobs_from_env leaves it (None: unset)"""
    return load().hostsim_hess_first_warmup(tv_window, -1 if knob is None else knob, win_align)


def hess_next_warmup(W, attempt, glen_max):
    return load().hostsim_hess_next_warmup(W, attempt, glen_max)


def hess_item_plan(track_steps, n_pb, W, waves, win_align):
    """the work items as (track, window c, of nc, pair block) rows, in launch order"""
    ts = np.ascontiguousarray(track_steps, dtype=np.int32)
    _i32 = C.POINTER(C.c_int32)
    n = load().hostsim_hess_item_plan(ts.ctypes.data_as(_i32), len(ts), n_pb, W, waves, win_align, None, 0)
    items = np.zeros((max(int(n), 1), 4), dtype=np.int32)
    assert load().hostsim_hess_item_plan(ts.ctypes.data_as(_i32), len(ts), n_pb, W, waves, win_align, items.ctypes.data_as(_i32), n) == n
    return items[:n]


class WindowPolicy:
    """WindowPolicy over one stand-in engine's chunk limits; call() is the loop ssde_eval runs around an evaluation."""

    def __init__(self, max_chunks=9, want_chunks=8):
        self._lib = load()
        self._h = self._lib.hostsim_policy_new(max_chunks, want_chunks)

    def __del__(self):
        self._lib.hostsim_policy_free(self._h)

    def state(self):
        out = np.zeros(len(POLICY_STATE))
        load().hostsim_policy_state(self._h, out.ctypes.data_as(_dp))
        return {k: (float(v) if k.startswith(("check", "last_check")) else int(v)) for k, v in zip(POLICY_STATE, out)}

    def widen(self, factor):
        load().hostsim_policy_widen(self._h, factor)

    def relax(self):
        load().hostsim_policy_relax(self._h)

    def call(self, checks, finite=True, one_window=False, dist=False, replans=False, forced=False):
        """One ssde_eval: `checks` is what each attempt's evaluation shows (a callable of the state, or a sequence whose last
        entry repeats).  Returns the actions asked of the engines, in order, and the number of evaluations run."""
        lib = load()
        lib.hostsim_policy_begin(self._h)
        actions, n = [], 0
        while True:
            chk = checks(self.state()) if callable(checks) else checks[min(n, len(checks) - 1)]
            n += 1
            r = lib.hostsim_policy_attempt(self._h, chk, int(finite), int(one_window), int(dist), int(replans))
            actions.append(CHUNK_ACTIONS[r >> 1])
            if not (r & 1):
                break
            assert n < 100
        actions.append(CHUNK_ACTIONS[lib.hostsim_policy_end(self._h, int(finite), int(forced))])
        return [a for a in actions if a != "none"], n


def smooth(pb, par):
    """The fixed-interval smoother by the lane math of csrc/ssde_smooth.hpp over csrc/ssde_dense.hpp (smooth_record_row ->
    dense_step per state row, then smooth_back_row over the records), one track after the other: what smooth_ref returns,
    {"mean": n x sdim, "cov": n x sdim x sdim, "resid": n x d}, NaN where no state / no update exists."""
    args, keep = twin_args(pb, par)
    d, sd, n = pb.n_dim, pb.sdim, pb.n
    mean, cov, res = np.full((n, sd), np.nan), np.full((n, sd, sd), np.nan), np.full((n, d), np.nan)
    st = load().hostsim_smooth(*args, ptr(mean), ptr(cov), ptr(res))
    assert st == 0
    return {"mean": mean, "cov": cov, "resid": res}


def _parmat_blocks(pb, par):
    """the linear predictors (n x q, column-major) and, per coefficient, (parameter j, index in par, design column)"""
    n, q = pb.n, pb.q
    parmat = np.zeros((n, q), order="F")
    blocks = []
    for j in range(q):
        for src, off, nc in ((pb.X_fe[j], pb.off_fe + pb.fe_off[j], pb.ncol_fe[j]),
                             (pb.X_re[j], pb.off_re + pb.re_off[j], pb.ncol_re[j])):
            for c in range(nc):
                col = np.ones(n) if src is None else src[:, c]
                parmat[:, j] += col * par[off + c]
                blocks.append((j, off + c, col))
    return parmat, blocks


def _p0_iso(pb):
    """P0 of the isotropic lanes: one dimension's block (p11, p12, p22), or the scalar models' variance"""
    if pb.model == "CTCRW":
        return np.array([1.0, 0.0, 10.0]) if pb.P0 is None else np.array([pb.P0[0, 0], pb.P0[0, 1], pb.P0[1, 1]])
    return np.array([10.0, 0, 0]) if pb.P0 is None else np.array([pb.P0[0, 0], 0, 0])


def kalman_adj_full(pb, par):
    """The reverse sweep on the FULL-covariance lanes (csrc/ssde_adj.hpp: AdjFull -- two response columns, per-row H_array or
    sigma_obs^2 I, any P0): nllk (data term) and gradient, the coefficient gradient formed here as X' G."""
    from smoothsde_amd.capi import MODEL_CODES
    lib = load()
    d, q, n = pb.n_dim, pb.q, pb.n
    assert d == 2
    par = np.asarray(par, dtype=np.float64)
    parmat, blocks = _parmat_blocks(pb, par)
    row0 = np.ascontiguousarray(pb.seg_start, dtype=np.int64)
    nrows = np.diff(np.append(pb.seg_start, n)).astype(np.int64)
    sd = 4 if pb.model == "CTCRW" else 2
    if pb.P0 is None:
        P0 = np.diag([1.0, 10.0, 1.0, 10.0]) if pb.model == "CTCRW" else np.diag([10.0, 10.0])
    else:
        P0 = np.asarray(pb.P0, dtype=float)
    p0f = np.asfortranarray(P0).ravel(order="F")
    a0 = None if pb.a0 is None else np.ascontiguousarray(pb.a0)
    harr = None if pb.H is None else np.ascontiguousarray(np.transpose(np.asarray(pb.H, dtype=float), (2, 1, 0)).reshape(n, 4))   # [i][col][row]: column-major d x d per row
    out = np.zeros(2)
    G = np.zeros((n, q), order="F")
    st = lib.hostsim_kalman_adj_full(MODEL_CODES[pb.model], int(pb.na_mode == 1), n, pb.n_seg, row0.ctypes.data_as(_lp),
                                     nrows.ctypes.data_as(_lp), pb.times.ctypes.data_as(_dp), pb.obs.ctypes.data_as(_dp),
                                     parmat.ctypes.data_as(_dp), q, float(par[0]), p0f.ctypes.data_as(_dp),
                                     None if a0 is None else a0.ctypes.data_as(_dp), None if harr is None else harr.ctypes.data_as(_dp),
                                     out.ctypes.data_as(_dp), G.ctypes.data_as(_dp))
    assert st == 0
    grad = np.zeros(pb.n_par_full)
    grad[0] = out[1]
    for j, pidx, col in blocks:
        grad[pidx] += float(col @ G[:, j])
    return out[0], grad


def kalman_adj(pb, par):
    """The same nllk (data term) + gradient by the REVERSE sweep of csrc/ssde_adj.hpp: one forward pass leaving a record
    per row, one backward pass giving d nllk / d par_mat(i, j); the coefficient gradient is X' G, formed here."""
    from smoothsde_amd.capi import MODEL_CODES
    lib = load()
    d, q, n = pb.n_dim, pb.q, pb.n
    par = np.asarray(par, dtype=np.float64)
    parmat, blocks = _parmat_blocks(pb, par)
    row0 = np.ascontiguousarray(pb.seg_start, dtype=np.int64)
    nrows = np.diff(np.append(pb.seg_start, n)).astype(np.int64)
    p0 = _p0_iso(pb)
    a0 = None if pb.a0 is None else np.ascontiguousarray(pb.a0)
    out = np.zeros(2)
    G = np.zeros((n, q), order="F")
    st = lib.hostsim_kalman_adj(MODEL_CODES[pb.model], d, int(pb.na_mode == 1), n, pb.n_seg, row0.ctypes.data_as(_lp),
                                nrows.ctypes.data_as(_lp), pb.times.ctypes.data_as(_dp), pb.obs.ctypes.data_as(_dp),
                                parmat.ctypes.data_as(_dp), q, float(par[0]), p0.ctypes.data_as(_dp),
                                None if a0 is None else a0.ctypes.data_as(_dp), out.ctypes.data_as(_dp), G.ctypes.data_as(_dp))
    assert st == 0
    grad = np.zeros(pb.n_par_full)
    grad[0] = out[1]
    for j, pidx, col in blocks:
        grad[pidx] += float(col @ G[:, j])
    return out[0], grad


def kalman_tv(pb, par):
    """Row-varying-coefficient isotropic Kalman nllk (data term) + gradient over the full parameter
    vector by the arithmetic of csrc/ssde_tv.hpp: linear predictors formed here, one lane per direction."""
    from smoothsde_amd.capi import MODEL_CODES
    lib = load()
    d, q, n = pb.n_dim, pb.q, pb.n
    par = np.asarray(par, dtype=np.float64)
    parmat = np.zeros((n, q), order="F")
    kinds, dims, pidx, wcols = [1], [0], [0], [np.ones(n)]          # log_sigma_obs
    for j in range(q):
        kind, dim = (2, j) if j < d else (3 + (j - d), 0)
        for src, off, nc in ((pb.X_fe[j], pb.off_fe + pb.fe_off[j], pb.ncol_fe[j]),
                             (pb.X_re[j], pb.off_re + pb.re_off[j], pb.ncol_re[j])):
            for c in range(nc):
                col = np.ones(n) if src is None else src[:, c]
                parmat[:, j] += col * par[off + c]
                kinds.append(kind); dims.append(dim); pidx.append(off + c); wcols.append(col)
    nd = len(kinds)
    wmat = np.ascontiguousarray(np.column_stack(wcols))
    row0 = np.ascontiguousarray(pb.seg_start, dtype=np.int64)
    nrows = np.diff(np.append(pb.seg_start, n)).astype(np.int64)
    p0 = _p0_iso(pb)
    a0 = None if pb.a0 is None else np.ascontiguousarray(pb.a0)
    ki, di = np.asarray(kinds, dtype=np.int32), np.asarray(dims, dtype=np.int32)
    out = np.zeros(1 + nd)
    _ipt = C.POINTER(C.c_int)
    st = lib.hostsim_kalman_tv(MODEL_CODES[pb.model], d, int(pb.na_mode == 1), n, pb.n_seg, row0.ctypes.data_as(_lp),
                               nrows.ctypes.data_as(_lp), pb.times.ctypes.data_as(_dp), pb.obs.ctypes.data_as(_dp),
                               parmat.ctypes.data_as(_dp), q, nd, ki.ctypes.data_as(_ipt), di.ctypes.data_as(_ipt),
                               wmat.ctypes.data_as(_dp), float(par[0]), p0.ctypes.data_as(_dp),
                               None if a0 is None else a0.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    assert st == 0
    grad = np.zeros(pb.n_par_full)
    grad[np.asarray(pidx)] = out[1:]
    return out[0], grad


def kalman_iso(pb, par, mask):
    """Constant-coefficient isotropic Kalman nllk + gradient by the kernel arithmetic."""
    from smoothsde_amd.capi import MODEL_CODES
    lib = load()
    d = pb.n_dim
    row0 = np.ascontiguousarray(pb.seg_start, dtype=np.int64)
    nrows = np.diff(np.append(pb.seg_start, pb.n)).astype(np.int64)
    theta = np.zeros(3 + d)
    theta[:len(par)] = par
    p0 = _p0_iso(pb)
    out = np.zeros(4 + d)
    st = lib.hostsim_kalman_iso(MODEL_CODES[pb.model], d, mask, int(pb.na_mode == 1), pb.n, pb.n_seg,
                                row0.ctypes.data_as(_lp), nrows.ctypes.data_as(_lp),
                                pb.times.ctypes.data_as(_dp), pb.obs.ctypes.data_as(_dp),
                                theta.ctypes.data_as(_dp), p0.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    assert st == 0
    return out[0], out[1:1 + pb.n_par_full]
