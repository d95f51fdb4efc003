"""ctypes mirror of include/ssde.h and the loader of the HIP engine library.

The product path is `libssde_hip.so` (hand-written HIP, gfx950).  There is NO CPU
fallback: if the library is missing, or no GPU is visible when an engine is created,
this module raises.  (The CPU oracle under oracle/ is test infrastructure and is never
imported from here.)

`Problem` carries the arguments of the reference's `tmb_dat` list
(/root/reference/R/sde.R:528-536, 542-598) as numpy arrays and exposes them as an
`ssde_desc`.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

ABI_VERSION = 12

MODEL_CODES = {"BM": 0, "OU": 1, "BM_SSM": 2, "OU_SSM": 3, "CTCRW": 4, "BM_t": 5, "ESEAL_SSM": 6, "CIR": 7}
KALMAN_MODELS = ("BM_SSM", "OU_SSM", "CTCRW")
# types the reference dispatches (src/smoothSDE.cpp:12-27) that this engine does not cover
UNSUPPORTED_MODELS = ()

NA_R_ONLY, NA_ANY_NAN = 0, 1
PATH_NAMES = {0: "direct", 1: "isotropic-register", 2: "dense", 3: "isotropic-row-varying"}
FLAG_DEVICE_DATA, FLAG_FORCE_DENSE, FLAG_NO_UNIFORM_DT, FLAG_EXACT_HESS = 0x1, 0x2, 0x4, 0x8

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class SsdePPBasis(C.Structure):
    _fields_ = [("x", C.c_void_p), ("n_knots", C.c_int32), ("n_cols", C.c_int32), ("knots", C.c_void_p),
                ("coef", C.c_void_p)]


class SsdeDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("model", C.c_int32), ("n_dim", C.c_int32), ("n_par", C.c_int32),
        ("n", C.c_int64),
        ("id", C.c_void_p), ("times", C.c_void_p), ("obs", C.c_void_p),
        ("ncol_fe", _ip), ("x_fe", C.POINTER(C.c_void_p)),
        ("ncol_re", _ip), ("x_re", C.POINTER(C.c_void_p)),
        ("n_smooth", C.c_int32), ("smooth_ncol", _ip), ("s_blocks", C.c_void_p),
        ("include_penalty", C.c_int32),
        ("n_seg", C.c_int64), ("a0", C.c_void_p), ("p0", C.c_void_p), ("h_array", C.c_void_p),
        ("par_fixed", C.c_void_p), ("na_mode", C.c_int32), ("device", C.c_int32),
        ("flags", C.c_uint32), ("reserved", C.c_uint32),
        ("other_data", C.c_void_p), ("n_other_data", C.c_int32),
        ("n_decay", C.c_int32), ("t_decay", C.c_void_p), ("n_decay_cols", C.c_int32), ("reserved3", C.c_int32),
        ("col_decay", C.c_void_p), ("ind_decay", C.c_void_p),
        ("eseal_h", C.c_void_p), ("eseal_R", C.c_void_p),
        ("basis_re", C.POINTER(C.POINTER(SsdePPBasis))),
        ("n_devices", C.c_int32), ("reserved4", C.c_int32), ("devices", _ip),
    ]


class SsdeLaplaceOpts(C.Structure):
    _fields_ = [("hess_step", C.c_double), ("fd_step", C.c_double), ("newton_tol", C.c_double),
                ("max_newton", C.c_int32), ("reserved", C.c_int32)]


class SsdeOccGrid(C.Structure):
    """ssde_occ_grid (include/ssde.h): the regular grid of ssde_path_occupancy"""
    _fields_ = [("x0", C.c_double), ("dx", C.c_double), ("y0", C.c_double), ("dy", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32)]


class SsdeSimDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("model", C.c_int32), ("n_dim", C.c_int32), ("n_steps", C.c_int32),
                ("track0", C.c_int64), ("n_tracks", C.c_int64), ("row0", C.c_void_p), ("n_rows", C.c_int64),
                ("row_offset", C.c_int64), ("mu", C.c_double * 8), ("z0", C.c_double * 8),
                ("tau", C.c_double), ("nu", C.c_double), ("kappa", C.c_double), ("sigma", C.c_double),
                ("sigma_obs", C.c_double), ("dt", C.c_double), ("seed", C.c_uint64), ("device", C.c_int32),
                ("reserved", C.c_int32)]


class SsdeBandsDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_par", C.c_int32), ("n", C.c_int64),
                ("ncol_fe", C.POINTER(C.c_int32)), ("x_fe", C.POINTER(C.c_void_p)), ("ncol_re", C.POINTER(C.c_int32)),
                ("x_re", C.POINTER(C.c_void_p)), ("link", C.POINTER(C.c_uint8)), ("coeff", C.POINTER(C.c_double)),
                ("n_post", C.c_int32), ("resp", C.c_int32), ("level", C.c_double), ("z", C.c_double),
                ("device", C.c_int32), ("budget_mb", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class SsdeSimrowsDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("budget_mb", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("model", C.c_int32), ("n_dim", C.c_int32), ("n_par", C.c_int32), ("n", C.c_int64), ("n_tracks", C.c_int64),
                ("row0", C.POINTER(C.c_int64)), ("times", C.POINTER(C.c_double)),
                ("ncol_fe", C.POINTER(C.c_int32)), ("x_fe", C.POINTER(C.c_void_p)), ("ncol_re", C.POINTER(C.c_int32)),
                ("x_re", C.POINTER(C.c_void_p)), ("link", C.POINTER(C.c_uint8)), ("coeff", C.POINTER(C.c_double)),
                ("n_coeff_rows", C.c_int32), ("n_coef", C.c_int32), ("sigma_obs", C.POINTER(C.c_double)), ("z0", C.c_double * 8),
                ("seed", C.c_uint64), ("rep0", C.c_int64), ("n_rep", C.c_int64), ("thr", C.POINTER(C.c_double)),
                ("n_thr", C.c_int32), ("reserved2", C.c_int32)]


OPT_KERNEL_STAMPS, OPT_COMM_DEFER, OPT_SMOOTH_BUDGET_MB, OPT_LAG_EARLY, OPT_LAG_HEAD_HOST = 1, 2, 3, 4, 5
LAG_CUTS = tuple(range(32, 129, 16))   # the early cuts of the lag statistics (csrc/ssde_lagstats.hpp)
# ssde_info_t.kernel_id (include/ssde.h: SSDE_KERNEL_*): the kernel family that ran the rows of the last evaluation
KERNEL_NAMES = {0: "none", 1: "direct_kernel", 2: "direct_fast_kernel", 3: "iso_shared_kernel", 4: "iso_mask_kernel",
                5: "iso_mask_kernel<uniform grid>", 6: "iso_quiet_kernel", 7: "iso_shared_kernel + general kernel (mixed batch)",
                8: "iso_kernel (direction parts)", 9: "iso_drift_kernel", 10: "iso_drift_general_kernel", 11: "iso_colvar_kernel",
                12: "iso_few_kernel", 13: "iso_full_kernel", 14: "dense_kernel", 15: "tv_filter_kernel", 16: "tv_filter_kernel<dense lanes>",
                17: "iso_adj_kernel"}
PHASE_NAMES = ("host_total", "host_enqueue", "gpu_pre", "kernel", "finalize", "allreduce", "readback", "reserved")


class SsdeInfo(C.Structure):
    _fields_ = [
        ("n_par_full", C.c_int32), ("n_free", C.c_int32), ("sdim", C.c_int32), ("path", C.c_int32),
        ("const_coeff", C.c_int32), ("uniform_dt", C.c_int32),
        ("n_tracks", C.c_int64), ("n_rows", C.c_int64), ("n_steps", C.c_int64), ("hbm_bytes", C.c_int64),
        ("algo_bytes_per_row", C.c_double), ("n_kernel_blocks", C.c_int32), ("lanes_per_track", C.c_int32),
        ("window", C.c_int32), ("window_retries", C.c_int32), ("window_check", C.c_double),
        ("main_kernel_ms", C.c_double), ("main_kernel_rows", C.c_int64),
        ("required_bytes_per_row", C.c_double), ("n_evals", C.c_int64), ("n_memo_hits", C.c_int64),
        ("n_devices", C.c_int32), ("comm_ranks", C.c_int32), ("window_check_max", C.c_double),
        ("n_rows_tiled", C.c_int64), ("n_groups", C.c_int32), ("n_clean_groups", C.c_int32),
        ("quiet_window", C.c_int32), ("kernel_id", C.c_int32), ("quiet_share", C.c_double),
        ("comm_ranks_reported", C.c_int32), ("exact_hess_scope", C.c_int32),
        ("lagstat_rows", C.c_int64), ("lagstat_create_ms", C.c_double),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


def na_real() -> float:
    """R's NA_real_: the NaN whose low word is 1954 (what R_IsNA tests)."""
    return float(np.array([0x7FF00000000007A2], dtype=np.uint64).view(np.float64)[0])


def _f64(a, order="F"):
    return np.require(np.asarray(a, dtype=np.float64), requirements=["ALIGNED"] + (["F"] if order == "F" else ["C"]))


def n_sde_par(model: str, n_dim: int) -> int:
    return n_dim + 1 if model in ("BM", "BM_SSM", "BM_t", "ESEAL_SSM") else n_dim + 2


def state_dim(model: str, n_dim: int) -> int:
    if model == "CTCRW":
        return 2 * n_dim
    if model == "ESEAL_SSM":
        return 2
    return n_dim if model in KALMAN_MODELS else 0


class Problem:
    """Host-side container for one model's data, in the reference's argument shapes.

    ID      : (n,) any dtype; only neighbour inequality matters (nllk_ctcrw.hpp:196)
    times   : (n,)
    obs     : (n, d)
    X_fe    : list of q arrays (n, ncol_fe[j]) or None (= intercept-only)
    X_re    : list of q arrays (n, ncol_re[j]) or None
    S_list  : list of penalty blocks (one per smooth), smooth order = column order of X_re
    """

    def __init__(self, model: str, ID, times, obs, X_fe: Optional[Sequence] = None,
                 X_re: Optional[Sequence] = None, S_list: Optional[Sequence] = None,
                 a0=None, P0=None, H=None, par_fixed=None, include_penalty: int = 1,
                 na_mode: int = NA_ANY_NAN, device: int = -1, flags: int = 0, other_data=None,
                 t_decay=None, col_decay=None, ind_decay=None, eseal_h=None, eseal_R=None, basis_re=None):
        if model in UNSUPPORTED_MODELS:
            raise NotImplementedError(f"SDE type {model!r} is outside this engine's scope")
        if model not in MODEL_CODES:
            raise ValueError("Unknown SDE type")  # src/smoothSDE.cpp:25
        self.model = model
        obs = np.asarray(obs, dtype=np.float64)
        if obs.ndim == 1:
            obs = obs[:, None]
        self.n, self.n_dim = obs.shape
        self.q = n_sde_par(model, self.n_dim)
        self.sdim = state_dim(model, self.n_dim)
        self.obs = _f64(obs)
        ID = np.asarray(ID)
        if ID.dtype.kind not in "fiu":
            _, ID = np.unique(ID, return_inverse=True)
        self.id = _f64(ID)
        self.times = _f64(times)
        if self.id.shape != (self.n,) or self.times.shape != (self.n,):
            raise ValueError("ID, times and obs must have the same number of rows")

        # basis_re[j]: a synth.PPBasis -- the random-effect block of parameter j as a piecewise-cubic function of one
        # covariate (include/ssde.h: ssde_ppbasis).  The dense block it stands for is kept in X_re[j] as well: the
        # oracle and the generic kernels use it, the engine's fast direct kernel evaluates the table instead.
        self.basis_re = [None] * self.q if basis_re is None else list(basis_re)
        if any(b is not None for b in self.basis_re):
            X_re = [None] * self.q if X_re is None else list(X_re)
            for j, b in enumerate(self.basis_re):
                if b is not None:
                    X_re[j] = b.dense()
        self.X_fe, self.X_re = [], []
        ncol_fe, ncol_re = [], []
        for j in range(self.q):
            xf = None if X_fe is None else X_fe[j]
            if xf is None:
                self.X_fe.append(None)
                ncol_fe.append(1)
            else:
                xf = _f64(np.asarray(xf, dtype=np.float64).reshape(self.n, -1))
                self.X_fe.append(xf)
                ncol_fe.append(xf.shape[1])
            xr = None if X_re is None else X_re[j]
            if xr is None or np.asarray(xr).size == 0:
                self.X_re.append(None)
                ncol_re.append(0)
            else:
                xr = _f64(np.asarray(xr, dtype=np.float64).reshape(self.n, -1))
                self.X_re.append(xr)
                ncol_re.append(xr.shape[1])
        self.ncol_fe = np.asarray(ncol_fe, dtype=np.int32)
        self.ncol_re = np.asarray(ncol_re, dtype=np.int32)
        self.n_fe, self.n_re = int(self.ncol_fe.sum()), int(self.ncol_re.sum())

        S_list = [] if S_list is None else [np.asarray(s, dtype=np.float64) for s in S_list]
        self.S_list = S_list
        self.smooth_ncol = np.asarray([s.shape[0] for s in S_list], dtype=np.int32)
        if int(self.smooth_ncol.sum()) != self.n_re:
            raise ValueError("penalty blocks do not match the random-effect columns")
        self.s_blocks = _f64(np.concatenate([s.flatten(order="F") for s in S_list])) if S_list else None
        self.n_smooth = len(S_list)
        self.include_penalty = int(include_penalty)

        self.kalman = model in KALMAN_MODELS or model == "ESEAL_SSM"     # Kalman-style penalty (no constants)
        # leading scalar parameters of the template: log_sigma_obs (nllk_ctcrw.hpp:135) or log_tau, a1, log_a2
        # (nllk_e_seal_ssm.hpp:114-116)
        self.lead_names = ["log_tau", "a1", "log_a2"] if model == "ESEAL_SSM" else (["log_sigma_obs"] if self.kalman else [])
        self.eseal_h = self.eseal_R = None
        if model == "ESEAL_SSM":
            if self.n_dim != 1:
                raise ValueError("ESEAL_SSM takes one response variable")
            if eseal_h is None or eseal_R is None or a0 is None:
                raise ValueError("ESEAL_SSM needs h (daily drift dives), R (non-lipid tissue mass) and a0 (R/sde.R:599-614)")
            self.eseal_h, self.eseal_R = _f64(eseal_h), _f64(eseal_R)
            if self.eseal_h.shape != (self.n,) or self.eseal_R.shape != (self.n,):
                raise ValueError("h and R must have one entry per row")
        first = np.ones(self.n, dtype=bool)
        first[1:] = self.id[1:] != self.id[:-1]
        self.seg_start = np.flatnonzero(first)
        self.n_seg = len(self.seg_start)
        self.a0 = None if a0 is None else _f64(np.asarray(a0, dtype=np.float64).reshape(self.n_seg, self.sdim))
        self.P0 = None if P0 is None else _f64(np.asarray(P0, dtype=np.float64).reshape(self.sdim, self.sdim))
        if H is not None:
            H = np.asarray(H, dtype=np.float64)
            if H.shape != (self.n_dim, self.n_dim, self.n):
                raise ValueError("H must be an array of shape (d, d, n)")
            H = _f64(H)
        self.H = H

        # decaying random-effect columns (direct families; nllk_sde.hpp:30-32, 47-58; R/sde.R:163-177):
        # col_decay / ind_decay are 0-based here (the R objects are 1-based)
        self.n_decay, self.t_decay, self.col_decay, self.ind_decay = 0, None, None, None
        self.decay_of_col = np.full(self.n_re, -1, dtype=int)
        if t_decay is not None:
            if self.kalman:
                raise ValueError("decaying terms are a feature of the direct families (BM, BM_t, OU)")
            self.t_decay = _f64(np.asarray(t_decay, dtype=np.float64).ravel())
            if self.t_decay.shape != (self.q * self.n,):
                raise ValueError("'t_decay' should be of length (number of parameters) x (number of data)")  # R/sde.R:170-173
            self.col_decay = np.ascontiguousarray(col_decay, dtype=np.int32)
            self.ind_decay = np.ascontiguousarray(ind_decay, dtype=np.int32)
            if self.col_decay.shape != self.ind_decay.shape:
                raise ValueError("Check length of 'ind_decay' and 'col_decay'")                               # R/sde.R:174-176
            if len(self.col_decay) and (self.col_decay.min() < 0 or self.col_decay.max() >= self.n_re):
                raise ValueError(f"'col_decay' should be between 0 and {self.n_re - 1}")                      # R/sde.R:637-640
            self.n_decay = int(self.ind_decay.max()) + 1 if len(self.ind_decay) else 0
            self.decay_of_col[self.col_decay] = self.ind_decay

        # full parameter vector layout (include/ssde.h)
        o = len(self.lead_names)
        self.off_sigobs = 0 if self.lead_names == ["log_sigma_obs"] else None
        self.off_fe = o
        o += self.n_fe
        self.off_lambda = o
        o += self.n_smooth
        self.off_decay = o
        o += self.n_decay
        self.off_re = o
        o += self.n_re
        self.n_par_full = o
        self.fe_off = np.concatenate([[0], np.cumsum(self.ncol_fe)[:-1]]).astype(int)
        self.re_off = np.concatenate([[0], np.cumsum(self.ncol_re)[:-1]]).astype(int)

        fixed = np.zeros(self.n_par_full, dtype=np.uint8)
        if par_fixed is not None:
            fixed[:] = np.asarray(par_fixed, dtype=np.uint8)
        if self.off_sigobs is not None and self.H is not None:
            fixed[0] = 1  # map log_sigma_obs = NA when H is supplied (R/sde.R:565, 595)
        self.par_fixed = fixed
        self.na_mode, self.device, self.flags = int(na_mode), int(device), int(flags)
        # DATA_VECTOR(other_data): the degrees of freedom of BM_t (R/sde.R:539-541)
        self.other_data = None if other_data is None else _f64(np.atleast_1d(np.asarray(other_data, dtype=np.float64)))
        if model == "BM_t":
            if self.n_dim != 1:
                raise ValueError("BM_t takes one response variable")
            if self.other_data is None or not (self.other_data[0] > 2):
                raise ValueError("BM_t needs other_data = df (degrees of freedom > 2)")
        self._keep = []

    @classmethod
    def from_torch(cls, model: str, ID, times, obs, par_fixed=None, na_mode: int = NA_ANY_NAN, flags: int = 0,
                   X_re=None, S_list=None, basis_re=None, H=None):
        """Problem whose data already live in HBM (torch CUDA tensors, fp64): the engine re-tiles /
        copies them on the device instead of uploading (SSDE_FLAG_DEVICE_DATA).  Fixed effects are
        intercept-only; `X_re[j]` may be an (n, k) CUDA tensor of streamed design columns for SDE
        parameter j, with the penalty blocks in `S_list` (numpy); `H`: per-row measurement covariances as a (d, d, n)
        CUDA tensor (H_array, Kalman families)."""
        import torch
        assert ID.is_cuda and times.is_cuda and obs.is_cuda
        self = cls.__new__(cls)
        if model not in MODEL_CODES:
            raise ValueError("Unknown SDE type")
        if model in ("ESEAL_SSM", "BM_t", "CIR"):
            raise NotImplementedError("device-resident construction covers BM, OU, BM_SSM, OU_SSM, CTCRW")
        self.model = model
        if obs.dim() == 1:
            obs = obs[:, None]
        self.n, self.n_dim = int(obs.shape[0]), int(obs.shape[1])
        self.q = n_sde_par(model, self.n_dim)
        self.sdim = state_dim(model, self.n_dim)
        self._t_id = ID.to(torch.float64).contiguous()
        self._t_times = times.to(torch.float64).contiguous()
        self._t_obs = obs.to(torch.float64).t().contiguous()     # (d, n) row-major == (n, d) column-major
        self.id = self.times = self.obs = None
        self.X_fe, self.X_re = [None] * self.q, [None] * self.q
        self.ncol_fe = np.ones(self.q, dtype=np.int32)
        self.ncol_re = np.zeros(self.q, dtype=np.int32)
        self.n_fe, self.n_re = self.q, 0
        self.S_list, self.smooth_ncol, self.s_blocks, self.n_smooth = [], np.zeros(0, dtype=np.int32), None, 0
        self._t_xre = [None] * self.q
        # basis_re[j]: synth.PPBasis whose covariate x is a CUDA tensor -- no n x K block exists anywhere
        self.basis_re = [None] * self.q if basis_re is None else list(basis_re)
        if X_re is None and any(b is not None for b in self.basis_re):
            X_re = [None] * self.q
        if X_re is not None:
            for j in range(self.q):
                if self.basis_re[j] is not None:
                    self.ncol_re[j] = self.basis_re[j].n_cols
                elif X_re[j] is not None:
                    xt = X_re[j].to(torch.float64)
                    self._t_xre[j] = xt.t().contiguous()          # (k, n) row-major == (n, k) column-major
                    self.ncol_re[j] = xt.shape[1]
            self.n_re = int(self.ncol_re.sum())
            self.S_list = [np.asarray(s_, dtype=np.float64) for s_ in (S_list or [])]
            self.smooth_ncol = np.asarray([s_.shape[0] for s_ in self.S_list], dtype=np.int32)
            self.s_blocks = _f64(np.concatenate([s_.flatten(order="F") for s_ in self.S_list])) if self.S_list else None
            self.n_smooth = len(self.S_list)
            if int(self.smooth_ncol.sum()) != self.n_re:
                raise ValueError("penalty blocks do not match the random-effect columns")
        self.include_penalty = 1
        self.kalman = model in KALMAN_MODELS
        self.lead_names = ["log_sigma_obs"] if self.kalman else []
        self.eseal_h = self.eseal_R = None
        first = torch.ones(self.n, dtype=torch.bool, device=ID.device)
        first[1:] = self._t_id[1:] != self._t_id[:-1]
        self.seg_start = first.nonzero().flatten().cpu().numpy()
        self.n_seg = len(self.seg_start)
        self.a0 = self.P0 = self.H = None
        o = 0
        self.off_sigobs = None
        if self.kalman:
            self.off_sigobs, o = 0, 1
        self.off_fe = o
        o += self.n_fe
        self.off_lambda = o
        o += self.n_smooth
        self.off_decay, self.n_decay, self.t_decay, self.col_decay, self.ind_decay = o, 0, None, None, None
        self.off_re = o
        o += self.n_re
        self.n_par_full = o
        self.decay_of_col = np.full(self.n_re, -1, dtype=int)
        self.fe_off = np.arange(self.q)
        self.re_off = np.concatenate([[0], np.cumsum(self.ncol_re)[:-1]]).astype(int)
        fixed = np.zeros(self.n_par_full, dtype=np.uint8)
        if par_fixed is not None:
            fixed[:] = np.asarray(par_fixed, dtype=np.uint8)
        self._t_h = None
        if H is not None:
            if not self.kalman or tuple(H.shape) != (self.n_dim, self.n_dim, self.n):
                raise ValueError("H must be a (d, d, n) tensor, Kalman families only")
            self._t_h = H.to(torch.float64).permute(2, 1, 0).contiguous()     # memory order of the column-major d x d x n array
            fixed[0] = 1                                                       # log_sigma_obs is not in the model then (R/sde.R:565, 595)
        self.par_fixed = fixed
        self.na_mode, self.device = int(na_mode), int(ID.device.index or 0)
        self.flags = int(flags) | FLAG_DEVICE_DATA
        self.other_data = None
        self._keep = []
        return self

    # -- parameter helpers ---------------------------------------------------------------
    def par_names(self):
        names = list(self.lead_names)
        for j in range(self.q):
            names += [f"coeff_fe[{j}][{c}]" for c in range(self.ncol_fe[j])]
        names += [f"log_lambda[{s}]" for s in range(self.n_smooth)]
        names += [f"log_decay[{k}]" for k in range(self.n_decay)]
        for j in range(self.q):
            names += [f"coeff_re[{j}][{c}]" for c in range(self.ncol_re[j])]
        return names

    def free_index(self):
        return np.flatnonzero(self.par_fixed == 0)

    # -- ctypes view ------------------------------------------------------------------------
    def desc(self) -> SsdeDesc:
        d = SsdeDesc()
        keep = self._keep = []

        def ptr(a):
            if a is None:
                return None
            keep.append(a)
            return a.ctypes.data

        d.abi_version = ABI_VERSION
        d.model = MODEL_CODES[self.model]
        d.n_dim, d.n_par, d.n = self.n_dim, self.q, self.n
        if getattr(self, "_t_id", None) is not None:
            d.id, d.times, d.obs = self._t_id.data_ptr(), self._t_times.data_ptr(), self._t_obs.data_ptr()
        else:
            d.id, d.times, d.obs = ptr(self.id), ptr(self.times), ptr(self.obs)
        d.ncol_fe = self.ncol_fe.ctypes.data_as(_ip)
        d.ncol_re = self.ncol_re.ctypes.data_as(_ip)
        xfe = (C.c_void_p * self.q)(*[ptr(x) for x in self.X_fe])
        if getattr(self, "_t_xre", None) is not None:
            xre = (C.c_void_p * self.q)(*[None if x is None else x.data_ptr() for x in self._t_xre])
        else:
            xre = (C.c_void_p * self.q)(*[ptr(x) for x in self.X_re])
        keep += [xfe, xre]
        d.x_fe, d.x_re = xfe, xre
        d.n_smooth = self.n_smooth
        d.smooth_ncol = self.smooth_ncol.ctypes.data_as(_ip) if self.n_smooth else None
        d.s_blocks = ptr(self.s_blocks)
        d.include_penalty = self.include_penalty
        d.n_seg = self.n_seg
        d.a0, d.p0, d.h_array = ptr(self.a0), ptr(self.P0), ptr(self.H)
        if getattr(self, "_t_h", None) is not None:
            d.h_array = self._t_h.data_ptr()
        d.par_fixed = ptr(self.par_fixed)
        d.na_mode, d.device, d.flags = self.na_mode, self.device, self.flags
        d.other_data = ptr(getattr(self, "other_data", None))
        d.n_other_data = 0 if getattr(self, "other_data", None) is None else len(self.other_data)
        d.n_decay = self.n_decay
        if self.n_decay > 0:
            d.t_decay, d.n_decay_cols = ptr(self.t_decay), len(self.col_decay)
            d.col_decay, d.ind_decay = ptr(self.col_decay), ptr(self.ind_decay)
        d.eseal_h, d.eseal_R = ptr(getattr(self, "eseal_h", None)), ptr(getattr(self, "eseal_R", None))
        bl = getattr(self, "basis_re", None)
        if bl is not None and any(b is not None for b in bl):
            arr = (C.POINTER(SsdePPBasis) * self.q)()
            for j, b in enumerate(bl):
                if b is None:
                    continue
                sb = SsdePPBasis()
                if hasattr(b.x, "data_ptr"):
                    sb.x = b.x.data_ptr()
                    keep.append(b.x)
                else:
                    sb.x = ptr(_f64(b.x))
                sb.n_knots, sb.n_cols = len(b.knots), b.n_cols
                sb.knots, sb.coef = ptr(b.knots), ptr(b.coef)
                keep.append(sb)
                arr[j] = C.pointer(sb)
            keep.append(arr)
            d.basis_re = arr
        return d


# ---------------------------------------------------------------------------------------------
_LIB = None


def lib_path() -> str:
    override = os.environ.get("SSDE_LIB")  # kernel-tuning builds (same ABI); the default is the in-tree library
    if override:
        return override
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libssde_hip.so")


def load_library():
    """Load libssde_hip.so; raise loudly if the HIP extension has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"HIP engine library not found at {path}: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
            "There is no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64
    # under an unversioned file name, so if this library pulled in /opt/rocm's copy first, torch
    # would later load a SECOND runtime that finds no device.  Importing torch first makes the
    # loader resolve our DT_NEEDED libamdhip64.so.7 to the runtime torch already mapped (same
    # soname).  Hosts without torch (the R shim) simply use /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path)
    lib.ssde_create.argtypes = [C.POINTER(SsdeDesc), C.POINTER(C.c_void_p)]
    lib.ssde_create.restype = C.c_int
    lib.ssde_eval.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_int32, _dp, _dp]
    lib.ssde_eval.restype = C.c_int
    lib.ssde_eval_device.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.ssde_eval_device.restype = C.c_int
    lib.ssde_penalty.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, _dp]
    lib.ssde_penalty.restype = C.c_int
    lib.ssde_report.argtypes = [C.c_void_p, _dp, C.c_int32, _dp]
    lib.ssde_report.restype = C.c_int
    lib.ssde_smooth.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, _dp, _dp]
    lib.ssde_smooth.restype = C.c_int
    lib.ssde_smooth_loo.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.c_int32, _dp, C.c_uint32]
    lib.ssde_smooth_loo.restype = C.c_int
    lib.ssde_forecast_scores.argtypes = [C.c_void_p, _dp, C.c_int32, C.POINTER(C.c_int32), C.c_int32, _dp, _dp, _dp, C.c_int32, _dp, C.c_uint32]
    lib.ssde_forecast_scores.restype = C.c_int
    lib.ssde_smooth_draws.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.c_void_p, C.c_uint32]
    lib.ssde_smooth_draws.restype = C.c_int
    lib.ssde_predict.argtypes = [C.c_void_p, _dp, C.c_int32, C.POINTER(C.c_int64), _dp, C.c_int64, _dp, _dp]
    lib.ssde_predict.restype = C.c_int
    lib.ssde_predict_draws.argtypes = [C.c_void_p, _dp, C.c_int32, C.POINTER(C.c_int64), _dp, C.c_int64, C.c_uint64, C.c_int64, C.c_int32,
                                       _dp, C.c_uint32]
    lib.ssde_predict_draws.restype = C.c_int
    lib.ssde_path_stats.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, _dp, C.c_int32, _dp, _dp, C.c_uint32]
    lib.ssde_path_stats.restype = C.c_int
    lib.ssde_path_speed.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, _dp, C.c_int32, _dp, _dp,
                                    C.POINTER(C.c_uint32), C.c_uint32]
    lib.ssde_path_speed.restype = C.c_int
    lib.ssde_path_occupancy.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(SsdeOccGrid), _dp,
                                        C.POINTER(C.c_int32), C.c_int32, _dp, _dp, C.c_uint32]
    lib.ssde_path_occupancy.restype = C.c_int
    lib.ssde_last_occupancy_form.argtypes = [C.c_void_p]
    lib.ssde_last_occupancy_form.restype = C.c_int
    lib.ssde_path_occupancy_fine.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(SsdeOccGrid), C.c_double,
                                             _dp, C.POINTER(C.c_int32), C.c_int32, _dp, _dp, C.c_uint32]
    lib.ssde_path_occupancy_fine.restype = C.c_int
    lib.ssde_last_occupancy_points.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.ssde_last_occupancy_points.restype = C.c_int
    _lp64 = C.POINTER(C.c_int64)
    lib.ssde_path_proximity.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, _lp64, _dp, _lp64, _dp, _lp64,
                                        C.c_int32, _dp, _dp, C.c_int32, _dp, C.c_uint32]
    lib.ssde_path_proximity.restype = C.c_int
    lib.ssde_last_proximity_plan.argtypes = [C.c_void_p, _lp64, _lp64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.ssde_last_proximity_plan.restype = C.c_int
    lib.ssde_last_hess_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp]
    lib.ssde_last_hess_plan.restype = C.c_int
    lib.ssde_widen_windows.argtypes = [C.c_void_p, C.c_int32]
    lib.ssde_widen_windows.restype = C.c_int
    lib.ssde_relax_windows.argtypes = [C.c_void_p]
    lib.ssde_relax_windows.restype = C.c_int
    lib.ssde_info.argtypes = [C.c_void_p, C.POINTER(SsdeInfo)]
    lib.ssde_info.restype = C.c_int
    lib.ssde_destroy.argtypes = [C.c_void_p]
    lib.ssde_destroy.restype = None
    lib.ssde_last_error.argtypes = [C.c_void_p]
    lib.ssde_last_error.restype = C.c_char_p
    lib.ssde_lagstats_host.argtypes = [_dp, C.POINTER(C.c_int64), C.c_int64, C.c_int, _dp, _dp, _dp,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.ssde_lagstats_host.restype = C.c_int
    lib.ssde_lagstats_read.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.ssde_lagstats_read.restype = C.c_int
    lib.ssde_lagforms_host.argtypes = [_dp, _dp, C.c_double, C.c_int32, _dp, C.c_double, _dp, C.c_int32, C.c_int32, C.c_int32,
                                       _dp, _dp, _dp, _dp]
    lib.ssde_lagforms_host.restype = C.c_int
    lib.ssde_lagstats_host_m.argtypes = [C.c_int32, _dp, C.POINTER(C.c_int64), C.c_int64, C.c_int, _dp, _dp, _dp, _dp,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.ssde_lagstats_host_m.restype = C.c_int
    lib.ssde_lagstats_read_m.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
    lib.ssde_lagstats_read_m.restype = C.c_int
    lib.ssde_lagstats_host_cut.argtypes = [_dp, C.POINTER(C.c_int64), C.c_int64, C.c_int, C.c_int32, _dp, _dp, _dp]
    lib.ssde_lagstats_host_cut.restype = C.c_int
    lib.ssde_lagstats_read_cut.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp]
    lib.ssde_lagstats_read_cut.restype = C.c_int
    lib.ssde_headstats_host.argtypes = [_dp, C.POINTER(C.c_int64), _dp, C.c_int64, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.ssde_headstats_host.restype = C.c_int
    lib.ssde_headstats_read.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.ssde_headstats_read.restype = C.c_int
    lib.ssde_headforms_host.argtypes = [_dp, _dp, C.c_double, C.c_int32, _dp, C.c_double, _dp, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp,
                                        C.POINTER(C.c_int32)]
    lib.ssde_headforms_host.restype = C.c_int
    lib.ssde_last_head_form.argtypes = [C.c_void_p]
    lib.ssde_last_head_form.restype = C.c_int
    lib.ssde_last_lag_cut.argtypes = [C.c_void_p]
    lib.ssde_last_lag_cut.restype = C.c_int
    lib.ssde_lagforms_host_m.argtypes = [C.c_int32, _dp, _dp, C.c_double, _dp, C.c_int32, _dp, C.c_double, _dp, C.c_int32, C.c_int32,
                                         C.c_int32, _dp, _dp, _dp, _dp]
    lib.ssde_lagforms_host_m.restype = C.c_int
    lib.ssde_reduce_host.argtypes = [_dp, _dp, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_double, _dp, C.POINTER(C.c_int16), C.POINTER(C.c_int16),
                                     C.c_int32, _dp]
    lib.ssde_reduce_host.restype = C.c_int
    lib.ssde_lagforms_host_isa.argtypes = [C.c_int32] + list(lib.ssde_lagforms_host.argtypes)
    lib.ssde_lagforms_host_isa.restype = C.c_int
    lib.ssde_reduce_host_head.argtypes = [_dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_double, _dp, C.POINTER(C.c_int16),
                                          C.POINTER(C.c_int16), C.c_int32, _dp]
    lib.ssde_reduce_host_head.restype = C.c_int
    lib.ssde_last_finish_form.argtypes = [C.c_void_p]
    lib.ssde_last_finish_form.restype = C.c_int
    for name in ("ssde_last_gain_feed", "ssde_last_gain_rows"):
        getattr(lib, name).argtypes = [C.c_void_p]
        getattr(lib, name).restype = C.c_int
    lib.ssde_abi_version.argtypes = []
    lib.ssde_abi_version.restype = C.c_int
    lib.ssde_laplace_eval.argtypes = [C.c_void_p, _dp, C.c_int32, C.c_int32, _dp, _dp, _dp, C.POINTER(SsdeLaplaceOpts)]
    lib.ssde_laplace_eval.restype = C.c_int
    lib.ssde_last_kernel_ms.argtypes = [C.c_void_p]
    lib.ssde_last_kernel_ms.restype = C.c_double
    lib.ssde_kernel_ms_history.argtypes = [C.c_void_p, _dp, C.c_int32]
    lib.ssde_kernel_ms_history.restype = C.c_int
    lib.ssde_forget.argtypes = [C.c_void_p]
    lib.ssde_forget.restype = C.c_int
    lib.ssde_comm_unique_id.argtypes = [C.c_void_p]
    lib.ssde_comm_unique_id.restype = C.c_int
    lib.ssde_comm_init_rank.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.ssde_comm_init_rank.restype = C.c_int
    lib.ssde_simulate.argtypes = [C.POINTER(SsdeSimDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ssde_simulate.restype = C.c_int
    lib.ssde_par_bands.argtypes = [C.POINTER(SsdeBandsDesc)] + [C.c_void_p] * 7
    lib.ssde_par_bands.restype = C.c_int
    lib.ssde_simulate_rows.argtypes = [C.POINTER(SsdeSimrowsDesc), C.c_void_p, C.c_void_p]
    lib.ssde_simulate_rows.restype = C.c_int
    lib.ssde_hess.argtypes = [C.c_void_p, _dp, C.c_int32, _ip, C.c_int32, _dp]
    lib.ssde_hess.restype = C.c_int
    lib.ssde_set_option.argtypes = [C.c_void_p, C.c_int32, C.c_int64]
    lib.ssde_set_option.restype = C.c_int
    lib.ssde_last_phase_ms.argtypes = [C.c_void_p, _dp]
    lib.ssde_last_phase_ms.restype = C.c_int
    lib.ssde_comm_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.ssde_comm_allreduce.restype = C.c_int
    if lib.ssde_abi_version() != ABI_VERSION:
        raise RuntimeError("libssde_hip.so ABI version mismatch")
    _LIB = lib
    return lib


class EngineError(RuntimeError):
    """a non-zero status from the C ABI; `.status` holds it (include/ssde.h: SSDE_ERR_*)"""
    status = None


PATH_MAX_REGIONS = 8   # SSDE_PATH_MAX_REGIONS (include/ssde.h)
SPEED_MAX_THR = 8      # SSDE_SPEED_MAX_THR: the most thresholds of one ssde_path_speed
LOO_MAX_THR = 8        # SSDE_LOO_MAX_THR: the most thresholds of one ssde_smooth_loo
AHEAD_MAX_H, AHEAD_MAX_STEP, AHEAD_MAX_THR = 8, 64, 8   # SSDE_AHEAD_MAX_*: horizons of one ssde_forecast_scores, the largest, thresholds
DRAWS_DEVICE_OUT = 1   # ssde_smooth_draws flag: `draws` is an HBM pointer on the handle's device (include/ssde.h)
OCC_FORCE_GLOBAL = 1   # ssde_path_occupancy flag: every wavefront group runs the global form (SSDE_OCC_FORCE_GLOBAL)
PROX_MAX_RADII = 8     # SSDE_PROX_MAX_RADII: the most radii of one ssde_path_proximity
BANDS_MAX_TAIL, BANDS_MAX_COLS, BANDS_MAX_PAR = 64, 64, 16   # SSDE_BANDS_MAX_*: order statistics of a tail, columns of a parameter, parameters
BANDS_DEVICE_DATA, BANDS_DEVICE_OUT = 1, 2                  # ssde_par_bands flags: the blocks / the n x q outputs are HBM pointers
SIMROWS_MAX_THR, SIMROWS_MAX_COEF = 8, 128                  # SSDE_SIMROWS_MAX_*: thresholds of one ssde_simulate_rows, coefficients of one row
SIMROWS_DEVICE_DATA, SIMROWS_DEVICE_OUT = 1, 2              # ssde_simulate_rows flags: the blocks / obs_rep are HBM pointers
OCC_MAX_SUB = 64       # SSDE_OCC_MAX_SUB: the most sub-steps ssde_path_occupancy_fine cuts an interval into

WINDOW_TOL = 1e-11  # largest tolerated relative hand-over disagreement between time windows

EXPORTED_SYMBOLS = ("ssde_create", "ssde_eval", "ssde_eval_device", "ssde_penalty", "ssde_report", "ssde_widen_windows", "ssde_relax_windows",
                    "ssde_info", "ssde_destroy", "ssde_last_error", "ssde_abi_version", "ssde_comm_unique_id", "ssde_comm_init_rank", "ssde_forget", "ssde_laplace_eval", "ssde_last_kernel_ms", "ssde_kernel_ms_history",
                    "ssde_simulate", "ssde_par_bands", "ssde_simulate_rows", "ssde_set_option", "ssde_hess", "ssde_last_phase_ms", "ssde_comm_allreduce", "ssde_lagstats_host", "ssde_lagstats_read", "ssde_lagforms_host", "ssde_smooth", "ssde_smooth_loo", "ssde_forecast_scores", "ssde_smooth_draws", "ssde_predict", "ssde_predict_draws", "ssde_path_stats", "ssde_path_speed", "ssde_path_occupancy", "ssde_last_occupancy_form", "ssde_path_occupancy_fine", "ssde_last_occupancy_points", "ssde_last_hess_plan", "ssde_path_proximity", "ssde_last_proximity_plan",
                    "ssde_lagstats_host_m", "ssde_lagstats_read_m", "ssde_lagforms_host_m", "ssde_reduce_host", "ssde_last_finish_form", "ssde_last_gain_feed", "ssde_last_gain_rows",
                    "ssde_lagstats_host_cut", "ssde_lagstats_read_cut", "ssde_last_lag_cut",
                    "ssde_headstats_host", "ssde_headstats_read", "ssde_headforms_host", "ssde_last_head_form",
                    "ssde_lagforms_host_isa", "ssde_reduce_host_head")


def reduce_host(sums, group_chk, n_out, map_, lag_acc=None, lag_chk=0.0, add=None, add_slot=None):
    """The final sums of an evaluation whose head finished on the host: `sums` [groups][windows][accumulators] wave
    sums and `group_chk` [groups] hand-over checks -> n_out sums and the check, in the fixed order of the device's reduction.
    `map_`: accumulator k >= 1 -> output slot or -1; `lag_acc`: the bulk's accumulators (the entry after the last one) or None;
    `add`, `add_slot`: up to four data-independent terms and their slots."""
    lib = load_library()
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    G, W, nacc = sums.shape
    chk = np.ascontiguousarray(group_chk, dtype=np.float64)
    mp = np.ascontiguousarray(map_, dtype=np.int16)
    if chk.shape != (G,) or mp.shape != (nacc - 1,):
        raise ValueError("reduce_host: shapes")
    ad = np.zeros(4); sl = np.full(4, -1, dtype=np.int16)
    if add is not None:
        ad[:len(add)] = add; sl[:len(add_slot)] = add_slot
    la = None if lag_acc is None else np.ascontiguousarray(lag_acc, dtype=np.float64)
    out = np.zeros(n_out + 1)
    i16 = C.POINTER(C.c_int16)
    st = lib.ssde_reduce_host(sums.ctypes.data_as(_dp), chk.ctypes.data_as(_dp), G, W, nacc, None if la is None else la.ctypes.data_as(_dp),
                              float(lag_chk), ad.ctypes.data_as(_dp), sl.ctypes.data_as(i16), mp.ctypes.data_as(i16), int(n_out), out.ctypes.data_as(_dp))
    if st != 0:
        raise ValueError(f"ssde_reduce_host: status {st}")
    return out

def reduce_host_head(sums0, chk0, n_groups, n_out, map_, lag_acc=None, lag_chk=0.0, add=None, add_slot=None):
    """reduce_host where every group but group 0 holds zeros, from group 0's record alone: `sums0` [windows][accumulators], `chk0` its
    check, `n_groups` the groups of the full array.  Equal (==) to reduce_host on that array."""
    lib = load_library()
    sums0 = np.ascontiguousarray(sums0, dtype=np.float64)
    W, nacc = sums0.shape
    mp = np.ascontiguousarray(map_, dtype=np.int16)
    if mp.shape != (nacc - 1,):
        raise ValueError("reduce_host_head: shapes")
    ad = np.zeros(4); sl = np.full(4, -1, dtype=np.int16)
    if add is not None:
        ad[:len(add)] = add; sl[:len(add_slot)] = add_slot
    la = None if lag_acc is None else np.ascontiguousarray(lag_acc, dtype=np.float64)
    out = np.zeros(n_out + 1)
    i16 = C.POINTER(C.c_int16)
    st = lib.ssde_reduce_host_head(sums0.ctypes.data_as(_dp), float(chk0), int(n_groups), W, nacc, None if la is None else la.ctypes.data_as(_dp),
                                   float(lag_chk), ad.ctypes.data_as(_dp), sl.ctypes.data_as(i16), mp.ctypes.data_as(i16), int(n_out),
                                   out.ctypes.data_as(_dp))
    if st != 0:
        raise ValueError(f"ssde_reduce_host_head: status {st}")
    return out


def lagstats_host(tracks, model="CTCRW", ref=None):
    """The lag statistics ssde_create builds for a stationary batch, computed on the host: `tracks` is a list of
    (rows x d) arrays of tiled rows.  Returns (M, s, n_bulk, first_row): M (taps x taps), s (2 x taps), the bulk rows, the bulk's first row.
    `model`: "CTCRW" and "BM_SSM" take the statistics of the increments, "OU_SSM" those of the levels y - `ref` (d numbers)."""
    lib = load_library()
    nt, a0 = C.c_int32(0), C.c_int32(0)
    lib.ssde_lagstats_host(None, None, 0, 1, None, None, None, C.byref(nt), C.byref(a0))
    d = int(tracks[0].shape[1])
    y = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.float64) for t in tracks]))
    rows = np.array([t.shape[0] for t in tracks], dtype=np.int64)
    M = np.zeros((nt.value, nt.value)); s = np.zeros((2, nt.value)); n = np.zeros(1)
    if model == "CTCRW" and ref is None:
        st = lib.ssde_lagstats_host(y.ctypes.data_as(_dp), rows.ctypes.data_as(C.POINTER(C.c_int64)), len(tracks), d,
                                    M.ctypes.data_as(_dp), s.ctypes.data_as(_dp), n.ctypes.data_as(_dp), C.byref(nt), C.byref(a0))
    else:
        rf = None if ref is None else np.ascontiguousarray(np.atleast_1d(ref), dtype=np.float64)
        if rf is not None and rf.size < d:
            raise ValueError("lagstats_host: ref holds fewer than d numbers")
        st = lib.ssde_lagstats_host_m(MODEL_CODES[model], y.ctypes.data_as(_dp), rows.ctypes.data_as(C.POINTER(C.c_int64)), len(tracks), d,
                                      None if rf is None else rf.ctypes.data_as(_dp), M.ctypes.data_as(_dp), s.ctypes.data_as(_dp),
                                      n.ctypes.data_as(_dp), C.byref(nt), C.byref(a0))
    if st != 0:
        raise ValueError(f"ssde_lagstats_host: status {st}")
    return M, s, float(n[0]), int(a0.value)


def lagstats_host_cut(tracks, cut):
    """lagstats_host (CTCRW: the increments) with the first bulk row `cut`: 256, or an early cut (LAG_CUTS).  Returns (M, s, n_bulk);
    the entries with a lag >= cut are zero."""
    lib = load_library()
    nt, a0 = C.c_int32(0), C.c_int32(0)
    lib.ssde_lagstats_host(None, None, 0, 1, None, None, None, C.byref(nt), C.byref(a0))
    d = int(tracks[0].shape[1])
    y = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.float64) for t in tracks]))
    rows = np.array([t.shape[0] for t in tracks], dtype=np.int64)
    M = np.zeros((nt.value, nt.value)); s = np.zeros((2, nt.value)); n = np.zeros(1)
    st = lib.ssde_lagstats_host_cut(y.ctypes.data_as(_dp), rows.ctypes.data_as(C.POINTER(C.c_int64)), len(tracks), d, int(cut),
                                    M.ctypes.data_as(_dp), s.ctypes.data_as(_dp), n.ctypes.data_as(_dp))
    if st != 0:
        raise ValueError(f"ssde_lagstats_host_cut: status {st}")
    return M, s, float(n[0])


def head_components():
    """components of the head's Gram statistics (129: the two of a0 and the 127 increments of the first 128 rows)"""
    nc = C.c_int32(0)
    load_library().ssde_headstats_host(None, None, None, 0, 2, None, None, None, None, C.byref(nc))
    return int(nc.value)


def headstats_host(tracks, a0):
    """The Gram statistics of the head's rows on the host: `tracks` a list of (rows x d) arrays of tiled rows, `a0`
    (tracks x 2 d) their initial states.  Returns (G, s, n), or None where a track is shorter than the statistics' 128 rows (not built)."""
    lib = load_library()
    nw = head_components()
    d = int(tracks[0].shape[1])
    y = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.float64) for t in tracks]))
    rows = np.array([t.shape[0] for t in tracks], dtype=np.int64)
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    if a0.shape != (len(tracks), 2 * d):
        raise ValueError("headstats_host: a0 is tracks x 2 d")
    G = np.zeros((nw, nw)); s = np.zeros((2, nw)); n = np.zeros(1); built = C.c_int32(0)
    st = lib.ssde_headstats_host(y.ctypes.data_as(_dp), rows.ctypes.data_as(C.POINTER(C.c_int64)), a0.ctypes.data_as(_dp), len(tracks), d,
                                 G.ctypes.data_as(_dp), s.ctypes.data_as(_dp), n.ctypes.data_as(_dp), C.byref(built), None)
    if st != 0:
        raise ValueError(f"ssde_headstats_host: status {st}")
    return (G, s, float(n[0])) if built.value else None


def headforms_host(G, s, n_tracks, theta, dt, cut, p0=None, mask=-1, full_probes=False):
    """The head's accumulators of one evaluation from its Gram statistics, on the host: CTCRW, d = 2, theta =
    (log sigma_obs, mu_1, mu_2, log tau, log nu), rows [0, cut).  Returns a dict: acc (6), gain (cut x 16: the gain row of every head
    row), trans (e, t12, b1, b2, de, dt12), n_probe (the response columns that ran as probes)."""
    lib = load_library()
    G = np.ascontiguousarray(G, dtype=np.float64); s = np.ascontiguousarray(s, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    nw = head_components()
    if G.shape != (nw, nw) or s.shape != (2, nw) or theta.size != 5:
        raise ValueError("headforms_host: shapes")
    p0a = None if p0 is None else np.ascontiguousarray(np.atleast_1d(p0), dtype=np.float64)
    acc = np.zeros(6); gain = np.zeros((int(cut), 16)); trans = np.zeros(6); npb = C.c_int32(0)
    st = lib.ssde_headforms_host(G.ctypes.data_as(_dp), s.ctypes.data_as(_dp), float(n_tracks), 2, theta.ctypes.data_as(_dp), float(dt),
                                 None if p0a is None else p0a.ctypes.data_as(_dp), int(cut), int(mask), 1 if full_probes else 0,
                                 acc.ctypes.data_as(_dp), gain.ctypes.data_as(_dp), trans.ctypes.data_as(_dp), C.byref(npb))
    if st != 0:
        raise ValueError(f"ssde_headforms_host: status {st}")
    return {"acc": acc, "gain": gain, "trans": trans, "n_probe": int(npb.value)}


def lagforms_host(M, s, n_bulk, theta, dt, K, d=None, p0=None, mask=-1, taps=None, model="CTCRW", ref=None, isa=None):
    """The bulk's forms of one evaluation on the lag-statistics path, on the host: CTCRW on a regular grid of
    step `dt` at theta = (log sigma_obs, mu_1 .. mu_d, log tau, log nu), cut at `K` taps (the check's cut: K - 16), from the
    statistics M, s, n_bulk.  `taps` (2 x taps: the impulse responses of u and r): used as they are when given, computed otherwise.
    Returns a dict: raw (2 x 6: S, C_1..3, su_1, su_2 of the cut K, then of K - 16), acc (the 4 + d accumulators), chk, taps.
    `model` "OU_SSM" (theta = log sigma_obs, mu, log tau, log kappa; `ref`: what the statistics were built with) or "BM_SSM" (theta =
    log sigma_obs, mu, log sigma): taps is 3 x taps (u, A1, A3) and raw 2 x 5 (S, S1, S3, su_1, su_2).
    `isa` (CTCRW): 0 the baseline build of the sums, 1 the AVX2 build (ValueError on a host without it); None: what an evaluation runs."""
    lib = load_library()
    M = np.ascontiguousarray(M, dtype=np.float64); s = np.ascontiguousarray(s, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    scal = model != "CTCRW"
    npar = 2 if model == "BM_SSM" else 3                   # log sigma_obs and the model's one or two scale parameters
    if d is None:
        d = theta.size - npar
    given = taps is not None
    nrow, nraw = (3, 5) if scal else (2, 6)
    tp = np.ascontiguousarray(taps, dtype=np.float64).copy() if given else np.zeros((nrow, M.shape[0]))
    if tp.shape != (nrow, M.shape[0]) or s.shape != (2, M.shape[0]) or theta.size != d + npar:
        raise ValueError("lagforms_host: shapes")
    p0a = None if p0 is None else np.ascontiguousarray(np.atleast_1d(p0), dtype=np.float64)
    raw = np.zeros((2, nraw)); acc = np.zeros(4 + d); chk = np.zeros(1)
    if isa is not None:
        if scal:
            raise ValueError("lagforms_host: isa is CTCRW's")
        st = lib.ssde_lagforms_host_isa(int(isa), M.ctypes.data_as(_dp), s.ctypes.data_as(_dp), float(n_bulk), d, theta.ctypes.data_as(_dp),
                                        float(dt), None if p0a is None else p0a.ctypes.data_as(_dp), int(K), int(mask), 1 if given else 0,
                                        tp.ctypes.data_as(_dp), raw.ctypes.data_as(_dp), acc.ctypes.data_as(_dp), chk.ctypes.data_as(_dp))
    elif not scal and ref is None:
        st = lib.ssde_lagforms_host(M.ctypes.data_as(_dp), s.ctypes.data_as(_dp), float(n_bulk), d, theta.ctypes.data_as(_dp), float(dt),
                                    None if p0a is None else p0a.ctypes.data_as(_dp), int(K), int(mask), 1 if given else 0,
                                    tp.ctypes.data_as(_dp), raw.ctypes.data_as(_dp), acc.ctypes.data_as(_dp), chk.ctypes.data_as(_dp))
    else:
        rf = None if ref is None else np.ascontiguousarray(np.atleast_1d(ref), dtype=np.float64)
        if rf is not None and rf.size < d:
            raise ValueError("lagforms_host: ref holds fewer than d numbers")
        st = lib.ssde_lagforms_host_m(MODEL_CODES[model], M.ctypes.data_as(_dp), s.ctypes.data_as(_dp), float(n_bulk),
                                      None if rf is None else rf.ctypes.data_as(_dp), d, theta.ctypes.data_as(_dp), float(dt),
                                      None if p0a is None else p0a.ctypes.data_as(_dp), int(K), int(mask), 1 if given else 0,
                                      tp.ctypes.data_as(_dp), raw.ctypes.data_as(_dp), acc.ctypes.data_as(_dp), chk.ctypes.data_as(_dp))
    if st != 0:
        raise ValueError(f"ssde_lagforms_host: status {st}")
    return {"raw": raw, "acc": acc, "chk": float(chk[0]), "taps": tp}


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """An ncclUniqueId (rank 0 makes it, the host ships it to the other ranks, every rank passes it to
    Engine.comm_init)."""
    lib = load_library()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    st = lib.ssde_comm_unique_id(buf)
    if st != 0:
        msg = lib.ssde_last_error(None)
        raise EngineError(f"ssde_comm_unique_id failed ({st}): {msg.decode() if msg else ''}")
    return buf.raw


def simulate_device(model: str, n_tracks: int, n_steps: int, n_dim: int = 2, *, mu=0.0, tau=2.0, nu=1.0, kappa=1.0,
                    sigma=1.0, sigma_obs=0.1, dt: float = 1.0, z0=0.0, seed: int = 1, track0: int = 0, row_offset=None,
                    lengths=None, device=None, want_id_times: bool = True):
    """ssde_simulate: tracks [track0, track0 + n_tracks) of the batch `seed` names, generated in HBM by the HIP
    simulator (exact transitions of R/sde.R:1434-1478 + observation error; counter-based, so a shard of a batch is the
    same numbers whoever generates it).  Returns torch CUDA tensors (ID, times, obs) with obs of shape (n, d) (a view of
    the column-major buffer the engine takes as it is).  `lengths`: per-track row counts (ragged batch, <= n_steps).
    Raises without a GPU: there is no CPU fallback."""
    import torch
    lib = load_library()
    if model not in MODEL_CODES:
        raise ValueError("Unknown SDE type")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    M, T, d = int(n_tracks), int(n_steps), int(n_dim)
    row0 = None
    if lengths is not None:
        ln = torch.as_tensor(lengths, dtype=torch.int64, device=dev)
        if ln.numel() != M or int(ln.max()) > T or int(ln.min()) < 1:
            raise ValueError("lengths: one entry per track, 1 <= length <= n_steps")
        row0 = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        row0[1:] = torch.cumsum(ln, 0)
        n = int(row0[-1])
    else:
        n = M * T
    sd = SsdeSimDesc()
    sd.abi_version, sd.model, sd.n_dim, sd.n_steps = ABI_VERSION, MODEL_CODES[model], d, T
    sd.track0, sd.n_tracks, sd.n_rows = int(track0), M, n
    sd.row0 = None if row0 is None else row0.data_ptr()
    sd.row_offset = int(track0) * T if row_offset is None else int(row_offset)
    for k, v in enumerate(np.broadcast_to(np.asarray(mu, dtype=np.float64), (d,))):
        sd.mu[k] = float(v)
    for k, v in enumerate(np.broadcast_to(np.asarray(z0, dtype=np.float64), (d,))):
        sd.z0[k] = float(v)
    sd.tau, sd.nu, sd.kappa, sd.sigma, sd.sigma_obs, sd.dt = float(tau), float(nu), float(kappa), float(sigma), float(sigma_obs), float(dt)
    sd.seed, sd.device = int(seed) & 0xFFFFFFFFFFFFFFFF, int(dev.index or 0)
    obs = torch.empty((d, n), dtype=torch.float64, device=dev)
    ID = torch.empty(n, dtype=torch.float64, device=dev) if want_id_times else None
    times = torch.empty(n, dtype=torch.float64, device=dev) if want_id_times else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    st = lib.ssde_simulate(C.byref(sd), None if ID is None else ID.data_ptr(), None if times is None else times.data_ptr(),
                           obs.data_ptr(), stream)
    if st != 0:
        msg = lib.ssde_last_error(None)
        raise EngineError(f"ssde_simulate failed ({st}): {msg.decode() if msg else ''}")
    return ID, times, obs.t()



def par_bands(X_fe, X_re, link, coeff, level=0.95, resp=True, simultaneous=True, device_out=False, budget_mb=0, *, z=None,
              want=None, device=None):
    """ssde_par_bands: pointwise and simultaneous confidence bands of the SDE parameters from a table of posterior
    coefficient draws, reduced on the device.  `X_fe`, `X_re`: one block per parameter, (n, k) numpy arrays or device tensors (all of
    one kind) or None (the intercept / no random effects); `link`: 0 identity, 1 log per parameter; `coeff`: (1 + n_post, n_coef),
    row 0 the point estimate, parameter j's columns contiguous, fixed effects first.  Returns {"est", "pw_low", "pw_upp"} (n, q) and,
    with `simultaneous`, {"sim_low", "sim_upp"} (n, q), "crit" (q,), "max_dev" (q, n_post); the (n, q) entries are device tensors
    with `device_out`.  `want`: the names of the outputs to compute (None: all that `simultaneous` allows).  `z` defaults to the
    normal quantile of (1 + level) / 2."""
    import statistics
    lib = load_library()
    q = len(X_fe)
    if len(X_re) != q or len(link) != q:
        raise ValueError("par_bands: one entry per parameter in X_fe, X_re and link")
    blocks = [b for b in list(X_fe) + list(X_re) if b is not None]
    on_dev = [hasattr(b, "data_ptr") for b in blocks]
    if any(on_dev) and not all(on_dev):
        raise ValueError("par_bands: the blocks are all numpy arrays or all device tensors")
    dev_data = bool(blocks) and all(on_dev)
    torch = None
    if dev_data or device_out:
        import torch
    keep, n = [], None

    def block(b):
        nonlocal n
        if b is None:
            return None, 0
        if dev_data:
            if b.dtype != torch.float64 or b.dim() != 2:
                raise ValueError("par_bands: device blocks are 2-d float64 tensors")
            t = b.t().contiguous()                       # column-major (n, k) = row-major (k, n)
            keep.append(t)
            rows, cols, p = int(b.shape[0]), int(b.shape[1]), t.data_ptr()
        else:
            a = np.asfortranarray(np.asarray(b, dtype=np.float64))
            if a.ndim != 2:
                raise ValueError("par_bands: a block is an (n, k) array")
            keep.append(a)
            rows, cols, p = a.shape[0], a.shape[1], a.ctypes.data
        if n is not None and rows != n:
            raise ValueError("par_bands: blocks with different numbers of rows")
        n = rows
        return p, cols

    pf = [block(b) for b in X_fe]
    pr = [block(b) for b in X_re]
    cf = np.ascontiguousarray(coeff, dtype=np.float64)
    if cf.ndim != 2:
        raise ValueError("par_bands: coeff is (1 + n_post, n_coef)")
    if n is None:
        n = 1                                              # intercepts only: one row says it all
    kf = np.array([1 if p is None else k for p, k in pf], dtype=np.int32)
    kr = np.array([k for _, k in pr], dtype=np.int32)
    if int(kf.sum() + kr.sum()) != cf.shape[1]:
        raise ValueError("par_bands: coeff has not one column per design column")
    xf = (C.c_void_p * q)(*[p for p, _ in pf])
    xr = (C.c_void_p * q)(*[(p if k else None) for p, k in pr])
    lk = np.ascontiguousarray(link, dtype=np.uint8)
    d = SsdeBandsDesc()
    d.abi_version, d.n_par, d.n = ABI_VERSION, q, n
    d.ncol_fe, d.x_fe = kf.ctypes.data_as(C.POINTER(C.c_int32)), xf
    d.ncol_re, d.x_re = kr.ctypes.data_as(C.POINTER(C.c_int32)), xr
    d.link, d.coeff = lk.ctypes.data_as(C.POINTER(C.c_uint8)), cf.ctypes.data_as(_dp)
    d.n_post, d.resp, d.level = cf.shape[0] - 1, 1 if resp else 0, float(level)
    d.z = float(z) if z is not None else (statistics.NormalDist().inv_cdf((1.0 + float(level)) / 2.0) if 0.0 < float(level) < 1.0 else float("nan"))
    d.budget_mb = int(budget_mb)
    d.flags = (BANDS_DEVICE_DATA if dev_data else 0) | (BANDS_DEVICE_OUT if device_out else 0)
    if torch is not None:
        dv = blocks[0].device if dev_data else (torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
        d.device = int(dv.index or 0)
    else:
        d.device = -1 if device is None else int(device)
    row_names = ["est", "pw_low", "pw_upp"] + (["sim_low", "sim_upp"] if simultaneous else [])
    names = row_names + (["crit", "max_dev"] if simultaneous else [])
    if want is not None:
        if any(w not in names for w in want):
            raise ValueError(f"par_bands: want is a subset of {names}")
        names = [w for w in names if w in want]
    out, ptrs = {}, {}
    for nm in names:
        if nm == "crit":
            out[nm] = np.zeros(q)
        elif nm == "max_dev":
            out[nm] = np.zeros((q, max(d.n_post, 0)))
        elif device_out:
            out[nm] = torch.empty((q, n), dtype=torch.float64, device=dv)
        else:
            out[nm] = np.zeros((q, n))
        ptrs[nm] = out[nm].data_ptr() if hasattr(out[nm], "data_ptr") else out[nm].ctypes.data
    if torch is not None:
        torch.cuda.synchronize(dv)
    st = lib.ssde_par_bands(C.byref(d), *[ptrs.get(nm) for nm in ("est", "pw_low", "pw_upp", "sim_low", "sim_upp", "crit", "max_dev")])
    if st != 0:
        msg = lib.ssde_last_error(None)
        err = EngineError(f"ssde_par_bands failed ({st}): {msg.decode() if msg else ''}")
        err.status = st
        raise err
    return {nm: (v if nm in ("crit", "max_dev") else (v.t() if device_out else v.T)) for nm, v in out.items()}


def simulate_rows(model, n_dim, row0, times, X_fe, X_re, link, coeff, *, sigma_obs=None, z0=0.0, seed=0, rep0=0, n_rep=1,
                  thresholds=None, want=("obs", "stats"), device_out=False, budget_mb=0, device=None):
    """ssde_simulate_rows: `n_rep` replicate data sets simulated on the rows the arguments describe -- the reference's
    SDE$simulate with row-varying parameters, dt = diff(time) and the ID segments as tracks -- and the check statistics of every
    (track, replicate).  `row0`: (n_tracks + 1,) first row of every track; `times`: (n,); `X_fe`, `X_re`, `link` as par_bands'
    (parameters mu_1 .. mu_d, then sigma | tau, kappa | tau, nu); `coeff`: (1, n_coef) or (n_rep, n_coef), replicate k uses row k;
    `sigma_obs`: None, a number or one per coefficient row; replicate k is replicate number rep0 + k of the stream `seed`.
    Returns {"obs": (n_rep, n, d), "stats": (n_rep, n_tracks, 3 d + 2 + n_thr)} with the entries `want` names; "obs" is a device
    tensor with `device_out`.  Raises EngineError (with .status) where the C call fails; without a GPU every call that passes the
    argument checks raises: there is no CPU fallback."""
    lib = load_library()
    if model not in MODEL_CODES:
        raise ValueError("Unknown SDE type")
    want = tuple(want)
    if any(w not in ("obs", "stats") for w in want):
        raise ValueError('simulate_rows: want is a subset of ("obs", "stats")')
    q = len(X_fe)
    if len(X_re) != q or len(link) != q:
        raise ValueError("simulate_rows: one entry per parameter in X_fe, X_re and link")
    r0 = np.ascontiguousarray(row0, dtype=np.int64)
    tm = np.ascontiguousarray(times, dtype=np.float64)
    if r0.ndim != 1 or r0.size < 1 or tm.ndim != 1:
        raise ValueError("simulate_rows: row0 is (n_tracks + 1,) and times (n,)")
    n, M, d = int(tm.size), int(r0.size) - 1, int(n_dim)
    blocks = [b for b in list(X_fe) + list(X_re) if b is not None]
    on_dev = [hasattr(b, "data_ptr") for b in blocks]
    if any(on_dev) and not all(on_dev):
        raise ValueError("simulate_rows: the blocks are all numpy arrays or all device tensors")
    dev_data = bool(blocks) and all(on_dev)
    torch = None
    if dev_data or device_out:
        import torch
    keep = []

    def block(b):
        if b is None:
            return None, 0
        if dev_data:
            if b.dtype != torch.float64 or b.dim() != 2:
                raise ValueError("simulate_rows: device blocks are 2-d float64 tensors")
            t = b.t().contiguous()                       # column-major (n, k) = row-major (k, n)
            keep.append(t)
            rows, cols, p = int(b.shape[0]), int(b.shape[1]), t.data_ptr()
        else:
            a = np.asfortranarray(np.asarray(b, dtype=np.float64))
            if a.ndim != 2:
                raise ValueError("simulate_rows: a block is an (n, k) array")
            keep.append(a)
            rows, cols, p = a.shape[0], a.shape[1], a.ctypes.data
        if rows != n:
            raise ValueError("simulate_rows: a block has not one row per time")
        return p, cols

    pf = [block(b) for b in X_fe]
    pr = [block(b) for b in X_re]
    cf = np.ascontiguousarray(np.atleast_2d(np.asarray(coeff, dtype=np.float64)))
    if cf.ndim != 2:
        raise ValueError("simulate_rows: coeff is (1, n_coef) or (n_rep, n_coef)")
    kf = np.array([1 if p is None else k for p, k in pf], dtype=np.int32)
    kr = np.array([k for _, k in pr], dtype=np.int32)
    xf = (C.c_void_p * q)(*[p for p, _ in pf])
    xr = (C.c_void_p * q)(*[(p if k else None) for p, k in pr])
    lk = np.ascontiguousarray(link, dtype=np.uint8)
    so = None
    if sigma_obs is not None:
        so = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_obs, dtype=np.float64), (cf.shape[0],)))
    thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).ravel())
    ds = SsdeSimrowsDesc()
    ds.abi_version, ds.budget_mb, ds.model, ds.n_dim, ds.n_par = ABI_VERSION, int(budget_mb), MODEL_CODES[model], d, q
    ds.n, ds.n_tracks = n, M
    ds.row0, ds.times = r0.ctypes.data_as(C.POINTER(C.c_int64)), tm.ctypes.data_as(_dp)
    ds.ncol_fe, ds.x_fe = kf.ctypes.data_as(C.POINTER(C.c_int32)), xf
    ds.ncol_re, ds.x_re = kr.ctypes.data_as(C.POINTER(C.c_int32)), xr
    ds.link, ds.coeff = lk.ctypes.data_as(C.POINTER(C.c_uint8)), cf.ctypes.data_as(_dp)
    ds.n_coeff_rows, ds.n_coef = cf.shape[0], cf.shape[1]
    if so is not None:
        ds.sigma_obs = so.ctypes.data_as(_dp)
    for k, v in enumerate(np.broadcast_to(np.asarray(z0, dtype=np.float64), (min(max(d, 0), 8),))):
        ds.z0[k] = float(v)
    ds.seed, ds.rep0, ds.n_rep = int(seed) & 0xFFFFFFFFFFFFFFFF, int(rep0), int(n_rep)
    if thr.size:
        ds.thr = thr.ctypes.data_as(_dp)
    ds.n_thr = int(thr.size)
    ds.flags = (SIMROWS_DEVICE_DATA if dev_data else 0) | (SIMROWS_DEVICE_OUT if device_out else 0)
    dv = None
    if torch is not None:
        dv = blocks[0].device if dev_data else (torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
        ds.device = int(dv.index or 0)
    else:
        ds.device = -1 if device is None else int(device)
    n_stat = 3 * d + 2 + int(thr.size)
    R = max(int(n_rep), 0)
    obs = stats = None
    if "obs" in want:
        obs = torch.empty((R, max(d, 0), n), dtype=torch.float64, device=dv) if device_out else np.zeros((R, max(d, 0), n))
    if "stats" in want:
        stats = np.zeros((R, max(n_stat, 0), M))
    if torch is not None:
        torch.cuda.synchronize(dv)
    st = lib.ssde_simulate_rows(C.byref(ds), None if obs is None else (obs.data_ptr() if device_out else obs.ctypes.data),
                                None if stats is None else stats.ctypes.data)
    if st != 0:
        msg = lib.ssde_last_error(None)
        err = EngineError(f"ssde_simulate_rows failed ({st}): {msg.decode() if msg else ''}")
        err.status = st
        raise err
    out = {}
    if obs is not None:
        out["obs"] = obs.permute(0, 2, 1) if device_out else obs.transpose(0, 2, 1)
    if stats is not None:
        out["stats"] = stats.transpose(0, 2, 1)
    return out


class Engine:
    """One created engine (= one `MakeADFun` object of the reference): on one GPU, or -- `devices=[...]` -- sharded
    by whole tracks over several GPUs of this process (ssde_desc.n_devices; one RCCL all-reduce per evaluation)."""

    def __init__(self, problem: Problem, devices: Optional[Sequence[int]] = None):
        self.lib = load_library()
        self.problem = problem
        self._h = C.c_void_p()
        d = problem.desc()
        if devices is not None and len(devices) > 1:
            self._devices = np.ascontiguousarray(devices, dtype=np.int32)
            d.n_devices = len(self._devices)
            d.devices = self._devices.ctypes.data_as(_ip)
        st = self.lib.ssde_create(C.byref(d), C.byref(self._h))
        if st != 0:
            msg = self.lib.ssde_last_error(None)
            raise EngineError(f"ssde_create failed ({st}): {msg.decode() if msg else ''}")
        self.n_par_full = problem.n_par_full

    def _check(self, st):
        if st != 0:
            msg = self.lib.ssde_last_error(self._h)
            err = EngineError(f"ssde call failed ({st}): {msg.decode() if msg else ''}")
            err.status = int(st)
            raise err

    def lagstats(self):
        """The lag statistics this engine built at create, read back from the device: (M, s, n_bulk), or None when it built none
        (the host reference is lagstats_host)."""
        nt, a0 = C.c_int32(0), C.c_int32(0)
        self.lib.ssde_lagstats_host(None, None, 0, 1, None, None, None, C.byref(nt), C.byref(a0))
        M = np.zeros((nt.value, nt.value)); s = np.zeros((2, nt.value)); n = np.zeros(1)
        st = self.lib.ssde_lagstats_read(self._h, M.ctypes.data_as(_dp), s.ctypes.data_as(_dp), n.ctypes.data_as(_dp))
        if st != 0:
            return None
        return M, s, float(n[0])

    def lagstats_cut(self, cut):
        """(M, s, n_bulk) of the lag statistics the handle built for the first bulk row `cut` (ssde_lagstats_read_cut; the host
        reference is lagstats_host_cut)."""
        nt, a0 = C.c_int32(0), C.c_int32(0)
        self.lib.ssde_lagstats_host(None, None, 0, 1, None, None, None, C.byref(nt), C.byref(a0))
        M = np.zeros((nt.value, nt.value)); s = np.zeros((2, nt.value)); n = np.zeros(1)
        self._check(self.lib.ssde_lagstats_read_cut(self._h, int(cut), M.ctypes.data_as(_dp), s.ctypes.data_as(_dp), n.ctypes.data_as(_dp)))
        return M, s, float(n[0])

    def last_lag_cut(self):
        """The first bulk row of the last evaluation (ssde_last_lag_cut): 256 or an early cut; 0 where every row was streamed."""
        return int(self.lib.ssde_last_lag_cut(self._h))

    def lagstats_ref(self):
        """The value the statistics' levels are centred on (OU_SSM: y - ref, one number per response coordinate, fixed at create;
        zeros for CTCRW and BM_SSM, whose statistics are those of the increments), or None when the engine built no statistics."""
        nt, a0 = C.c_int32(0), C.c_int32(0)
        self.lib.ssde_lagstats_host(None, None, 0, 1, None, None, None, C.byref(nt), C.byref(a0))
        M = np.zeros((nt.value, nt.value)); s = np.zeros((2, nt.value)); n = np.zeros(1); ref = np.zeros(2)
        st = self.lib.ssde_lagstats_read_m(self._h, M.ctypes.data_as(_dp), s.ctypes.data_as(_dp), n.ctypes.data_as(_dp), ref.ctypes.data_as(_dp))
        if st != 0:
            return None
        return ref

    def info(self) -> dict:
        inf = SsdeInfo()
        self._check(self.lib.ssde_info(self._h, C.byref(inf)))
        return inf.as_dict()

    def eval(self, par, order: int = 1):
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        val = C.c_double()
        grad = np.zeros(self.n_par_full)
        self._check(self.lib.ssde_eval(self._h, par.ctypes.data_as(_dp), self.n_par_full, order,
                                       C.byref(val), grad.ctypes.data_as(_dp)))
        return (val.value, grad) if order >= 1 else val.value

    def comm_init(self, n_ranks: int, rank: int, unique_id: bytes):
        """Join this rank's engine with the other ranks' (one process per GPU): every later eval / eval_device returns
        the RCCL all-reduced batch result.  Collective: every rank calls it with the same id."""
        assert len(unique_id) == COMM_ID_BYTES
        buf = C.create_string_buffer(unique_id, COMM_ID_BYTES)
        self._check(self.lib.ssde_comm_init_rank(self._h, n_ranks, rank, buf))

    def laplace_eval(self, par, order: int = 1, want_hessian: bool = False, hess_step: float = 0.0, fd_step: float = 0.0,
                     newton_tol: float = 0.0, max_newton: int = 0):
        """Marginal nllk (coeff_re integrated out by the Laplace approximation, ssde_laplace_eval) at the outer entries
        of `par`, warm-started at its coeff_re entries.  Returns (value, grad, par_with_u_hat[, H_uu])."""
        p = np.array(par, dtype=np.float64)
        if p.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        val = C.c_double()
        grad = np.zeros(self.n_par_full)
        pb = self.problem
        nu = int(np.sum(pb.par_fixed[pb.off_re:pb.off_re + pb.n_re] == 0))
        H = np.zeros((nu, nu), order="F") if want_hessian else None
        opts = SsdeLaplaceOpts(hess_step, fd_step, newton_tol, max_newton, 0)
        self._check(self.lib.ssde_laplace_eval(self._h, p.ctypes.data_as(_dp), self.n_par_full, order, C.byref(val),
                                               grad.ctypes.data_as(_dp), None if H is None else H.ctypes.data_as(_dp),
                                               C.byref(opts)))
        out = (val.value, grad, p)
        return out + (H,) if want_hessian else out

    def bound_eval(self, order: int = 1):
        """ssde_eval with preallocated buffers and pre-resolved ctypes objects: call(par_array) -> (value, grad_view).
        For timing loops: `Engine.eval` spends ~5 us per call on argument conversion and a fresh gradient array."""
        val = C.c_double()
        grad = np.zeros(self.n_par_full)
        gp, vp, f, h, n = grad.ctypes.data_as(_dp), C.byref(val), self.lib.ssde_eval, self._h, self.n_par_full

        def call(par):
            st = f(h, par.ctypes.data_as(_dp), n, order, vp, gp)
            if st != 0:
                self._check(st)
            return val.value, grad

        return call

    def last_kernel_ms(self) -> float:
        return float(self.lib.ssde_last_kernel_ms(self._h))

    def kernel_ms_history(self, n: int) -> np.ndarray:
        """Dominant-kernel durations of the last n (<= 64) evaluations, most recent first; 0 where there is no stamp."""
        out = np.zeros(int(n))
        self._check(self.lib.ssde_kernel_ms_history(self._h, out.ctypes.data_as(_dp), int(n)))
        return out

    def last_phase_ms(self) -> dict:
        """Where the last stamped synchronous eval spent its time (ssde_last_phase_ms), in ms, by PHASE_NAMES."""
        out = np.zeros(8)
        self._check(self.lib.ssde_last_phase_ms(self._h, out.ctypes.data_as(_dp)))
        return dict(zip(PHASE_NAMES[:7], out[:7].tolist()))

    def comm_allreduce(self, buf_ptr: int, count: int, stream: int = 0):
        """Sum `count` doubles at the HBM address buf_ptr over the ranks of this handle's communicator (enqueue only)."""
        self._check(self.lib.ssde_comm_allreduce(self._h, C.c_void_p(buf_ptr), int(count), C.c_void_p(stream)))

    def hess(self, par, idx):
        """ssde_hess: exact second derivatives of the joint penalised nllk over the full-parameter indices `idx` -- what
        info()["exact_hess_scope"] says: 3 every free entry (state-space models on the lane = direction path -- row-varying
        coefficients, per-row H_array, ESEAL_SSM -- or created with FLAG_EXACT_HESS; track shards and communicator ranks summed),
        2 the coefficients of the direct families BM / OU / BM_t / CIR, decaying columns and log_decay included (+ log_lambda),
        1 the drift coefficients of a smooth-drift state-space
        batch (+ log_lambda), 0 nothing: EngineError with status 2, difference the gradient.  Returns an (len(idx), len(idx)) array."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        ix = np.ascontiguousarray(idx, dtype=np.int32)
        H = np.zeros((len(ix), len(ix)), order="F")
        self._check(self.lib.ssde_hess(self._h, par.ctypes.data_as(_dp), self.n_par_full, ix.ctypes.data_as(_ip), len(ix),
                                       H.ctypes.data_as(_dp)))
        return H

    def hess_plan(self):
        """What the last hess() ran on the hyper-dual lanes (ssde_last_hess_plan): {"warm_up": rows of the accepted attempt (0: one
        sequential window per track), "windows_max": the most windows a track was cut into, "attempts", "check": the accepted
        hand-over check}; the largest of each over shards or a companion; zeros before any call and where no windowed pass ran."""
        w, n, a, c = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.ssde_last_hess_plan(self._h, C.byref(w), C.byref(n), C.byref(a), C.byref(c)))
        return dict(warm_up=int(w.value), windows_max=int(n.value), attempts=int(a.value), check=float(c.value))

    def set_option(self, option: int, value: int):
        self._check(self.lib.ssde_set_option(self._h, option, value))

    def last_head_form(self) -> int:
        """the head of the last evaluation: 0 a launch, 1 its Gram statistics on the host (OPT_LAG_HEAD_HOST)"""
        return int(self.lib.ssde_last_head_form(self._h))

    def headstats(self):
        """(G, s, n) of the head's Gram statistics the handle built (ssde_headstats_read; the host reference is headstats_host)"""
        nw = head_components()
        G = np.zeros((nw, nw)); s = np.zeros((2, nw)); n = np.zeros(1)
        self._check(self.lib.ssde_headstats_read(self._h, G.ctypes.data_as(_dp), s.ctypes.data_as(_dp), n.ctypes.data_as(_dp)))
        return G, s, float(n[0])

    def last_finish_form(self) -> int:
        """What finished the last evaluation: 0 a finalize launch, 1 the main launch itself, 2 the host."""
        return int(self.lib.ssde_last_finish_form(self._h))

    def last_gain_feed(self) -> int:
        """How the last evaluation's main launch got its gain table: 0 a copy on the stream, 1 by value in its argument block."""
        return int(self.lib.ssde_last_gain_feed(self._h))

    def last_gain_rows(self) -> int:
        """Rows of the last evaluation's gain table (the covariance transient, in rows)."""
        return int(self.lib.ssde_last_gain_rows(self._h))

    def forget(self):
        """Drop the memoised last result: the next eval runs on the device even at the same par."""
        self._check(self.lib.ssde_forget(self._h))

    def widen_windows(self, factor: int = 4):
        self._check(self.lib.ssde_widen_windows(self._h, factor))

    def relax_windows(self):
        self._check(self.lib.ssde_relax_windows(self._h))

    def eval_device(self, par, out_ptr: int, order: int = 1, stream: int = 0):
        """Asynchronous evaluation of the data term into an HBM buffer of 2+n_par_full doubles:
        [nllk, grad..., window_check]; the caller rejects the result if window_check > WINDOW_TOL."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        self._check(self.lib.ssde_eval_device(self._h, par.ctypes.data_as(_dp), self.n_par_full, order,
                                              C.c_void_p(out_ptr), C.c_void_p(stream)))

    def penalty(self, par, want_grad: bool = True):
        par = np.ascontiguousarray(par, dtype=np.float64)
        val = C.c_double()
        grad = np.zeros(self.n_par_full)
        self._check(self.lib.ssde_penalty(self._h, par.ctypes.data_as(_dp), self.n_par_full, C.byref(val),
                                          grad.ctypes.data_as(_dp) if want_grad else None))
        return val.value, grad

    def report(self, par):
        par = np.ascontiguousarray(par, dtype=np.float64)
        out = np.zeros((self.problem.n, self.problem.sdim), order="F")
        self._check(self.lib.ssde_report(self._h, par.ctypes.data_as(_dp), self.n_par_full,
                                         out.ctypes.data_as(_dp)))
        return out

    def smooth(self, par, cov: bool = True, resid: bool = True) -> dict:
        """Fixed-interval smoother at `par` (ssde_smooth): {"mean": (n x sdim), "cov": (n x sdim x sdim) or None,
        "resid": (n x d) whitened one-step-ahead innovations or None}.  NaN on rows without a state (a track's first row) and, for
        "resid", on rows without an update (those, NA rows)."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        n, sd, d = self.problem.n, self.problem.sdim, self.problem.n_dim
        mean = np.zeros((n, sd), order="F")
        P = np.zeros((n, sd, sd), order="F") if cov else None
        e = np.zeros((n, d), order="F") if resid else None
        self._check(self.lib.ssde_smooth(self._h, par.ctypes.data_as(_dp), self.n_par_full, mean.ctypes.data_as(_dp),
                                         P.ctypes.data_as(_dp) if cov else None, e.ctypes.data_as(_dp) if resid else None))
        return {"mean": mean, "cov": P, "resid": e}

    def smooth_loo(self, par, cov: bool = True, thresholds=None, lpd: bool = True, stats: bool = True) -> dict:
        """Leave-one-out residuals and predictive densities at `par` (ssde_smooth_loo): what every OTHER fix of the
        track says about fix j.  {"mean": (n x d) E[y_j | y_-j], "cov": (n x d x d) its covariance or None, "resid": (n x d) the
        whitened deletion residuals (N(0, I) at every row, but not independent between rows), "lpd": (n,) log p(y_j | y_-j) or None,
        "stats": (n_tracks, 4 + n_thr) or None -- per track the served rows, the sum of lpd (its leave-one-out score), the largest
        q_j = |resid_j|^2, the row of the data (0-based) attaining it, then per threshold the served rows with q_j above it}.  NaN
        on rows that are not served (a track's first row, NA rows, rows without an update).  `thresholds`: at most LOO_MAX_THR finite
        numbers >= 0 on the q scale (chi-square quantiles with d degrees of freedom) or None.  An uncoupled wide response (column
        pairs) serves neither "lpd" nor "stats": pass lpd=False, stats=False there."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)
        if thr.ndim != 1:
            raise ValueError("thresholds must be a list of numbers")
        n, d, n_trk = self.problem.n, self.problem.n_dim, self.problem.n_seg
        mean = np.zeros((n, d), order="F")
        V = np.zeros((n, d, d), order="F") if cov else None
        e = np.zeros((n, d), order="F")
        lp = np.zeros(n) if lpd else None
        st = np.zeros((4 + len(thr), n_trk)) if stats else None                          # element (t, k) at t + n_tracks k
        self._check(self.lib.ssde_smooth_loo(self._h, par.ctypes.data_as(_dp), self.n_par_full, mean.ctypes.data_as(_dp),
                                             V.ctypes.data_as(_dp) if cov else None, e.ctypes.data_as(_dp),
                                             lp.ctypes.data_as(_dp) if lpd else None, thr.ctypes.data_as(_dp) if len(thr) else None,
                                             len(thr), st.ctypes.data_as(_dp) if stats else None, 0))
        return {"mean": mean, "cov": V, "resid": e, "lpd": lp, "stats": None if st is None else st.T}

    def forecast_scores(self, par, horizons, thresholds=None, z: bool = True, lpd: bool = True, stats: bool = True) -> dict:
        """Multi-step-ahead forecast errors and scores at `par` (ssde_forecast_scores): fix t predicted from the
        data through row t - k for every listed horizon k (strictly increasing, 1 .. AHEAD_MAX_STEP, at most AHEAD_MAX_H of them,
        counted in the caller's rows).  {"z": (n x d x n_h) whitened forecast errors or None, "lpd": (n x n_h) log predictive
        densities or None, "stats": (n_tracks, 5 + n_thr, n_h) or None -- per track and horizon the scored targets, the sums of
        lpd, of q = |z|^2, of the squared error and of the lead time, then per threshold the targets with q above it}.  NaN where
        a target is not scored (fewer than k rows into its track, a missing fix, no positive definite predictive covariance).
        `thresholds`: at most AHEAD_MAX_THR finite numbers >= 0 on the q scale, or None.  An uncoupled wide response (column pairs)
        serves "z" alone: pass lpd=False, stats=False there."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        hz = np.ascontiguousarray(horizons, dtype=np.int32)
        thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)
        if hz.ndim != 1 or thr.ndim != 1:
            raise ValueError("horizons and thresholds must be lists of numbers")
        n, d, n_trk, nh = self.problem.n, self.problem.n_dim, self.problem.n_seg, len(hz)
        zz = np.zeros((n, d, nh), order="F") if z else None
        lp = np.zeros((n, nh), order="F") if lpd else None
        st = np.zeros((nh, 5 + len(thr), n_trk)) if stats else None                       # element (t, s, j) at t + n_tracks (s + n_stat j)
        self._check(self.lib.ssde_forecast_scores(self._h, par.ctypes.data_as(_dp), self.n_par_full, hz.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  nh, zz.ctypes.data_as(_dp) if z else None, lp.ctypes.data_as(_dp) if lpd else None,
                                                  thr.ctypes.data_as(_dp) if len(thr) else None, len(thr),
                                                  st.ctypes.data_as(_dp) if stats else None, 0))
        return {"z": zz, "lpd": lp, "stats": None if st is None else np.ascontiguousarray(st.transpose(2, 1, 0))}

    def smooth_draws(self, par, n_draws: int, seed: int = 0, draw0: int = 0, out=None):
        """Joint posterior draws of the whole state path at `par` (ssde_smooth_draws): an array of shape
        (n_draws, n, sdim), draw k being draw number draw0 + k of the stream `seed`; NaN on rows without a state (a track's first
        row).  A draw is the same numbers whichever call, batch or device computes it.  `out`: a contiguous float64 torch tensor of
        that shape on the handle's device -- the draws are left in HBM (SSDE_DRAWS_DEVICE_OUT) and `out` is returned."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        n, sd = self.problem.n, self.problem.sdim
        if out is not None:
            import torch
            if tuple(out.shape) != (n_draws, sd, n) or not out.is_contiguous() or not out.is_cuda or out.dtype != torch.float64:
                raise ValueError("out must be a contiguous float64 device tensor of shape (n_draws, sdim, n): the C layout of the draws")
            self._check(self.lib.ssde_smooth_draws(self._h, par.ctypes.data_as(_dp), self.n_par_full, int(seed), int(draw0), int(n_draws),
                                                   C.c_void_p(out.data_ptr()), DRAWS_DEVICE_OUT))
            return out.transpose(1, 2)
        buf = np.zeros((max(int(n_draws), 0), sd, n))                                  # element (i, c, k) at i + n (c + sdim k)
        self._check(self.lib.ssde_smooth_draws(self._h, par.ctypes.data_as(_dp), self.n_par_full, int(seed), int(draw0), int(n_draws),
                                               buf.ctypes.data_as(C.c_void_p), 0))
        return buf.transpose(0, 2, 1)

    def predict(self, par, rows, offsets, cov: bool = True) -> dict:
        """The smoothed state at any time at `par` (ssde_predict).  Query k is (rows[k], offsets[k]): a row of the
        data (0-based) and an offset >= 0 past its time stamp -- inside the row's interval an interpolation, past a track's last row
        a forecast.  {"mean": (n_query x sdim), "cov": (n_query x sdim x sdim) or None}; NaN for a query on a track's first row, past
        the track's next fix, or on a row that rejected its update."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        offsets = np.ascontiguousarray(offsets, dtype=np.float64).ravel()
        if rows.shape != offsets.shape:
            raise ValueError("rows and offsets must have the same length")
        m, sd = len(rows), self.problem.sdim
        mean = np.zeros((m, sd), order="F")
        P = np.zeros((m, sd, sd), order="F") if cov else None
        self._check(self.lib.ssde_predict(self._h, par.ctypes.data_as(_dp), self.n_par_full, rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                          offsets.ctypes.data_as(_dp), m, mean.ctypes.data_as(_dp), P.ctypes.data_as(_dp) if cov else None))
        return {"mean": mean, "cov": P}

    def predict_draws(self, par, rows, offsets, n_draws: int, seed: int = 0, draw0: int = 0):
        """Joint posterior draws of the state at any time at `par` (ssde_predict_draws): an array of shape
        (n_draws, n_query, sdim).  Queries as predict's; draw k is draw number draw0 + k of the stream `seed`, the path smooth_draws
        returns for it, refined inside the intervals and continued past a track's last row.  The offsets of one interval must go
        into one call to be jointly distributed.  NaN where predict gives NaN."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        offsets = np.ascontiguousarray(offsets, dtype=np.float64).ravel()
        if rows.shape != offsets.shape:
            raise ValueError("rows and offsets must have the same length")
        m, sd = len(rows), self.problem.sdim
        buf = np.zeros((max(int(n_draws), 0), sd, m))                                  # element (k, c, q) at k + m (c + sdim q)
        self._check(self.lib.ssde_predict_draws(self._h, par.ctypes.data_as(_dp), self.n_par_full, rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                                offsets.ctypes.data_as(_dp), m, int(seed), int(draw0), int(n_draws),
                                                buf.ctypes.data_as(_dp), 0))
        return buf.transpose(0, 2, 1)

    def path_stats(self, par, n_draws: int, seed: int = 0, draw0: int = 0, regions=None, weight=None):
        """Summaries of posterior state paths at `par`, reduced on the device (ssde_path_stats): an array of shape
        (n_draws, n_tracks, n_stat), n_stat = 2 + n_regions -- path length, net displacement, then per region the sum of `weight`
        over the track's state rows whose position is inside.  Draw k is draw number draw0 + k of the stream `seed`, the path
        smooth_draws returns for it.  `regions`: (n_regions, 4) rows of lo_1, hi_1, lo_2, hi_2 (at most PATH_MAX_REGIONS; +-inf
        allowed) or None; `weight`: one number per row of the data, or None for 1.  NaN for a one-row track and for a (track, draw)
        with a non-finite position."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        if regions is None:
            reg = np.zeros((0, 4))
        else:
            reg = np.ascontiguousarray(regions, dtype=np.float64)
            if reg.ndim != 2 or reg.shape[1] != 4:
                raise ValueError("regions must have shape (n_regions, 4): lo_1, hi_1, lo_2, hi_2")
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.float64)
            if w.shape != (self.problem.n,):
                raise ValueError("weight must hold one number per row of the data")
        n_stat = 2 + len(reg)
        n_trk = self.problem.n_seg
        buf = np.zeros((max(int(n_draws), 0), n_stat, n_trk))                          # element (t, k, q) at t + n_tracks (k + n_stat q)
        self._check(self.lib.ssde_path_stats(self._h, par.ctypes.data_as(_dp), self.n_par_full, int(seed), int(draw0), int(n_draws),
                                             reg.ctypes.data_as(_dp) if len(reg) else None, len(reg),
                                             None if w is None else w.ctypes.data_as(_dp), buf.ctypes.data_as(_dp), 0))
        return buf.transpose(0, 2, 1)

    def path_speed(self, par, n_draws: int, seed: int = 0, draw0: int = 0, thresholds=None, weight=None, rows: bool = True):
        """Speed along posterior state paths of a CTCRW at `par`, reduced on the device (ssde_path_speed):
        (stats, row_below).  stats has shape (n_draws, n_tracks, n_stat), n_stat = 5 + n_thr -- the weighted sum of the speeds over
        the track's state rows, the largest speed, the row of the data (0-based) that attains it, the two components of the
        resultant sum of w v / |v|, then per threshold the sum of `weight` over the state rows with a speed at or below it.
        row_below has shape (n, n_thr), dtype uint32: per row of the data the number of the call's draws with a finite speed at or
        below each threshold (0 on rows without a state); None when `rows` is False or there is no threshold.  Draw k is draw
        number draw0 + k of the stream `seed`, the path smooth_draws returns for it.  `thresholds`: at most SPEED_MAX_THR numbers
        >= 0 (+inf allowed) or None; `weight`: one number per row of the data, or None for 1.  NaN for a one-row track and for a
        (track, draw) with a non-finite velocity."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        thr = np.zeros(0) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)
        if thr.ndim != 1:
            raise ValueError("thresholds must be a list of numbers")
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.float64)
            if w.shape != (self.problem.n,):
                raise ValueError("weight must hold one number per row of the data")
        n_stat = 5 + len(thr)
        n, n_trk = self.problem.n, self.problem.n_seg
        buf = np.zeros((max(int(n_draws), 0), n_stat, n_trk))                          # element (t, k, q) at t + n_tracks (k + n_stat q)
        cnt = np.zeros((len(thr), n), dtype=np.uint32) if (rows and len(thr)) else None   # element (j, r) at j + n r
        self._check(self.lib.ssde_path_speed(self._h, par.ctypes.data_as(_dp), self.n_par_full, int(seed), int(draw0), int(n_draws),
                                             thr.ctypes.data_as(_dp) if len(thr) else None, len(thr),
                                             None if w is None else w.ctypes.data_as(_dp), buf.ctypes.data_as(_dp),
                                             None if cnt is None else cnt.ctypes.data_as(C.POINTER(C.c_uint32)), 0))
        return buf.transpose(0, 2, 1), (None if cnt is None else cnt.T)

    def path_occupancy(self, par, n_draws: int, grid, seed: int = 0, draw0: int = 0, weight=None, group=None, n_groups=None,
                       force_global: bool = False):
        """The weighted time posterior state paths at `par` spend in every cell of a regular grid, summed on the device
        (ssde_path_occupancy): (occ, outside) with occ of shape (n_groups, ny, nx) and outside of shape (n_groups,),
        the weight that fell in no cell.  `grid`: a dict (or anything indexable by name) with x0, dx, nx and, for two position
        columns, y0, dy, ny; the cell of a position is floor((p - x0) / dx), floor((p - y0) / dy).  Draw k is draw number draw0 + k of
        the stream `seed`, the path smooth_draws returns.  `weight`: one finite number >= 0 per row of the data, or None for 1;
        `group`: one label per track in -1 ... n_groups - 1 (-1: the track is left out), or None for one pooled grid; `n_groups`
        defaults to max(group) + 1.  The sums are integers of a fixed quantum: the same bits whatever the chunking, the devices
        or the kernel form (`force_global` picks the form that adds straight into HBM)."""
        return self._occupancy(None, par, n_draws, grid, seed, draw0, weight, group, n_groups, force_global)

    def path_occupancy_fine(self, par, n_draws: int, grid, max_step: float, seed: int = 0, draw0: int = 0, weight=None, group=None,
                            n_groups=None, force_global: bool = False):
        """path_occupancy on the paths refined between the fixes (ssde_path_occupancy_fine): every interval longer than
        `max_step` is cut into m = min(OCC_MAX_SUB, ceil(interval / max_step)) equal sub-steps, the draw's state at the m - 1 inner
        times is the one predict_draws returns for those offsets, and the row's weight is shared equally among the interval's m
        points (whole quanta; the remainder stays with the row's own point).  Everything else, and the result's shape, is
        path_occupancy's; max_step = inf places every weight as path_occupancy does, bit for bit.  The same bits whatever the
        chunking, the devices or the kernel form; the sums of calls over parts of a draw range equal the whole range's call only to
        within the bound of include/ssde.h (rule 5), since a share is a whole number of a quantum that depends on n_draws."""
        return self._occupancy(float(max_step), par, n_draws, grid, seed, draw0, weight, group, n_groups, force_global)

    def _occupancy(self, max_step, par, n_draws, grid, seed, draw0, weight, group, n_groups, force_global):
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        g = SsdeOccGrid(float(grid["x0"]), float(grid["dx"]), float(grid.get("y0", 0.0)), float(grid.get("dy", 1.0)),
                        int(grid["nx"]), int(grid.get("ny", 1)))
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.float64)
            if w.shape != (self.problem.n,):
                raise ValueError("weight must hold one number per row of the data")
        grp = None
        if group is not None:
            grp = np.ascontiguousarray(group, dtype=np.int32)
            if grp.shape != (self.problem.n_seg,):
                raise ValueError("group must hold one label per track")
            if n_groups is None:
                n_groups = int(grp.max(initial=0)) + 1
        ng = 1 if n_groups is None else int(n_groups)
        occ = np.zeros((max(ng, 0), max(g.ny, 0), max(g.nx, 0)))                        # element (ix, iy, g) at ix + nx (iy + ny g)
        outside = np.zeros(max(ng, 0))
        head = (self._h, par.ctypes.data_as(_dp), self.n_par_full, int(seed), int(draw0), int(n_draws), C.byref(g))
        tail = (None if w is None else w.ctypes.data_as(_dp), None if grp is None else grp.ctypes.data_as(C.POINTER(C.c_int32)), ng,
                occ.ctypes.data_as(_dp), outside.ctypes.data_as(_dp), OCC_FORCE_GLOBAL if force_global else 0)
        if max_step is None:
            self._check(self.lib.ssde_path_occupancy(*head, *tail))
        else:
            self._check(self.lib.ssde_path_occupancy_fine(*head, max_step, *tail))
        return occ, outside

    def last_occupancy_form(self) -> int:
        """The kernel forms of the last path_occupancy (ssde_last_occupancy_form): 0 none yet, 1 the LDS-tile form in every wavefront
        group, 2 the global form in every group, 3 both.  path_occupancy_fine reports here too."""
        return int(self.lib.ssde_last_occupancy_form(self._h))

    def last_occupancy_points(self):
        """(n_points, n_capped) of the last path_occupancy_fine (ssde_last_occupancy_points): the path points per draw that carried
        weight, and the intervals whose sub-steps were cut to OCC_MAX_SUB."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.ssde_last_occupancy_points(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def path_proximity(self, par, qa_rows, qa_offs, qb_rows, qb_offs, pair_ptr, n_draws: int, seed: int = 0, draw0: int = 0,
                       radii=None, weight=None):
        """How close the posterior paths of two tracks come, reduced on the device (ssde_path_proximity): an array
        of shape (n_draws, n_pairs, n_stat), n_stat = 2 + n_radii.  Point i compares the query (qa_rows[i], qa_offs[i]) with
        (qb_rows[i], qb_offs[i]), both queries of predict_draws; pair p owns the points pair_ptr[p] .. pair_ptr[p + 1] - 1.  Per pair
        and draw: the smallest distance between the two drawn positions, the index inside the pair of the first point that attains
        it, then per radius the sum of `weight` (one finite number >= 0 per point, or None for 1) over the points within it.  Draw k
        is draw number draw0 + k of the stream `seed`: the states are the ones predict_draws returns for the A queries followed by
        the B queries.  The sums are integers of a fixed quantum that does not depend on n_draws: the same bits whatever the
        chunking, the devices or how a draw range is cut over calls.  NaN for an empty pair and for a (pair, draw) with a position
        that is not finite (a query on a track's first row)."""
        par = np.ascontiguousarray(par, dtype=np.float64)
        if par.shape != (self.n_par_full,):
            raise ValueError(f"par must have length {self.n_par_full}")
        ra, rb, pp = (np.ascontiguousarray(v, dtype=np.int64).ravel() for v in (qa_rows, qb_rows, pair_ptr))
        oa, ob = (np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (qa_offs, qb_offs))
        if not (ra.shape == rb.shape == oa.shape == ob.shape):
            raise ValueError("the four query arrays must have the same length")
        if len(pp) < 1 or (len(pp) > 1 and int(pp[-1]) != len(ra)):
            raise ValueError("pair_ptr must hold n_pairs + 1 entries and end at the number of points")
        rad = np.zeros(0) if radii is None else np.ascontiguousarray(radii, dtype=np.float64).ravel()
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.float64)
            if w.shape != ra.shape:
                raise ValueError("weight must hold one number per point")
        n_pairs, n_stat = len(pp) - 1, 2 + len(rad)
        lp = C.POINTER(C.c_int64)
        buf = np.zeros((max(int(n_draws), 0), max(n_stat, 0), max(n_pairs, 0)))         # element (p, k, q) at p + n_pairs (k + n_stat q)
        self._check(self.lib.ssde_path_proximity(self._h, par.ctypes.data_as(_dp), self.n_par_full, int(seed), int(draw0), int(n_draws),
                                                 ra.ctypes.data_as(lp), oa.ctypes.data_as(_dp), rb.ctypes.data_as(lp), ob.ctypes.data_as(_dp),
                                                 pp.ctypes.data_as(lp), n_pairs, None if w is None else w.ctypes.data_as(_dp),
                                                 rad.ctypes.data_as(_dp) if len(rad) else None, len(rad), buf.ctypes.data_as(_dp), 0))
        return buf.transpose(0, 2, 1)

    def last_proximity_plan(self):
        """Of the last path_proximity (ssde_last_proximity_plan): a dict with n_tiles (every pair is cut into tiles of 256 points),
        tiles_max (the most tiles of one pair), n_batches (of draws) and route (1: the positions never left the device, 2: they were
        gathered from the shards of a multi-device handle); zeros before any call."""
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
        self._check(self.lib.ssde_last_proximity_plan(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"n_tiles": int(a.value), "tiles_max": int(b.value), "n_batches": int(c.value), "route": int(d.value)}

    def close(self):
        if self._h:
            self.lib.ssde_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def forecast_scores(engine, par, horizons, thresholds=None, z=True, lpd=True, stats=True):
    """Engine.forecast_scores as a function of the engine (ssde_forecast_scores)"""
    return engine.forecast_scores(par, horizons, thresholds=thresholds, z=z, lpd=lpd, stats=stats)
