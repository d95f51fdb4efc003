"""Host-side mirror of the reference's `SDE` R6 class for the nllk/gradient path.

The reference host is R (`SDE$new`, `$setup()`, `$fit()`, `logLik.SDE`:
/root/reference/R/sde.R:45-182, 491-720, R/utility.R:115-123).  R is not in this image, so
this module restates that surface in Python with the same names, argument meaning and error
behaviour; the R glue that a maintainer would drop into the package is R_glue/ (see
INTEGRATION.md).  What changes underneath: `$setup()` builds an `Engine` (HIP, via the C ABI)
instead of calling `TMB::MakeADFun`, and returns an object with the same `par`, `fn`, `gr`
members that `$fit()` hands to a BFGS optimiser (the reference uses `optim(method = "BFGS")`,
R/sde.R:694-697).

Out of scope here, as in SURVEY.md: mgcv smooth construction (stays in R; a B-spline stand-in
is provided for `s(x, k=)` and an identity-penalised indicator block for `s(ID, bs="re")`),
sdreport, plotting, posterior simulation.  The Laplace approximation over `coeff_re`
(`random = "coeff_re"`, R/sde.R:522) is provided by `smoothsde_amd.laplace` on top of the GPU
gradient (finite-difference Hessian / outer gradient instead of TMB's AD).
"""
from __future__ import annotations

import re
import time
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import capi
from .synth import bspline_basis, second_difference_penalty

PAR_NAMES = {
    "BM": lambda d: _mu_names(d) + ["sigma"],
    "BM_t": lambda d: ["mu", "sigma"],                   # R/sde.R:61
    "BM_SSM": lambda d: _mu_names(d) + ["sigma"],
    "ESEAL_SSM": lambda d: ["mu", "sigma"],              # R/sde.R:70
    "OU": lambda d: _mu_names(d) + ["tau", "kappa"],
    "OU_SSM": lambda d: _mu_names(d) + ["tau", "kappa"],
    "CIR": lambda d: _mu_names(d) + ["beta", "sigma"],   # R/sde.R:66-67 (every parameter on the log scale)
    "CTCRW": lambda d: _mu_names(d) + ["tau", "nu"],
}


def _mu_names(d):  # c(mu = lapply(1:n_dim, ...)) names: "mu" for one dimension, "mu1", "mu2", ... otherwise
    return ["mu"] if d == 1 else [f"mu{i + 1}" for i in range(d)]


class Design:
    """Pre-built design blocks of one SDE parameter (what mgcv::gam(fit=FALSE) gives the reference,
    R/sde.R:396-424): X_fe (n x nsdf, first column the intercept), X_re (n x k) and the penalty
    blocks S (one per smooth, sizes adding up to k)."""

    def __init__(self, X_fe=None, X_re=None, S: Optional[Sequence] = None, names_fe=None, names_re=None):
        self.X_fe = None if X_fe is None else np.asarray(X_fe, dtype=np.float64)
        self.X_re = None if X_re is None else np.asarray(X_re, dtype=np.float64)
        self.S = [] if S is None else [np.asarray(s, dtype=np.float64) for s in S]
        self.names_fe, self.names_re = names_fe, names_re


def _parse_formula(form: str, data: Dict[str, np.ndarray], n: int) -> Design:
    """Tiny stand-in for mgcv's formula interface: `~ 1`, `~ x1 + x2`, `s(x, k = K)`, `s(ID, bs = "re")`."""
    rhs = form.strip()
    if rhs.startswith("~"):
        rhs = rhs[1:]
    terms = [t.strip() for t in re.split(r"\+(?![^()]*\))", rhs) if t.strip()]
    X_fe, names_fe = [np.ones(n)], ["(Intercept)"]
    X_re, S, names_re = [], [], []
    for t in terms:
        if t == "1":
            continue
        m = re.fullmatch(r"s\(\s*([A-Za-z_][\w.]*)\s*(?:,(.*))?\)", t)
        if m:
            var, opts = m.group(1), (m.group(2) or "")
            if var not in data:
                raise KeyError(f"variable '{var}' not found in 'data'")
            if re.search(r"bs\s*=\s*[\"']re[\"']", opts):
                codes, inv = np.unique(np.asarray(data[var]), return_inverse=True)
                Z = np.zeros((n, len(codes)))
                Z[np.arange(n), inv] = 1.0
                X_re.append(Z)
                S.append(np.eye(len(codes)))
                names_re += [f"s({var}).{i + 1}" for i in range(len(codes))]
            else:
                km = re.search(r"k\s*=\s*(\d+)", opts)
                k = int(km.group(1)) if km else 10
                x = np.asarray(data[var], dtype=np.float64)
                lo, hi = np.nanmin(x), np.nanmax(x)
                xs = (x - lo) / (hi - lo) if hi > lo else np.zeros_like(x)
                # k B-splines with the sum-to-zero constraint absorbed as mgcv does (k - 1 columns): without it the
                # columns add up to the intercept and the marginal likelihood is flat along that direction
                B = bspline_basis(xs, n_basis=k)
                Sk = second_difference_penalty(k)
                Q, _ = np.linalg.qr(B.sum(axis=0)[:, None], mode="complete")
                Z = Q[:, 1:]                                   # null space of the constraint 1'B c = 0
                Sz = Z.T @ Sk @ Z
                if re.search(r"bs\s*=\s*[\"'](ts|cs)[\"']", opts):
                    # shrinkage smooths (the vignette's bs = "ts"): the penalty's null space gets a small eigenvalue
                    w, V = np.linalg.eigh(0.5 * (Sz + Sz.T))
                    pos = w > 1e-8 * w[-1]
                    w = np.where(pos, w, 0.1 * w[pos].min())
                    Sz = (V * w) @ V.T
                X_re.append(B @ Z)
                S.append(Sz)
                names_re += [f"s({var}).{i + 1}" for i in range(k - 1)]
        else:
            if t not in data:
                raise KeyError(f"variable '{t}' not found in 'data'")
            X_fe.append(np.asarray(data[t], dtype=np.float64))
            names_fe.append(t)
    return Design(np.column_stack(X_fe), np.column_stack(X_re) if X_re else None, S, names_fe, names_re)


class TmbObj:
    """The members of a `MakeADFun` object that the reference uses: `par`, `fn`, `gr` over the FREE
    parameters (fixed ones are held at their values, TMB's `map`).  `fn`/`gr` arrive as separate
    calls with the same x (R/sde.R:694-697): one GPU evaluation serves both."""

    def __init__(self, engine, par_full: np.ndarray, free: np.ndarray):
        self.engine = engine
        self.par_full = np.array(par_full, dtype=np.float64)
        self.free = free
        self.par = self.par_full[free].copy()
        self._last_x = None
        self._last = None
        self.n_eval = 0

    def _eval(self, x):
        x = np.asarray(x, dtype=np.float64)
        if self._last_x is None or not np.array_equal(x, self._last_x):
            full = self.par_full.copy()
            full[self.free] = x
            val, grad = self.engine.eval(full, order=1)
            self._last_x, self._last = x.copy(), (val, grad[self.free])
            self.n_eval += 1
        return self._last

    def fn(self, x=None):
        return self._eval(self.par if x is None else x)[0]

    def gr(self, x=None):
        return self._eval(self.par if x is None else x)[1]

    def he(self, x=None):
        """Hessian over the free parameters by central differences of the GPU gradient (`tmb_obj$he`,
        used by edf_conditional, R/sde.R:1363)."""
        from .report import fd_hessian
        return fd_hessian(self.gr, self.par if x is None else np.asarray(x, dtype=np.float64))


class SDE:
    def __init__(self, formulas=None, data=None, type=None, response=None, par0=None, fixpar=None, other_data=None):
        if data is None or type is None or response is None:
            raise TypeError("SDE(formulas, data, type, response, ...) needs data, type and response")
        self.type_ = type
        self.response_ = [response] if isinstance(response, str) else list(response)
        self.fixpar_ = None if fixpar is None else list(fixpar)
        self.other_data_ = other_data or {}
        if hasattr(data, "to_dict") and hasattr(data, "columns"):
            data = {c: data[c].to_numpy() for c in data.columns}
        data = dict(data)
        if any(r not in data for r in self.response_):
            raise ValueError("'response' not found in 'data'")          # R/sde.R:51-52
        if type in capi.UNSUPPORTED_MODELS:
            raise NotImplementedError(f"SDE type {type!r} is outside this engine's scope")
        if type not in PAR_NAMES:
            raise ValueError("Unknown SDE type")
        n_dim = len(self.response_)
        names = PAR_NAMES[type](n_dim)
        if formulas is None:
            formulas = {k: "~1" for k in names}                         # R/sde.R:93-94
        elif len(formulas) != len(names):
            raise ValueError(f"'formulas' should be a list of length {len(names)} for the model {type}, "
                             f"with components {', '.join(names)}")    # R/sde.R:95-100
        elif list(formulas.keys()) != names:
            raise ValueError(f"'formulas' should be a list with components {', '.join(names)}")
        if self.fixpar_:
            for f in self.fixpar_:
                if not (isinstance(formulas[f], str) and formulas[f].replace(" ", "") == "~1"):
                    raise ValueError("formulas should be ~1 for fixed parameters")   # R/sde.R:106-108
        self.formulas_ = dict(formulas)
        n = len(np.asarray(data[self.response_[0]]))
        if "ID" not in data:
            warnings.warn("No ID column found in 'data', assuming same ID for all observations")  # R/sde.R:112-115
            data["ID"] = np.ones(n)
        if "time" not in data:
            raise ValueError("'data' should have a time column")        # R/sde.R:121-123
        self.data_ = data
        self.n_ = n
        self.names_ = names
        self.make_mat()
        self.coeff_fe_ = np.zeros(int(np.sum(self.terms_["ncol_fe"])))   # R/sde.R:138-140
        self.coeff_re_ = np.zeros(int(np.sum(self.terms_["ncol_re_par"])))
        self.lambda_vals_ = np.ones(len(self.terms_["ncol_re"]))
        if par0 is not None:
            if len(par0) != len(names):
                raise ValueError(f"'par0' should be of length {len(names)} with one entry for each SDE parameter "
                                 f"({', '.join(names)})")               # R/sde.R:147-151
            i0 = np.concatenate([[0], np.cumsum(self.terms_["ncol_fe"])[:-1]]).astype(int)
            for i, nm in enumerate(names):                               # link: identity for mu*, log otherwise
                identity = nm.startswith("mu") and type != "CIR"          # CIR: log link for mu too (R/sde.R:66)
                self.coeff_fe_[i0[i]] = par0[i] if identity else np.log(par0[i])
        self.tmb_obj_ = None
        self.tmb_obj_joint_ = None
        self.tmb_rep_ = None
        self.out_ = None
        self.engine_ = None

    # -- accessors (R/sde.R:188-360) --------------------------------------------------------------
    def formulas(self): return self.formulas_
    def data(self): return self.data_
    def type(self): return self.type_
    def response(self): return self.response_
    def fixpar(self): return self.fixpar_
    def coeff_fe(self): return self.coeff_fe_
    def coeff_re(self): return self.coeff_re_
    def lambda_(self): return self.lambda_vals_    # `lambda` is a Python keyword
    def terms(self): return self.terms_
    def mats(self): return self.mats_
    def out(self): return self.out_
    def tmb_obj(self): return self.tmb_obj_
    def tmb_obj_joint(self): return self.tmb_obj_joint_
    def tmb_rep(self): return self.tmb_rep_

    def obs(self):
        return np.column_stack([np.asarray(self.data_[r], dtype=np.float64) for r in self.response_])

    def ind_fixcoeff(self):
        """Indices (in coeff_fe) of the coefficients of fixed SDE parameters (R/sde.R ind_fixcoeff)."""
        if not self.fixpar_:
            return np.zeros(0, dtype=int)
        i0 = np.concatenate([[0], np.cumsum(self.terms_["ncol_fe"])[:-1]]).astype(int)
        return np.array([i0[self.names_.index(f)] for f in self.fixpar_], dtype=int)

    # -- design matrices (R/sde.R:378-455) -------------------------------------------------------------
    def make_mat(self):
        designs: List[Design] = []
        for nm in self.names_:
            f = self.formulas_[nm]
            designs.append(f if isinstance(f, Design) else _parse_formula(f, self.data_, self.n_))
        ncol_fe = [1 if d.X_fe is None else d.X_fe.shape[1] for d in designs]
        ncol_re_par = [0 if d.X_re is None else d.X_re.shape[1] for d in designs]
        ncol_re = [s.shape[0] for d in designs for s in d.S]
        self.designs_ = designs
        self.terms_ = dict(ncol_fe=np.array(ncol_fe), ncol_re=np.array(ncol_re, dtype=int),
                           ncol_re_par=np.array(ncol_re_par))
        self.mats_ = dict(X_list_fe=[d.X_fe for d in designs], X_list_re=[d.X_re for d in designs],
                          S_list=[s for d in designs for s in d.S])
        return self.mats_

    # -- TMB setup counterpart (R/sde.R:491-670) -----------------------------------------------------------
    def _problem(self, include_penalty=1, fix_lambda=True, **over):
        X_fe = []
        for d in self.designs_:
            # an intercept-only block is passed as "no column" (broadcast), SURVEY 7.3-5
            X_fe.append(None if (d.X_fe is None or (d.X_fe.shape[1] == 1 and np.all(d.X_fe == 1.0))) else d.X_fe)
        X_re = [d.X_re for d in self.designs_]
        kw = dict(a0=None, P0=self.other_data_.get("P0"), H=self.other_data_.get("H"), include_penalty=include_penalty,
                  other_data=self.other_data_.get("df") if self.type_ == "BM_t" else None)   # R/sde.R:539-541
        if self.type_ == "ESEAL_SSM":                          # R/sde.R:599-614: a0 = (1, first dep_fat of every track)
            ids = np.asarray(self.data_["ID"])
            first = np.r_[True, ids[1:] != ids[:-1]]
            kw.update(a0=np.column_stack([np.ones(first.sum()), np.asarray(self.data_["dep_fat"], dtype=float)[first]]),
                      P0=np.diag([0.0, 10.0]), eseal_h=self.data_["h"], eseal_R=self.data_["R"])
        if self.other_data_.get("t_decay") is not None:        # decaying response model, R/sde.R:635-644 (1-based in R)
            kw.update(t_decay=self.other_data_["t_decay"],
                      col_decay=np.asarray(self.other_data_["col_decay"], dtype=int) - 1,
                      ind_decay=np.asarray(self.other_data_["ind_decay"], dtype=int) - 1)
        kw.update(over)
        pb = capi.Problem(self.type_, self.data_["ID"], self.data_["time"], self.obs(), X_fe, X_re,
                          self.mats_["S_list"], **kw)
        fixed = pb.par_fixed.copy()
        for k in self.ind_fixcoeff():                      # map$coeff_fe with NA for fixed coefficients
            fixed[pb.off_fe + k] = 1
        if fix_lambda:                                     # joint fit: smoothing parameters held at their values
            fixed[pb.off_lambda:pb.off_lambda + pb.n_smooth] = 1
        pb.par_fixed = fixed
        return pb

    def _par_full(self, pb):
        p = np.zeros(pb.n_par_full)
        if pb.lead_names == ["log_sigma_obs"]:
            p[0] = 0.0                                      # log_sigma_obs = 0 (R/sde.R:560, 590)
        elif self.type_ == "ESEAL_SSM":
            p[0:3] = [np.log(1.0), -0.578, np.log(1.214)]   # ssm_par, R/sde.R:606-608
        p[pb.off_fe:pb.off_fe + pb.n_fe] = self.coeff_fe_
        p[pb.off_lambda:pb.off_lambda + pb.n_smooth] = np.log(self.lambda_vals_)
        if pb.n_decay:
            p[pb.off_decay:pb.off_decay + pb.n_decay] = np.log(getattr(self, "rho_", np.ones(pb.n_decay)))   # R/sde.R:177
        p[pb.off_re:pb.off_re + pb.n_re] = self.coeff_re_
        return p

    def setup(self, silent=True, map=None, laplace=None):
        """laplace=None: integrate coeff_re out (Laplace approximation, like `random = "coeff_re"` in the
        reference, R/sde.R:522) whenever there are random effects; laplace=False: joint penalised
        likelihood with the smoothing parameters held fixed."""
        has_re = len(self.mats_["S_list"]) > 0
        self.laplace_ = has_re if laplace is None else (bool(laplace) and has_re)
        pb = self._problem(include_penalty=1, fix_lambda=not self.laplace_)
        self.problem_ = pb
        if self.laplace_:                                  # exact H_uu / H_u,theta wherever the batch is evaluated (include/ssde.h)
            pb.flags |= capi.FLAG_EXACT_HESS
        self.engine_ = capi.Engine(pb)
        self.joint_obj_ = TmbObj(self.engine_, self._par_full(pb), pb.free_index())   # all free parameters, fixed + random
        self.tmb_obj_ = self.joint_obj_
        if self.laplace_:
            from .laplace import EngineLaplaceObjective
            free = set(pb.free_index().tolist())
            idx_r = [k for k in range(pb.off_re, pb.off_re + pb.n_re) if k in free]
            idx_o = [k for k in sorted(free) if k not in set(idx_r)]
            # fn / gr = ssde_laplace_eval: the entry point an R or C host uses for random = "coeff_re"
            self.tmb_obj_ = EngineLaplaceObjective(self.engine_, self._par_full(pb), idx_o, idx_r)
        # joint object "excluding penalty" (R/sde.R:663-669): include_penalty = 0 is honoured by the
        # direct families only (Q7); the Kalman families share the same engine
        if pb.kalman or pb.n_smooth == 0:
            self.tmb_obj_joint_ = self.joint_obj_
        else:
            pbj = self._problem(include_penalty=0, fix_lambda=not self.laplace_)
            self.engine_joint_ = capi.Engine(pbj)
            self.tmb_obj_joint_ = TmbObj(self.engine_joint_, self._par_full(pbj), pbj.free_index())
        return self.tmb_obj_

    def fit(self, silent=True, map=None, maxiter=200, optimizer="scipy", staged=True):
        """optimizer = "scipy": scipy's BFGS; "optim": R's optim(method = "BFGS") restated (smoothsde_amd/optim.py, the
        reference's own call, R/sde.R:694-697 -- pure backtracking from a unit step along -g, which on n >> 10^3 rows
        first jumps to absurd log-scale values exactly as it does in R).
        staged: with random effects, first fit the fixed effects alone (coeff_re = 0, log_lambda at its start) and
        start the Laplace fit from there.  The reference starts the Laplace fit directly from par0 with
        log_sigma_obs = 0; with a finite-difference Laplace layer that start is outside the region where the inner
        problem is well conditioned."""
        if self.tmb_obj_ is None:
            self.setup(silent=silent, map=map)
        if self.problem_.n_smooth > 0 and not self.laplace_:
            warnings.warn("random effects present: optimising the joint penalised likelihood with the smoothing "
                          "parameters fixed (setup(laplace=False)); the default integrates them out (Laplace)")
        obj = self.tmb_obj_
        t0 = time.perf_counter()

        def _minimise(fn, gr, x0):
            if optimizer == "scipy":
                from scipy.optimize import minimize
                r = minimize(fn, x0, jac=gr, method="BFGS", options=dict(maxiter=maxiter))
                return dict(par=r.x, value=r.fun, counts=(r.nfev, r.njev), convergence=int(not r.success), message=r.message)
            from .optim import optim_bfgs
            out = optim_bfgs(fn, gr, x0, maxit=maxiter)
            out["message"] = None
            return out

        if self.laplace_ and staged:
            pbk = self.problem_
            not_lam = np.array([not (pbk.off_lambda <= k < pbk.off_lambda + pbk.n_smooth) for k in obj.io])
            if not_lam.any():
                u0 = np.zeros(len(obj.ir))
                memo = {}

                def _j1(x):
                    key = x.tobytes()
                    if key not in memo:
                        memo.clear()
                        th = obj.par.copy()
                        th[not_lam] = x
                        v, g = obj.joint(obj._full(th, u0))
                        memo[key] = (v, g[obj.io][not_lam])
                    return memo[key]
                r1 = _minimise(lambda x: _j1(np.asarray(x, dtype=np.float64))[0],
                               lambda x: _j1(np.asarray(x, dtype=np.float64))[1], obj.par[not_lam].copy())
                if np.isfinite(r1["value"]):
                    obj.par[not_lam] = r1["par"]
                    obj.u_hat = u0.copy()
        if optimizer not in ("scipy", "optim"):
            raise ValueError("optimizer must be 'scipy' or 'optim'")
        self.out_ = _minimise(obj.fn, obj.gr, obj.par)
        self.out_["systime"] = time.perf_counter() - t0

        xhat = np.asarray(self.out_["par"], dtype=np.float64)
        full = obj.par_full.copy()
        if self.laplace_:
            full[obj.io] = xhat
            obj.fn(xhat)
            full[obj.ir] = obj.u_hat
        else:
            full[obj.free] = xhat
        pb = self.problem_
        self.par_full_ = full
        self.tmb_rep_ = None
        self.log_sigma_obs_ = full[0] if pb.lead_names == ["log_sigma_obs"] else None
        self.coeff_fe_ = full[pb.off_fe:pb.off_fe + pb.n_fe].copy()        # R/sde.R:707-713
        self.coeff_re_ = full[pb.off_re:pb.off_re + pb.n_re].copy()
        if pb.n_smooth:
            self.lambda_vals_ = np.exp(full[pb.off_lambda:pb.off_lambda + pb.n_smooth])   # R/sde.R:712
        if pb.n_decay:
            self.rho_ = np.exp(full[pb.off_decay:pb.off_decay + pb.n_decay])             # R/sde.R:715-718
        return self.out_

    def _exact_hess(self, par_full, idx):
        """tmb_obj_joint$he counterpart where the engine has exact second derivatives (ssde_hess: BM / OU); None elsewhere."""
        try:
            return self.engine_.hess(par_full, idx)
        except capi.EngineError:
            return None

    def report(self):
        """sdreport counterpart (R/sde.R:702-704): estimates, cov.fixed and the joint precision of
        (fixed, random) built from finite differences of the GPU gradient (smoothsde_amd/report.py)."""
        from .report import sdreport
        pb = self.problem_
        full = self.par_full_ if getattr(self, "par_full_", None) is not None else self.tmb_obj_.par_full
        if self.laplace_:
            lap = self.tmb_obj_
            u_keep = lap.u_hat.copy()

            def marg(theta):
                lap.u_hat = u_keep.copy()
                return lap.fn(theta, update_warm_start=False)
            rep = sdreport(pb, lambda p: self.engine_.eval(p, order=1), full, lap.io, lap.ir, marginal_fn=marg, joint_hess=self._exact_hess)
            lap.u_hat = u_keep
        else:
            free = pb.free_index()
            ir = np.array([k for k in free if pb.off_re <= k < pb.off_re + pb.n_re], dtype=int)
            io = np.array([k for k in free if k not in set(ir.tolist())], dtype=int)
            rep = sdreport(pb, lambda p: self.engine_.eval(p, order=1), full, io, ir, marginal_fn=None, joint_hess=self._exact_hess)
        self.tmb_rep_ = rep
        return rep

    def post_coeff(self, n_post, seed=None):
        """Posterior draws of all coefficients from MVN(par_all, jointCov) (R/sde.R:871-915): a dict with one
        (n_post x k) matrix per parameter block."""
        rep = self.tmb_rep_ if self.tmb_rep_ is not None else self.report()
        cov = np.linalg.inv(rep.jointPrecision) if rep.jointPrecision is not None else rep.cov_fixed   # prec_to_cov
        cov = 0.5 * (cov + cov.T)
        draws = np.random.default_rng(seed).multivariate_normal(rep.par_all(), cov, size=int(n_post), method="eigh")
        names = rep.names_all()
        out = {nm: draws[:, [i for i, k in enumerate(names) if k == nm]] for nm in dict.fromkeys(names)}
        out.setdefault("coeff_re", np.zeros((int(n_post), 0)))          # R/sde.R:907-910
        return out

    def _joint_free_x(self):
        obj = self.tmb_obj_joint_
        x = self.par_full_[obj.free] if getattr(self, "par_full_", None) is not None else obj.par
        return obj, x

    def edf_conditional(self):
        """Effective degrees of freedom (R/sde.R:1360-1375): fixed-effect count + tr(H_re V_re), H the Hessian of
        the joint objective `tmb_obj_joint` (excluding the penalty for the direct families; the Kalman families
        ignore that flag, Q7), V the joint covariance."""
        n_lambda = self.problem_.n_smooth if getattr(self, "laplace_", False) else 0
        edf = float(len(self.tmb_obj_.par) - n_lambda)
        rep = self.tmb_rep_ if self.tmb_rep_ is not None else self.report()
        if rep.jointPrecision is not None:
            pb = self.problem_
            jobj, x = self._joint_free_x()
            H = jobj.he(x)
            ind_h = [i for i, k in enumerate(jobj.free) if pb.off_re <= k < pb.off_re + pb.n_re]
            V = np.linalg.inv(rep.jointPrecision)
            ind_v = [i for i, nm in enumerate(rep.names_all()) if nm == "coeff_re"]
            edf += float(np.trace(H[np.ix_(ind_h, ind_h)] @ V[np.ix_(ind_v, ind_v)]))
        return edf

    def logLik(self):
        """- tmb_obj_joint$fn(par_all) with attributes df = edf_conditional() and nobs (R/utility.R:115-123)."""
        obj, x = self._joint_free_x()
        return dict(value=-obj.fn(x), df=self.edf_conditional(), nobs=self.n_)

    def AIC_conditional(self):
        ll = self.logLik()
        return -2.0 * ll["value"] + 2.0 * ll["df"]                       # R/sde.R:1318-1328

    def AIC_marginal(self):
        n_lambda = 0 if not getattr(self, "laplace_", False) else self.problem_.n_smooth
        return 2.0 * self.out_["value"] + 2.0 * (len(self.out_["par"]) - n_lambda)   # R/sde.R:1340-1349

    # -- state estimates and model checking (R/sde.R:1186-1228) -------------------------------------------------
    def _current_par_full(self):
        if self.engine_ is None:
            raise RuntimeError("call setup() or fit() first")
        full = getattr(self, "par_full_", None)
        return self._par_full(self.problem_) if full is None else full

    def smooth_states(self, cov=True):
        """Smoothed states of a state-space model (CTCRW, OU_SSM, BM_SSM) at the current parameters: E[state at row i | the whole
        track] and, with cov=True, its covariance (ssde_smooth).  Columns in the order of the reference's aest_all
        (CTCRW: x, vx, y, vy, ...).  Returns {"mean": n x sdim, "cov": n x sdim x sdim or None}; NaN on a track's first row, which
        carries no state (the prior is the state at the second row)."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"smooth_states: no latent state in the model {self.type_!r}")
        out = self.engine_.smooth(self._current_par_full(), cov=cov, resid=False)
        return {"mean": out["mean"], "cov": out["cov"]}

    def loo(self, thresholds=None):
        """Leave-one-out check of a state-space model (CTCRW, OU_SSM, BM_SSM) at the current parameters (ssde_smooth_loo, DESIGN.md
        §3.20): every fix predicted from all the OTHER fixes of its track, without a refit.  Returns {"mean": n x d, "cov": n x d x d,
        "resid": n x d whitened deletion residuals, "lpd": n log predictive densities, "stats": n_tracks x (4 + n_thr), "elpd": the
        sum of the tracks' leave-one-out scores (stats column 1) -- a cross-validation score that compares the three models on
        the same data}.  NaN on rows without a fix to leave out (a track's first row, missing rows)."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"loo: no latent state in the model {self.type_!r}")
        out = self.engine_.smooth_loo(self._current_par_full(), cov=True, thresholds=thresholds)
        out["elpd"] = float(np.sum(out["stats"][:, 1]))
        return out

    def outliers(self, level=0.999):
        """The rows of the data whose deletion residual is improbably large: q_j = |resid_j|^2 of loo() above the chi-square
        quantile `level` with d degrees of freedom.  Returns {"rows": their 0-based rows, ascending, "q": their q_j, "threshold":
        the quantile, "counts": per track the number of such rows}.  The rows come from q_j formed here from "resid", the counts from
        the q_j the device formed in its own arithmetic (the last bit may differ): a q_j within rounding of the quantile can be in one
        and not in the other."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"outliers: no latent state in the model {self.type_!r}")
        if not 0.0 < level < 1.0:
            raise ValueError("level must lie strictly between 0 and 1")
        from scipy.stats import chi2
        d = self.engine_.problem.n_dim
        thr = float(chi2.ppf(level, d))
        out = self.engine_.smooth_loo(self._current_par_full(), cov=False, thresholds=[thr])
        q = np.sum(out["resid"] ** 2, axis=1)
        with np.errstate(invalid="ignore"):
            rows = np.nonzero(q > thr)[0]
        return {"rows": rows, "q": q[rows], "threshold": thr, "counts": out["stats"][:, 4].astype(np.int64)}

    def forecast_skill(self, horizons=(1, 2, 5, 10), level=0.95):
        """Forecast skill of a state-space model (CTCRW, OU_SSM, BM_SSM) at the current parameters as a function of the lead
        (ssde_forecast_scores): every fix predicted from the data `k` rows back, for every k of `horizons`,
        without rebuilding the data.  Returns {"horizons", "level", "threshold": the chi-square quantile `level` with d degrees of
        freedom, "pooled": {...}, "tracks": {...}}; each of the two holds, per horizon (pooled over the tracks: n_h numbers; per
        track: n_tracks x n_h), "n": the scored targets, "log_score": their mean log predictive density, "mean_q": their mean
        q = |z|^2 (about d under the model), "rmse": the root of their mean squared error, "lead": their mean lead time and
        "coverage": the share of them inside the `level` predictive region (q <= threshold).  NaN where nothing was scored."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"forecast_skill: no latent state in the model {self.type_!r}")
        if not 0.0 < level < 1.0:
            raise ValueError("level must lie strictly between 0 and 1")
        from scipy.stats import chi2
        d = self.engine_.problem.n_dim
        thr = float(chi2.ppf(level, d))
        hz = [int(k) for k in horizons]
        st = self.engine_.forecast_scores(self._current_par_full(), hz, thresholds=[thr], z=False, lpd=False)["stats"]

        def ratios(s):                                                    # s: (..., 6, n_h) sums -> the means
            with np.errstate(invalid="ignore", divide="ignore"):
                cnt = s[..., 0, :]
                return {"n": cnt.astype(np.int64), "log_score": s[..., 1, :] / cnt, "mean_q": s[..., 2, :] / cnt,
                        "rmse": np.sqrt(s[..., 3, :] / cnt), "lead": s[..., 4, :] / cnt, "coverage": 1.0 - s[..., 5, :] / cnt}
        return {"horizons": hz, "level": level, "threshold": thr, "pooled": ratios(st.sum(axis=0)), "tracks": ratios(st)}

    def _rows_and_offsets(self, ID, time):
        """(rows, offsets) of the queries (ID[k], time[k]): the last row of track ID[k] with a time stamp <= time[k] and the time past
        it; row -1 for an unknown ID, a time that is not finite or one before the track's first time stamp."""
        ID, time = np.asarray(ID).ravel(), np.asarray(time, dtype=np.float64).ravel()
        if ID.shape != time.shape:
            raise ValueError("ID and time must have the same length")
        ids = np.asarray(self.data_["ID"])
        t = np.asarray(self.data_["time"], dtype=np.float64)
        n, m = len(ids), len(ID)
        start = np.r_[0, np.nonzero(ids[1:] != ids[:-1])[0] + 1]
        end = np.r_[start[1:], n]
        seg_of = {}
        for k, s0 in enumerate(start):
            seg_of.setdefault(ids[s0], k)
        rows = np.full(m, -1, dtype=np.int64)
        for k in range(m):
            seg = seg_of.get(ID[k])
            if seg is None or not np.isfinite(time[k]):
                continue
            j = int(np.searchsorted(t[start[seg]:end[seg]], time[k], side="right")) - 1      # the last row with time <= the query's
            if j >= 0:
                rows[k] = start[seg] + j
        offs = np.zeros(m)
        ok = rows >= 0
        offs[ok] = time[ok] - t[rows[ok]]
        return rows, offs

    def predict_states(self, ID, time, cov=True):
        """Smoothed states of a state-space model (CTCRW, OU_SSM, BM_SSM) at any times, at the current parameters (ssde_predict,
        DESIGN.md §3.11).  `ID` and `time` are arrays of equal length: query k asks for the state of track ID[k] at time[k].  Between two
        rows of the track the state is interpolated (with the covariates of the row before), after its last row it is a forecast.
        Returns {"mean": n_query x sdim, "cov": n_query x sdim x sdim or None}, columns as in smooth_states; NaN for an unknown ID
        and for a time before the track's second time stamp (the first row carries no state)."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"predict_states: no latent state in the model {self.type_!r}")
        if self.engine_ is None:
            raise RuntimeError("call setup() or fit() first")
        rows, offs = self._rows_and_offsets(ID, time)
        m, sd = len(rows), self.problem_.sdim
        ok = rows >= 0
        mean = np.full((m, sd), np.nan)
        P = np.full((m, sd, sd), np.nan) if cov else None
        if ok.any():
            out = self.engine_.predict(self._current_par_full(), rows[ok], offs[ok], cov=cov)
            mean[ok] = out["mean"]
            if cov:
                P[ok] = out["cov"]
        return {"mean": mean, "cov": P}

    def sample_states(self, n_draws, seed=0):
        """Joint posterior draws of the whole state path of a state-space model (CTCRW, OU_SSM, BM_SSM) at the current parameters
        (ssde_smooth_draws): an array (n_draws, n, sdim), columns as in smooth_states, NaN on a track's first row.
        Unlike the row-wise smooth_states, a draw carries the dependence between rows: speed, distance travelled, time inside a
        region or multiple imputation of the true positions are summaries of these paths."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"sample_states: no latent state in the model {self.type_!r}")
        return self.engine_.smooth_draws(self._current_par_full(), n_draws, seed=seed)

    def sample_states_at(self, ID, time, n_draws, seed=0):
        """Joint posterior draws of the state of a state-space model (CTCRW, OU_SSM, BM_SSM) at any times, at the current parameters
        (ssde_predict_draws): an array (n_draws, n_query, sdim), columns as in smooth_states.  `ID` and `time` as
        predict_states takes them.  Draw k is the path sample_states(n_draws, seed) returns as draw k, refined between its rows (with
        the covariates of the row before) and continued past a track's last row: querying the data's own times returns
        sample_states' numbers.  All the times of interest go into one call -- the answers inside one interval are jointly
        distributed only within a call.  NaN for an unknown ID and for a time before the track's second time stamp."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"sample_states_at: no latent state in the model {self.type_!r}")
        if self.engine_ is None:
            raise RuntimeError("call setup() or fit() first")
        rows, offs = self._rows_and_offsets(ID, time)
        ok = rows >= 0
        out = np.full((int(n_draws), len(rows), self.problem_.sdim), np.nan)
        if ok.any():
            out[:, ok, :] = self.engine_.predict_draws(self._current_par_full(), rows[ok], offs[ok], n_draws, seed=seed)
        return out

    def path_summary(self, n_draws, seed=0, regions=None, weight="dt"):
        """Summaries of the posterior state paths of a state-space model (CTCRW, OU_SSM, BM_SSM) at the current parameters, reduced
        on the device (ssde_path_stats): no draw comes home.  {"length": (n_draws, n_tracks) distance travelled
        along the drawn path, "displacement": (n_draws, n_tracks) distance between its two ends, "in_region": (n_draws, n_tracks,
        n_regions) weighted rows inside each region}.  `regions`: rows of lo_1, hi_1, lo_2, hi_2 or None.  `weight`: "dt" weighs a
        row by the time to the track's next row (0 at its last row), so "in_region" is time spent inside; an array (one number per
        row) is passed through; None counts rows.  The draws are those of sample_states(n_draws, seed)."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"path_summary: no latent state in the model {self.type_!r}")
        if isinstance(weight, str):
            if weight != "dt":
                raise ValueError('weight must be "dt", an array or None')
            weight = self._dt_weights()
        st = self.engine_.path_stats(self._current_par_full(), n_draws, seed=seed, regions=regions, weight=weight)
        return {"length": st[:, :, 0], "displacement": st[:, :, 1], "in_region": st[:, :, 2:]}

    def speed_summary(self, n_draws, seed=0, thresholds=None, weight="dt"):
        """The speed |v| along the posterior state paths of a CTCRW at the current parameters, reduced on the device
        (ssde_path_speed): no draw comes home.  {"mean_speed": (n_draws, n_tracks) the weighted mean of the speed
        over the track's state rows, "max_speed": (n_draws, n_tracks), "max_row": (n_draws, n_tracks) the row of the data that
        attains it, "persistence": (n_draws, n_tracks) the length of the weighted resultant of the headings over the sum of the
        weights (1: one heading throughout), "time_below": (n_draws, n_tracks, n_thr) weighted rows at or below each threshold,
        "p_below": (n, n_thr) per row of the data the share of the draws at or below each threshold, NaN on rows without a state}.
        `weight` as path_summary's: "dt" makes mean_speed a time average and time_below a time.  The draws are those of
        sample_states(n_draws, seed).  A model other than the CTCRW raises the engine's model error: no other state holds a
        velocity."""
        if isinstance(weight, str):
            if weight != "dt":
                raise ValueError('weight must be "dt", an array or None')
            weight = self._dt_weights()
        thr = np.zeros(0) if thresholds is None else np.asarray(thresholds, dtype=np.float64).ravel()
        st, below = self.engine_.path_speed(self._current_par_full(), n_draws, seed=seed, thresholds=thr, weight=weight)
        pb = self.problem_
        w = np.ones(pb.n) if weight is None else np.asarray(weight, dtype=np.float64)
        has_state = np.ones(pb.n, dtype=bool)
        has_state[np.asarray(pb.seg_start, dtype=np.int64)] = False
        wsum = np.add.reduceat(np.where(has_state, w, 0.0), np.asarray(pb.seg_start, dtype=np.int64))
        with np.errstate(invalid="ignore", divide="ignore"):
            p_below = np.full((pb.n, len(thr)), np.nan)
            if below is not None:
                p_below[has_state] = below[has_state] / float(n_draws)
            return {"mean_speed": st[:, :, 0] / wsum[None, :], "max_speed": st[:, :, 1], "max_row": st[:, :, 2],
                    "persistence": np.hypot(st[:, :, 3], st[:, :, 4]) / wsum[None, :], "time_below": st[:, :, 5:], "p_below": p_below}

    def _dt_weights(self):
        """the time from a row to its track's next row, 0 at a track's last row"""
        ids, t = np.asarray(self.data_["ID"]), np.asarray(self.data_["time"], dtype=np.float64)
        weight = np.zeros(len(t))
        same = ids[1:] == ids[:-1]
        weight[:-1][same] = (t[1:] - t[:-1])[same]
        return weight

    def _proximity_points(self, pairs, times):
        """per pair of (ID_a, ID_b): the clock times compared (an empty array for an unknown ID or an empty window)"""
        ids = np.asarray(self.data_["ID"])
        t = np.asarray(self.data_["time"], dtype=np.float64)
        start = np.r_[0, np.nonzero(ids[1:] != ids[:-1])[0] + 1]
        end = np.r_[start[1:], len(ids)]
        seg_of = {}
        for k, s0 in enumerate(start):
            seg_of.setdefault(ids[s0], k)
        given = None if times is None else np.sort(np.asarray(times, dtype=np.float64).ravel())
        out = []
        for a, b in pairs:
            sa, sb = seg_of.get(a), seg_of.get(b)
            if sa is None or sb is None or min(end[sa] - start[sa], end[sb] - start[sb]) < 2:
                out.append(np.zeros(0))
                continue
            ta, tb = t[start[sa]:end[sa]], t[start[sb]:end[sb]]
            lo = max(ta[1], tb[1])                                    # the later of the two second stamps: both have a state
            if given is None:
                hi = min(ta[-1], tb[-1])                              # the earlier of the two last stamps: both have data
                u = np.union1d(ta, tb)
                out.append(u[(u >= lo) & (u <= hi)])
            else:
                out.append(given[np.isfinite(given) & (given >= lo)])  # later times are kept: forecasts
        return out

    def proximity(self, pairs, radii, n_draws, seed=0, times=None, weight="dt"):
        """How close the posterior paths of pairs of tracks come, of a state-space model (CTCRW, OU_SSM, BM_SSM) at the current
        parameters, reduced on the device (ssde_path_proximity): no draw comes home.  `pairs`: a sequence of
        (ID_a, ID_b); `radii`: up to eight distances.  `times=None` compares every pair at the sorted union of both tracks' time stamps
        inside the window where both have a state and data (from the later of the two second stamps to the earlier of the two last
        stamps); an array compares every pair at those clock times, without the ones before either track's second stamp (later
        times are kept: forecasts).  `weight`: "dt" weighs a point by the time to the pair's next point (0 at the last), so
        "time_within" is time; None counts points.  Draw k of either track is the path sample_states(n_draws, seed) returns as draw k
        (tracks are independent given the parameters, so the two form a joint draw).  Returns {"min_dist": (n_draws, n_pairs),
        "t_min": (n_draws, n_pairs) the clock time of the closest approach, "time_within": (n_draws, n_pairs, n_radii), "p_within":
        (n_pairs, n_radii) the share of the finite draws whose minimum distance is <= the radius, "times": the list of the pairs'
        clock times}.  A pair with an unknown ID or an empty window is NaN and does not fail the call.  The arguments the engine's
        path_proximity got (qa_rows, qa_offs, qb_rows, qb_offs, pair_ptr, weight) stay in `proximity_queries_`."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"proximity: no latent state in the model {self.type_!r}")
        if self.engine_ is None:
            raise RuntimeError("call setup() or fit() first")
        if weight is not None and not (isinstance(weight, str) and weight == "dt"):
            raise ValueError('weight must be "dt" or None')
        pairs = [tuple(p) for p in pairs]
        rad = np.asarray(radii, dtype=np.float64).ravel()
        n_draws, n_pairs = int(n_draws), len(pairs)
        tlist = self._proximity_points(pairs, times)
        pair_ptr = np.r_[0, np.cumsum([len(u) for u in tlist])].astype(np.int64)
        st = np.full((n_draws, n_pairs, 2 + len(rad)), np.nan)
        if pair_ptr[-1] > 0 and n_pairs > 0:
            clock = np.concatenate(tlist)
            ida = np.concatenate([np.full(len(u), p[0], dtype=object) for p, u in zip(pairs, tlist)])
            idb = np.concatenate([np.full(len(u), p[1], dtype=object) for p, u in zip(pairs, tlist)])
            ra, oa = self._rows_and_offsets(ida, clock)
            rb, ob = self._rows_and_offsets(idb, clock)
            w = None
            if weight is not None:
                w = np.concatenate([np.r_[np.diff(u), 0.0] if len(u) else u for u in tlist])
            self.proximity_queries_ = (ra, oa, rb, ob, pair_ptr, w)
            st = self.engine_.path_proximity(self._current_par_full(), ra, oa, rb, ob, pair_ptr, n_draws, seed=seed, radii=rad, weight=w)
        t_min = np.full((n_draws, n_pairs), np.nan)
        for p, u in enumerate(tlist):
            ok = np.isfinite(st[:, p, 1])
            t_min[ok, p] = u[st[ok, p, 1].astype(np.int64)] if len(u) else np.nan
        finite = np.isfinite(st[:, :, 0])
        with np.errstate(invalid="ignore", divide="ignore"):
            p_within = (finite[:, :, None] & (st[:, :, :1] <= rad[None, None, :])).sum(axis=0) / finite.sum(axis=0)[:, None]
        return {"min_dist": st[:, :, 0], "t_min": t_min, "time_within": st[:, :, 2:], "p_within": p_within, "times": tlist}

    def utilisation(self, n_draws, seed=0, cells=(64, 64), extent=None, by=None, weight="dt", max_step=None):
        """The utilisation distribution of a state-space model (CTCRW, OU_SSM, BM_SSM) at the current parameters: the share of the
        weighted time that the posterior state paths spend in every cell of a regular grid, summed on the device
        (ssde_path_occupancy).  `cells`: (nx, ny) (an integer, or ny = 1, for one response column); `extent`:
        (x_lo, x_hi, y_lo, y_hi), or None for the bounding box of the observed positions widened by 5 % on each side; `by`: None
        pools every track, "ID" gives one grid per track, an integer array one group label per track (-1: left out); `weight`
        as path_summary's.  {"x_edges": (nx + 1,), "y_edges": (ny + 1,), "density": (n_groups, ny, nx), "outside": (n_groups,)}:
        the sums divided per group by n_draws times the group's total weight, so density and outside together sum to 1 (NaN
        for a group without weight).  The draws are those of sample_states(n_draws, seed).  `max_step`: None places every
        interval's weight at the row that starts it; a positive number spreads it along the path refined between the fixes
        (ssde_path_occupancy_fine, DESIGN.md §3.15: intervals longer than max_step are cut into equal sub-steps, the states inside
        them are sample_states_at's) and adds "n_points", the path points per draw that carried weight; a warning is issued when an
        interval needed more sub-steps than the cap allows."""
        if self.type_ not in ("CTCRW", "OU_SSM", "BM_SSM"):
            raise NotImplementedError(f"utilisation: no latent state in the model {self.type_!r}")
        pb = self.problem_
        d = pb.n_dim
        if d > 2:
            raise NotImplementedError("utilisation: one or two response columns")
        nx, ny = (int(cells), 1) if np.isscalar(cells) else (int(cells[0]), int(cells[1]) if d == 2 and len(cells) > 1 else 1)
        if extent is None:
            Z = np.asarray(self.obs(), dtype=np.float64).reshape(len(pb.times), -1)
            lo, hi = np.nanmin(Z, axis=0), np.nanmax(Z, axis=0)
            pad = 0.05 * np.where(hi > lo, hi - lo, 1.0)
            ext = np.column_stack([lo - pad, hi + pad])
        else:
            ext = np.asarray(extent, dtype=np.float64).reshape(-1, 2)
        grid = {"x0": ext[0, 0], "dx": (ext[0, 1] - ext[0, 0]) / nx, "nx": nx}
        if d == 2:
            grid.update(y0=ext[1, 0], dy=(ext[1, 1] - ext[1, 0]) / ny, ny=ny)
        if isinstance(weight, str):
            if weight != "dt":
                raise ValueError('weight must be "dt", an array or None')
            weight = self._dt_weights()
        n_seg = pb.n_seg
        if by is None:
            group = None
        elif isinstance(by, str):
            if by != "ID":
                raise ValueError('by must be None, "ID" or one integer label per track')
            group = np.arange(n_seg, dtype=np.int32)
        else:
            group = np.ascontiguousarray(by, dtype=np.int32)
        extra = {}
        if max_step is None:
            occ, outside = self.engine_.path_occupancy(self._current_par_full(), n_draws, grid, seed=seed, weight=weight, group=group)
        else:
            occ, outside = self.engine_.path_occupancy_fine(self._current_par_full(), n_draws, grid, max_step, seed=seed, weight=weight,
                                                            group=group)
            extra["n_points"], n_capped = self.engine_.last_occupancy_points()
            if n_capped > 0:
                warnings.warn(f"utilisation: {n_capped} intervals need more than {capi.OCC_MAX_SUB} sub-steps of max_step={max_step}; "
                              "they were cut into that many", stacklevel=2)
        # the total weight of every group's state rows (a track's first row carries no state)
        start = np.asarray(pb.seg_start, dtype=np.int64)
        w = np.ones(len(pb.times)) if weight is None else np.array(weight, dtype=np.float64)
        w[start] = 0.0
        per_track = np.add.reduceat(w, start)
        labels = np.zeros(n_seg, dtype=np.int64) if group is None else group.astype(np.int64)
        total = np.bincount(labels[labels >= 0], weights=per_track[labels >= 0], minlength=len(outside)) * n_draws
        with np.errstate(invalid="ignore", divide="ignore"):
            density, out = occ / total[:, None, None], outside / total
        return {"x_edges": grid["x0"] + grid["dx"] * np.arange(nx + 1),
                "y_edges": (grid["y0"] + grid["dy"] * np.arange(ny + 1)) if d == 2 else np.array([-np.inf, np.inf]),
                "density": density, "outside": out, **extra}

    def residuals(self):
        """Model residuals, iid N(0, 1) under the model (one column per response variable).

        BM / BM_t / OU: the reference's SDE$residuals() (R/sde.R:1186-1228) on the host: row i holds the standardised transition
        i -> i + 1 (for BM_t scaled by sqrt(df / (df - 2)), the t scale), and the LAST row of every track is NaN.
        CTCRW / OU_SSM / BM_SSM (where the reference stops): the whitened one-step-ahead innovations C_i^-1 (y_i - Z a_i) of the
        Kalman filter, C_i the lower Cholesky factor of the innovation covariance (ssde_smooth); row i is row i's own innovation,
        so the FIRST row of every track is NaN (it carries no state), as is every row without an update (NA rows).
        CIR / ESEAL_SSM raise NotImplementedError, as the reference stops."""
        if self.type_ in ("CTCRW", "OU_SSM", "BM_SSM"):
            if self.engine_ is None:
                raise RuntimeError("call setup() or fit() first")
            return self.engine_.smooth(self._current_par_full(), cov=False, resid=True)["resid"]
        if self.type_ not in ("BM", "BM_t", "OU"):
            raise NotImplementedError(f"Residuals not implemented for model {self.type_}")
        ids = np.asarray(self.data_["ID"])
        n = len(ids)
        brk = np.nonzero(ids[1:] != ids[:-1])[0]
        start = np.r_[0, brk + 1]
        end = np.r_[brk, n - 1]
        keep_from = np.setdiff1d(np.arange(n), end)                  # -end_ind
        keep_to = np.setdiff1d(np.arange(n), start)                  # -start_ind
        t = np.asarray(self.data_["time"], dtype=np.float64)
        dt = t[keep_to] - t[keep_from]
        par = self.par()
        Z = self.obs()
        mu = np.column_stack([par[k] for k in self.names_ if k.startswith("mu")])[keep_from]
        if self.type_ in ("BM", "BM_t"):
            mean = Z[keep_from] + mu * dt[:, None]
            sd = (par["sigma"][keep_from] * np.sqrt(dt))[:, None]
            if self.type_ == "BM_t":
                df = self.other_data_["df"]
                sd = sd / np.sqrt(df / (df - 2))                      # the t scale, not the sd
        else:
            tau, kappa = par["tau"][keep_from][:, None], par["kappa"][keep_from][:, None]
            mean = mu + np.exp(-dt[:, None] / tau) * (Z[keep_from] - mu)
            sd = np.sqrt(kappa * (1 - np.exp(-2 * dt[:, None] / tau)))
        res = np.full((n, Z.shape[1]), np.nan)
        res[keep_from] = (Z[keep_to] - mean) / sd
        return res

    def par(self, t=None):
        """SDE parameters on the natural scale for every row (R/sde.R:749-856, new_data = NULL)."""
        out = {}
        fe_off = np.concatenate([[0], np.cumsum(self.terms_["ncol_fe"])]).astype(int)
        re_off = np.concatenate([[0], np.cumsum(self.terms_["ncol_re_par"])]).astype(int)
        for j, (nm, d) in enumerate(zip(self.names_, self.designs_)):
            cf = self.coeff_fe_[fe_off[j]:fe_off[j + 1]]
            lp = (np.full(self.n_, cf[0]) if d.X_fe is None else d.X_fe @ cf)
            if d.X_re is not None:
                lp = lp + d.X_re @ self.coeff_re_[re_off[j]:re_off[j + 1]]
            out[nm] = lp if (nm.startswith("mu") and self.type_ != "CIR") else np.exp(lp)
        return out

    # -- uncertainty of the SDE parameters (R/sde.R:941-1180) -----------------------------------------------------------------
    def _links(self):
        """0 identity (mu*, except CIR), 1 log: the inverse link par() applies"""
        return np.array([0 if (nm.startswith("mu") and self.type_ != "CIR") else 1 for nm in self.names_], dtype=np.uint8)

    def _band_table(self, n_post, seed=None, term=None):
        """The coefficient table of ssde_par_bands: row 0 the estimates, rows 1 .. n_post the draws of post_coeff(n_post, seed);
        parameter j's fixed-effect coefficients, then its random-effect coefficients.  The coefficients of a fixed parameter keep
        their value in every draw (R/sde.R:904-915).  `term`: the coefficients whose name does not contain it are zeroed in every
        row (the reference's substring rule, R/utility.R:137-144)."""
        ncol_fe, ncol_re = self.terms_["ncol_fe"], self.terms_["ncol_re_par"]
        fe_off = np.concatenate([[0], np.cumsum(ncol_fe)]).astype(int)
        re_off = np.concatenate([[0], np.cumsum(ncol_re)]).astype(int)
        post = self.post_coeff(n_post, seed=seed)
        fe = np.tile(self.coeff_fe_, (int(n_post), 1))
        fixed = set(self.fixpar_ or [])
        est = np.array([k for j, nm in enumerate(self.names_) if nm not in fixed for k in range(fe_off[j], fe_off[j + 1])], dtype=int)
        if post["coeff_fe"].shape[1] != len(est) or post["coeff_re"].shape[1] != len(self.coeff_re_):
            raise ValueError("post_coeff does not match the model's free coefficients")
        fe[:, est] = post["coeff_fe"]
        fe = np.vstack([self.coeff_fe_, fe])
        re_ = np.vstack([self.coeff_re_, post["coeff_re"]])
        if term is not None:
            for j, d in enumerate(self.designs_):
                nf = d.names_fe if d.names_fe is not None else ["(Intercept)"] + [""] * (ncol_fe[j] - 1)
                nr = d.names_re if d.names_re is not None else [""] * ncol_re[j]
                fe[:, fe_off[j]:fe_off[j + 1]] *= np.array([term in nm for nm in nf], dtype=float)
                re_[:, re_off[j]:re_off[j + 1]] *= np.array([term in nm for nm in nr], dtype=float)
        return np.hstack([np.hstack([fe[:, fe_off[j]:fe_off[j + 1]], re_[:, re_off[j]:re_off[j + 1]]]) for j in range(len(self.names_))])

    def _band_blocks(self, t=None, designs=None):
        """the design blocks of the rows `t` (None: row 0 of the fitted data, or every row of `designs` when given; "all": every
        row; else row indices, 0-based) as ssde_par_bands takes them"""
        if t is None:
            t = "all" if designs is not None else [0]
        designs = self.designs_ if designs is None else list(designs)
        if len(designs) != len(self.names_):
            raise ValueError("designs: one Design per SDE parameter")
        rows = slice(None) if isinstance(t, str) and t == "all" else np.atleast_1d(np.asarray(t, dtype=int))
        X_fe = [None if d.X_fe is None else np.asarray(d.X_fe, dtype=np.float64)[rows] for d in designs]
        X_re = [None if d.X_re is None else np.asarray(d.X_re, dtype=np.float64)[rows] for d in designs]
        for j, (a, b) in enumerate(zip(X_fe, X_re)):
            if (1 if a is None else a.shape[1]) != self.terms_["ncol_fe"][j] or (0 if b is None else b.shape[1]) != self.terms_["ncol_re_par"][j]:
                raise ValueError(f"designs: the blocks of {self.names_[j]} have not the fitted model's columns")
        return X_fe, X_re

    def post_par(self, n_post=100, resp=True, term=None, seed=None):
        """Posterior draws of the SDE parameters on the fitted rows (R/sde.R:941-962): an (n, n_par, n_post) array.  It is the
        matrix CI_pointwise and CI_simultaneous never build -- numpy, for small n."""
        tab = self._band_table(n_post, seed=seed, term=term)
        X_fe, X_re = self._band_blocks("all")
        link, off = self._links(), 0
        out = np.zeros((self.n_, len(self.names_), int(n_post)))
        for j in range(len(self.names_)):
            X = np.hstack([np.ones((self.n_, 1)) if X_fe[j] is None else X_fe[j]] + ([] if X_re[j] is None else [X_re[j]]))
            lp = X @ tab[1:, off:off + X.shape[1]].T
            out[:, j, :] = np.exp(lp) if (resp and link[j] == 1) else lp
            off += X.shape[1]
        return out

    def _bands(self, simultaneous, t, designs, level, n_post, resp, term, seed):
        X_fe, X_re = self._band_blocks(t, designs)
        tab = self._band_table(n_post, seed=seed, term=term)
        want = ("sim_low", "sim_upp") if simultaneous else ("pw_low", "pw_upp")
        out = capi.par_bands(X_fe, X_re, self._links(), tab, level=level, resp=resp, simultaneous=simultaneous, want=want)
        return {"low": out[want[0]], "upp": out[want[1]], "names": list(self.names_)}

    def CI_pointwise(self, t=None, designs=None, level=0.95, n_post=1000, resp=True, term=None, seed=None):
        """Pointwise confidence intervals of the SDE parameters by posterior simulation (R/sde.R:1003-1043), reduced on the device
        (ssde_par_bands): {"low", "upp"} (n_t, n_par) arrays in the order of "names".  `t`: rows of the fitted
        data, 0-based (None: row 0; "all": every row); `designs`: one Design per parameter in place of the fitted blocks (the
        reference's new_data; then t defaults to "all"); `term`: only the coefficients whose name contains it."""
        return self._bands(False, t, designs, level, n_post, resp, term, seed)

    def CI_simultaneous(self, t=None, designs=None, level=0.95, n_post=1000, resp=True, term=None, seed=None):
        """Simultaneous confidence intervals (R/sde.R:1079-1180; Ruppert et al. 2003, §6.5), arguments and result as
        CI_pointwise.  One table of draws serves the standard errors and the deviations (the reference draws twice)."""
        return self._bands(True, t, designs, level, n_post, resp, term, seed)

    # -- simulation and posterior checks (R/sde.R:1395-1508, 1259-1306) -------------------------------------------------------
    def _coeff_estimate(self):
        """row 0 of _band_table without the draws: parameter j's fixed-effect, then its random-effect coefficients"""
        fe_off = np.concatenate([[0], np.cumsum(self.terms_["ncol_fe"])]).astype(int)
        re_off = np.concatenate([[0], np.cumsum(self.terms_["ncol_re_par"])]).astype(int)
        return np.concatenate([np.concatenate([self.coeff_fe_[fe_off[j]:fe_off[j + 1]], self.coeff_re_[re_off[j]:re_off[j + 1]]])
                               for j in range(len(self.names_))])[None, :]

    def _sim_rows(self, designs=None, ID=None, time=None):
        """(row0, ID, time, X_fe, X_re) of the rows a simulation runs on: the fitted rows, or those of `designs`, `ID`, `time`; row0 the
        first row of every run of equal IDs"""
        if designs is None:
            if ID is not None or time is not None:
                raise ValueError("simulate: new rows need designs, ID and time together")
            ID, time = self.data_["ID"], self.data_["time"]
        elif time is None:
            raise ValueError("'data' should have a column named 'time'")                 # R/sde.R:1397-1399
        time = np.asarray(time, dtype=np.float64).ravel()
        ids = np.ones(len(time)) if ID is None else np.asarray(ID).ravel()               # R/sde.R:1400-1402
        if len(ids) != len(time):
            raise ValueError("ID and time must have the same length")
        X_fe, X_re = self._band_blocks("all", designs)
        for b in list(X_fe) + list(X_re):
            if b is not None and b.shape[0] != len(time):
                raise ValueError("designs: one row per time")
        # an intercept-only block is passed as "no column", as _problem does: the device then evaluates the parameter once
        X_fe = [None if (b is None or (b.shape[1] == 1 and np.all(b == 1.0))) else b for b in X_fe]
        row0 = np.r_[0, np.nonzero(ids[1:] != ids[:-1])[0] + 1, len(ids)].astype(np.int64) if len(ids) else np.zeros(1, dtype=np.int64)
        return row0, ids, time, X_fe, X_re

    def _sim_sigma_obs(self, n_rows, seed, posterior):
        """sigma_obs of the replicates: exp(log_sigma_obs) of a fitted state-space model (its posterior draws with `posterior`)"""
        ls = getattr(self, "log_sigma_obs_", None)
        if ls is None:
            return None
        if not posterior:
            return np.full(n_rows, np.exp(ls))
        post = self.post_coeff(n_rows, seed=seed)                                         # the draws _band_table(n_rows, seed) holds
        if "log_sigma_obs" not in post or post["log_sigma_obs"].shape[1] != 1:
            return np.full(n_rows, np.exp(ls))
        return np.exp(post["log_sigma_obs"][:, 0])

    def simulate(self, z0=0, posterior=False, seed=0, designs=None, ID=None, time=None):
        """One data set simulated from the model on the fitted rows (R/sde.R:1395-1508) by the device (ssde_simulate_rows, DESIGN.md
        §3.19): an (n, d) array.  With `designs` (one Design per parameter, as in CI_pointwise), `ID` and `time` it runs on new rows
        -- the reference's `data` argument.  `posterior`: the coefficients are one posterior draw, row 1 of _band_table(1, seed);
        else the estimates.  A fitted state-space model (BM_SSM, OU_SSM, CTCRW) adds its observation error, sd exp(log_sigma_obs), to
        what it writes: the reference has no such branch (its simulator writes the latent path), but the data these models are
        fitted to carry that error.  Models other than BM, OU, CTCRW, BM_SSM, OU_SSM raise the engine's model error."""
        row0, _, tm, X_fe, X_re = self._sim_rows(designs, ID, time)
        coeff = self._band_table(1, seed)[1:] if posterior else self._coeff_estimate()
        out = capi.simulate_rows(self.type_, len(self.response_), row0, tm, X_fe, X_re, self._links(), coeff,
                                 sigma_obs=self._sim_sigma_obs(1, seed, posterior), z0=z0, seed=seed, n_rep=1, want=("obs",))
        return np.ascontiguousarray(out["obs"][0])

    @staticmethod
    def _check_names(d, n_thr):
        cols = [""] if d == 1 else [str(c + 1) for c in range(d)]
        return ([f"{s}{c}" for c in cols for s in ("mean_incr", "sd_incr", "acf1_incr")] + ["mean_step", "max_step"]
                + [f"share_below_{r + 1}" for r in range(n_thr)])

    @staticmethod
    def _pool_check_stats(stats, row0, d, n_thr):
        """The built-in check statistics of every replicate from ssde_simulate_rows' per-track sums, pooled over the tracks in track
        order: stats (n_rep, n_tracks, 3 d + 2 + n_thr) -> (3 d + 2 + n_thr, n_rep).  N the increments of all tracks with two or
        more rows, N2 the pairs of successive increments inside a track: mean = S1 / N, var = (S2 - S1 mean) / (N - 1), sd =
        sqrt(var), acf1 = (S11 / N2 - mean^2) / (var (N - 1) / N), mean_step = SL / N, max_step = the largest of the tracks' maxima,
        share = count / N.  A NaN track makes its replicate NaN."""
        ln = np.diff(np.asarray(row0, dtype=np.int64))
        use = ln >= 2
        N, N2 = float(np.sum(ln[use] - 1)), float(np.sum(ln[use] - 2))
        out = np.full((3 * d + 2 + n_thr, stats.shape[0]), np.nan)
        if N < 1:
            return out
        st = stats[:, use, :]
        tot = np.zeros((stats.shape[0], stats.shape[2]))
        for t in range(st.shape[1]):                                                     # in track order
            tot += st[:, t, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            for c in range(d):
                s1, s2, s11 = tot[:, 3 * c], tot[:, 3 * c + 1], tot[:, 3 * c + 2]
                mean = s1 / N
                var = (s2 - s1 * mean) / (N - 1.0) if N > 1 else np.full_like(s1, np.nan)
                out[3 * c], out[3 * c + 1] = mean, np.sqrt(var)
                # lag-1 autocorrelation of the increments about the pooled mean, over the pairs inside a track, by the pooled variance
                out[3 * c + 2] = (s11 / N2 - mean * mean) / (var * (N - 1.0) / N) if N2 >= 1 else np.nan
            out[3 * d] = tot[:, 3 * d] / N
            out[3 * d + 1] = np.max(st[:, :, 3 * d + 1], axis=1)                          # (np.max hands a NaN on)
            for r in range(n_thr):
                out[3 * d + 2 + r] = tot[:, 3 * d + 2 + r] / N
        return out

    @staticmethod
    def _track_check_sums(obs, row0, thr):
        """ssde_simulate_rows' per-track statistics of one data set in numpy: (n_tracks, 3 d + 2 + n_thr)"""
        obs = np.asarray(obs, dtype=np.float64)
        d, M = obs.shape[1], len(row0) - 1
        out = np.full((M, 3 * d + 2 + len(thr)), np.nan)
        for t in range(M):
            y = obs[row0[t]:row0[t + 1]]
            if len(y) < 2 or not np.all(np.isfinite(y)):
                continue
            D = np.diff(y, axis=0)
            L = np.sqrt(np.sum(D * D, axis=1))
            for c in range(d):
                out[t, 3 * c:3 * c + 3] = [np.sum(D[:, c]), np.sum(D[:, c] ** 2), np.sum(D[1:, c] * D[:-1, c])]
            out[t, 3 * d], out[t, 3 * d + 1] = np.sum(L), np.max(L)
            out[t, 3 * d + 2:] = [np.sum(L <= r) for r in thr]
        return out

    def check_post(self, check_fn=None, n_sims=100, seed=0, thresholds=None, posterior=True, budget_mb=256):
        """Posterior predictive check (R/sde.R:1259-1306): `n_sims` replicate data sets simulated on the fitted rows, each with its
        own posterior coefficient draw -- the rows _band_table(n_sims, seed)[1:]; the estimates throughout with posterior=False --
        and a statistic of each against the data's.  {"obs_stat": (n_stat,), "stats": (n_stat, n_sims), "names"}: the reference's
        list without the plot.  check_fn=None: the built-in statistics, reduced on the device without a replicate ever coming home
        -- per column the mean, sd and lag-1 autocorrelation of the increments, the mean and the largest step length, the share of
        steps at or below each of `thresholds` -- pooled over the tracks; the same definition in numpy gives obs_stat.  A callable
        receives (ID, time, obs) of the data and of every replicate and returns a vector; the replicates then come home in batches
        of at most `budget_mb` MiB."""
        row0, ids, tm, X_fe, X_re = self._sim_rows()
        d, n_sims = len(self.response_), int(n_sims)
        coeff = self._band_table(n_sims, seed)[1:] if posterior else self._coeff_estimate()
        so = self._sim_sigma_obs(n_sims if posterior else 1, seed, posterior)
        if check_fn is None:
            thr = np.zeros(0) if thresholds is None else np.asarray(thresholds, dtype=np.float64).ravel()
            st = capi.simulate_rows(self.type_, d, row0, tm, X_fe, X_re, self._links(), coeff, sigma_obs=so, seed=seed, n_rep=n_sims,
                                    thresholds=thr, want=("stats",))["stats"]
            stats = self._pool_check_stats(st, row0, d, len(thr))
            obs_stat = self._pool_check_stats(self._track_check_sums(self.obs(), row0, thr)[None], row0, d, len(thr))[:, 0]
            return {"obs_stat": obs_stat, "stats": stats, "names": self._check_names(d, len(thr))}
        obs_stat = np.atleast_1d(np.asarray(check_fn(ids, tm, self.obs()), dtype=np.float64))
        stats = np.zeros((len(obs_stat), n_sims))
        per = max(1, int((int(budget_mb) << 20) // max(8 * len(tm) * d, 1)))
        for k0 in range(0, n_sims, per):
            nk = min(per, n_sims - k0)
            rows = slice(k0, k0 + nk) if posterior else slice(0, 1)
            obs = capi.simulate_rows(self.type_, d, row0, tm, X_fe, X_re, self._links(), coeff[rows], sigma_obs=None if so is None else so[rows],
                                     seed=seed, rep0=k0, n_rep=nk, want=("obs",), budget_mb=budget_mb)["obs"]
            for k in range(nk):
                stats[:, k0 + k] = check_fn(ids, tm, np.ascontiguousarray(obs[k]))
        return {"obs_stat": obs_stat, "stats": stats, "names": [f"statistic {k + 1}" for k in range(len(obs_stat))]}
