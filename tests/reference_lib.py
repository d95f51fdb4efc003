"""Loader for the REFERENCE's own likelihood sources, compiled behind the TMB stand-in (oracle/_ref/, built by `make -C oracle ref`
from a checkout of the reference: oracle/ref_capi.cpp, oracle/tmb_shim/) -- test infrastructure only.

This is the second, independent route to a number: oracle_lib evaluates the project's restatement (oracle/ssde_oracle.hpp),
this module the reference's program text.  CPU tests compare the two (tests/test_reference_parity.py); GPU tests never load it,
they read the results recorded in tests/golden/reference_results.json (tests/golden/gen_reference_results.py)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from smoothsde_amd.capi import Problem, SsdeDesc

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ORACLE_DIR = os.path.join(_ROOT, "oracle")
_REF_DIR = os.path.join(_ORACLE_DIR, "_ref")
# where the reference checkout lives (the default of oracle/Makefile's REFERENCE)
REFERENCE_DIR = os.environ.get("SSDE_REFERENCE_DIR", "/root/reference")
_dp = C.POINTER(C.c_double)
_LIB = None
_QLIB = None


def reference_checkout_present() -> bool:
    return os.path.exists(os.path.join(REFERENCE_DIR, "src", "smoothSDE.cpp"))


def reference_built() -> bool:
    return all(os.path.exists(os.path.join(_REF_DIR, f)) for f in ("libssde_ref.so", "libssde_ref_quad.so"))


def available() -> bool:
    """False only when the reference checkout is absent AND oracle/_ref/ holds no build: the one permitted reason to skip."""
    return reference_built() or reference_checkout_present()


def build_reference():
    subprocess.run(["make", "-s", "-C", _ORACLE_DIR, "ref", f"REFERENCE={REFERENCE_DIR}"], check=True)


def _load():
    global _LIB, _QLIB
    if _LIB is None:
        if reference_checkout_present():
            build_reference()              # make: nothing to do when oracle/_ref/ is up to date
        lib = C.CDLL(os.path.join(_REF_DIR, "libssde_ref.so"))
        lib.ref_eval.argtypes = [C.POINTER(SsdeDesc), _dp, C.c_int, C.c_int, _dp, _dp, _dp]
        lib.ref_eval.restype = C.c_int
        lib.ref_n_par_full.argtypes = [C.POINTER(SsdeDesc)]
        lib.ref_n_par_full.restype = C.c_int
        qlib = C.CDLL(os.path.join(_REF_DIR, "libssde_ref_quad.so"))
        qlib.ref_eval_quad.argtypes = [C.POINTER(SsdeDesc), _dp, C.c_int, C.c_int, _dp, _dp, C.c_double]
        qlib.ref_eval_quad.restype = C.c_int
        _LIB, _QLIB = lib, qlib
    return _LIB, _QLIB


def ref_eval(problem: Problem, par, order: int = 1, report: bool = False):
    """The reference's objective_function<Type>::operator() at `par`: value (Type = double), gradient over the full parameter
    vector (dual numbers through the reference's templates; 0 at par_fixed entries) and optionally REPORT(aest_all) (n x sdim)."""
    lib, _ = _load()
    d = problem.desc()
    par = np.ascontiguousarray(par, dtype=np.float64)
    assert lib.ref_n_par_full(C.byref(d)) == problem.n_par_full == par.size
    val = C.c_double()
    grad = np.zeros(problem.n_par_full)
    aest, ap = None, None
    if report:
        aest = np.zeros((problem.n, problem.sdim), order="F")
        ap = aest.ctypes.data_as(_dp)
    st = lib.ref_eval(C.byref(d), par.ctypes.data_as(_dp), par.size, order, C.byref(val), grad.ctypes.data_as(_dp), ap)
    assert st == 0, f"ref_eval returned {st}"
    out = [val.value]
    if order >= 1:
        out.append(grad)
    if report:
        out.append(aest)
    return out[0] if len(out) == 1 else tuple(out)


def ref_eval_quad(problem: Problem, par, order: int = 0, fd_step: float = 1e-10):
    """The same program text with Type = IEEE binary128: the value rounded to double once (and, with order = 1, the gradient
    by central differences of the binary128 function)."""
    _, qlib = _load()
    d = problem.desc()
    par = np.ascontiguousarray(par, dtype=np.float64)
    val = C.c_double()
    grad = np.zeros(problem.n_par_full)
    st = qlib.ref_eval_quad(C.byref(d), par.ctypes.data_as(_dp), par.size, order, C.byref(val), grad.ctypes.data_as(_dp), fd_step)
    assert st == 0, f"ref_eval_quad returned {st}"
    return (val.value, grad) if order >= 1 else val.value
