"""GPU suite (-m gpu): the HIP engine against what the REFERENCE's own program computed, on every golden case.

tests/golden/reference_results.json holds value, gradient and REPORT(aest_all) of the reference's src/smoothSDE.cpp and
src/nllk/*.hpp, compiled unmodified behind the TMB stand-in and evaluated on the records of tests/golden/cases.json
(tests/golden/gen_reference_results.py; tests/test_reference_parity.py keeps the file equal to a fresh evaluation).  The other
GPU suites compare the engine with the project's restatement of those sources (the oracle, and golden vectors it wrote); these
tests compare it with the reference's numbers directly.  They read fixtures only -- no reference checkout, no oracle/_ref/ --
and a missing fixture fails them.

Tolerances: the project's standing ones, as tests/test_gpu_parity.py scales them (value 1e-10 * max(1, |v|), gradient
1e-8 * max|g| + 1e-10, aest_all rtol = atol = 1e-10)."""
import functools
import json
import os

import numpy as np
import pytest

from cases import problem_from_spec
from golden_io import dec, load_golden
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

GOLD = load_golden()
KALMAN = [r for r in GOLD if r["model"] in ("CTCRW", "OU_SSM", "BM_SSM")]
# where test_gpu_parity.py::test_paths_agree forces the dense and the non-hoisted paths
KALMAN_CONST = [r for r in KALMAN if r.get("X_fe") is None and r.get("H") is None and r.get("P0") is None]
VT = 1e-10


@functools.lru_cache(maxsize=None)
def _reference():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_results.json")
    with open(path) as f:                                   # a missing fixture is an error, never a skip
        recs = [dec(r) for r in json.load(f)]
    out = {r["name"]: r for r in recs}
    assert sorted(out) == sorted(r["name"] for r in GOLD), "reference_results.json does not cover cases.json"
    return out


def _close(val, grad, ref):
    rv, rg = float(ref["value"]), np.asarray(ref["grad"], dtype=np.float64)
    assert np.isfinite(rv) and np.all(np.isfinite(rg))
    assert abs(val - rv) <= VT * max(1.0, abs(rv)), (val, rv)
    assert np.max(np.abs(grad - rg)) <= 1e-8 * np.max(np.abs(rg)) + 1e-10, (grad, rg)


@pytest.mark.parametrize("rec", GOLD, ids=[r["name"] for r in GOLD])
def test_engine_equals_the_reference(rec):
    ref = _reference()[rec["name"]]
    eng = capi.Engine(problem_from_spec(rec))
    val, grad = eng.eval(rec["par"], order=1)
    _close(val, grad, ref)
    assert eng.eval(rec["par"], order=0) == val
    eng.close()


@pytest.mark.parametrize("rec", KALMAN_CONST, ids=[r["name"] for r in KALMAN_CONST])
@pytest.mark.parametrize("flags", [capi.FLAG_FORCE_DENSE, capi.FLAG_NO_UNIFORM_DT])
def test_forced_paths_equal_the_reference(rec, flags):
    ref = _reference()[rec["name"]]
    eng = capi.Engine(problem_from_spec(rec, flags=flags))
    assert eng.info()["path"] == (2 if flags == capi.FLAG_FORCE_DENSE else 1)
    val, grad = eng.eval(rec["par"], order=1)
    _close(val, grad, ref)
    eng.close()


@pytest.mark.parametrize("rec", KALMAN, ids=[r["name"] for r in KALMAN])
def test_report_equals_the_reference_report(rec):
    exp = np.asarray(_reference()[rec["name"]]["aest_all"], dtype=np.float64)
    eng = capi.Engine(problem_from_spec(rec))
    aest = eng.report(rec["par"])
    assert aest.shape == exp.shape
    assert np.allclose(aest, exp, rtol=1e-10, atol=1e-10, equal_nan=True), np.nanmax(np.abs(aest - exp))
    eng.close()
