#!/usr/bin/env python3
"""tests/golden/gen_reference_results.py -- writes tests/golden/reference_results.json: what the REFERENCE's own program computes
for every record of tests/golden/cases.json.

The numbers come from oracle/_ref/ alone (the reference's src/smoothSDE.cpp and src/nllk/*.hpp compiled unmodified behind
oracle/tmb_shim/, entry point oracle/ref_capi.cpp; tests/reference_lib.py) -- never from oracle/ssde_oracle.hpp.  Per case:
the value and the gradient in double (the gradient by dual numbers through the reference's templates), the exact value from the
binary128 instantiation rounded to double once, and REPORT(aest_all) for the state-space families.  They are OUTPUTS of the
reference's program, kept as a fixture so that the GPU suite can compare the engine with the reference on a machine that has
neither the checkout nor oracle/_ref/ (tests/test_gpu_reference.py); tests/test_reference_parity.py asserts that the committed
file equals a fresh evaluation.  Hex encoding of tests/golden_io.py."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from cases import problem_from_spec  # noqa: E402
from gen_golden import enc  # noqa: E402
from golden_io import load_golden  # noqa: E402
from reference_lib import ref_eval, ref_eval_quad  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "reference_results.json")


def reference_record(rec):
    """name, value, grad, value_binary128 and (state-space families) aest_all of one golden record, as numpy / floats"""
    pb = problem_from_spec(rec)
    par = rec["par"]
    out = dict(name=rec["name"])
    if pb.model in ("CTCRW", "OU_SSM", "BM_SSM"):       # (the ESEAL template has no REPORT)
        out["value"], out["grad"], out["aest_all"] = ref_eval(pb, par, order=1, report=True)
    else:
        out["value"], out["grad"] = ref_eval(pb, par, order=1)
    out["value_binary128"] = ref_eval_quad(pb, par, order=0)
    return out


def main():
    out = []
    for rec in load_golden():
        r = reference_record(rec)
        out.append({k: (v if isinstance(v, str) else enc(np.asarray(v, dtype=np.float64))) for k, v in r.items()})
    with open(PATH, "w") as f:
        json.dump(out, f)
    cases = os.path.getsize(os.path.join(ROOT, "tests", "golden", "cases.json"))
    print(f"wrote {len(out)} records to {PATH} ({os.path.getsize(PATH) / 1024:.0f} kB; cases.json: {cases / 1024:.0f} kB)")


if __name__ == "__main__":
    main()
