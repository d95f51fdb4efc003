"""The lane math of ssde_smooth_loo on the CPU: tests/hostsim compiles csrc/ssde_loo.hpp over csrc/ssde_smooth.hpp
with g++ and walks each track the way one lane of k_smooth_loo.hip does -- smooth_record_row into a plain per-row record,
dense_step, then loo_back_row, loo_fold and loo_finish over the records (loosim_lib.smooth_loo).  That twin is compared with the
numpy definition (tests/loo_ref.py) for the three Kalman families at every width the engine instantiates (d = 1 ... 8) and on the
row-varying, a0 / P0, NA and det F <= 0 inputs; the stand-alone sanitizer program runs as well.

Limits (loo_cases.py): mean 1e-10 (1 + max|ref|), covariance 1e-9 max|ref|, residual 1e-9, NaN patterns, served rows, rows of the
maxima and threshold counts identical; lpd and the statistics k = 1, 2 at 1e-11 (1 + max|ref|).  Largest gaps measured on these
inputs, the twin against loo_ref: mean 4.4e-16, covariance 3.2e-15, residual 2.5e-14, lpd 2.9e-15, sum of lpd 2.0e-15, largest q
5.3e-15 (loo_ref against the joint Gaussian: test_loo_host.py)."""
import subprocess

import numpy as np
import pytest

import loo_cases as LC
import loosim_lib
from loo_ref import _stats, loo_ref

CASES = LC.host_cases()
GAPS = {}                                                     # the largest gaps seen (printed by -s runs)


@pytest.mark.parametrize("cid", [c for c, _, _, _ in CASES])
def test_twin_against_the_definition(cid):
    build = next(b for c, b, _, _ in CASES if c == cid)
    pb, par = build()
    with np.errstate(invalid="ignore"):
        thr = LC.midway_thresholds(loo_ref(pb, par)["q"])
        ref = loo_ref(pb, par, thr)
    got = loosim_lib.smooth_loo(pb, par, thr)
    LC.compare(got, ref, list(pb.seg_start) + [pb.n], GAPS)
    print(cid, {k: f"{v:.1e}" for k, v in GAPS.items()})
    assert ref["stats"][:, 0].sum() == ref["white"].sum() > 0


def test_twin_without_thresholds_and_with_a_row_map():
    # no thresholds: n_stat = 4; a row map (what a lattice-padded handle hands the kernel): rows mapped to -1 leave every output and
    # count, the row of a maximum is the caller's
    pb, par = LC.width_case("CTCRW", 2)
    ref = loo_ref(pb, par)
    got = loosim_lib.smooth_loo(pb, par)
    assert got["stats"].shape == (4, 4)
    LC.compare(got, ref, list(pb.seg_start) + [pb.n])
    crow = np.arange(pb.n, dtype=np.int64) * 3 + 1
    out = [5, 30, 31, 60]
    crow[out] = -1
    thr = LC.midway_thresholds(ref["q"], 3)
    got = loosim_lib.smooth_loo(pb, par, thr, crow=crow)
    want = {k: ref[k].copy() for k in ("mean", "cov", "resid", "lpd", "q", "white")}
    for k in ("mean", "cov", "resid", "lpd", "q"):
        want[k][out] = np.nan
    want["white"][out] = False
    want["stats"] = _stats(pb.n_seg, list(pb.seg_start) + [pb.n], want["q"], want["lpd"], want["white"], thr, crow=crow)
    LC.compare(got, want, list(pb.seg_start) + [pb.n])
    assert np.all(np.isnan(got["lpd"][out])) and np.all((got["stats"][[0, 1, 3], 3] - 1) % 3 == 0)


def test_sanitizer_program():
    """loo_san: the twin under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own.  It also holds the one row
    no data set reaches robustly: a record whose M_j is positive but whose D_j = 1 / M_j overflows -- served, loo_mean and loo_cov
    kept, no residual, no lpd, no statistic."""
    loosim_lib.load()
    r = subprocess.run([loosim_lib.SAN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "loo_san ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
