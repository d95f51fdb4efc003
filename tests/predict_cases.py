"""Shared cases of the ssde_predict tests (test infrastructure): the small problems of the CPU suites, the query sets that go
through every rule of DESIGN.md §3.11, and the comparison under the smoother's own limits (§3.9)."""
import numpy as np

from cases import make_spec, problem_from_spec

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS = [9, 1, 2, 3, 7]                    # rows 0-8, 9, 10-11, 12-14, 15-21
NA_ROWS = (4, 8, 17)                         # row 8 ends the first track
GAPS = {}                                    # tag -> (mean gap, covariance gap): what DESIGN.md §3.11's table is filled from


def small_problem(model, d, irregular=True, variant="const", with_HP=False, seed=0):
    spec = make_spec(f"pr_{model}_{d}_{irregular}_{variant}_{with_HP}", model, d, seed=71 + d + seed, lengths=LENGTHS,
                     na_rows=NA_ROWS, irregular=irregular, variant=variant, with_H=with_HP, with_P0=with_HP)
    return problem_from_spec(spec), np.array(spec["par"], dtype=np.float64)


def intervals(pb):
    """(first, last, dt): flags of every track's first and last row, dtimes with the reference's dtimes(n - 1) = 1"""
    n = pb.n
    first = np.zeros(n, dtype=bool); first[pb.seg_start] = True
    last = np.zeros(n, dtype=bool); last[np.r_[pb.seg_start[1:] - 1, n - 1]] = True
    t = np.asarray(pb.times, dtype=np.float64)
    return first, last, np.r_[t[1:] - t[:-1], 1.0]


def query_set(pb, seed=0, per_row=True, shuffle=True):
    """Queries over every rule: on every interior row the offsets 0, Delta and two inside; forecasts at 0 and past every track's
    last row; a query on every first row and one past the next fix (both NaN); duplicates; in no particular order."""
    rng = np.random.default_rng(seed)
    first, last, dt = intervals(pb)
    rows, offs = [], []
    for j in range(pb.n):
        if first[j]:
            rows += [j]; offs += [0.1 * float(rng.uniform(0.0, 1.0))]
        elif last[j]:
            rows += [j] * 4; offs += [0.0, 0.25, 1.7, 6.0]
        elif per_row or rng.uniform() < 0.3:
            rows += [j] * 4; offs += [0.0, dt[j], 0.37 * dt[j], float(rng.uniform(0.0, 1.0)) * dt[j]]
    inner = np.flatnonzero(~first & ~last)
    if len(inner):
        j = int(inner[len(inner) // 2])
        rows += [j, j, j]; offs += [1.5 * dt[j], 0.37 * dt[j], 0.37 * dt[j]]          # past the next fix; a duplicate pair
    rows, offs = np.array(rows, dtype=np.int64), np.array(offs, dtype=np.float64)
    if shuffle:
        p = rng.permutation(len(rows))
        rows, offs = rows[p], offs[p]
    return rows, offs


def expected_nan(pb, rows, offs):
    first, last, dt = intervals(pb)
    rows = np.asarray(rows)
    return first[rows] | (~last[rows] & (np.asarray(offs) > dt[rows] * (1.0 + 1e-9)))


def compare(got, ref, tag, mean_tol=1e-10, cov_tol=1e-9):
    """mean: mean_tol (1 + max|ref|); covariance: cov_tol max|ref|; NaN patterns identical.  Returns and records the two gaps."""
    gm, rm = np.asarray(got["mean"]), np.asarray(ref["mean"])
    assert gm.shape == rm.shape, tag
    assert np.array_equal(np.isnan(gm), np.isnan(rm)), tag
    ok = ~np.isnan(rm)
    gap_m = np.max(np.abs(gm[ok] - rm[ok]), initial=0.0) / (1.0 + np.max(np.abs(rm[ok]), initial=0.0))
    gap_c = 0.0
    if got.get("cov") is not None and ref.get("cov") is not None:
        gc, rc = np.asarray(got["cov"]), np.asarray(ref["cov"])
        assert np.array_equal(np.isnan(gc), np.isnan(rc)), tag
        okc = ~np.isnan(rc)
        gap_c = np.max(np.abs(gc[okc] - rc[okc]), initial=0.0) / max(np.max(np.abs(rc[okc]), initial=0.0), 1e-300)
    print(f"GAP {tag}: mean {gap_m:.2e} cov {gap_c:.2e}")
    old = GAPS.get(tag.split(":")[0], (0.0, 0.0))
    GAPS[tag.split(":")[0]] = (max(old[0], gap_m), max(old[1], gap_c))
    assert gap_m <= mean_tol, (tag, gap_m)
    assert gap_c <= cov_tol, (tag, gap_c)
    return gap_m, gap_c
