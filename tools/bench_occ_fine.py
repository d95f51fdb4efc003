"""Times ssde_path_occupancy_fine on a CTCRW d = 2 batch of irregular tracks (intervals uniform on 0.5 .. 1.5) with dt
weights and a pooled grid, on ONE handle:
  (a) ssde_path_occupancy (the kernel of §3.13, unchanged);
  (b) the new call at max_step = +inf (every m = 1: the same numbers through the new kernels);
  (c) the new call at --max-step (0.28: a mean m of about 4);
and, on a second handle of the first --today-tracks tracks (as many as today's host plan takes in reasonable time),
  (c') the new call at --max-step again, and
  (d) today's route at the same points: ssde_predict_draws with (c)'s offsets for the inner points and the binning in numpy
      (np.bincount with the points' shares).  The rows' own points come from ssde_smooth_draws: asking ssde_predict_draws for them
      as offset-0 queries would give the inner offsets of every slot the next rank, i.e. another (equally distributed) path than
      (c)'s.  That call's share of (d) is timed apart and reported, so (d) can also be read without it.
Whole-call wall times, best of --reps after a warm-up; the result line is printed and appended to --out (profiles/occ_fine_bench.txt).
(d) scaled to all tracks is an EXTRAPOLATION and labelled so.  Kernel times come from a run of its own under rocprofv3:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o occ_fine -- python tools/bench_occ_fine.py --no-today --out /dev/null
    python tools/bench_occ_fine.py --kernel-stats OUT/.../occ_fine_kernel_stats.csv

(dense_kernel<..., 0, 2> is the forward record pass, predict_draws_walk_kernel the draws' walk that leaves the ends of every slot,
path_occ_fine_kernel<4, 2, true> the new kernel in the LDS-tile form, path_occ_kernel<4, 2, true> call (a)'s.)"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smoothsde_amd import capi  # noqa: E402


def kernel_rows(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if any(k in name for k in ("path_occ_fine_kernel", "path_occ_kernel", "predict_draws_walk_kernel", "dense_kernel")):
                rows.append(f"{name.split('(')[0]}: calls {r.get('Calls')}, total {float(r.get('TotalDurationNs', 0)) / 1e6:.3f} ms, "
                            f"average {float(r.get('AverageNs', 0)) / 1e6:.3f} ms")
    return rows


def fine_points(times, T, max_step):
    """per state row that is not its track's last: m, and the inner points' (row, offset, share of the row's weight)"""
    n = len(times)
    j = np.arange(n)
    inner = (j % T != 0) & (j % T != T - 1)
    dt = np.r_[np.diff(times), 1.0]
    m = np.ones(n, dtype=np.int64)
    m[inner] = np.clip(np.ceil(dt[inner] / max_step), 1, 64).astype(np.int64)
    rows = np.repeat(j, m - 1)
    k = np.arange(len(rows)) - np.repeat(np.cumsum(m - 1) - (m - 1), m - 1) + 1
    return m, rows, (k * dt[rows]) / m[rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=1_000)
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--max-step", type=float, default=0.28)
    ap.add_argument("--today-tracks", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-today", action="store_true", help="leave today's route out (a kernel trace of the three calls alone)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occ_fine_bench.txt"))
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv: append its kernel times to --out and stop")
    a = ap.parse_args()
    if a.kernel_stats:
        lines = ["Kernel times (rocprofv3 --kernel-trace --stats, one run of tools/bench_occ_fine.py --no-today: a warm-up and --reps calls of each):"] + kernel_rows(a.kernel_stats)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    import torch
    M, T = a.tracks, a.rows
    ID, times, obs = capi.simulate_device("CTCRW", M, T, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=3)
    ID, obs = ID.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy())
    del times
    torch.cuda.empty_cache()
    rng = np.random.default_rng(1)
    times = np.cumsum(rng.uniform(0.5, 1.5, size=(M, T)), axis=1).ravel()            # irregular fixes
    par = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    q = np.array([np.quantile(obs[:, c], [.02, .98]) for c in range(2)])
    nc = a.cells
    grid = {"x0": q[0, 0], "dx": (q[0, 1] - q[0, 0]) / nc, "nx": nc, "y0": q[1, 0], "dy": (q[1, 1] - q[1, 0]) / nc, "ny": nc}

    def weights(tm):
        w = np.r_[np.diff(tm), 0.0]
        w[T - 1::T] = 0.0
        return w

    def best(fn):
        fn()                                                          # warm-up (allocations, code objects)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return 1e3 * min(ts)

    pb = capi.Problem("CTCRW", ID, times, obs)
    eng = capi.Engine(pb)
    w = weights(times)
    res = {}
    ms_a = best(lambda: res.__setitem__("a", eng.path_occupancy(par, a.draws, grid, seed=1, weight=w)))
    ms_b = best(lambda: res.__setitem__("b", eng.path_occupancy_fine(par, a.draws, grid, np.inf, seed=1, weight=w)))
    ms_c = best(lambda: res.__setitem__("c", eng.path_occupancy_fine(par, a.draws, grid, a.max_step, seed=1, weight=w)))
    n_points, n_capped = eng.last_occupancy_points()
    form = eng.last_occupancy_form()
    eng.close()
    state_w = w.copy()
    state_w[::T] = 0.0
    total = a.draws * float(state_w.sum())
    out = {"tracks": M, "rows_per_track": T, "n": pb.n, "draws": a.draws, "cells": nc, "max_step": a.max_step,
           "mean_m": n_points / (pb.n - M), "n_points": n_points, "n_capped": n_capped, "form": form,
           "ms_a_path_occupancy": ms_a, "ms_b_fine_inf": ms_b, "ms_c_fine": ms_c, "b_minus_a_ms": ms_b - ms_a,
           "b_equals_a_bitwise": bool(np.array_equal(res["a"][0], res["b"][0]) and np.array_equal(res["a"][1], res["b"][1])),
           "conservation_rel_gap": {k: abs(float(v[0].sum() + v[1].sum()) - total) / total for k, v in res.items()},
           "inside_share": {k: float(v[0].sum()) / total for k, v in res.items()},
           "empty_cells": {k: int(np.count_nonzero(v[0] == 0)) for k, v in res.items()}}
    if not a.no_today:
        Mt = min(a.today_tracks, M)
        nt = Mt * T
        pbt = capi.Problem("CTCRW", ID[:nt], times[:nt], np.ascontiguousarray(obs[:nt]))
        engt = capi.Engine(pbt)
        wt = weights(times[:nt])
        ms_ct = best(lambda: res.__setitem__("ct", engt.path_occupancy_fine(par, a.draws, grid, a.max_step, seed=1, weight=wt)))
        m, q_rows, q_offs = fine_points(times[:nt], T, a.max_step)

        t_rows = []

        def today():
            t0 = time.perf_counter()
            rows = engt.smooth_draws(par, a.draws, seed=1)                               # (draws, n, 4)
            t_rows.append(time.perf_counter() - t0)
            inner = engt.predict_draws(par, q_rows, q_offs, a.draws, seed=1)             # (draws, n_query, 4)
            share = wt / m
            occ = np.zeros(nc * nc)
            for pos, sh in ((rows[:, :, [0, 2]], share), (inner[:, :, [0, 2]], share[q_rows])):
                with np.errstate(invalid="ignore"):
                    ix = np.floor((pos[:, :, 0] - grid["x0"]) / grid["dx"])
                    iy = np.floor((pos[:, :, 1] - grid["y0"]) / grid["dy"])
                ok = (ix >= 0) & (ix < nc) & (iy >= 0) & (iy < nc)
                cell = (ix + nc * iy)[ok].astype(np.int64)
                occ += np.bincount(cell, weights=np.broadcast_to(sh[None, :], ok.shape)[ok], minlength=nc * nc)
            res["d"] = occ

        ms_d = best(today)
        engt.close()
        gap = float(np.max(np.abs(res["d"].reshape(nc, nc) - res["ct"][0][0])) / np.max(res["ct"][0][0]))
        ms_rows = 1e3 * min(t_rows[1:])
        out.update(today_tracks=Mt, today_queries=int(len(q_rows)), ms_c_fine_on_today_tracks=ms_ct, ms_d_today_route=ms_d,
                   ms_d_row_draws_part=ms_rows, c_faster_than_d=bool(ms_ct < ms_d), d_over_c=ms_d / ms_ct,
                   c_faster_than_d_without_row_draws=bool(ms_ct < ms_d - ms_rows), d_vs_c_largest_cell_gap_rel=gap,
                   ms_d_EXTRAPOLATED_to_all_tracks=ms_d * M / Mt)
    line = json.dumps(out)
    print(line)
    with open(a.out, "a") as f:
        f.write(f"tools/bench_occ_fine.py --tracks {M} --rows {T} --draws {a.draws} --cells {nc} --max-step {a.max_step} "
                f"--today-tracks {a.today_tracks} (best of {a.reps} after a warm-up; whole-call wall times, ms):\n{line}\n")


if __name__ == "__main__":
    main()
