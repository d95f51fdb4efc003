"""Times ssde_path_occupancy on a CTCRW d = 2 batch with dt weights: a pooled grid in the LDS-tile form, the same grid
with SSDE_OCC_FORCE_GLOBAL, and one grid per track (the global form) -- next to ssde_path_stats with 8 regions and ssde_smooth_draws
with SSDE_DRAWS_DEVICE_OUT on the same handle.  Whole-call wall times, best of --reps; the result line is printed and appended to
--out (profiles/occ_bench.txt).  Kernel times come from a run of its own under rocprofv3, whose kernel statistics --kernel-stats then
adds to the same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o occ -- python tools/bench_occ.py --out /dev/null
    python tools/bench_occ.py --kernel-stats OUT/.../occ_kernel_stats.csv

(dense_kernel<..., 0, 2> is the forward record pass; path_occ_kernel<4, 2, true> the LDS-tile form, <4, 2, false> the global form.)"""
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
    """name, calls, total ms and average ms of the record, draws, path and occupancy kernels in a rocprofv3 kernel_stats.csv"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if any(k in name for k in ("path_occ_kernel", "path_stats_kernel", "smooth_draws_kernel", "dense_kernel", "path_row_map_kernel")):
                rows.append(f"{name.split('(')[0]}: calls {r.get('Calls')}, total {float(r.get('TotalDurationNs', 0)) / 1e6:.3f} ms, "
                            f"average {float(r.get('AverageNs', 0)) / 1e6:.3f} ms")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=1_000)
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--cells", type=int, default=64, help="the pooled grid is cells x cells")
    ap.add_argument("--track-cells", type=int, default=32, help="the per-track grids are track-cells x track-cells")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occ_bench.txt"))
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv: append its kernel times to --out and stop")
    a = ap.parse_args()
    if a.kernel_stats:
        lines = ["Kernel times (rocprofv3 --kernel-trace --stats, one run of tools/bench_occ.py: a warm-up and --reps calls of each):"] + kernel_rows(a.kernel_stats)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    import torch
    ID, times, obs = capi.simulate_device("CTCRW", a.tracks, a.rows, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=3)
    ID, times, obs = ID.cpu().numpy(), times.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy())
    pb = capi.Problem("CTCRW", ID, times, obs)
    torch.cuda.empty_cache()
    par = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    eng = capi.Engine(pb)
    n, sd, n_trk = pb.n, 4, pb.n_seg
    q = np.array([np.quantile(obs[:, c], [.02, .98]) for c in range(2)])
    grid = lambda nc: {"x0": q[0, 0], "dx": (q[0, 1] - q[0, 0]) / nc, "nx": nc, "y0": q[1, 0], "dy": (q[1, 1] - q[1, 0]) / nc, "ny": nc}
    e = np.array([np.quantile(obs[:, c], [.25, .75]) for c in range(2)])
    reg = np.array([[e[0, 0] + k, e[0, 1] + k, e[1, 0] - k, e[1, 1] - k] for k in range(8)])
    w = np.r_[np.diff(times), 0.0]
    w[pb.seg_start[1:] - 1] = 0.0

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

    res, forms = {}, {}

    def occ(key, **kw):
        res[key] = eng.path_occupancy(par, a.draws, seed=1, weight=w, **kw)
        forms[key] = eng.last_occupancy_form()

    ms_tile = best(lambda: occ("tile", grid=grid(a.cells)))
    ms_global = best(lambda: occ("global", grid=grid(a.cells), force_global=True))
    ms_track = best(lambda: occ("track", grid=grid(a.track_cells), group=np.arange(n_trk, dtype=np.int32), n_groups=n_trk))
    ms_path = best(lambda: eng.path_stats(par, a.draws, seed=1, regions=reg, weight=w))
    buf = torch.empty((a.draws, sd, n), dtype=torch.float64, device="cuda:0")
    ms_dev = best(lambda: eng.smooth_draws(par, a.draws, seed=1, out=buf))
    del buf
    eng.close()
    state_w = w.copy()
    state_w[pb.seg_start] = 0.0
    total = a.draws * float(state_w.sum())
    out = {"tracks": a.tracks, "rows_per_track": a.rows, "n": n, "draws": a.draws, "cells": a.cells, "track_cells": a.track_cells,
           "ms_occ_pooled_tile": ms_tile, "ms_occ_pooled_global": ms_global, "ms_occ_per_track_global": ms_track,
           "ms_path_stats_8_regions": ms_path, "ms_draws_device_out": ms_dev, "forms": forms,
           "tile_vs_path_stats": ms_tile / ms_path,
           "forms_bitwise_equal": bool(np.array_equal(res["tile"][0], res["global"][0]) and np.array_equal(res["tile"][1], res["global"][1])),
           "conservation_rel_gap": {k: abs(float(v[0].sum() + v[1].sum()) - total) / total for k, v in res.items()},
           "inside_share_pooled": float(res["tile"][0].sum()) / total}
    line = json.dumps(out)
    print(line)
    with open(a.out, "a") as f:
        f.write(f"tools/bench_occ.py --tracks {a.tracks} --rows {a.rows} --draws {a.draws} --cells {a.cells} --track-cells {a.track_cells} "
                f"(best of {a.reps}; whole-call wall times, ms):\n{line}\n")


if __name__ == "__main__":
    main()
