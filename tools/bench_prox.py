"""Times ssde_path_proximity on a CTCRW d = 2 batch next to the route a caller had without it: ssde_predict_draws
of the same queries brought to the host, reduced there by the vectorised numpy form of tests/prox_ref.py.  Pair p compares tracks 2p
and 2p + 1 at --points points (two per interval: on the row and half-way to the next).  Whole-call wall times that end in a device
synchronise, --warmup calls first, then the median of --reps; the two routes alternate.  The result line is printed and appended to
--out (profiles/prox_bench.txt).  Kernel times come from a run of its own under rocprofv3, whose kernel statistics --kernel-stats then
adds to the same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o prox -- python tools/bench_prox.py --no-host --reps 1 --warmup 1
    python tools/bench_prox.py --kernel-stats OUT/.../prox_kernel_stats.csv

(dense_kernel<..., 0, 2> is the forward record pass, predict_draws_walk_kernel the backward walk that stores the ends of the wanted
intervals, predict_draws_query_kernel the bridges, prox_tile_kernel and prox_fold_kernel the reduction this call adds)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from smoothsde_amd import capi  # noqa: E402

KERNELS = ("prox_tile_kernel", "prox_fold_kernel", "prox_gather_kernel", "predict_draws_walk_kernel", "predict_draws_query_kernel",
           "dense_kernel")


def kernel_rows(path):
    """name, calls, total ms and average ms of the call's kernels in a rocprofv3 kernel_stats.csv, and the share of the two new ones"""
    rows, total, new = [], 0.0, 0.0
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if any(k in name for k in KERNELS):
                ms = float(r.get("TotalDurationNs", 0)) / 1e6
                total += ms
                if "prox_tile_kernel" in name or "prox_fold_kernel" in name:
                    new += ms
                rows.append(f"{name.split('(')[0]}: calls {r.get('Calls')}, total {ms:.3f} ms, average {float(r.get('AverageNs', 0)) / 1e6:.3f} ms")
    rows.append(f"prox_tile_kernel + prox_fold_kernel: {new:.3f} ms of {total:.3f} ms of the call's kernels ({100.0 * new / max(total, 1e-30):.2f} %)")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000)
    ap.add_argument("--points", type=int, default=1_000)
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--radii", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (2 x points x pairs x sdim x draws doubles of host memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prox_bench.txt"))
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv: append its kernel times to --out and stop")
    a = ap.parse_args()
    if a.kernel_stats:
        lines = ["Kernel times (rocprofv3 --kernel-trace --stats):"] + kernel_rows(a.kernel_stats)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    import torch
    import prox_ref
    rows_per_track = (a.points + 1) // 2 + 2                          # a first row, (points + 1) / 2 rows that start an interval, a last row
    ID, times, obs = capi.simulate_device("CTCRW", 2 * a.pairs, rows_per_track, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=3)
    ID, times, obs = ID.cpu().numpy(), times.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy())
    pb = capi.Problem("CTCRW", ID, times, obs)
    torch.cuda.empty_cache()
    par = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    eng = capi.Engine(pb)
    sd, D = 4, 2
    i = np.arange(a.points)
    start = np.asarray(pb.seg_start, dtype=np.int64)
    qa = (start[0::2, None] + 1 + i[None, :] // 2).ravel()
    qb = (start[1::2, None] + 1 + i[None, :] // 2).ravel()
    dt = np.r_[np.diff(times), 1.0]
    oa, ob = (i[None, :] % 2 * 0.5).repeat(a.pairs, axis=0).ravel() * dt[qa], (i[None, :] % 2 * 0.5).repeat(a.pairs, axis=0).ravel() * dt[qb]
    pair_ptr = np.arange(a.pairs + 1, dtype=np.int64) * a.points
    n_point = a.pairs * a.points
    w = np.tile(np.r_[np.full(a.points - 1, 0.5), 0.0], a.pairs)
    # radii around the quartiles of the distance between the observed tracks at the rows
    d_obs = np.sqrt(((obs[qa] - obs[qb]) ** 2).sum(axis=1))
    radii = np.r_[np.quantile(d_obs, np.linspace(0.1, 0.5, max(a.radii - 1, 0))), np.inf][:a.radii] if a.radii else np.zeros(0)
    rows, offs = np.r_[qa, qb], np.r_[oa, ob]
    res = {}

    def device():
        res["dev"] = eng.path_proximity(par, qa, oa, qb, ob, pair_ptr, a.draws, seed=1, radii=radii, weight=w)

    def host():
        at = eng.predict_draws(par, rows, offs, a.draws, seed=1)
        res["host"] = prox_ref.proximity_fast(at, "CTCRW", 2, pair_ptr, radii, w)

    routes = [("ms_path_proximity", device)] + ([] if a.no_host else [("ms_predict_draws_host_numpy", host)])
    ts = {k: [] for k, _ in routes}
    for it in range(a.warmup + a.reps):
        for k, fn in routes:                                          # the routes alternate
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ts[k].append(1e3 * (time.perf_counter() - t0))
    plan = eng.last_proximity_plan()
    eng.close()
    out = {"pairs": a.pairs, "points_per_pair": a.points, "n_point": n_point, "draws": a.draws, "radii": len(radii), "n_rows": pb.n}
    for k in ts:
        out[k] = float(np.median(ts[k]))
        out[k + "_spread"] = [float(min(ts[k])), float(max(ts[k]))]
    out.update(plan=plan, all_finite=bool(np.isfinite(res["dev"]).all()),
               # per point and draw: what the two new kernels read (2 D position doubles and the weight's quanta once per draw) and
               # write (a tile's record shared by its points), what the query kernel writes into the batch buffer and the proximity
               # call never copies home, and what the call does copy home
               bytes_per_point_draw_new_kernels_read=8 * 2 * D + 8,
               bytes_per_point_draw_partial_records=8 * 11 * plan["n_tiles"] / n_point,
               bytes_per_point_draw_query_kernel_writes=8 * 2 * sd,
               bytes_per_point_draw_copied_home_by_predict_draws=8 * 2 * sd,
               bytes_copied_home_by_path_proximity=8 * a.pairs * (2 + len(radii)) * a.draws,
               bytes_copied_home_by_predict_draws=8 * 2 * n_point * sd * a.draws)
    if "host" in res:
        same = np.array_equal(res["dev"][:, :, 1:], res["host"][:, :, 1:], equal_nan=True)
        gap = float(np.nanmax(np.abs(res["dev"][:, :, 0] - res["host"][:, :, 0]) / np.maximum(res["host"][:, :, 0], 1e-300)))
        out.update(index_and_sums_bitwise_equal=bool(same), min_dist_rel_gap=gap)
    line = json.dumps(out)
    print(line)
    with open(a.out, "a") as f:
        f.write(f"tools/bench_prox.py --pairs {a.pairs} --points {a.points} --draws {a.draws} --radii {a.radii} ({a.warmup} warm-up calls, "
                f"median of {a.reps}; whole-call wall times, ms):\n{line}\n")


if __name__ == "__main__":
    main()
