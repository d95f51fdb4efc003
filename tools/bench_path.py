"""Times ssde_path_stats on a CTCRW d = 2 batch next to the two ways of getting the same summaries from
ssde_smooth_draws on the same handle: the draws left in HBM (SSDE_DRAWS_DEVICE_OUT) and the draws brought to the host.  Whole-call
wall times, best of --reps; the result line is printed and appended to --out (profiles/path_bench.txt).  Kernel times come from a
run of its own under rocprofv3, whose kernel statistics --kernel-stats then adds to the same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o path -- python tools/bench_path.py --tracks 10000 --rows 1000 --draws 32 --no-host
    python tools/bench_path.py --kernel-stats OUT/.../path_kernel_stats.csv

(dense_kernel<..., 0, 2> is the forward record pass, path_stats_kernel the backward pass that reduces the draws in registers,
smooth_draws_kernel the one that stores them)."""
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
    """name, calls, total ms and average ms of the record, draws and path kernels in a rocprofv3 kernel_stats.csv"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if any(k in name for k in ("path_stats_kernel", "smooth_draws_kernel", "dense_kernel", "path_row_map_kernel")):
                rows.append(f"{name.split('(')[0]}: calls {r.get('Calls')}, total {float(r.get('TotalDurationNs', 0)) / 1e6:.3f} ms, "
                            f"average {float(r.get('AverageNs', 0)) / 1e6:.3f} ms")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=1_000)
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--regions", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip ssde_smooth_draws to the host (n x sdim x draws doubles of host memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_bench.txt"))
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv: append its kernel times to --out and stop")
    a = ap.parse_args()
    if a.kernel_stats:
        lines = ["Kernel times (rocprofv3 --kernel-trace --stats):"] + kernel_rows(a.kernel_stats)
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
    # boxes around the quartiles of the observations, shifted by whole units; the weights are the time to the track's next row
    e = np.array([np.quantile(obs[:, c], [.25, .75]) for c in range(2)])
    reg = np.array([[e[0, 0] + k, e[0, 1] + k, e[1, 0] - k, e[1, 1] - k] for k in range(a.regions)])
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

    stats = {}
    ms_path = best(lambda: stats.__setitem__("s", eng.path_stats(par, a.draws, seed=1, regions=reg, weight=w)))
    buf = torch.empty((a.draws, sd, n), dtype=torch.float64, device="cuda:0")
    ms_dev = best(lambda: eng.smooth_draws(par, a.draws, seed=1, out=buf))
    # the statistics of draw 0 from the draws themselves: the path the reduction saw
    p = buf[0, [0, 2]].cpu().numpy().reshape(2, n_trk, a.rows)[:, :, 1:]
    length = np.sqrt((np.diff(p, axis=2) ** 2).sum(axis=0)).sum(axis=1)
    gap = float(np.max(np.abs(stats["s"][0, :, 0] - length)) / (1.0 + np.max(np.abs(length))))
    del buf
    torch.cuda.empty_cache()
    ms_host = None if a.no_host else best(lambda: eng.smooth_draws(par, a.draws, seed=1))
    eng.close()
    out = {"tracks": a.tracks, "rows_per_track": a.rows, "n": n, "draws": a.draws, "regions": a.regions,
           "ms_path_stats": ms_path, "ms_draws_device_out": ms_dev, "ms_draws_host": ms_host,
           "host_out_bytes_path_stats": 8 * n_trk * (2 + a.regions) * a.draws, "out_bytes_draws": 8 * n * sd * a.draws,
           "length_gap_draw0": gap, "all_finite": bool(np.isfinite(stats["s"]).all())}
    line = json.dumps(out)
    print(line)
    with open(a.out, "a") as f:
        f.write(f"tools/bench_path.py --tracks {a.tracks} --rows {a.rows} --draws {a.draws} --regions {a.regions} (best of {a.reps}; whole-call wall times, ms):\n{line}\n")


if __name__ == "__main__":
    main()
