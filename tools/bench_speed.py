"""Times ssde_path_speed on a CTCRW d = 2 batch, with and without the per-row counts, next to the two ways of
getting the same numbers from ssde_smooth_draws on the same handle: the draws left in HBM (SSDE_DRAWS_DEVICE_OUT) and the draws
brought to the host and reduced there in numpy (tests/speed_ref.py).  Whole-call wall times, best of --reps (the host route once);
the result line is printed and appended to --out (profiles/speed_bench.txt).  Kernel times come from a run of its own under
rocprofv3, whose kernel statistics --kernel-stats then adds to the same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o speed -- python tools/bench_speed.py --tracks 10000 --rows 1000 --draws 32 --no-host
    python tools/bench_speed.py --kernel-stats OUT/.../speed_kernel_stats.csv

(dense_kernel<..., 0, 2> is the forward record pass, path_speed_kernel the backward pass that reduces the draws in registers and
counts the rows, smooth_draws_kernel the one that stores the draws)."""
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
    """name, calls, total ms and average ms of the record, draws and speed kernels in a rocprofv3 kernel_stats.csv"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if any(k in name for k in ("path_speed_kernel", "smooth_draws_kernel", "dense_kernel", "path_row_map_kernel")):
                rows.append(f"{name.split('(')[0]}: calls {r.get('Calls')}, total {float(r.get('TotalDurationNs', 0)) / 1e6:.3f} ms, "
                            f"average {float(r.get('AverageNs', 0)) / 1e6:.3f} ms")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=1_000)
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--thresholds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip ssde_smooth_draws to the host and its numpy reduction (n x sdim x draws doubles of host memory, and as much again while reducing)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speed_bench.txt"))
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
    # thresholds spread over the speeds a CTCRW with nu = 1 visits; the weights are the time to the track's next row
    thr = np.linspace(0.25, 2.0, a.thresholds)
    w = np.r_[np.diff(times), 0.0]
    w[pb.seg_start[1:] - 1] = 0.0

    def best(fn, reps):
        fn()                                                          # warm-up (allocations, code objects)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return 1e3 * min(ts)

    got = {}
    ms_both = best(lambda: got.__setitem__("both", eng.path_speed(par, a.draws, seed=1, thresholds=thr, weight=w)), a.reps)
    ms_stats = best(lambda: got.__setitem__("stats", eng.path_speed(par, a.draws, seed=1, thresholds=thr, weight=w, rows=False)), a.reps)
    same = bool(np.array_equal(got["both"][0], got["stats"][0], equal_nan=True))
    buf = torch.empty((a.draws, sd, n), dtype=torch.float64, device="cuda:0")
    ms_dev = best(lambda: eng.smooth_draws(par, a.draws, seed=1, out=buf), a.reps)
    # statistic 0 of draw 0 from the draws themselves: the path the reduction saw
    v = buf[0, [1, 3]].cpu().numpy().reshape(2, n_trk, a.rows)[:, :, 1:]
    total = (np.sqrt((v ** 2).sum(axis=0)) * w.reshape(n_trk, a.rows)[:, 1:]).sum(axis=1)
    gap = float(np.max(np.abs(got["both"][0][0, :, 0] - total)) / (1.0 + np.max(np.abs(total))))
    del buf, v
    torch.cuda.empty_cache()
    ms_host = ms_host_reduce = differs = None
    if not a.no_host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from speed_ref import speed_ref
        t0 = time.perf_counter()
        draws = eng.smooth_draws(par, a.draws, seed=1)
        ms_host = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = speed_ref(draws, pb.seg_start, 2, thresholds=thr, weight=w)
        ms_host_reduce = 1e3 * (time.perf_counter() - t0)
        differs = int(np.count_nonzero(ref[1] != got["both"][1]))         # (a speed within rounding of a threshold may fall either way)
        del draws
    eng.close()
    out = {"tracks": a.tracks, "rows_per_track": a.rows, "n": n, "draws": a.draws, "thresholds": a.thresholds,
           "ms_path_speed": ms_both, "ms_path_speed_no_row_below": ms_stats, "ms_draws_device_out": ms_dev, "ms_draws_host": ms_host,
           "ms_host_numpy_reduce": ms_host_reduce,
           "host_out_bytes_stats": 8 * n_trk * (5 + a.thresholds) * a.draws, "host_out_bytes_row_below": 4 * n * a.thresholds,
           "out_bytes_draws": 8 * n * sd * a.draws, "sum_gap_draw0": gap, "stats_alone_bitwise": same, "row_below_entries_differing_from_numpy": differs,
           "all_finite": bool(np.isfinite(got["both"][0]).all())}
    line = json.dumps(out)
    print(line)
    with open(a.out, "a") as f:
        f.write(f"tools/bench_speed.py --tracks {a.tracks} --rows {a.rows} --draws {a.draws} --thresholds {a.thresholds} (best of {a.reps}; whole-call wall times, ms):\n{line}\n")


if __name__ == "__main__":
    main()
