"""Times ssde_smooth_loo on a CTCRW d = 2 batch next to ssde_smooth on the same handle: whole-call wall times
(best of --reps) of the smoother with mean + resid and with the covariance, and of the new call with every output, with the per-row
outputs but no covariance, and with lpd + stats alone; the bytes per row each moves.  The result line is printed and appended to
--out (profiles/loo_bench.txt).  Kernel times come from a run of its own under rocprofv3, whose kernel trace --kernel-trace then
adds to the same file, launch by launch in the order the calls were made:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o loo -- python tools/bench_loo.py --tracks 10000 --rows 1000
    python tools/bench_loo.py --kernel-trace OUT/.../loo_kernel_trace.csv

(dense_kernel<..., 0, 2> is the forward record pass both calls share, smooth_back_kernel the smoother's backward pass,
loo_back_kernel the new one)."""
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

# the calls in the order they are made (each once to warm up, then --reps times)
CALLS = ("smooth mean + resid", "smooth mean + cov + resid", "loo every output", "loo mean + resid + lpd + stats", "loo lpd + stats")


def trace_rows(path):
    """per kernel of interest, its launches' durations in ms in start order, from a rocprofv3 kernel_trace.csv"""
    runs = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for k in ("loo_back_kernel", "smooth_back_kernel", "dense_kernel", "path_row_map_kernel"):
                if k in name:
                    runs.setdefault(name.split("(")[0], []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return [f"{name}: {len(v)} launches, ms in start order: " + " ".join(f"{ms:.3f}" for _, ms in sorted(v)) for name, v in sorted(runs.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=1_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--thresholds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_bench.txt"))
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 kernel_trace.csv: append its launches' times to --out and stop")
    a = ap.parse_args()
    if a.kernel_trace:
        lines = ["Kernel times (rocprofv3 --kernel-trace), the calls in the order: " + "; ".join(CALLS) + f" (each 1 + {a.reps} launches):"]
        lines += trace_rows(a.kernel_trace)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    import torch
    ID, times, obs = capi.simulate_device("CTCRW", a.tracks, a.rows, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=3)
    pb = capi.Problem("CTCRW", ID.cpu().numpy(), times.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy()))
    del ID, times, obs
    torch.cuda.empty_cache()
    par = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    eng = capi.Engine(pb)
    n, sd, d, R = pb.n, 4, 2, 31
    thr = np.array([5.99, 9.21, 13.82, 18.42, 23.03, 27.63, 32.24, 36.84][:a.thresholds])      # chi-square_2 quantiles 0.95, 0.99, 0.999, ...

    def best(fn):
        fn()                                                          # warm-up (allocations, code objects)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return 1e3 * min(ts)

    lib, h = eng.lib, eng._h
    P = lambda x: None if x is None else x.ctypes.data_as(capi._dp)
    mean, cov, res, lpd = np.zeros((n, d), order="F"), np.zeros((n, d, d), order="F"), np.zeros((n, d), order="F"), np.zeros(n)
    st = np.zeros((4 + len(thr), pb.n_seg))

    def loo(m, c, e, l, s):
        rc = lib.ssde_smooth_loo(h, P(par), pb.n_par_full, P(m), P(c), P(e), P(l), P(thr) if s is not None and len(thr) else None,
                                 len(thr) if s is not None else 0, P(s), 0)
        assert rc == 0, rc

    out = {"tracks": a.tracks, "rows_per_track": a.rows, "n": n, "thresholds": len(thr)}
    out["ms_smooth_mean_resid"] = best(lambda: eng.smooth(par, cov=False))
    out["ms_smooth_cov"] = best(lambda: eng.smooth(par, cov=True))
    out["ms_loo_all"] = best(lambda: loo(mean, cov, res, lpd, st))
    out["ms_loo_no_cov"] = best(lambda: loo(mean, None, res, lpd, st))
    out["ms_loo_lpd_stats"] = best(lambda: loo(None, None, None, lpd, st))
    ok = np.isfinite(lpd)
    out["served_rows"] = int(ok.sum())
    out["elpd"] = float(st[1].sum())
    out["elpd_gap_to_row_sum"] = float(abs(st[1].sum() - lpd[ok].sum()) / abs(lpd[ok].sum()))
    out["rows_over_thresholds"] = [int(v) for v in st[4:].sum(axis=1)]
    # bytes per row: the record pass reads the tiles (a regular grid: y, 2 doubles) and writes the record; the backward pass of the
    # smoother reads all 31 record doubles, the new one 19 (V 2, F^-1 3, K 8, T 2, E 2, the measured columns of A 2) -- never P
    out["record_bytes_per_row"] = 8 * R
    out["smooth_back_read_bytes_per_row"] = 8 * R
    out["loo_back_read_bytes_per_row"] = 8 * 19
    out["loo_back_write_bytes_per_row_all"] = 8 * (d + d * d + d + 1)
    out["d2h_bytes_loo_all"] = 8 * n * (d + d * d + d + 1)
    out["d2h_bytes_smooth_cov"] = 8 * n * (sd + sd * sd + d)
    eng.close()
    line = json.dumps(out)
    print(line)
    with open(a.out, "a") as f:
        f.write(f"tools/bench_loo.py --tracks {a.tracks} --rows {a.rows} --thresholds {len(thr)} (best of {a.reps}; whole-call wall times, ms):\n{line}\n")


if __name__ == "__main__":
    main()
