"""Times ssde_forecast_scores on a CTCRW d = 2 batch next to ssde_smooth on the same handle: the time of one call
with horizons (1, 2, 5, 10, 20), with the statistics alone and with the per-row outputs as well, and next to each the time of one
ssde_smooth call (the same forward record pass plus one backward pass: the yardstick).  Every call is synchronous, so it is timed
between two HIP events on the null stream around it and by the host's clock; warm (two calls first), the median of --reps runs.  The
result line is printed and appended to --out (profiles/forecast_scores_bench.txt)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smoothsde_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=1_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forecast_scores_bench.txt"))
    a = ap.parse_args()
    import torch
    ID, times, obs = capi.simulate_device("CTCRW", a.tracks, a.rows, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=3)
    pb = capi.Problem("CTCRW", ID.cpu().numpy(), times.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy()))
    del ID, times, obs
    torch.cuda.empty_cache()
    par = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    eng = capi.Engine(pb)
    n, d = pb.n, 2
    hz = np.array([1, 2, 5, 10, 20], dtype=np.int32)
    thr = np.array([5.991464547107979])
    lib, h = eng.lib, eng._h
    P = lambda x: None if x is None else x.ctypes.data_as(capi._dp)
    z, lpd = np.zeros((n, d, len(hz)), order="F"), np.zeros((n, len(hz)), order="F")
    st = np.zeros((len(hz), 6, pb.n_seg))
    mean, res = np.zeros((n, 4), order="F"), np.zeros((n, d), order="F")

    def ahead(zz, ll):
        rc = lib.ssde_forecast_scores(h, P(par), pb.n_par_full, hz.ctypes.data_as(capi.C.POINTER(capi.C.c_int32)), len(hz), P(zz), P(ll),
                                      P(thr), 1, P(st), 0)
        assert rc == 0, rc

    def smooth(with_mean):
        rc = lib.ssde_smooth(h, P(par), pb.n_par_full, P(mean) if with_mean else None, None, P(res))
        assert rc == 0, rc

    def median(fn):
        fn(); fn()                                                    # warm: allocations, code objects
        ev, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(e0.elapsed_time(e1))
        return {"events_ms": round(statistics.median(ev), 3), "wall_ms": round(statistics.median(wall), 3),
                "min_ms": round(min(ev), 3), "max_ms": round(max(ev), 3)}

    out = {"tracks": a.tracks, "rows_per_track": a.rows, "n": n, "horizons": hz.tolist(), "reps": a.reps}
    out["forecast_stats_only"] = median(lambda: ahead(None, None))
    out["smooth_resid_only"] = median(lambda: smooth(False))
    out["forecast_stats_and_rows"] = median(lambda: ahead(z, lpd))
    out["smooth_mean_resid"] = median(lambda: smooth(True))
    cnt = st[:, 0, :].sum(axis=1)
    out["scored_targets"] = [int(v) for v in cnt]
    out["mean_q"] = [round(float(v), 4) for v in st[:, 2, :].sum(axis=1) / cnt]
    out["coverage_95"] = [round(float(v), 4) for v in 1.0 - st[:, 5, :].sum(axis=1) / cnt]
    out["d2h_bytes_rows"] = int(8 * n * (d + 1) * len(hz))
    eng.close()
    line = json.dumps(out)
    print(line)
    with open(a.out, "a") as f:
        f.write(f"tools/bench_forecast.py --tracks {a.tracks} --rows {a.rows} (median of {a.reps} warm runs; one synchronous call between two "
                f"HIP events / by the host clock, ms):\n{line}\n")


if __name__ == "__main__":
    main()
