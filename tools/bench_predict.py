"""Times ssde_predict on a CTCRW d = 2 batch on a regular grid, next to ssde_smooth (mean + covariance) on the
same handle: whole-call wall time, and the bytes the layout moves per row and per query.  Kernel times come from a run of its own
under rocprofv3:

    rocprofv3 --kernel-trace --stats -d OUT -o predict -- python tools/bench_predict.py --tracks 10000 --rows 1000 --per-track 10

(dense_kernel<..., 0, 2> is the forward record pass, predict_walk_kernel the backward walk that fills the packets,
predict_query_kernel the queries; smooth_back_kernel is ssde_smooth's backward pass on the same batch)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smoothsde_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=1_000)
    ap.add_argument("--per-track", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-smooth", action="store_true", help="leave ssde_smooth out (a kernel trace of ssde_predict alone)")
    a = ap.parse_args()
    import torch
    ID, times, obs = capi.simulate_device("CTCRW", a.tracks, a.rows, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=3)
    pb = capi.Problem("CTCRW", ID.cpu().numpy(), times.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy()))
    del ID, times, obs
    torch.cuda.empty_cache()
    par = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    eng = capi.Engine(pb)
    # R mirrors SmoothRec<M_CTCRW, 2>::R (ssde_smooth.hpp), SW / PK PredictPk<M_CTCRW, 2>::SW / SZ (ssde_predict.hpp): change them together
    n, sd, d, R, SW, PK = pb.n, 4, 2, 31, 5, 33
    rng = np.random.default_rng(1)
    dt = float(pb.times[1] - pb.times[0])
    # per track: per_track - 1 times inside the track (any state row but the last, any offset inside its interval) and one forecast
    trk = np.repeat(np.arange(a.tracks, dtype=np.int64), a.per_track)
    step = rng.integers(1, a.rows - 1, size=len(trk))
    step[::a.per_track] = a.rows - 1
    rows = trk * a.rows + step
    offs = rng.uniform(0.0, dt, size=len(trk))
    out = eng.predict(par, rows, offs)                                # warm-up (allocations, code objects)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = eng.predict(par, rows, offs)
        ts.append(time.perf_counter() - t0)
    slots = len(np.unique(rows))
    res = {"tracks": a.tracks, "rows_per_track": a.rows, "n": n, "queries": len(rows), "queries_per_track": a.per_track, "slots": slots,
           "ms_predict": 1e3 * min(ts),
           # forward: tiles read (dt-less regular grid: y, 2 doubles), record and side row written; walk: the records once, the side row
           # and the packet of a wanted step; query: the packet and the offset read, 20 doubles written
           "bytes_per_row": 8 * (d + R + SW + R), "bytes_per_slot": 8 * (SW + PK), "bytes_per_query": 8 * (PK + 1 + 2 + sd + sd * sd),
           "host_out_bytes": 8 * len(rows) * (sd + sd * sd),
           "all_finite": bool(np.isfinite(out["mean"]).all() and np.isfinite(out["cov"]).all())}
    if not a.no_smooth:
        eng.smooth(par, cov=True, resid=False)
        tm = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            eng.smooth(par, cov=True, resid=False)
            tm.append(time.perf_counter() - t0)
        res.update(ms_smooth_mean_cov=1e3 * min(tm), smooth_host_out_bytes=8 * n * (sd + sd * sd))
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
