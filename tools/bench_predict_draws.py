"""Times ssde_predict_draws on a CTCRW d = 2 batch of irregular tracks -- per track two intervals with four offsets
each and two forecasts, 32 draws -- next to the route a user has today on the same data: ssde_create on the problem with NA rows at
the query times, ssde_smooth_draws on it and the gather of the wanted rows.  Whole-call wall times, best of --reps after a warm-up.
Kernel times come from a run of its own under rocprofv3:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o predict_draws -- python tools/bench_predict_draws.py --no-today

(dense_kernel<..., 0, 2> is the forward record pass, predict_draws_walk_kernel the draws' walk that stores the ends of the wanted
intervals, predict_draws_query_kernel the bridges)."""
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
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-today", action="store_true", help="leave today's route out (a kernel trace of ssde_predict_draws alone)")
    a = ap.parse_args()
    import torch
    M, T = a.tracks, a.rows
    ID, times, obs = capi.simulate_device("CTCRW", M, T, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=3)
    ID, obs = ID.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy())
    del times
    torch.cuda.empty_cache()
    rng = np.random.default_rng(1)
    times = np.cumsum(rng.uniform(0.5, 1.5, size=(M, T)), axis=1).ravel()            # irregular fixes
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    # per track: two interior rows with four offsets inside their intervals, and two forecasts past the last row
    trk = np.arange(M, dtype=np.int64)
    s1 = rng.integers(1, T // 2, size=M); s2 = rng.integers(T // 2, T - 1, size=M)
    rows = np.concatenate([np.repeat(trk * T + s1, 4), np.repeat(trk * T + s2, 4), np.repeat(trk * T + T - 1, 2)])
    dt = times[rows + 1 - (rows % T == T - 1)] - times[rows]
    frac = np.concatenate([np.tile([0.2, 0.4, 0.6, 0.8], 2 * M), np.tile([1.0, 2.0], M)])
    offs = np.where(rows % T == T - 1, frac, frac * dt)
    eng = capi.Engine(pb)
    out = eng.predict_draws(par, rows, offs, a.draws, seed=1)                        # warm-up (allocations, code objects)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = eng.predict_draws(par, rows, offs, a.draws, seed=1)
        ts.append(time.perf_counter() - t0)
    eng.close()
    sd = 4
    res = {"tracks": M, "rows_per_track": T, "n": pb.n, "queries": len(rows), "draws": a.draws, "slots": int(len(np.unique(rows))),
           "ms_predict_draws": 1e3 * min(ts), "host_out_bytes": 8 * len(rows) * sd * a.draws, "all_finite": bool(np.isfinite(out).all())}
    del out
    if not a.no_today:
        # today's route: NA rows at the query times (covariate-free model: nothing else to copy), a handle on them, every draw home
        t0 = time.perf_counter()
        qt = times[rows] + offs
        order = np.lexsort((np.r_[times, qt], np.r_[ID, ID[rows]]))
        ID2, t2 = np.r_[ID, ID[rows]][order], np.r_[times, qt][order]
        obs2 = np.r_[obs, np.full((len(rows), 2), np.nan)][order]
        where = np.empty(len(order), dtype=np.int64); where[order] = np.arange(len(order))
        pb2 = capi.Problem("CTCRW", ID2, t2, np.ascontiguousarray(obs2))
        t_aug = time.perf_counter() - t0
        t0 = time.perf_counter()
        eng2 = capi.Engine(pb2)
        t_create = time.perf_counter() - t0
        td = []
        for _ in range(1 + max(a.reps - 1, 1)):
            t0 = time.perf_counter()
            got = eng2.smooth_draws(par, a.draws, seed=1)[:, where[pb.n:], :]
            td.append(time.perf_counter() - t0)
            ok = bool(np.isfinite(got).all())
            del got
        eng2.close()
        res.update(ms_today_augment=1e3 * t_aug, ms_today_create=1e3 * t_create, ms_today_smooth_draws_and_gather=1e3 * min(td[1:]),
                   today_host_out_bytes=8 * pb2.n * sd * a.draws, today_all_finite=ok)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
