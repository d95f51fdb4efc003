"""Times ssde_smooth on a CTCRW d = 2 batch: wall time of the call with and without the covariance output, and
the bytes per row the layout moves.  Kernel times come from a run of its own under rocprofv3:

    rocprofv3 --kernel-trace --stats -d OUT -o smooth -- python tools/bench_smooth.py --tracks 10000 --rows 1000

(dense_kernel<..., 0, 2> is the forward record pass, smooth_back_kernel the backward one)."""
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
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    ID, times, obs = capi.simulate_device("CTCRW", a.tracks, a.rows, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=3)
    pb = capi.Problem("CTCRW", ID.cpu().numpy(), times.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy()))
    del ID, times, obs
    torch.cuda.empty_cache()
    par = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    eng = capi.Engine(pb)
    n = pb.n
    out = {"tracks": a.tracks, "rows_per_track": a.rows, "n": n}
    for cov in (False, True):
        eng.smooth(par, cov=cov)                                     # warm-up (allocations, code objects)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            eng.smooth(par, cov=cov)
            ts.append(time.perf_counter() - t0)
        out["ms_call_cov" if cov else "ms_call_mean_resid"] = 1e3 * min(ts)
    sd, d, R = 4, 2, 31
    out["record_bytes_per_row"] = 8 * R
    # forward: tiles read (dt-less regular grid: y, 2 doubles) + record write; backward: record read + outputs written
    out["bytes_per_row_mean_resid"] = 8 * (d + 2 * R + sd + d)
    out["bytes_per_row_cov"] = 8 * (d + 2 * R + sd + sd * sd + d)
    out["d2h_bytes_cov"] = 8 * n * (sd + sd * sd + d)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
