"""Times ssde_smooth_draws on a CTCRW d = 2 batch: wall time of a call that leaves its draws in HBM
(SSDE_DRAWS_DEVICE_OUT), per draw, and the bytes the layout moves.  Kernel times come from a run of its own under rocprofv3:

    rocprofv3 --kernel-trace --stats -d OUT -o draws -- python tools/bench_draws.py --tracks 10000 --rows 1000 --draws 32

(dense_kernel<..., 0, 2> is the forward record pass, smooth_draws_kernel the backward sampling pass; tools/bench_smooth.py gives the
smoother's backward pass, smooth_back_kernel, on the same batch)."""
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
    a = ap.parse_args()
    import torch
    ID, times, obs = capi.simulate_device("CTCRW", a.tracks, a.rows, 2, tau=2.0, nu=1.0, sigma_obs=0.1, seed=3)
    pb = capi.Problem("CTCRW", ID.cpu().numpy(), times.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy()))
    del ID, times, obs
    torch.cuda.empty_cache()
    par = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    eng = capi.Engine(pb)
    # R mirrors SmoothRec<M_CTCRW, 2>::R (ssde_smooth.hpp), DRAW_CH the draws per wave (ssde_device.hpp): change them together
    n, sd, d, R, DRAW_CH = pb.n, 4, 2, 31, 4
    buf = torch.empty((a.draws, sd, n), dtype=torch.float64, device="cuda:0")
    eng.smooth_draws(par, a.draws, seed=1, out=buf)                  # warm-up (allocations, code objects)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        eng.smooth_draws(par, a.draws, seed=1, out=buf)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    state = int(n - a.tracks)
    finite = int(torch.isfinite(buf[0, 0]).sum().item())
    out = {"tracks": a.tracks, "rows_per_track": a.rows, "n": n, "draws": a.draws, "draws_per_wave": DRAW_CH,
           "ms_call": 1e3 * min(ts), "ms_call_per_draw": 1e3 * min(ts) / a.draws,
           "record_bytes_per_row": 8 * R,
           # forward: tiles read (dt-less regular grid: y, 2 doubles) + record write; backward: the records once per chunk of 4 draws,
           # the draws written
           "bytes_per_row": 8 * (d + R + R * ((a.draws + DRAW_CH - 1) // DRAW_CH) + sd * a.draws),
           "hbm_out_bytes": 8 * n * sd * a.draws,
           "state_rows_finite": finite == state}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
