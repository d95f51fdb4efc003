"""Times ssde_simulate_rows, one --case per run, and appends the result line to --out (profiles/simrows_bench.txt):

    long    one track x 10^4 rows x 1000 replicates, CTCRW, two columns, tau and nu on 9-column smooths, a coefficient row per
            replicate: the statistics alone, and with obs_rep written to HBM
    batch   10^4 tracks x 10^3 rows x 1 replicate, CTCRW, two columns, constant parameters, obs_rep in HBM -- beside ssde_simulate
            on the same batch on the same device; the ratio is the price of row-varying parameters and of forming the factors per
            row (reported, not tuned against)
    check   100 tracks x 10^3 rows x 100 replicates, check_post's ordinary shape (tau and nu smooth, statistics alone), with the
            bytes of design rows the lanes read per second -- every lane reads its row: rows x replicates x design columns x 8 B,
            of which rows x columns x 8 B are distinct --, and the numpy definition (tests/simrows_ref.py) on the CPU for a tenth
            of it (10 tracks)

Whole-call wall times in ms after one warm-up call: the best and the median of --reps."""
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
from smoothsde_amd.synth import bspline_basis  # noqa: E402


def problem(n_tracks, n_steps, n_rep, smooth, seed=1):
    """CTCRW, two columns: (row0, times, X_fe, X_re, link, coeff)"""
    rng = np.random.default_rng(seed)
    n = n_tracks * n_steps
    times = np.tile(np.cumsum(rng.uniform(0.5, 1.5, size=n_steps)), n_tracks)
    X_fe, X_re = [None] * 4, [None] * 4
    chat = [0.05, -0.03]
    for j in (2, 3):
        if smooth:
            X_re[j] = bspline_basis((np.sin(0.002 * (j + 1) * np.arange(n)) + 1) / 2, 9)
            chat += [0.3 if j == 2 else -0.2] + list(rng.uniform(-0.4, 0.4, 9))
        else:
            chat += [0.3 if j == 2 else -0.2]
    chat = np.asarray(chat)
    coeff = chat[None, :] + (0.05 * rng.standard_normal((n_rep, len(chat))) if n_rep > 1 else 0.0)
    return np.arange(n_tracks + 1, dtype=np.int64) * n_steps, times, X_fe, X_re, np.array([0, 0, 1, 1], dtype=np.uint8), coeff


def timed(fn, reps, sync):
    fn()                                                              # warm-up (allocations, code objects)
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"best": min(ts), "median": statistics.median(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("long", "batch", "check"), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the rows of a track (a quick look, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simrows_bench.txt"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    out = {"case": a.case}
    if a.case == "long":
        T, R = int(10_000 * a.scale), 1000
        row0, times, X_fe, X_re, link, coeff = problem(1, T, R, smooth=True)
        X_re = [None if b is None else torch.as_tensor(b, device=dev) for b in X_re]
        run = lambda want, dout: capi.simulate_rows("CTCRW", 2, row0, times, X_fe, X_re, link, coeff, sigma_obs=0.05, seed=1, n_rep=R,
                                                    thresholds=[0.5, 2.0], want=want, device_out=dout)
        out.update(tracks=1, rows=T, replicates=R, n_coef=int(coeff.shape[1]))
        out["ms_stats_only"] = timed(lambda: run(("stats",), False), a.reps, sync)
        out["ms_with_obs_in_hbm"] = timed(lambda: run(("obs", "stats"), True), a.reps, sync)
        out["obs_bytes"] = 8 * T * 2 * R
    elif a.case == "batch":
        M, T = 10_000, int(1000 * a.scale)
        row0, times, X_fe, X_re, link, coeff = problem(M, T, 1, smooth=False)
        dt = 1.0
        times = np.tile(dt * np.arange(1, T + 1), M)                    # ssde_simulate's regular grid
        got = {}
        out.update(tracks=M, rows=T, replicates=1)
        out["ms_simulate_rows"] = timed(lambda: got.__setitem__("rows", capi.simulate_rows(
            "CTCRW", 2, row0, times, X_fe, X_re, link, coeff, sigma_obs=0.05, seed=1, want=("obs",), device_out=True)["obs"]), a.reps, sync)
        out["ms_ssde_simulate"] = timed(lambda: got.__setitem__("sim", capi.simulate_device(
            "CTCRW", M, T, 2, mu=[0.05, -0.03], tau=float(np.exp(0.3)), nu=float(np.exp(-0.2)), sigma_obs=0.05, dt=dt, seed=1,
            want_id_times=False)[2]), a.reps, sync)
        out["ratio"] = out["ms_simulate_rows"]["best"] / out["ms_ssde_simulate"]["best"]
        out["gap_between_the_two"] = float((got["rows"][0] - got["sim"]).abs().max())
    else:
        M, T, R = 100, int(1000 * a.scale), 100
        row0, times, X_fe, X_re, link, coeff = problem(M, T, R, smooth=True)
        Xd = [None if b is None else torch.as_tensor(b, device=dev) for b in X_re]
        out.update(tracks=M, rows=T, replicates=R, n_coef=int(coeff.shape[1]))
        out["ms_stats_only"] = timed(lambda: capi.simulate_rows("CTCRW", 2, row0, times, X_fe, Xd, link, coeff, sigma_obs=0.05, seed=1,
                                                                 n_rep=R, thresholds=[0.5, 2.0], want=("stats",)), a.reps, sync)
        cols = 18
        s = out["ms_stats_only"]["best"] / 1e3
        out["design_GB_per_s_read_by_the_lanes"] = 8.0 * M * (T - 1) * cols * R / s / 1e9
        out["design_GB_per_s_distinct"] = 8.0 * M * (T - 1) * cols / s / 1e9
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from simrows_ref import simrows_ref
        m = M // 10
        rows = slice(0, m * T)
        t0 = time.perf_counter()
        simrows_ref("CTCRW", 2, row0[:m + 1], times[rows], X_fe, [None if b is None else b[rows] for b in X_re], link, coeff, sigma_obs=0.05,
                    seed=1, n_rep=R, thr=[0.5, 2.0])
        out["ms_numpy_definition_on_a_tenth"] = 1e3 * (time.perf_counter() - t0)
    line = json.dumps(out)
    print(line)
    with open(a.out, "a") as f:
        f.write(f"tools/bench_simrows.py --case {a.case} --reps {a.reps}" + (f" --scale {a.scale}" if a.scale != 1.0 else "")
                + f" (whole-call wall times, ms):\n{line}\n")


if __name__ == "__main__":
    main()
