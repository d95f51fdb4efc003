"""Times ssde_par_bands at --rows rows, four parameters -- two with --cols columns (an intercept and uniform
columns), two with the intercept alone --, --draws posterior draws, level 0.95, the blocks and the outputs in HBM: the call with the
pointwise outputs alone and with the simultaneous ones, next to the same numbers from torch on the same device -- per chunk of rows a
matmul that builds the chunk's rows x draws matrix, kthvalue for the four order statistics, and for the simultaneous band a second
matmul, |dev / se| and a maximum over the chunk.  Whole-call wall times, best of --reps; the result line is printed and appended to
--out (profiles/bands_bench.txt).  The torch route runs on --torch-rows rows (the first ones) and its time is reported for those
rows, not scaled.  Kernel times come from a run of its own under rocprofv3, whose kernel statistics --kernel-stats then adds to the
same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o bands -- python tools/bench_bands.py --no-torch --reps 1
    python tools/bench_bands.py --kernel-stats OUT/.../bands_kernel_stats.csv

(bands_rows_kernel is pass 1, bands_dev_kernel pass 2, bands_max_kernel its reduction, bands_sim_kernel pass 3)."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from smoothsde_amd import capi  # noqa: E402


def kernel_rows(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"bands_\w+(<\d+>)?", r.get("Name", ""))
            if m:
                rows.append(f"{m.group(0)}: calls {r.get('Calls')}, total {float(r.get('TotalDurationNs', 0)) / 1e6:.3f} ms, "
                            f"average {float(r.get('AverageNs', 0)) / 1e6:.3f} ms")
    return rows


def torch_bands(torch, Xs, coeff, offs, links, level, z, simultaneous, chunk):
    """the pointwise bands (and crit) of the rows of Xs by matmul + kthvalue, chunk rows at a time; returns (low, upp, crit)"""
    n, n_post = Xs[0].shape[0], coeff.shape[0] - 1
    alpha = (1.0 - level) / 2.0
    q = len(Xs)
    low = torch.empty((n, q), dtype=torch.float64, device=coeff.device)
    upp = torch.empty_like(low)
    md = torch.zeros((q, n_post), dtype=torch.float64, device=coeff.device)

    def quant(lp, p):
        h = (n_post - 1) * p
        lo = int(np.floor(h))
        hi = min(lo + 1, n_post - 1)
        a, b = lp.kthvalue(lo + 1, dim=1).values, lp.kthvalue(hi + 1, dim=1).values
        return a, b, h - lo

    for j in range(q):
        C = coeff[:, offs[j]:offs[j + 1]]
        g = torch.exp if links[j] else (lambda v: v)
        for r0 in range(0, n, chunk):
            X = Xs[j][r0:r0 + chunk]
            lp = X @ C[1:].T
            a, b, f = quant(lp, alpha)
            low[r0:r0 + chunk, j] = g(a) + f * (g(b) - g(a))
            a2, b2, f2 = quant(lp, 1.0 - alpha)
            upp[r0:r0 + chunk, j] = g(a2) + f2 * (g(b2) - g(a2))
            if simultaneous:
                se = (X @ C[0] - (a + f * (b - a))) / z
                dev = (X @ (C[1:] - C[0]).T / se[:, None]).abs_()
                md[j] = torch.maximum(md[j], torch.nan_to_num(dev, nan=0.0).amax(dim=0))
    crit = torch.quantile(md, level, dim=1) if simultaneous else None
    return low, upp, crit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=10)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--level", type=float, default=0.95)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=1_000_000)
    ap.add_argument("--torch-chunk", type=int, default=100_000)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bands_bench.txt"))
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv: append its kernel times to --out and stop")
    a = ap.parse_args()
    if a.kernel_stats:
        lines = ["Kernel times (rocprofv3 --kernel-trace --stats):"] + kernel_rows(a.kernel_stats)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    n, K = a.rows, a.cols

    def block():
        X = torch.rand((K, n), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
        X[0] = 1.0
        return X.t()                                                  # (n, K) column-major: the call takes it without a copy

    X_fe = [block(), None, block(), None]
    X_re = [None] * 4
    links = [1, 0, 1, 1]
    rng = np.random.default_rng(2)
    n_coef = 2 * K + 2
    chat = rng.uniform(-0.6, 0.6, n_coef)
    coeff = np.vstack([chat, chat + 0.25 * rng.standard_normal((a.draws, n_coef))])
    z = statistics.NormalDist().inv_cdf((1.0 + a.level) / 2.0)

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
    kw = dict(level=a.level, resp=True, device_out=True)
    ms_pw = best(lambda: got.__setitem__("pw", capi.par_bands(X_fe, X_re, links, coeff, simultaneous=False, **kw)), a.reps)
    ms_sim = best(lambda: got.__setitem__("sim", capi.par_bands(X_fe, X_re, links, coeff, simultaneous=True, **kw)), a.reps)
    same = bool(torch.equal(got["pw"]["pw_low"], got["sim"]["pw_low"]))
    out = {"rows": n, "cols": K, "n_par": 4, "draws": a.draws, "level": a.level, "ms_pointwise": ms_pw, "ms_with_simultaneous": ms_sim,
           "pointwise_alone_bitwise": same, "crit": [float(v) for v in got["sim"]["crit"]],
           "all_finite": bool(torch.isfinite(got["sim"]["sim_upp"]).all())}
    if not a.no_torch:
        m = min(a.torch_rows, n)
        ones = torch.ones((m, 1), dtype=torch.float64, device=dev)
        Xs = [ones if b is None else b[:m] for b in X_fe]
        ct = torch.as_tensor(coeff, device=dev)
        offs = [0, K, K + 1, 2 * K + 1, 2 * K + 2]
        res = {}
        out["torch_rows"] = m
        out["ms_torch_pointwise"] = best(lambda: res.__setitem__("pw", torch_bands(torch, Xs, ct, offs, links, a.level, z, False, a.torch_chunk)), a.reps)
        out["ms_torch_with_simultaneous"] = best(lambda: res.__setitem__("sim", torch_bands(torch, Xs, ct, offs, links, a.level, z, True, a.torch_chunk)), a.reps)
        low = res["pw"][0]
        ref = got["pw"]["pw_low"][:m]
        out["pw_low_gap_to_torch"] = float(((low - ref).abs() / (1.0 + ref.abs())).max())
    line = json.dumps(out)
    print(line)
    with open(a.out, "a") as f:
        f.write(f"tools/bench_bands.py --rows {n} --cols {K} --draws {a.draws} --level {a.level} (best of {a.reps}; whole-call wall times, ms):\n{line}\n")


if __name__ == "__main__":
    main()
