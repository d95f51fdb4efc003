"""Where the lag-statistics path starts to pay, per model: bench.py on the same batch with SSDE_LAGSTATS=0 (every
row streamed) and =2 (the statistics forced), alternating, `--reps` repetitions per shape -- the procedure behind
profiles/r07_c_lagstats_crossover.txt, for any of CTCRW / OU_SSM / BM_SSM.  Every run is a fresh child process.  One line per run:

    model tracks rows mode rep ms_per_step median_of_steps bulk_rows_past_256

then, per model and shape, whether the path was faster in every pairing, what building the statistics cost ssde_create
(lagstat_create_ms, and the rows an evaluation then took from them -- a probe of its own, outside the timing), and the model's
threshold: the smallest measured size at which the path's ms_per_step is below the streamed one in every repetition (never below
--floor, the rule's floor).

    python tools/lagstats_crossover.py --models OU_SSM BM_SSM --out profiles/NAME.txt
    python tools/lagstats_crossover.py --models OU_SSM --shapes 10000x10000 --reps 3        # the headline shape only
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAG_A = 256
DEFAULT_SHAPES = ["10000x400", "10000x700", "10000x1000", "10000x1500", "10000x2000", "10000x3000"]     # 1.4e6 .. 2.7e7 bulk rows

PROBE = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from smoothsde_amd import capi
model, M, T, d = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), 2
ID, times, obs = capi.simulate_device(model, M, T, d, mu=0.0, tau=2.0, nu=1.0, kappa=1.0, sigma=1.0, sigma_obs=0.1, seed=1, track0=0,
                                      device=torch.device("cuda:0"))
fixed = np.zeros(1 + capi.n_sde_par(model, d), dtype=np.uint8); fixed[1:1 + d] = 1
eng = capi.Engine(capi.Problem.from_torch(model, ID, times, obs, par_fixed=fixed))
th = np.zeros(eng.n_par_full); th[0] = np.log(0.1); th[1 + d] = np.log(2.0)
eng.eval(th)
inf = eng.info()
print(json.dumps({k: inf[k] for k in ("lagstat_rows", "lagstat_create_ms", "main_kernel_rows", "n_steps", "kernel_id", "window_check")}))
"""


def child(cmd, env, timeout):
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
    for ln in reversed(p.stdout.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise SystemExit("no JSON line from: " + " ".join(cmd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["OU_SSM", "BM_SSM"])
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, help="TRACKSxROWS")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--floor", type=float, default=4.4e6, help="bulk rows below which no threshold is set")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None

    def emit(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()

    emit("# bench.py --gpus 1 --steps %d --warmup %d --model MODEL --tracks M --rows T, SSDE_LAGSTATS=0 (streamed) / =2 (lag statistics forced),"
         % (args.steps, args.warmup))
    emit("# alternating, %d repetitions (a, b, ..) per shape; d = 2, mu fixed" % args.reps)
    emit("# model tracks rows mode rep ms_per_step median_of_steps bulk_rows_past_%d" % LAG_A)
    summary = []
    for model in args.models:
        wins = []
        for shape in args.shapes:
            M, T = (int(v) for v in shape.lower().split("x"))
            bulk = M * max(0, T - 1 - LAG_A)
            res = {0: [], 2: []}
            for rep in range(args.reps):
                for mode in (0, 2):
                    env = dict(os.environ, SSDE_LAGSTATS=str(mode))
                    line = child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup),
                                  "--model", model, "--tracks", str(M), "--rows", str(T)], env, args.timeout)
                    ms, med = line["ms_per_step"], line["extra"]["ms_per_step_median"]
                    res[mode].append(ms)
                    emit("%s %d %d SSDE_LAGSTATS=%d %s %.5f %.5f %.2e" % (model, M, T, mode, chr(ord("a") + rep), ms, med, bulk))
            probe = child([sys.executable, "-c", PROBE, ROOT, model, str(M), str(T)], dict(os.environ, SSDE_LAGSTATS="2"), args.timeout)
            every = max(res[2]) < min(res[0])
            wins.append((bulk, every))
            summary.append("# %s %.2e bulk rows (%d x %d): streamed %.4f-%.4f, path %.4f-%.4f ms_per_step: path %s; lagstat_create_ms %.1f, "
                           "lagstat_rows %d of %d steps, window_check %.1e"
                           % (model, bulk, M, T, min(res[0]), max(res[0]), min(res[2]), max(res[2]),
                              "faster in every pairing" if every else "NOT faster in every pairing", probe["lagstat_create_ms"], probe["lagstat_rows"],
                              probe["n_steps"], probe["window_check"]))
        ok = [b for b, e in sorted(wins) if e and b >= args.floor]
        # (the smallest measured size from which on the path won at every larger measured size too)
        thr = None
        for b, e in sorted(wins, reverse=True):
            if not e:
                break
            if b >= args.floor:
                thr = b
        summary.append("# %s threshold: %s" % (model, ("%.2e bulk rows" % thr) if thr is not None and ok else "none of the measured sizes"))
    for s in summary:
        emit(s)
    if out:
        out.close()


if __name__ == "__main__":
    main()
