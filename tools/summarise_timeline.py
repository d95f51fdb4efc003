#!/usr/bin/env python3
"""tools/summarise_timeline.py DIR STEM [WARMUP] -- the timeline of one lag-path evaluation from a rocprofv3 run
(--kernel-trace --memory-copy-trace --hip-trace --output-format csv -d DIR -o STEM, bench.py after `--`).

An evaluation = the commands around one iso_shared_kernel (or iso_shared_wg_kernel) dispatch: host-to-device copies and the forms' launch before it (where
the trace shows them), the finalize launch and device-to-host copies after it.  Prints, as medians over the evaluations that have
the most frequent shape (the timed steps; the first WARMUP of them dropped, default 5 = bench.py's): each command's duration, each
gap, the span from the first command's start to the last one's end, and the host side from the HIP API trace -- the evaluation's
first HIP call (its gain-table copy) to its first launch, first to last launch, and the blocking read-back call."""
import csv
import glob
import os
import re
import statistics
import sys

d, stem = sys.argv[1], sys.argv[2]
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5


def rows(kind):
    f = glob.glob(os.path.join(d, "**", f"{stem}_{kind}.csv"), recursive=True)
    if not f:
        return []
    with open(f[0]) as fh:
        return list(csv.DictReader(fh))


ev = []
for r in rows("kernel_trace"):
    m = re.search(r"(\w+_kernel)", r["Kernel_Name"])
    if "ssde::" in r["Kernel_Name"] and m:
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(1)))
for r in rows("memory_copy_trace"):
    dirn = r.get("Direction", "")
    n = "copy H2D" if "HOST_TO_DEVICE" in dirn else "copy D2H" if "DEVICE_TO_HOST" in dirn else "copy " + dirn
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n))
ev.sort()
HEADS = ("iso_shared_kernel", "iso_shared_wg_kernel", "iso_shared_cut_kernel")      # (the second: one workgroup per track group, the third: its waves the direction parts of window 0)
heads = [i for i, e in enumerate(ev) if e[2] in HEADS]
if not heads:
    sys.exit("no iso_shared_kernel / iso_shared_wg_kernel / iso_shared_cut_kernel dispatch in the trace")
NEAR = 200000       # ns: a command further than this from the head launch belongs to something else
evals = []
for a, b in zip(heads, heads[1:] + [len(ev)]):
    lo = a
    while lo > 0 and ev[lo - 1][2] in ("copy H2D", "lag_forms_kernel") and ev[a][0] - ev[lo - 1][0] < NEAR:
        lo -= 1
    hi = a
    while hi + 1 < b and ev[hi + 1][2] in ("iso_finalize_kernel", "copy D2H") and ev[hi + 1][0] - ev[a][1] < NEAR:
        hi += 1
    evals.append(ev[lo:hi + 1])
shape = statistics.mode(tuple(e[2] for e in x) for x in evals)
evals = [x for x in evals if tuple(e[2] for e in x) == shape][warm:]


def med(v):
    return statistics.median(v) / 1000.0 if v else float("nan")


print(f"# {len(evals)} evaluations of the shape {' -> '.join(shape)}; microseconds, medians")
for k, name in enumerate(shape):
    print(f"{name:24s} duration {med([x[k][1] - x[k][0] for x in evals]):8.2f}")
    if k + 1 < len(shape):
        print(f"{'  gap to ' + shape[k + 1]:24s}          {med([x[k + 1][0] - x[k][1] for x in evals]):8.2f}")
print(f"{'first start -> last end':24s}          {med([x[-1][1] - x[0][0] for x in evals]):8.2f}")
print(f"{'kernels, summed':24s}          {med([sum(e[1] - e[0] for e in x if 'copy' not in e[2]) for x in evals]):8.2f}")
print(f"{'evaluation to evaluation':24s}          {med([b[0][0] - a[0][0] for a, b in zip(evals, evals[1:])]):8.2f}")
# host: the HIP calls between one blocking read-back (hipMemcpy) and the next are one synchronous evaluation
calls = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Function"]) for r in rows("hip_api_trace")
               if r["Function"].startswith("hipMemcpy") or "LaunchKernel" in r["Function"])
sync = [i for i, c in enumerate(calls) if c[2] == "hipMemcpy"]
n_launch = sum(1 for n in shape if "copy" not in n)
host = []
for a, b in zip(sync, sync[1:]):
    seg = calls[a + 1:b + 1]
    launches = [c for c in seg if "Launch" in c[2]]
    if len(launches) != n_launch or not seg[0][2].startswith("hipMemcpyAsync"):
        continue
    host.append({"first HIP call (gain-table copy) -> first launch": launches[0][0] - seg[0][0],
                 "first launch -> last launch": launches[-1][0] - launches[0][0],
                 "last launch returned -> read-back call": seg[-1][0] - launches[-1][1],
                 "read-back call (blocks until the GPU is done)": seg[-1][1] - seg[-1][0]})
host = host[warm:]
for k in (host[0] if host else ()):
    print(f"host {k:48s} {med([h[k] for h in host]):8.2f}   ({len(host)} evaluations)")
if not host:
    print("host: no evaluation ends in a blocking hipMemcpy in this trace (a published result has no read-back call): not measured")
