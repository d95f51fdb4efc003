#!/usr/bin/env python3
"""tools/head_phases.py LABEL file... -- the phases of the lag-path head's waves from SSDE_WAVE_CLOCK files of a build with
-DSSDE_HEAD_STAMPS (tools/build_variant.sh stamps k_iso_shared_cut.hip "-DSSDE_HEAD_STAMPS"; k_iso_shared_cut.hip packs the four
phase stamps of part p into component p of the record of the workgroup's fourth wave; entry = the kernel's first instruction, block here = the
argument block has arrived and the padding workgroups have left): per direction part, median and range over the
workgroups of every file, in us.  E.g.  SSDE_LIB=.../libssde_hip_stamps.so SSDE_WAVE_CLOCK=wc.txt python tools/bench_c2.py 10000"""
import sys
import numpy as np
label, files = sys.argv[1], sys.argv[2:]
ph = {p: [] for p in range(3)}
for fn in files:
    rec = {}
    for ln in open(fn):
        if ln.startswith("#"): continue
        f = ln.split()
        rec[int(f[0])] = [float(x) for x in f[1:]]
    for i, r in rec.items():
        if i % 4 != 3: continue
        for p in range(3):
            w = rec.get(i - 3 + p)
            if w is None or r[p] == 0: continue
            k = int(r[p]); f0 = k & 255; st = [((k >> 8) >> (11 * j)) & 2047 for j in range(4)]
            tot = w[1] - w[0]
            ph[p].append([f0, st[0] - f0, st[1] - st[0], st[2] - st[1], st[3] - st[2], tot - st[3], tot, w[3]])
names = ["entry->block here", "block->first row", "table rows", "stationary rows", "wait at barrier", "barrier->end", "whole wave"]
for p in range(3):
    a = np.array(ph[p])
    if a.size == 0: continue
    print(f"{label} part {p}: {len(a)} waves, rows {int(a[:,7].min())}-{int(a[:,7].max())}")
    for j, n in enumerate(names):
        c = a[:, j] / 100.0
        print(f"    {n:18s} median {np.median(c):6.2f}  min {c.min():6.2f}  max {c.max():6.2f} us")
