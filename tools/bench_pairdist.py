#!/usr/bin/env python3
"""Throughput of dmx_pairdist on the similarity pass's own shape: one group of 1000 reads of
about 1200 nt (dmx.synth.amplicon_bin: four amplicon families, 10 % reverse-complemented), every
pair the 5 % rule keeps, forward NW.  Device time is dmx_pairdist_ms (HIP events around the
kernels), the median of --reps calls after --warmup.  Reports pairs/s, cell updates/s (query
length x target length per pair), word-steps/s (64-row words x target columns) and that as a
fraction of a VALU ceiling: --valu-gops 64-bit-lane integer operations per second (measured
peak, profiles/r2_valu_ceiling.json when present) over the kernel's operations per word-step.
The CPU comparator is dmx_pairdist_host on 16 threads over a sample of the pairs: the project's
own full-matrix DP, NOT edlib.  Writes one JSON record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "nanopore-barcoding-orc_amd"))
from dmx import lib, sorter, synth  # noqa: E402

OPS_PER_WORD_STEP = 40   # 32-bit VALU instructions of one column step of one word (estimate
                         # from the kernel's source: 17 64-bit logic / add / shift pairs + selects)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--families", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=2000)
    ap.add_argument("--valu-gops", type=float, default=0.0,
                    help="measured VALU peak in 1e9 32-bit lane-ops/s (0: fraction not reported)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reads = [r.encode() for r in synth.amplicon_bin(a.reads, a.families, (1150, 1250),
                                                    (0.03, 0.12), 0.1, seed=9)]
    ln = np.array([len(r) for r in reads], dtype=np.int64)
    q, t = sorter.pairs([np.arange(len(reads))], ln)
    blob = np.frombuffer(b"".join(reads), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
    p = lib.pack(blob, offs, ln.astype(np.uint32))
    cells = float((ln[q] * ln[t]).sum())
    wsteps = float((((ln[q] + 63) // 64) * ln[t]).sum())
    rec = {"tool": "bench_pairdist", "reads": len(reads), "families": a.families,
           "mean_len": float(ln.mean()), "pairs": int(len(q)), "cells": cells,
           "word_steps": wsteps, "group_sizes": lib.pairdist_group_sizes()}
    with lib.Context(a.device) as ctx:
        ctx.load(p)
        ms, wall = [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            d = ctx.pairdist(q, t, lib.PD_NW)
            w = time.perf_counter() - t0
            if i >= a.warmup:
                ms.append(ctx.pairdist_ms())
                wall.append(w * 1e3)
        dev = float(np.median(ms))
        rec.update({"device_ms_median": dev, "device_ms_all": [float(x) for x in ms],
                    "call_ms_median": float(np.median(wall)),
                    "pairs_per_s": len(q) / (dev * 1e-3), "cells_per_s": cells / (dev * 1e-3),
                    "word_steps_per_s": wsteps / (dev * 1e-3),
                    "ops_per_word_step_estimate": OPS_PER_WORD_STEP})
        if a.valu_gops > 0:
            rec["valu_peak_gops"] = a.valu_gops
            rec["fraction_of_valu_peak"] = (wsteps / (dev * 1e-3)) * OPS_PER_WORD_STEP / \
                (a.valu_gops * 1e9)
    k = min(a.cpu_pairs, len(q))
    pick = np.random.default_rng(0).choice(len(q), k, replace=False)
    t0 = time.perf_counter()
    h = lib.pairdist_host(p, q[pick], t[pick], lib.PD_NW, n_threads=16)
    cpu = time.perf_counter() - t0
    rec.update({"cpu_comparator": "dmx_pairdist_host (the project's full-matrix DP, not edlib), "
                                  "16 threads", "cpu_pairs": int(k),
                "cpu_pairs_per_s": k / cpu, "cpu_cells_per_s": float((ln[q[pick]] * ln[t[pick]]).sum()) / cpu,
                "cpu_sample_matches_gpu": bool((h == d[pick]).all())})
    rec["speedup_vs_cpu_dp"] = rec["pairs_per_s"] / rec["cpu_pairs_per_s"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
