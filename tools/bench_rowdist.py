#!/usr/bin/env python3
"""One pass of the assignment loop (process_consensuslist, amplicon_sorter.py:1628-1691) on its
own shape: --reads synthetic reads of about 1,200 nt (dmx.synth.amplicon_bin, one family per
consensus, copies mutated 3-12 %) against --consensuses consensuses (the families themselves),
every pair the 5 % rule keeps, forward NW.  Three ways, the same distances:
  rowdist   dmx_rowdist on the resident batch, the consensuses uploaded as rows with the call;
  appended  the only way without it: the consensuses appended to the reads, the whole bin
            packed and loaded again (dmx_pack, dmx_load), then dmx_pairdist;
  host      dmx_rowdist_host on 16 threads over --cpu-pairs of the pairs (the project's own
            full-matrix DP, NOT edlib).
Device time is dmx_rowdist_ms / dmx_pairdist_ms (HIP events around the kernels), call time the
wall clock of everything a pass has to do (for `appended`: pack + load + pairdist).  Medians of
--reps after --warmup.  Writes one JSON record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "nanopore-barcoding-orc_amd"))
from dmx import lib, synth  # noqa: E402


def pack(seqs):
    ln = np.array([len(s) for s in seqs], dtype=np.int64)
    blob = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
    return lib.pack(blob, offs, ln.astype(np.uint32))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--consensuses", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-pairs", type=int, default=4000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    per = (a.reads + a.consensuses - 1) // a.consensuses
    reads, cons = [], []
    for f in range(a.consensuses):
        reads += [r.encode() for r in synth.amplicon_bin(per, 1, (1150, 1250), (0.03, 0.12), 0.0,
                                                         seed=400 + f)]
        # the same seed and no mutation: the family's own sequence
        cons.append(synth.amplicon_bin(1, 1, (1150, 1250), (0.0, 0.0), 0.0, seed=400 + f)[0]
                    .encode())
    reads = reads[:a.reads]
    ln = np.array([len(s) for s in reads], dtype=np.float64)
    lc = np.array([len(s) for s in cons], dtype=np.float64)
    keep = ~((ln[:, None] * 1.05 < lc[None, :]) | (lc[None, :] * 1.05 < ln[:, None]))
    q, g = np.nonzero(keep)
    q, g = q.astype(np.uint32), g.astype(np.uint32)
    cells = float((ln[q] * lc[g]).sum())
    rows = [lib.mask_row(s) for s in cons]
    rec = {"tool": "bench_rowdist", "reads": len(reads), "consensuses": len(cons),
           "mean_read_len": float(ln.mean()), "mean_consensus_len": float(lc.mean()),
           "pairs": int(len(q)), "pairs_dropped_by_5_percent_rule": int(keep.size - len(q)),
           "cells": cells, "session": "a single session"}
    p = pack(reads)
    with lib.Context(a.device) as ctx:
        dev, wall = [], []
        ctx.load(p)
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            d_row = ctx.rowdist(rows, q, g)
            w = time.perf_counter() - t0
            if i >= a.warmup:
                dev.append(ctx.rowdist_ms())
                wall.append(w * 1e3)
        dev2, wall2, prep2 = [], [], []
        t = (g + len(reads)).astype(np.uint32)
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            ctx.load(pack(reads + cons))
            t1 = time.perf_counter()
            d_app = ctx.pairdist(q, t, lib.PD_NW)
            w = time.perf_counter() - t0
            if i >= a.warmup:
                dev2.append(ctx.pairdist_ms())
                wall2.append(w * 1e3)
                prep2.append((t1 - t0) * 1e3)
    same = bool(np.array_equal(d_row, d_app))
    md, mw = float(np.median(dev)), float(np.median(wall))
    md2, mw2 = float(np.median(dev2)), float(np.median(wall2))
    rec["rowdist"] = {"device_ms_median": md, "device_ms_all": [float(x) for x in dev],
                      "call_ms_median": mw, "call_ms_all": [float(x) for x in wall],
                      "pairs_per_s_device": len(q) / (md * 1e-3),
                      "cells_per_s_device": cells / (md * 1e-3),
                      "pairs_per_s_call": len(q) / (mw * 1e-3)}
    rec["appended_pairdist"] = {"device_ms_median": md2, "device_ms_all": [float(x) for x in dev2],
                                "pack_and_load_ms_median": float(np.median(prep2)),
                                "call_ms_median": mw2, "call_ms_all": [float(x) for x in wall2],
                                "pairs_per_s_device": len(q) / (md2 * 1e-3),
                                "pairs_per_s_call": len(q) / (mw2 * 1e-3)}
    rec["rowdist_equals_appended_pairdist"] = same
    rec["call_speedup_vs_appended"] = mw2 / mw
    rec["device_time_ratio_rowdist_over_pairdist"] = md / md2
    k = min(a.cpu_pairs, len(q))
    pick = np.random.default_rng(1).choice(len(q), k, replace=False)
    t0 = time.perf_counter()
    host = lib.rowdist_host(p, rows, q[pick], g[pick], n_threads=16)
    cpu = time.perf_counter() - t0
    host_same = bool(np.array_equal(host, d_row[pick]))
    rec["host"] = {"comparator": "dmx_rowdist_host (the project's full-matrix DP, not edlib), "
                                 "16 threads", "pairs": int(k), "pairs_per_s": k / cpu,
                   "matches_gpu": host_same}
    rec["call_speedup_vs_host_dp"] = rec["rowdist"]["pairs_per_s_call"] / rec["host"]["pairs_per_s"]
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if same and host_same else 1


if __name__ == "__main__":
    sys.exit(main())
