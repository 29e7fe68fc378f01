#!/usr/bin/env python3
"""Device time of dmx_pairalign (NW distance + edit path) on a consensus-shaped workload: the
reads of one synthetic bin (dmx.synth.amplicon_bin, about 1,215 nt), each aligned as the query
against the longest read of its family as the target, which is what create_alignment does in
its first round for a fresh consensus.  Reported: the device time of pairalign and of its two
passes (the forward pass that writes the trace, the traceback), the device time of dmx_pairdist
(NW, no cap) on the same pairs as the yardstick, their ratio, the trace's size and the rate it
is written at, and dmx_pairalign_host (the project's full-matrix DP, NOT edlib) on 16 threads
over a sample.  Distances and the sample's paths are checked.  Medians of --reps calls after
--warmup.  Writes one JSON record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "nanopore-barcoding-orc_amd"))
from dmx import lib, synth  # noqa: E402

TRACE_BYTES = 18   # per word-step: Pv, Mv (16) + the word's last-row score (2)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--families", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=200)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    # one family per call, so that the family of every read is known
    reads, q, t = [], [], []
    per = a.reads // a.families
    for f in range(a.families):
        fam = [r.encode() for r in synth.amplicon_bin(per, 1, (1150, 1250), (0.03, 0.12), 0.0,
                                                      seed=90 + f)]
        base = len(reads)
        longest = base + int(np.argmax([len(r) for r in fam]))
        reads += fam
        q += [base + i for i in range(len(fam)) if base + i != longest]
        t += [longest] * (len(fam) - 1)
    q, t = np.array(q, dtype=np.uint32), np.array(t, dtype=np.uint32)
    ln = np.array([len(r) for r in reads], dtype=np.int64)
    blob = np.frombuffer(b"".join(reads), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
    p = lib.pack(blob, offs, ln.astype(np.uint32))
    wsteps = float((((ln[q] + 63) // 64) * ln[t]).sum())
    rec = {"tool": "bench_pairalign", "reads": len(reads), "families": a.families,
           "mean_len": float(ln.mean()), "pairs": int(len(q)),
           "cells": float((ln[q] * ln[t]).sum()), "word_steps": wsteps,
           "trace_bytes": wsteps * TRACE_BYTES}
    with lib.Context(a.device) as ctx:
        ctx.load(p)
        tot, fwd, tb, wall, pd = [], [], [], [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            dist, off, ops = ctx.pairalign(q, t)
            w = time.perf_counter() - t0
            st = ctx.pairalign_stats()
            dd = ctx.pairdist(q, t, lib.PD_NW)
            if i >= a.warmup:
                tot.append(ctx.pairalign_ms())
                fwd.append(st["forward"])
                tb.append(st["traceback"])
                wall.append(w * 1e3)
                pd.append(ctx.pairdist_ms())
        dev, dpd = float(np.median(tot)), float(np.median(pd))
        f_ms, t_ms = float(np.median(fwd)), float(np.median(tb))
        rec.update({"pairalign_device_ms_median": dev,
                    "pairalign_device_ms_all": [float(x) for x in tot],
                    "forward_ms_median": f_ms, "traceback_ms_median": t_ms,
                    "dominant_pass": "forward trace" if f_ms >= t_ms else "traceback",
                    "launches": st["launches"], "call_ms_median": float(np.median(wall)),
                    "pairdist_device_ms_median": dpd,
                    "pairalign_over_pairdist": dev / dpd,
                    "forward_over_pairdist": f_ms / dpd,
                    "pairs_per_s": len(q) / (dev * 1e-3),
                    "word_steps_per_s_forward": wsteps / (f_ms * 1e-3),
                    "trace_write_GB_per_s": wsteps * TRACE_BYTES / (f_ms * 1e-3) / 1e9,
                    "path_ops": int(off[-1]),
                    "traceback_ops_per_s": float(off[-1]) / (t_ms * 1e-3),
                    "distances_match_pairdist": bool((dist == dd).all())})
    k = min(a.cpu_pairs, len(q))
    pick = np.sort(np.random.default_rng(0).choice(len(q), k, replace=False))
    t0 = time.perf_counter()
    hd, hoff, hops = lib.pairalign_host(p, q[pick], t[pick], n_threads=16)
    cpu = time.perf_counter() - t0
    same = bool((hd == dist[pick]).all()) and all(
        np.array_equal(hops[hoff[x]:hoff[x + 1]], ops[off[i]:off[i + 1]])
        for x, i in enumerate(pick))
    rec.update({"cpu_comparator": "dmx_pairalign_host (the project's full-matrix DP and "
                                  "traceback, not edlib), 16 threads",
                "cpu_pairs": int(k), "cpu_pairs_per_s": k / cpu,
                "cpu_sample_matches_gpu": same})
    rec["speedup_vs_cpu_dp"] = rec["pairs_per_s"] / rec["cpu_pairs_per_s"]
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if same and rec["distances_match_pairdist"] else 1


if __name__ == "__main__":
    sys.exit(main())
