#!/usr/bin/env python3
"""The consensus comparison of comp_consensus_groups / compare_consensus (iden_consensus,
amplicon_sorter.py:1140-1159) on its own shape: --consensuses synthetic consensuses of about
1,200 nt in --families families (dmx.synth.amplicon_bin, copies mutated 1-6 %), every pair
y < z the 8 % length rule keeps, HW on both strands, a hit where the larger identity is >= 0.60.
Three ways, the same hits:
  rowhits   dmx_rowhits: the consensuses uploaded as rows with the call, both strands, the
            decision and the compaction on the device; the resident bin stays loaded;
  resident  the only way without it: the consensuses packed as reads and loaded over the bin
            (dmx_pack, dmx_load), dmx_pairdist(HW) twice (forward, DMX_PD_RC), the decision in
            numpy, and the bin's reads packed and loaded again afterwards;
  host      dmx_rowhits_host on 16 threads over --cpu-pairs of the pairs (the project's own
            full-matrix DP, NOT edlib).
Device time is dmx_rowhits_ms / dmx_pairdist_ms (HIP events around the kernels), call time the
wall clock of everything a cycle has to do.  Medians of --reps after --warmup.  Writes one JSON
record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "nanopore-barcoding-orc_amd"))
from dmx import lib, sorter, synth  # noqa: E402


def pack(seqs):
    ln = np.array([len(s) for s in seqs], dtype=np.int64)
    blob = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
    return lib.pack(blob, offs, ln.astype(np.uint32))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--consensuses", type=int, default=2000)
    ap.add_argument("--families", type=int, default=50)
    ap.add_argument("--bin-reads", type=int, default=10000,
                    help="reads of the bin that is resident meanwhile (the second route reloads it)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-pairs", type=int, default=4000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    per = (a.consensuses + a.families - 1) // a.families
    cons = []
    for f in range(a.families):
        cons += [r.encode() for r in synth.amplicon_bin(per, 1, (1150, 1250), (0.01, 0.06), 0.0,
                                                        seed=700 + f)]
    cons = cons[:a.consensuses]
    rng = np.random.default_rng(2)
    cons = [sorter.revcomp(c) if rng.random() < 0.3 else c for c in cons]   # both strands occur
    bin_reads = [r.encode() for r in synth.amplicon_bin(a.bin_reads, 20, (1150, 1250),
                                                        (0.03, 0.12), 0.0, seed=699)]
    ln = np.array([len(c) for c in cons], dtype=np.int64)
    y, z = np.triu_indices(len(cons), 1)
    la, lb = ln[y].astype(np.float64), ln[z].astype(np.float64)
    ldc = 8.0 / 100 + 1
    keep = ~((la * ldc < lb) | (lb * ldc < la))
    dropped = int(keep.size - keep.sum())
    y, z = y[keep], z[keep]
    swap = ln[y] > ln[z]
    q, t = np.where(swap, z, y).astype(np.uint32), np.where(swap, y, z).astype(np.uint32)
    lt = ln[t]
    caps = {int(L): sorter.identity_cap(int(L), 0.60) for L in np.unique(lt)}
    cap = np.array([caps[int(L)] for L in lt], dtype=np.int32)
    cells = 2.0 * float((ln[q] * lt).sum())
    rows = [lib.mask_row(c) for c in cons]
    rec = {"tool": "bench_rowhits", "consensuses": len(cons), "families": a.families,
           "mean_consensus_len": float(ln.mean()), "pairs": int(len(q)),
           "pairs_dropped_by_8_percent_rule": dropped, "cells_both_strands": cells,
           "bin_reads": len(bin_reads), "session": "a single session"}
    p_bin = pack(bin_reads)
    rcf = np.full(len(q), lib.PD_RC, dtype=np.uint8)
    with lib.Context(a.device) as ctx:
        ctx.load(p_bin)
        dev, wall = [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            hits = ctx.rowhits(rows, q, t, cap, lib.PD_HW)
            w = time.perf_counter() - t0
            if i >= a.warmup:
                dev.append(ctx.rowhits_ms())
                wall.append(w * 1e3)
        dev2, wall2, prep2 = [], [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            ctx.load(pack(cons))
            t1 = time.perf_counter()
            df = ctx.pairdist(q, t, lib.PD_HW, caps=np.maximum(cap, 0).astype(np.uint32))
            ms = ctx.pairdist_ms()
            dr = ctx.pairdist(q, t, lib.PD_HW, flags=rcf, caps=np.maximum(cap, 0).astype(np.uint32))
            ms += ctx.pairdist_ms()
            d = np.minimum(df, dr)
            k = np.flatnonzero((cap >= 0) & (d.astype(np.int64) <= cap))
            hits2 = (k.astype(np.uint32), d[k], (dr < df)[k].astype(np.uint8))
            t2 = time.perf_counter()
            ctx.load(pack(bin_reads))
            w = time.perf_counter() - t0
            if i >= a.warmup:
                dev2.append(ms)
                wall2.append(w * 1e3)
                prep2.append((t1 - t0 + time.perf_counter() - t2) * 1e3)
    same = all(np.array_equal(x, yy) for x, yy in zip(hits, hits2))
    md, mw = float(np.median(dev)), float(np.median(wall))
    md2, mw2 = float(np.median(dev2)), float(np.median(wall2))
    rec["hits"] = int(len(hits[0]))
    rec["reverse_hits"] = int(hits[2].sum())
    rec["rowhits"] = {"device_ms_median": md, "device_ms_all": [float(x) for x in dev],
                      "call_ms_median": mw, "call_ms_all": [float(x) for x in wall],
                      "pairs_per_s_device": len(q) / (md * 1e-3),
                      "cells_per_s_device": cells / (md * 1e-3),
                      "pairs_per_s_call": len(q) / (mw * 1e-3)}
    rec["resident_pairdist"] = {"device_ms_median": md2, "device_ms_all": [float(x) for x in dev2],
                                "pack_and_load_both_ways_ms_median": float(np.median(prep2)),
                                "call_ms_median": mw2, "call_ms_all": [float(x) for x in wall2],
                                "pairs_per_s_device": len(q) / (md2 * 1e-3),
                                "pairs_per_s_call": len(q) / (mw2 * 1e-3)}
    rec["rowhits_equals_resident_pairdist"] = bool(same)
    rec["call_speedup_vs_resident"] = mw2 / mw
    rec["device_time_ratio_rowhits_over_pairdist"] = md / md2
    k = min(a.cpu_pairs, len(q))
    pick = np.sort(np.random.default_rng(1).choice(len(q), k, replace=False))
    t0 = time.perf_counter()
    host = lib.rowhits_host(rows, q[pick], t[pick], cap[pick], lib.PD_HW, n_threads=16)
    cpu = time.perf_counter() - t0
    sel = np.isin(hits[0], pick)
    host_same = (np.array_equal(pick[host[0]], hits[0][sel]) and
                 np.array_equal(host[1], hits[1][sel]) and np.array_equal(host[2], hits[2][sel]))
    rec["host"] = {"comparator": "dmx_rowhits_host (the project's full-matrix DP, not edlib), "
                                 "16 threads", "pairs": int(k), "pairs_per_s": k / cpu,
                   "matches_gpu": bool(host_same)}
    rec["call_speedup_vs_host_dp"] = rec["rowhits"]["pairs_per_s_call"] / rec["host"]["pairs_per_s"]
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if same and host_same else 1


if __name__ == "__main__":
    sys.exit(main())
