#!/usr/bin/env python3
"""Device time of dmx_groupalign on the shape make_consensus feeds create_consensus
(amplicon_sorter.py:1227-1240): synthetic families (dmx.synth.amplicon_bin, about 1,200 nt) cut
into --groups groups of --per reads, cycle 1 only (the longest read of a group seeds it, the
others are aligned against the growing row in lock-step rounds).  Reported: rounds, launches,
the device time of the three passes (forward trace, traceback, merge) and which dominates,
alignments per second, the final row lengths, and, rerun in the same session, dmx_pairalign on
the same number of pairs of the same reads (every member against its group's seed read: the
ungapped first round, tools/bench_pairalign.py's procedure) for the per-alignment time next to
it.  The CPU comparator is dmx_groupalign_host (the project's sequential full-matrix DP, NOT
edlib) on 16 threads over --cpu-groups groups; its columns are checked against the GPU's.
Medians of --reps calls after --warmup.  Writes one JSON record.

--strands all / half stores every (every other) member reverse-complemented in the batch and
flags it (dmx_groupalign_strands), so the alignments are the same as with --strands none (the
unflagged entry point) and the difference is what reading a member backwards costs per pass.
--consensus-ab also times sorter.make_consensus on the groups with their seeds put back (a
random half of the reads turned round) against the host route it replaces: orient on the
resident batch, turn the reads on the host, pack and load again, sorter.consensus."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "nanopore-barcoding-orc_amd"))
from dmx import lib, synth  # noqa: E402


def consensus_ab(a, reads, groups, seed_idx, comp):
    """make_consensus on a mixed-strand bin against the route it replaces, both from the reads
    as Python bytes to the consensus strings, alternating, medians of --reps after --warmup."""
    from dmx import sorter
    rng = np.random.default_rng(7)
    k = min(a.consensus_ab, len(groups))
    full = [[seed_idx[g]] + groups[g] for g in range(k)]
    used = sorted({i for g in full for i in g})
    place = {i: n for n, i in enumerate(used)}
    bin_reads = [reads[i][::-1].translate(comp) if rng.random() < 0.5 else reads[i] for i in used]
    full = [[place[i] for i in g] for g in full]
    t_new, t_old, same = [], [], True
    with lib.Context(a.device) as ctx:
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            new = sorter.make_consensus(ctx, bin_reads, full)
            t1 = time.perf_counter()
            mem, st = sorter.orient(ctx, bin_reads, full)
            turned = list(bin_reads)
            for m, s in zip(mem, st):
                for r, f in zip(m, s):
                    if f:
                        turned[r] = bin_reads[r][::-1].translate(comp)
            old = sorter.consensus(ctx, turned, mem)
            t2 = time.perf_counter()
            same = same and new == old
            if i >= a.warmup:
                t_new.append((t1 - t0) * 1e3)
                t_old.append((t2 - t1) * 1e3)
    return {"groups": k, "reads": len(bin_reads),
            "make_consensus_ms_median": float(np.median(t_new)), "make_consensus_ms_all": t_new,
            "host_turn_route_ms_median": float(np.median(t_old)), "host_turn_route_ms_all": t_old,
            "host_turn_route": "orient on the resident batch, reads turned on the host, pack and "
                               "load again, sorter.consensus",
            "same_consensus": bool(same)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--per", type=int, default=50)
    ap.add_argument("--families", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-groups", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--strands", choices=("none", "all", "half"), default="none")
    ap.add_argument("--consensus-ab", type=int, default=0, metavar="GROUPS",
                    help="also time make_consensus against the host-turn route on this many groups")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reads, seeds, groups, seed_idx = [], [], [], []
    gpf = (a.groups + a.families - 1) // a.families
    for f in range(a.families):
        fam = [r.encode() for r in synth.amplicon_bin(gpf * a.per, 1, (1150, 1250), (0.03, 0.12),
                                                      0.0, seed=190 + f)]
        for k in range(gpf):
            if len(groups) == a.groups:
                break
            base = len(reads)
            g = fam[k * a.per:(k + 1) * a.per]
            order = np.argsort([-len(r) for r in g], kind="stable")
            reads += g
            seeds.append(g[order[0]])
            seed_idx.append(base + int(order[0]))
            groups.append([base + int(i) for i in order[1:]])
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    strands = None
    if a.strands != "none":   # the flagged members lie reverse-complemented in the batch
        step = 1 if a.strands == "all" else 2
        strands = [[1 if k % step == 0 else 0 for k in range(len(g))] for g in groups]
        for g, s in zip(groups, strands):
            for i, f in zip(g, s):
                if f:
                    reads[i] = reads[i][::-1].translate(comp)
    ln = np.array([len(r) for r in reads], dtype=np.int64)
    blob = np.frombuffer(b"".join(reads), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
    p = lib.pack(blob, offs, ln.astype(np.uint32))
    n_align = sum(len(g) for g in groups)
    # the same pairs for dmx_pairalign: every member against its group's seed read
    pq = np.array([i for g in groups for i in g], dtype=np.uint32)
    pt = np.repeat(np.array(seed_idx, dtype=np.uint32), [len(g) for g in groups])
    rec = {"tool": "bench_groupalign", "groups": len(groups), "reads_per_group": a.per,
           "families": a.families, "mean_len": float(ln.mean()), "alignments": int(n_align),
           "cycle": "1 of 3 (seed = the group's longest read)", "strands": a.strands,
           "reversed_members": int(sum(sum(s) for s in strands)) if strands else 0}
    with lib.Context(a.device) as ctx:
        ctx.load(p)
        fwd, tb, mg, wall, pa, pf, pt_ms = [], [], [], [], [], [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            res = ctx.groupalign(seeds, groups, strands=strands)
            w = time.perf_counter() - t0
            st = ctx.groupalign_stats()
            ctx.pairalign(pq, pt)
            ps = ctx.pairalign_stats()
            if i >= a.warmup:
                fwd.append(st["forward"])
                tb.append(st["traceback"])
                mg.append(st["merge"])
                wall.append(w * 1e3)
                pa.append(ctx.pairalign_ms())
                pf.append(ps["forward"])
                pt_ms.append(ps["traceback"])
        passes = {"forward trace": float(np.median(fwd)), "traceback": float(np.median(tb)),
                  "merge": float(np.median(mg))}
        dev = sum(passes.values())
        rows = np.diff(res["col_off"].astype(np.int64))
        rec.update({"rounds": st["rounds"], "launches": st["launches"],
                    "forward_ms_median": passes["forward trace"],
                    "traceback_ms_median": passes["traceback"],
                    "merge_ms_median": passes["merge"],
                    "device_ms_median": dev,
                    "device_ms_all": [float(x + y + z) for x, y, z in zip(fwd, tb, mg)],
                    "dominant_pass": max(passes, key=passes.get),
                    "call_ms_median": float(np.median(wall)),
                    "alignments_per_s_device": n_align / (dev * 1e-3),
                    "alignments_per_s_call": n_align / (float(np.median(wall)) * 1e-3),
                    "us_per_alignment_device": dev * 1e3 / n_align,
                    "pairs_per_round": len(groups),
                    "final_row_len": {"min": int(rows.min()), "median": float(np.median(rows)),
                                      "max": int(rows.max())},
                    "pairalign_same_pairs": {
                        "pairs": int(len(pq)), "launches": ps["launches"],
                        "device_ms_median": float(np.median(pa)),
                        "forward_ms_median": float(np.median(pf)),
                        "traceback_ms_median": float(np.median(pt_ms)),
                        "us_per_alignment_device": float(np.median(pa)) * 1e3 / len(pq)}})
    k = min(a.cpu_groups, len(groups))
    t0 = time.perf_counter()
    host = lib.groupalign_host(p, seeds[:k], groups[:k], n_threads=16,
                               strands=strands[:k] if strands else None)
    cpu = time.perf_counter() - t0
    n = int(host["col_off"][-1])
    same = bool(np.array_equal(host["col_off"], res["col_off"][:k + 1]) and
                np.array_equal(host["mask"], res["mask"][:n]) and
                np.array_equal(host["count"], res["count"][:n]) and
                np.array_equal(host["first"], res["first"][:n]) and
                np.array_equal(host["dist"], res["dist"][:len(host["dist"])]))
    cpu_n = sum(len(g) for g in groups[:k])
    rec.update({"cpu_comparator": "dmx_groupalign_host (the project's sequential full-matrix DP, "
                                  "traceback and merge, not edlib), 16 threads, one group per "
                                  "thread",
                "cpu_groups": int(k), "cpu_alignments_per_s": cpu_n / cpu,
                "cpu_sample_matches_gpu": same})
    rec["speedup_vs_cpu_dp_call"] = rec["alignments_per_s_call"] / rec["cpu_alignments_per_s"]
    if a.consensus_ab:
        rec["consensus_ab"] = consensus_ab(a, reads, groups, seed_idx, comp)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
