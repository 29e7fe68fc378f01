#!/usr/bin/env python3
"""Wall time of the gene groups of a bin two ways, on bench_pairdist.py's shape
(one group of 1000 reads of about 1200 nt, dmx.synth.amplicon_bin) and on a bin of --groups
such groups (10 by default; 0 skips it):
  (a) sorter.similarity (the lines, through the dense distances) followed by a Python
      restatement of update_list's best-hit filter and grouping;
  (b) sorter.gene_groups (dmx_pairhits + dmx_hitgroups: one label per read comes back),
      with the device time of the distance launches, the compaction and the components kernels
      from dmx_hitgroups_stats.
Medians of --reps calls after --warmup.  Also times dmx_pairdist on the same pairs (the forward
call and the reverse-complement retries, as similarity() makes them) against the distance
launches inside dmx_pairhits: the same kernel, so the two should agree within their spread.
Writes one JSON record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "nanopore-barcoding-orc_amd"))
from dmx import lib, sorter, synth  # noqa: E402


def groups_from_lines(lines):
    """update_list's result from the similarity lines: per longer read the lines of the largest
    identity, ties kept, then the components of those links (a union-find instead of the
    reference's quadratic loops, which would only make (a) slower)."""
    best = {}
    rows = [x.split(":")[:3] for x in lines]
    for i, j, iden in rows:
        f = float(iden)
        if f > best.get(j, -1.0):
            best[j] = f
    parent = {}

    def find(v):
        while parent.setdefault(v, v) != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for i, j, iden in rows:
        if float(iden) == best[j]:
            a, b = find(int(i)), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    out = {}
    for v in parent:
        out.setdefault(find(v), []).append(v)
    return sorted(sorted(g) for g in out.values())


def timed(fn, warmup, reps, after=None):
    wall, extra, res = [], [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        res = fn()
        w = (time.perf_counter() - t0) * 1e3
        print(f"bench_genegroups: call {i + 1} of {warmup + reps}: {w:.1f} ms", file=sys.stderr,
              flush=True)
        if i >= warmup:
            wall.append(w)
            if after:
                extra.append(after())
    return res, wall, extra


def bench_bin(ctx, name, reads, a):
    rec = {"bin": name, "reads": len(reads)}
    lines_holder = {}

    def path_a():
        lines_holder["lines"] = sorter.similarity(ctx, reads, minlength=a.minlength)
        return groups_from_lines(lines_holder["lines"])

    ga, wall_a, _ = timed(path_a, a.warmup, a.reps)
    gb, wall_b, st = timed(lambda: sorter.gene_groups(ctx, reads, minlength=a.minlength),
                           a.warmup, a.reps, ctx.hitgroups_stats)
    rec.update({"lines": len(lines_holder["lines"]), "groups": len(gb),
                "groups_agree": sorted(g.tolist() for g in gb) == ga,
                "a_similarity_then_update_list_ms": float(np.median(wall_a)),
                "a_ms_all": wall_a,
                "b_gene_groups_ms": float(np.median(wall_b)), "b_ms_all": wall_b,
                "b_device_forward_ms": float(np.median([s["forward"] for s in st])),
                "b_device_compact_ms": float(np.median([s["compact"] for s in st])),
                "b_device_components_ms": float(np.median([s["components"] for s in st])),
                "b_hook_rounds": st[-1]["rounds"]})
    # the distance launches: dmx_pairdist as similarity() calls it, against dmx_pairhits'
    p, ln, q, t, cap_sg, cap_half = sorter._similarity_plan(reads, 80.0, a.minlength, None, 10000,
                                                            False)
    rec["pairs"] = int(len(q))
    ctx.load(p)
    fcap = np.maximum(np.maximum(cap_half, cap_sg), 0).astype(np.uint32)

    def pairdist_both():
        df = ctx.pairdist(q, t, lib.PD_NW, caps=fcap).astype(np.int64)
        ms = ctx.pairdist_ms()
        rcs = np.flatnonzero(~(df <= cap_sg) & (df > cap_half) & (cap_sg >= 0))
        if len(rcs):
            ctx.pairdist(q[rcs], t[rcs], lib.PD_NW, np.full(len(rcs), lib.PD_RC, dtype=np.uint8),
                         cap_sg[rcs].astype(np.uint32))
            ms += ctx.pairdist_ms()
        return ms

    for _ in range(a.warmup):
        pairdist_both()
    pd_ms = [pairdist_both() for _ in range(a.reps)]
    ph_ms = []
    for _ in range(a.reps):
        ctx.pairhits(q, t, cap_sg, cap_half)
        ph_ms.append(ctx.hitgroups_stats()["forward"])
    rec.update({"pairdist_forward_ms_median": float(np.median(pd_ms)), "pairdist_forward_ms_all": pd_ms,
                "pairhits_forward_ms_median": float(np.median(ph_ms)), "pairhits_forward_ms_all": ph_ms})
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--groups", type=int, default=10, help="groups of the large bin (0: skip it)")
    ap.add_argument("--minlength", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"tool": "bench_genegroups", "warmup": a.warmup, "reps": a.reps, "bins": []}
    with lib.Context(a.device) as ctx:
        one = synth.amplicon_bin(a.reads, 4, (1150, 1250), (0.03, 0.12), 0.1, seed=9)
        rec["bins"].append(bench_bin(ctx, "one_group", one, a))
        if a.groups:
            many = []
            for g in range(a.groups):
                many += synth.amplicon_bin(a.reads, 4, (1150, 1250), (0.03, 0.12), 0.1, seed=20 + g)
            rec["bins"].append(bench_bin(ctx, f"{a.groups}_groups", many, a))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
