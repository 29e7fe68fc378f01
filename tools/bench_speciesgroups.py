#!/usr/bin/env python3
"""Wall time of the ssg estimate and the species groups of a bin two ways, on the
two bins of bench_genegroups.py (one group of 1000 reads of about 1200 nt, and --groups such
groups, 10 by default; 0 skips it).  The gene groups are sorter.gene_groups', made once.
  (a) sorter.similarity (the lines), then Python restatements of SSG (:810-836, the float sums)
      and of read_indexes' first half (:1363-1411) per gene group: the threshold and membership
      test per line, the best lines per longer read, ties kept, and a union-find instead of the
      reference's quadratic loops, which would only make (a) slower;
  (b) sorter.estimate_ssg + sorter.species_groups (dmx_pairhits, dmx_hithist,
      dmx_pairhits_cross, dmx_hitgroups_within), with the device times of the histogram, the last
      compaction and the components run from dmx_hitgroups_stats, and the number of cross hits.
Medians of --reps calls after --warmup.  Writes one JSON record; `library` names the libdmx it
ran on (DMX_LIBDMX selects another build of it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "nanopore-barcoding-orc_amd"))
from dmx import lib, sorter, synth  # noqa: E402


def ssg_from_lines(lines):
    total, counts = 0, {}
    for x in lines:
        s = float(x.split(":")[2])
        counts[s] = counts.get(s, 0) + 1
        total += s
    b = int(total * 0.06)
    n6 = 0
    for s in sorted(counts, reverse=True):
        n6 += counts[s] * s
        if n6 >= b:
            return int(s * 100)
    return None


def species_from_lines(lines, groups, ssg):
    rows = [x.split(":")[:3] for x in lines]
    rows = [(int(i), int(j), float(f)) for i, j, f in rows if float(f) >= ssg / 100]
    out = []
    for g in groups:
        idx = set(int(x) for x in g)
        mine = [r for r in rows if r[0] in idx or r[1] in idx]
        best = {}
        for i, j, f in mine:
            if f > best.get(j, -1.0):
                best[j] = f
        parent = {}

        def find(v):
            while parent.setdefault(v, v) != v:
                parent[v] = parent[parent[v]]
                v = parent[v]
            return v

        for i, j, f in mine:
            if f == best[j]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
        comp = {}
        for v in parent:
            comp.setdefault(find(v), []).append(v)
        out.append(sorted(sorted(m) for m in comp.values() if len(m) > 3))
    return out


def timed(name, fn, warmup, reps, after=None):
    wall, extra, res = [], [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        res = fn()
        w = (time.perf_counter() - t0) * 1e3
        print(f"bench_speciesgroups: {name}: call {i + 1} of {warmup + reps}: {w:.1f} ms",
              file=sys.stderr, flush=True)
        if i >= warmup:
            wall.append(w)
            if after:
                extra.append(after())
    return res, wall, extra


def bench_bin(ctx, name, reads, a):
    groups = sorter.gene_groups(ctx, reads, minlength=a.minlength)
    rec = {"bin": name, "reads": len(reads), "gene_groups": len(groups)}
    hold = {}

    def path_a():
        hold["lines"] = sorter.similarity(ctx, reads, minlength=a.minlength)
        ssg = ssg_from_lines(hold["lines"])
        return ssg, species_from_lines(hold["lines"], groups, ssg)

    def path_b():
        ssg = sorter.estimate_ssg(ctx, reads, minlength=a.minlength)
        hold["hist_ms"] = ctx.hitgroups_stats()["hist"]
        return ssg, sorter.species_groups(ctx, reads, groups, ssg, minlength=a.minlength)

    def stats():
        st = ctx.hitgroups_stats()
        st["hist"] = hold["hist_ms"]     # the histogram ran in estimate_ssg's pairhits state
        return st

    (ssg_a, sp_a), wall_a, _ = timed(name + " (a)", path_a, a.warmup, a.reps)
    (ssg_b, sp_b), wall_b, st = timed(name + " (b)", path_b, a.warmup, a.reps, stats)
    # the cross hits of the last call's tables, counted once more outside the timing
    p, ln, q, t, cap_sg, cap_half = sorter._similarity_plan(reads, 80.0, a.minlength, None, 10000,
                                                            False)
    label = np.full(len(ln), lib.LG_NONE, dtype=np.uint32)
    for k, g in enumerate(groups):
        label[g] = k
    cap2 = np.array([sorter.identity_cap(int(L), ssg_b / 100) for L in ln], dtype=np.int32)
    ctx.load(p)
    _, n_hits = ctx.pairhits(q, t, cap_sg, cap_half)
    rec.update({"pairs": int(len(q)), "lines": len(hold["lines"]), "hits": int(n_hits),
                "cross_hits": int(len(ctx.pairhits_cross(label, cap2)[0])),
                "ssg_a": ssg_a, "ssg_b": ssg_b,
                "species_groups": sum(len(s) for s in sp_b),
                "results_agree": ssg_a == ssg_b and
                [sorted(m.tolist() for m in s) for s in sp_b] == sp_a,
                "a_lines_then_python_ms": float(np.median(wall_a)), "a_ms_all": wall_a,
                "b_estimate_and_species_ms": float(np.median(wall_b)), "b_ms_all": wall_b,
                "b_device_hist_ms": float(np.median([s["hist"] for s in st])),
                "b_device_compact_ms": float(np.median([s["compact"] for s in st])),
                "b_device_components_ms": float(np.median([s["components"] for s in st])),
                "b_hook_rounds": st[-1]["rounds"]})
    # the histogram kernel alone, on the resident outcomes
    bin_off, bins = sorter._identity_table(ln, t, cap_sg)
    hist_ms = []
    for _ in range(a.warmup + 2 * a.reps):
        ctx.hithist(bin_off, bins, sorter.N_CLASSES)
        hist_ms.append(ctx.hitgroups_stats()["hist"])
    rec["hist_kernel_ms_median"] = float(np.median(hist_ms[a.warmup:]))
    rec["hist_kernel_ms_all"] = hist_ms[a.warmup:]
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
    rec = {"tool": "bench_speciesgroups", "library": os.path.basename(lib.LIB_PATH),
           "warmup": a.warmup, "reps": a.reps, "bins": []}
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
