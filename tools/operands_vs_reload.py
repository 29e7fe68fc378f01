#!/usr/bin/env python3
"""Gene groups of every kept well, two ways: from the well files the fused loop
wrote (read + inflate, clean + pack, dmx_load, kernels: today's dmx-similarity --groups path), and
from the resident operands (dmx-demux-loop --groups).  Prints one report; the numbers in
profiles/operands_vs_reload.txt come from it.

    python tools/operands_vs_reload.py [--reads 1000000] [--workdir DIR] [--batch-mb 8192]
"""
import argparse
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nanopore-barcoding-orc_amd"))

from dmx import lib, sorter, synth  # noqa: E402

LOOP = os.path.join(ROOT, "nanopore-barcoding-orc_amd", "bin", "dmx-demux-loop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--batch-mb", type=int, default=8192)
    a = ap.parse_args()
    work = a.workdir or tempfile.mkdtemp(prefix="opsvsreload_")
    os.makedirs(os.path.join(work, "pychopped"), exist_ok=True)
    infile = os.path.join(work, "pychopped", "pychopped_c2.fastq")
    t0 = time.perf_counter()
    d = synth.generate("c2", n=a.reads, seed=12)
    seqs = synth.to_strings(d)
    with open(infile, "w") as f:
        for i, s in enumerate(seqs):
            f.write(f"@read{i}\n{s}\n+\n{'I' * len(s)}\n")
    print(f"workload: c2, {a.reads} reads, {sum(map(len, seqs))} nt, written in "
          f"{time.perf_counter() - t0:.1f} s", flush=True)
    del seqs, d
    out = os.path.join(work, "demuxed")
    g = os.path.join(work, "groups.tsv")
    env = dict(os.environ, DMX_PROFILE_IO="1")
    t0 = time.perf_counter()
    r = subprocess.run([LOOP, infile, "--outdir", out, "--groups", g, "--batch-mb",
                        str(a.batch_mb)], env=env, stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    wall = time.perf_counter() - t0
    prof = [ln for ln in r.stderr.splitlines() if ln.startswith("io profile")]
    print(f"resident operands: dmx-demux-loop --groups, exit {r.returncode}, wall {wall:.2f} s")
    print("  " + (prof[0] if prof else r.stderr[-2000:]))
    print("  groups = gene groups of all kept wells on resident operands (wall, s); groups_kernel"
          " = their device time (dmx_hitgroups_stats: forward + compact + components);"
          " groups_build = dmx_result_operands (synchronous call); groups_exec = dmx_exec_checked"
          " of the same batch (synchronous call); read+inflate, clean+pack, dmx_load: none",
          flush=True)
    if r.returncode:
        return 1
    wells = sorted(glob.glob(os.path.join(out, "SP27", "*.fastq.gz")))
    t = dict(read=0.0, pack=0.0, load=0.0, rest=0.0, kernel=0.0)
    n_groups = n_reads = 0
    t0 = time.perf_counter()
    with lib.Context(0) as ctx:
        for w in wells:
            ta = time.perf_counter()
            reads = sorter.read_sequences(w)
            tb = time.perf_counter()
            plan = sorter._similarity_plan(reads, 80.0, 300, None, 10000, False)
            tc = time.perf_counter()
            if len(plan[2]):
                ctx.load(plan[0])
            td = time.perf_counter()
            groups = sorter.gene_groups(ctx, reads)
            te = time.perf_counter()
            # gene_groups repeats the plan and the load: counted once, as one dmx-similarity run
            t["read"] += tb - ta
            t["pack"] += tc - tb
            t["load"] += td - tc
            t["rest"] += max(0.0, (te - td) - (tc - tb) - (td - tc))
            if len(plan[2]):
                st = ctx.hitgroups_stats()
                t["kernel"] += (st["forward"] + st["compact"] + st["components"]) / 1000
            n_groups += len(groups)
            n_reads += len(reads)
    total = t["read"] + t["pack"] + t["load"] + t["rest"]
    print(f"reload: {len(wells)} well files, {n_reads} records, {n_groups} gene groups")
    print(f"  read+inflate {t['read']:.2f} s, clean+pack {t['pack']:.2f} s, dmx_load "
          f"{t['load']:.2f} s, pairs + kernels + groups {t['rest']:.2f} s (device time "
          f"{t['kernel']:.2f} s): {total:.2f} s; loop over the wells, wall "
          f"{time.perf_counter() - t0:.2f} s")
    with open(g) as f:
        labels = {ln.split("\t")[0] + ln.split("\t")[2] for ln in f if not ln.endswith("\t-\n")}
    print(f"resident operands: {len(labels)} gene groups")
    return 0


if __name__ == "__main__":
    sys.exit(main())
