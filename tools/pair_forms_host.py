#!/usr/bin/env python3
"""Wall time of Context.pairdist and Context.rowassign on one fixed list each, for two builds of
the libraries (the host path of csrc/dmx_pairdist.hip: planning, staging, the launch epilogue).

usage: pair_forms_host.py --parent DIR --branch DIR [--runs 7] --out FILE.json

DIR holds a build of every library (DMX_LIBDIR).  The builds alternate, one process per run, each
under its own time limit; a run loads the batch, makes one warm-up call and reports the median of
five timed calls.  Criterion: the branch's median over the runs lies inside the parent's min-max
range, for both calls.  Lists (seed 7): about 10^5 pairs of ~700-nt reads (pairdist: 2,000 reads,
100,000 random pairs, NW; rowassign: 1,000 reads against 100 rows, every pair the 5 % rule
keeps)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "nanopore-barcoding-orc_amd"),
                os.path.join(ROOT, "oracle")]


def child(call):
    import numpy as np

    import pairdist_cases as pc
    import rowassign_cases as ra
    from dmx import lib

    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    founders = [rng.choice(acgt, 720) for _ in range(8)]

    def copy_of(f):
        s = f.copy()
        hit = rng.random(len(s)) < 0.05
        s[hit] = rng.choice(acgt, int(hit.sum()))
        return s[:len(s) - int(rng.integers(0, 40))].tobytes()

    n_reads = 2000 if call == "pairdist" else 1000
    reads = [copy_of(founders[k % 8]) for k in range(n_reads)]
    with lib.Context(0) as ctx:
        ctx.load(pc.pack_reads(reads))
        if call == "pairdist":
            q = rng.integers(0, n_reads, 100_000).astype(np.uint32)
            t = rng.integers(0, n_reads, 100_000).astype(np.uint32)
            run = lambda: ctx.pairdist(q, t, lib.PD_NW)
            n_pairs = len(q)
        else:
            rows = [lib.mask_row(copy_of(founders[k % 8])) for k in range(100)]
            sel = np.arange(n_reads, dtype=np.uint32)
            tb = ra.tables(range(600, 721))
            run = lambda: ctx.rowassign(rows, sel, *tb)
            n_pairs = int(run()[3])
        run()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            run()
            times.append(time.perf_counter() - t0)
    print(json.dumps({"call": call, "lib": lib.LIB_PATH, "n_pairs": n_pairs,
                      "wall_s": [round(x, 6) for x in times],
                      "median_s": round(statistics.median(times), 6)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--parent")
    ap.add_argument("--branch")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    dirs = {"parent": os.path.abspath(a.parent), "branch": os.path.abspath(a.branch)}
    out = {"what": __doc__.split("usage")[0].strip(), "runs": {}, "summary": {}}
    for call in ("pairdist", "rowassign"):
        runs = {"parent": [], "branch": []}
        for k in range(a.runs):
            for who in (("parent", "branch") if k % 2 == 0 else ("branch", "parent")):
                env = dict(os.environ, DMX_LIBDIR=dirs[who])
                env.pop("DMX_LIBDMX", None)
                res = subprocess.run([sys.executable, __file__, "--child", call], env=env,
                                     capture_output=True, text=True, timeout=120)
                if res.returncode != 0:   # nothing more is started on the GPU after a failure
                    sys.exit(f"{who} {call} run {k}: exit {res.returncode}\n{res.stderr[-2000:]}")
                rec = json.loads(res.stdout.strip().splitlines()[-1])
                assert rec["lib"].startswith(dirs[who])
                runs[who].append(rec)
                print(who, call, k, rec["median_s"], flush=True)
        pm = [r["median_s"] for r in runs["parent"]]
        bm = [r["median_s"] for r in runs["branch"]]
        out["runs"][call] = runs
        out["summary"][call] = {"parent_range_s": [min(pm), max(pm)],
                                "parent_median_s": statistics.median(pm),
                                "branch_median_s": statistics.median(bm),
                                "branch_range_s": [min(bm), max(bm)],
                                "inside": min(pm) <= statistics.median(bm) <= max(pm)}
        if a.out:   # kept up to date, so a later failure leaves what was measured
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
    print(json.dumps(out["summary"], indent=1))


if __name__ == "__main__":
    main()
