#!/usr/bin/env python3
"""Device time of the end-window stage against the regular 5' round it is
modelled on: the synthetic c2x24 reads, the SP5 panel (24 adapters) given as regular `-g`
adapters (the yardstick: the internal-adapter pipeline's round 0, --rc), as `^` adapters and as
`X` adapters, all in DMX_MODE_SINGLE on one resident batch.

Per panel: one warm-up dmx_exec, then the median of --repeats timed ones (HIP events on the
context's stream, dmx_stats), and for the restricted panels the share of (view, orientation,
adapter) triples that reached the exact DP.  One JSON record on stdout and in --out.

The kernel's VALU fraction comes from counter runs of their own: rocprofv3 --pmc with this script
after `--` (--panels anchored,noninternal --repeats 1), summarised by tools/ends_pmc_summary.py;
this script does not start a profiler."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nanopore-barcoding-orc_amd"))

from dmx import lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--panels", default="regular,anchored,noninternal")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    d = synth.generate("c2x24", n=args.reads)
    p = lib.pack(d["blob"], d["offsets"], d["lengths"])
    sp5 = list(d["sp5"])
    wheres = {"regular": lib.DMX_FRONT, "anchored": lib.DMX_FRONT | lib.DMX_ANCHORED,
              "noninternal": lib.DMX_FRONT | lib.DMX_NONINTERNAL}
    rec = {"workload": "c2x24", "reads": int(p.n_reads), "nt": int(p.lengths.sum()),
           "adapters": len(sp5), "repeats": args.repeats, "panels": {}}
    with lib.Context(args.device) as ctx:
        ctx.load(p)
        ctx.set_mode(lib.MODE_SINGLE)
        for name in args.panels.split(","):
            ctx.set_panel_ex(0, sp5, [wheres[name]] * len(sp5), True, 0.1, 3)
            ctx.exec()
            ctx.sync()
            total, ends, st = [], [], None
            for _ in range(args.repeats):
                ctx.exec()
                ctx.sync()
                st = ctx.stats()
                total.append(st["ms"]["total"])
                ends.append(st["ms"]["ends0"])
            res = ctx.fetch()
            if st["flags"]:
                raise SystemExit(f"{name}: pipeline flags {st['flags']}")
            seen, dp = st["ends_seen"][0], st["ends_dp"][0]
            rec["panels"][name] = {
                "ms_per_step": round(statistics.median(total), 3),
                "ms_runs": [round(x, 3) for x in total],
                "ends_ms": round(statistics.median(ends), 3),
                "triples": int(seen), "exact_dp": int(dp),
                "exact_dp_share": round(dp / seen, 5) if seen else None,
                "matched": int((res["bin1"] >= 0).sum()),
                "reverse_complemented": int(res["rc1"].sum()),
            }
    if "regular" in rec["panels"]:
        base = rec["panels"]["regular"]["ms_per_step"]
        for name, v in rec["panels"].items():
            v["vs_regular"] = round(v["ms_per_step"] / base, 3) if base else None
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
