#!/usr/bin/env python3
"""One pass of the assignment loop on tools/bench_rowdist.py's shape (--reads synthetic reads of
about 1,200 nt, one family per consensus, copies mutated 3-12 %, against --consensuses
consensuses), two ways, the same best list:
  assign       dmx.sorter.assign: dmx_rowdist, every distance to the host, the decision, the
               reverse-complement call and the lines in Python (the existing code, the baseline);
  assign_best  dmx.sorter.assign_best: one dmx_rowassign call, the pairs generated in C++, the
               decision and the best line per read on the device, one record per read back.
Wall time is the whole call on a resident batch; device time is the HIP-event time of the
kernels (dmx_rowdist_ms summed over assign's calls, dmx_rowassign_ms).  For assign_best the wall
time is split into the Python part before the call (cleaning, tables, mask rows), the
dmx_rowassign call and the Python part after it; the call's own split (pair generation, planning,
upload, read-back) is the call's wall time minus its device time and is not instrumented further.
Medians of --reps after --warmup, in one session.  Writes one JSON record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "nanopore-barcoding-orc_amd"))
from dmx import lib, sorter, synth  # noqa: E402


class Timed(lib.Context):
    """A Context that adds up the device and wall time of its rowdist / rowassign calls."""
    dev_ms = 0.0
    call_ms = 0.0

    def rowdist(self, *a, **kw):
        t0 = time.perf_counter()
        out = super().rowdist(*a, **kw)
        self.call_ms += (time.perf_counter() - t0) * 1e3
        self.dev_ms += self.rowdist_ms()
        return out

    def rowassign(self, *a, **kw):
        t0 = time.perf_counter()
        out = super().rowassign(*a, **kw)
        self.call_ms += (time.perf_counter() - t0) * 1e3
        self.dev_ms += self.rowassign_ms()
        self.last = out
        return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--consensuses", type=int, default=200)
    ap.add_argument("--similar", type=float, default=0.93)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    per = (a.reads + a.consensuses - 1) // a.consensuses
    reads, cons = [], []
    for f in range(a.consensuses):
        reads += synth.amplicon_bin(per, 1, (1150, 1250), (0.03, 0.12), 0.25, seed=400 + f)
        cons.append(synth.amplicon_bin(1, 1, (1150, 1250), (0.0, 0.0), 0.0, seed=400 + f)[0])
    reads = reads[:a.reads]
    un = np.arange(len(reads))
    rec = {"tool": "bench_rowassign", "reads": len(reads), "consensuses": len(cons),
           "similar": a.similar, "session": "a single session"}
    res = {}
    with Timed(a.device) as ctx:
        for name, fn in (("assign", lambda: sorter.assign(ctx, reads, un, cons, a.similar)[1:]),
                         ("assign_best", lambda: tuple(sorter.assign_best(ctx, reads, un, cons,
                                                                          a.similar)))):
            wall, dev, call = [], [], []
            for i in range(a.warmup + a.reps):
                ctx.dev_ms = ctx.call_ms = 0.0
                t0 = time.perf_counter()
                out = fn()
                w = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    wall.append(w), dev.append(ctx.dev_ms), call.append(ctx.call_ms)
            res[name] = out
            rec[name] = {"wall_ms_median": float(np.median(wall)), "wall_ms_all": wall,
                         "device_ms_median": float(np.median(dev)), "device_ms_all": dev,
                         "library_calls_ms_median": float(np.median(call)),
                         "python_around_the_calls_ms_median":
                             float(np.median(np.array(wall) - np.array(call))),
                         "library_calls_minus_device_ms_median":
                             float(np.median(np.array(call) - np.array(dev)))}
        rec["pairs"] = int(ctx.last[3])
        rec["lines"] = int(ctx.last[4])
    same = tuple(res["assign"]) == tuple(res["assign_best"])
    rec["reads_with_a_line"] = len(res["assign_best"][0])
    rec["assign_best_equals_assign"] = same
    rec["wall_speedup_assign_best_over_assign"] = (rec["assign"]["wall_ms_median"] /
                                                   rec["assign_best"]["wall_ms_median"])
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
