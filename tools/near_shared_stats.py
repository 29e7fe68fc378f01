"""Gate for the near-start cells inside the shared suffix (near_shared): on a
build that hands every near piece to every adapter (the parent, or DMX_NEAR_ALL=1), how many of
round 1's tasks and candidate cells are copies that only adapter 0 needs.

    python tools/near_shared_stats.py [--workload c2x24] [--reads 2000000]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nanopore-barcoding-orc_amd"))

from dmx import lib, synth  # noqa: E402
from near_stats import common  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2x24")
    ap.add_argument("--reads", type=int, default=2_000_000)
    a = ap.parse_args()
    d = synth.generate(a.workload, n=a.reads, threads=16)
    ads = d["sp5"]
    ms = np.array([len(s) for s in ads])
    kk = (0.1 * ms).astype(np.int64)
    pl, sl = common(ads, False), min(common(ads, True), 32)
    jsplit = int((ms - pl + kk).max())
    jS = int(sl - kk.max())
    out = {"workload": a.workload, "reads": a.reads, "pre_len": pl, "suffix_len": sl,
           "jsplit": jsplit, "near_shared": jS, "lib": os.path.basename(lib.LIB_PATH)}
    with lib.Context(0) as ctx:
        ctx.set_panel(0, ads, lib.DMX_FRONT | lib.DMX_RC, 0.1)
        ctx.load(lib.pack(d["blob"], d["offsets"], d["lengths"]))
        ctx.set_mode(lib.MODE_SINGLE)
        ctx.exec()
        ctx.sync()
        t = ctx.debug_fetch(lib.DBG_TASKS, 0)
        c0 = ctx.debug_fetch(lib.DBG_CANDS0, 0)
        c1 = ctx.debug_fetch(lib.DBG_CANDS1, 0)
        st = ctx.stats()
    tj1, tj2, ta = t["j1"].astype(np.int64), t["j2"].astype(np.int64), t["info"].astype(np.int64)
    near = tj2 < jsplit                       # a near piece ends at min(j2, jsplit - 1)
    drop = near & (ta != 0) & (tj2 <= jS)
    cut = near & (ta != 0) & (tj2 > jS) & (tj1 <= jS)
    out["tasks"] = int(len(t))
    out["near_tasks"] = int(near.sum())
    out["near_tasks_dropped"] = int(drop.sum())
    out["near_tasks_shortened"] = int(cut.sum())
    out["dropped_share_of_tasks"] = round(float(drop.sum()) / max(len(t), 1), 4)
    out["stats_tasks"] = st["tasks"]
    out["stats_resolved"] = st["resolved"]
    for nm, c in (("cands0", c0), ("cands1", c1)):
        j, ca = c["j"].astype(np.int64), c["a"].astype(np.int64)
        lastrow = c["iend"].astype(np.int64) == ms[ca]
        inS = lastrow & (j <= jS)
        out[nm] = {"n": int(len(c)), "j_le_near_shared": int(inS.sum()),
                   "of_adapter_0": int((inS & (ca == 0)).sum()),
                   "by_adapter": np.bincount(ca[inS], minlength=len(ads)).tolist()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
