#!/usr/bin/env python3
"""Rebuild a recorded mismatch of a tools/parity_sweep.py run on the CPU (no GPU, no oracle) from
its seed and k, and write that case (parameters + every read) as JSON, so it can be run alone
against the oracle with any libdmx build (--run, on the GPU box).  With the library of the tree,
`python tools/parity_sweep.py --case SEED:K` does both steps at once.

usage: python tools/replay_sweep.py SWEEP_JSON [--which 0] --out CASE_JSON
       python tools/replay_sweep.py --run CASE_JSON        (GPU: per-read diff vs the oracle)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "nanopore-barcoding-orc_amd"), os.path.join(ROOT, "oracle"),
          os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

import oracle  # noqa: E402  (checker only)


def find(sweep_json, which, out):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sweep_cases as sw
    rec = json.load(open(sweep_json))
    target = rec["mismatches"][which]
    if "k" not in target:
        print("this sweep was recorded before every case had a stream of its own "
              "(tools/parity_sweep.py): its draws cannot be replayed")
        return 1
    case = sw.sweep_case(rec["seed"], target["k"])
    if case["kind"] != "single":
        print(f"case {case['id']} is no single-round case: python tools/parity_sweep.py "
              f"--case {case['id']}")
        return 1
    params = dict(kind="random", panel=case["panels"][0], wheres=case["wheres"][0], e=case["e"],
                  min_overlap=case["min_overlap"], rc=case["rc"])
    json.dump(dict(case=target["k"], params=params, reads=case["reads"]), open(out, "w"))
    print(f"case {case['id']}: {len(case['reads'])} reads -> {out}")
    return 0


def run(case_json):
    from dmx import lib
    c = json.load(open(case_json))
    p, seqs = c["params"], c["reads"]
    assert p["kind"] == "random", "only random single-round cases"
    blob, offs, lens = oracle.pack_ascii(seqs)
    exp = oracle.run_batch(oracle.Panel(p["panel"], p["wheres"], max_errors=p["e"],
                                        min_overlap=p["min_overlap"]), None, blob, offs, lens,
                           mode=0, use_rc=p["rc"], threads=8)
    with lib.Context(0) as ctx:
        ctx.set_panel_mixed(0, p["panel"], [lib.DMX_FRONT if w == oracle.FRONT else lib.DMX_BACK
                                            for w in p["wheres"]], p["rc"], p["e"],
                            p["min_overlap"])
        ctx.set_mode(lib.MODE_SINGLE)
        got = ctx.run(lib.pack(blob, offs, lens))
    g = got.view(np.uint8).reshape(len(got), -1)
    e = exp.view(np.uint8).reshape(len(exp), -1)
    bad = np.nonzero((g != e).any(axis=1))[0]
    print(f"{lib.LIB_PATH}: {len(bad)} of {len(seqs)} reads differ")
    for i in bad[:12]:
        print(i, repr(seqs[i][:80]), len(seqs[i]))
        print("  got", got[i])
        print("  exp", exp[i])
    return 1 if len(bad) else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("sweep", nargs="?")
    ap.add_argument("--which", type=int, default=0)
    ap.add_argument("--out")
    ap.add_argument("--run")
    a = ap.parse_args()
    sys.exit(run(a.run) if a.run else find(a.sweep, a.which, a.out))
