#!/usr/bin/env python3
"""Wall and device time of dmx.sorter.finetune on --groups species groups of
--per reads of about --length nt, every other group a mix of two species 6 % apart (3/5 and 2/5
of its reads, in random order), reads at 3 % noise, four in ten stored reverse-complemented.
Per shape:
  lock-step      one call over all groups: wall time, and per call kind (pairdist, rowdist,
                 groupalign, rowpairdist) the calls, the pairs or alignments they carried, their
                 wall time and their device time (the library's own events; groupalign's by
                 pass: forward, traceback, merge), groupalign's lock-step rounds and the
                 alignments per round, and what of groupalign's wall time is not device time
                 (its per-round synchronous downloads and host work), per round;
  one by one     the same groups handed over one at a time, the reference's order: the only
                 comparison with a baseline in this repository; the results must be equal;
  host twin      sorter.finetune(None, ...) on --threads threads: the project's own host twins
                 (full-matrix DPs), NOT edlib.
Medians of --reps calls after --warmup.  Writes one JSON record per shape, a list in --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "nanopore-barcoding-orc_amd"))
from dmx import lib, sorter  # noqa: E402

COMP = bytes.maketrans(b"ACGT", b"TGCA")
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def mutate(rng, s: np.ndarray, rate: float) -> bytes:
    """s with a substitution, an insertion or a deletion at about `rate` of its positions."""
    hit = rng.random(len(s)) < rate
    kind = rng.integers(0, 3, size=len(s))
    other = BASES[rng.integers(0, 4, size=len(s))]
    out = s.copy()
    sub = hit & (kind == 0)
    out[sub] = other[sub]
    keep = ~(hit & (kind == 2))
    reps = np.where(hit & (kind == 1), 2, 1)[keep]
    grown = np.repeat(out[keep], reps)
    at = np.cumsum(reps)[reps == 2] - 1              # the second copy is the inserted base
    grown[at] = BASES[rng.integers(0, 4, size=len(at))]
    return grown.tobytes()


def make_groups(n_groups, per, length, seed=838):
    rng = np.random.default_rng(seed)
    reads, groups = [], []
    for g in range(n_groups):
        a = BASES[rng.integers(0, 4, size=length)]
        b = a.copy()
        where = rng.choice(length, size=int(length * 0.06), replace=False)
        b[where] = BASES[(np.searchsorted(BASES, b[where]) + rng.integers(1, 4, len(where))) % 4]
        is_b = rng.permutation(per) < ((2 * per) // 5 if g % 2 else 0)
        is_b[0] = False                             # the first species anchors the group
        first = len(reads)
        for k in range(per):
            r = mutate(rng, b if is_b[k] else a, 0.03)
            reads.append(r[::-1].translate(COMP) if k and rng.random() < 0.4 else r)
        groups.append(np.arange(first, first + per, dtype=np.int64))
    return reads, groups


class Meter:
    """A Context that notes, per sorting call, its kind, size, wall time and device time."""

    def __init__(self, ctx):
        object.__setattr__(self, "_c", ctx)
        object.__setattr__(self, "log", [])

    def __getattr__(self, k):
        return getattr(self._c, k)

    def __setattr__(self, k, v):
        setattr(self._c, k, v)

    def _note(self, kind, n, fn, dev):
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        self.log.append(dict(kind=kind, n=int(n), wall_ms=wall, **dev()))
        return out

    def pairdist(self, q, t, *a, **k):
        return self._note("pairdist", len(q), lambda: self._c.pairdist(q, t, *a, **k),
                          lambda: {"device_ms": self._c.pairdist_ms()})

    def rowdist(self, rows, q, r, *a, **k):
        return self._note("rowdist", len(q), lambda: self._c.rowdist(rows, q, r, *a, **k),
                          lambda: {"device_ms": self._c.rowdist_ms()})

    def rowpairdist(self, rows, q, t, *a, **k):
        return self._note("rowpairdist", len(q),
                          lambda: self._c.rowpairdist(rows, q, t, *a, **k),
                          lambda: {"device_ms": self._c.rowhits_ms()})

    def groupalign(self, seeds, groups, *a, **k):
        def dev():
            s = self._c.groupalign_stats()
            return {"device_ms": s["forward"] + s["traceback"] + s["merge"],
                    "forward_ms": s["forward"], "traceback_ms": s["traceback"],
                    "merge_ms": s["merge"], "rounds": s["rounds"], "launches": s["launches"]}
        return self._note("groupalign", sum(len(g) for g in groups),
                          lambda: self._c.groupalign(seeds, groups, *a, **k), dev)


def by_kind(log):
    out = {}
    for e in log:
        k = out.setdefault(e["kind"], {"calls": 0, "items": 0, "wall_ms": 0.0, "device_ms": 0.0})
        k["calls"] += 1
        k["items"] += e["n"]
        k["wall_ms"] += e["wall_ms"]
        k["device_ms"] += e["device_ms"]
        for f in ("forward_ms", "traceback_ms", "merge_ms", "rounds", "launches"):
            if f in e:
                k[f] = k.get(f, 0) + e[f]
    ga = out.get("groupalign")
    if ga and ga["rounds"]:
        ga["alignments_per_round"] = ga["items"] / ga["rounds"]
        ga["wall_ms_per_round"] = ga["wall_ms"] / ga["rounds"]
        ga["device_ms_per_round"] = ga["device_ms"] / ga["rounds"]
        ga["not_device_ms_per_round"] = (ga["wall_ms"] - ga["device_ms"]) / ga["rounds"]
    return out


def same(a, b):
    return ([x.tolist() for x in a[0]] == [x.tolist() for x in b[0]]
            and list(a[1]) == list(b[1]))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--per", type=int, default=200)
    ap.add_argument("--length", type=int, default=1200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-by-one-reps", type=int, default=None,
                    help="repetitions of the one-by-one route (default: --reps)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true", help="skip the host twin")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    obo_reps = a.reps if a.one_by_one_reps is None else a.one_by_one_reps
    recs = []
    with lib.Context(a.device) as real:
        ctx = Meter(real)
        for n_groups in a.groups:
            reads, groups = make_groups(n_groups, a.per, a.length)
            cons = ["ACGT"] * len(groups)
            rec = {"tool": "bench_finetune", "groups": n_groups, "reads_per_group": a.per,
                   "mean_len": float(np.mean([len(r) for r in reads])),
                   "mixed_groups": n_groups // 2, "warmup": a.warmup, "reps": a.reps}
            walls, kinds, answer = [], None, None
            for i in range(a.warmup + a.reps):
                ctx.log.clear()
                t0 = time.perf_counter()
                answer = sorter.finetune(ctx, reads, groups, cons)
                wall = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    walls.append(wall)
                    kinds = by_kind(ctx.log)       # the calls are the same every time
            rec["lock_step"] = {"wall_ms_median": float(np.median(walls)), "wall_ms_all": walls,
                                "by_kind_last_rep": kinds,
                                "groups_out": len(answer[0]),
                                "wall_not_in_sorting_calls_ms":
                                    walls[-1] - sum(k["wall_ms"] for k in kinds.values())}
            walls, eq = [], True
            for i in range(a.warmup + obo_reps):
                ctx.log.clear()
                t0 = time.perf_counter()
                out_g, out_c, add_g, add_c = [], [], [], []
                for g, c in zip(groups, cons):
                    one_g, one_c = sorter.finetune(ctx, reads, [g], [c])
                    out_g.append(one_g[0])
                    out_c.append(one_c[0])
                    add_g += one_g[1:]
                    add_c += one_c[1:]
                wall = (time.perf_counter() - t0) * 1e3
                eq = eq and same((out_g + add_g, out_c + add_c), answer)
                if i >= a.warmup:
                    walls.append(wall)
                    kinds = by_kind(ctx.log)
            rec["one_by_one"] = {"wall_ms_median": float(np.median(walls)), "wall_ms_all": walls,
                                 "reps": obo_reps, "by_kind_last_rep": kinds,
                                 "same_result": bool(eq)}
            rec["one_by_one_over_lock_step"] = (rec["one_by_one"]["wall_ms_median"]
                                                / rec["lock_step"]["wall_ms_median"])
            if not a.no_host:
                t0 = time.perf_counter()
                host = sorter.finetune(None, reads, groups, cons, n_threads=a.threads)
                rec["host_twin"] = {"what": "sorter.finetune(None, ...): the project's host "
                                            "twins (full-matrix DPs), not edlib",
                                    "threads": a.threads, "runs": 1,
                                    "wall_ms": (time.perf_counter() - t0) * 1e3,
                                    "same_result": bool(same(host, answer))}
            print(json.dumps(rec), flush=True)
            recs.append(rec)
            if a.out:                               # what is measured so far is kept
                with open(a.out, "w") as f:
                    json.dump(recs, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
