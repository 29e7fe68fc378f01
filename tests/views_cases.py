"""Cases for the view runs (dmx_set_views / dmx_chop_views): a seeded
generator of reads and view lists per stratum, a Python model of pychopper's PASS rule and of
view composition, and the two references of tests/test_views.py:

  (a) the CPU oracle on the extracted, oriented view strings (oracle.run_batch; the Python
      oracle of ends_cases for panels with restricted adapters);
  (b) the merged path: the same strings packed as reads of their own and run whole.

Run as a program it is the bounds pass: strata M, B and E on the library DMX_DEBUG_BOUNDS
selects, one JSON line (tests/test_views.py runs it in a child process)."""
from __future__ import annotations

import functools
import json
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "nanopore-barcoding-orc_amd"), os.path.join(ROOT, "oracle"),
           os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle  # noqa: E402  (checker)
import ends_cases as ec  # noqa: E402
import sweep_cases as sw  # noqa: E402
from dmx import lib, synth  # noqa: E402

SEED = 31755
MIN_OVERLAP = 3
COMP = str.maketrans("ACGTN", "TGCAN")


def revcomp(s: str) -> str:
    return s.translate(COMP)[::-1]


# ---- the Python models ----------------------------------------------------------------------

def pass_model(nseg, segs, qc_ok, min_len):
    """pychopper's PASS rule (dmx/chop.py, Reorienter.batch) in plain Python: read r gives its
    segment iff it has exactly one, qc_ok is None or qc_ok[r], and stop - start >= min_len."""
    out, si = [], 0
    for r, ns in enumerate(nseg):
        if ns == 1 and (qc_ok is None or qc_ok[r]):
            g = segs[si]
            if int(g["stop"]) - int(g["start"]) >= min_len:
                out.append((r, int(g["start"]), int(g["stop"]), 1 if g["strand"] else 0))
        si += int(ns)
    return out


def extract(reads, views):
    """The oriented view strings: read[start:stop], reverse-complemented on strand 1."""
    out = []
    for r, a, b, st in zip(*views):
        s = reads[int(r)][int(a):int(b)]
        out.append(revcomp(s) if st else s)
    return out


def compose(start, stop, strand, a, b, o):
    """Sub-range [a, b) of orient(V, o), V = orient(read[start:stop], strand), as (start, stop,
    strand) on the read: the rule the finalize kernels apply to build round 1's view."""
    t = strand ^ o
    return (stop - b, stop - a, t) if t else (start + a, start + b, t)


def counts_of(res, a0, a1, two_round):
    """dmx_counts of a result array: (bin1, bin2) bins, then the RC counts of both rounds."""
    n1 = a1 + 1 if two_round else 1
    out = np.zeros((a0 + 1) * n1 + 2, dtype=np.uint64)
    b1 = res["bin1"].astype(np.int64) + 1
    b2 = res["bin2"].astype(np.int64) + 1 if two_round else np.zeros(len(res), np.int64)
    np.add.at(out, b1 * n1 + b2, 1)
    out[-2] = int((res["rc1"] == 1).sum())
    out[-1] = int(((res["rc2"] == 1) & (res["bin1"] >= 0)).sum()) if two_round else 0
    return out


def view_arrays(views):
    v = list(views)
    return (np.array([x[0] for x in v], np.uint32), np.array([x[1] for x in v], np.int32),
            np.array([x[2] for x in v], np.int32), np.array([x[3] for x in v], np.uint8))


# ---- panels and reads ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bench_panels():
    d = synth.generate("c1", n=1)
    return list(d["sp5"]), list(d["sp27"])


def demux_reads(rng, n, sp5, sp27, lo=150, hi=600):
    """Reads of lo..hi nt: flank + an SP5 copy + body + an SP27 copy + flank (copies with up to
    8 % edits, each missing in a fifth of the reads), a third stored reverse-complemented."""
    out = []
    for _ in range(n):
        f = sw.mutate(rng, sp5[int(rng.integers(len(sp5)))], 0.08) if rng.random() < 0.8 else ""
        b = sw.mutate(rng, sp27[int(rng.integers(len(sp27)))], 0.08) if rng.random() < 0.8 else ""
        lf, rf = sw.rand_seq(rng, rng.integers(0, 30)), sw.rand_seq(rng, rng.integers(0, 30))
        body = max(1, int(rng.integers(lo, hi + 1)) - len(f) - len(b) - len(lf) - len(rf))
        s = lf + f + sw.rand_seq(rng, body) + b + rf
        out.append(revcomp(s) if rng.random() < 0.33 else s)
    return out


@dataclass
class Case:
    name: str
    reads: list
    views: tuple            # (read, start, stop, strand) arrays
    r0: tuple               # (seqs, wheres, rc, e, overlap), ends_cases' convention
    r1: tuple | None = None

    @property
    def two_round(self):
        return self.r1 is not None

    @property
    def restricted(self):
        return any(w not in (ec.F, ec.B) for r in (self.r0, self.r1) if r for w in r[1])

    def packed(self):
        return lib.pack(*oracle.pack_ascii(self.reads))

    def strings(self):
        return extract(self.reads, self.views)

    def set_panels(self, ctx):
        for rnd, r in enumerate((self.r0, self.r1)):
            if r is None:
                continue
            s, w, rc, e, o = r
            if len(set(w)) == 1 and w[0] in (ec.F, ec.B):   # the benchmark's path
                ctx.set_panel(rnd, s, w[0] | (lib.DMX_RC if rc else 0), e, o)
            else:
                ctx.set_panel_ex(rnd, s, w, rc, e, o)
        ctx.set_mode(lib.MODE_TWO_ROUND if self.two_round else lib.MODE_SINGLE)

    def n_adapters(self):
        return len(self.r0[0]), len(self.r1[0]) if self.r1 else 0

    def expected(self) -> np.ndarray:
        """(a): the oracle on the extracted strings."""
        if getattr(self, "_exp", None) is None:
            strs = self.strings()
            if self.restricted:
                if self.r1 is None:
                    s, w, rc, e, o = self.r0
                    self._exp = ec.demux(s, w, strs, rc, e, o)
                else:
                    self._exp = ec.two_round_expected(strs, self.r0, self.r1, ec.demux)
            else:
                def pan(r):
                    s, w, _, e, o = r
                    return oracle.Panel(s, [oracle.FRONT if x == ec.F else oracle.BACK for x in w],
                                        max_errors=e, min_overlap=o)
                blob, offs, lens = oracle.pack_ascii(strs)
                self._exp = oracle.run_batch(pan(self.r0), pan(self.r1) if self.r1 else None,
                                             blob, offs, lens, mode=1 if self.r1 else 0,
                                             use_rc=self.r0[2], threads=8)
        return self._exp


def _bench_rounds(two=True):
    sp5, sp27 = bench_panels()
    r0 = (sp5, [ec.F] * len(sp5), True, 0.1, MIN_OVERLAP)
    r1 = (sp27, [ec.B] * len(sp27), True, 0.1, MIN_OVERLAP)
    return r0, (r1 if two else None)


def _rand_views(rng, reads, n, shuffle=True):
    idx = rng.integers(0, len(reads), size=n) if shuffle else np.arange(n) % len(reads)
    out = []
    for r in idx:
        L = len(reads[int(r)])
        a = int(rng.integers(0, L + 1))
        b = int(rng.integers(a, L + 1))
        if rng.random() < 0.5:
            a, b = (0, b) if rng.random() < 0.5 else (a, L)
        out.append((int(r), a, b, int(rng.integers(2))))
    return out


STRATA = ("I", "M", "S", "Z", "B", "Bb", "O", "E", "G", "N", "R")


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    rng = np.random.default_rng([SEED, STRATA.index(name)])
    sp5, sp27 = bench_panels()
    r0, r1 = _bench_rounds()
    if name == "I":      # identity views: the plain whole-read run of the same batch
        reads = demux_reads(rng, 400, sp5, sp27)
        return Case(name, reads, view_arrays((i, 0, len(s), 0) for i, s in enumerate(reads)), r0, r1)
    if name == "M":      # three views per read: more views than reads
        reads = demux_reads(rng, 300, sp5, sp27)
        v = []
        for i, s in enumerate(reads):
            L = len(s)
            v += [(i, 0, L // 2, 0), (i, L // 4, 3 * L // 4, 1), (i, L // 3, L, 0)]
        return Case(name, reads, view_arrays(v), r0, r1)
    if name == "S":      # fewer views than reads, shuffled, one listed twice
        reads = demux_reads(rng, 500, sp5, sp27)
        v = _rand_views(rng, reads, 199)
        v.insert(77, v[3])
        return Case(name, reads, view_arrays(v), r0, r1)
    if name == "Z":      # views of 0, 1, min_overlap - 1, min_overlap nt: the tail of an SP5 copy
        reads, v = [], []
        for i in range(160):
            ad = sp5[i % len(sp5)]
            lf = sw.rand_seq(rng, 20 + i % 50)
            s = lf + ad + sw.rand_seq(rng, 150)
            n = (0, 1, MIN_OVERLAP - 1, MIN_OVERLAP)[i % 4]
            stored = revcomp(s) if i % 8 >= 4 else s
            p = len(lf) + len(ad) - n           # the last n nt of the copy, on the oriented read
            a, b = (len(s) - p - n, len(s) - p) if i % 8 >= 4 else (p, p + n)
            reads.append(stored)
            v.append((i, a, b, 1 if i % 8 >= 4 else 0))
        return Case(name, reads, view_arrays(v), r0, r1)
    if name == "B":      # 5' copies across the view boundary
        reads, v = [], []
        for i in range(240):
            ad = sp5[i % len(sp5)]
            m = len(ad)
            lf = sw.rand_seq(rng, 120 + i % 40)
            s = lf + ad + sw.rand_seq(rng, 200)
            p = len(lf)
            k = i % 4
            if k == 0:    # half of the copy inside the view's start
                a, b = p + m // 2, len(s)
            elif k == 1:  # the copy just before the view: only what the oracle finds inside
                a, b = p + m, len(s)
            elif k == 2:  # the copy just past the view's end
                a, b = p - 100, p
            else:         # all but the copy's first nt
                a, b = p + 1, p + m + 50
            st = (i // 4) % 2
            stored = revcomp(s) if st else s
            if st:
                a, b = len(s) - b, len(s) - a
            reads.append(stored)
            v.append((i, a, b, st))
        return Case(name, reads, view_arrays(v), r0, r1)
    if name == "Bb":     # 3' copies: ending exactly at the view's last nt, cut by it, just outside
        reads, v = [], []
        for i in range(240):
            ad = sp27[i % len(sp27)]
            m = len(ad)
            lf = sw.rand_seq(rng, 150 + i % 40)
            s = lf + ad + sw.rand_seq(rng, 120)
            p = len(lf)
            k = i % 4
            a, b = ((p - 100, p + m), (p - 100, p + m // 2), (p - 100, p), (p + m, len(s)))[k]
            st = (i // 4) % 2
            stored = revcomp(s) if st else s
            if st:
                a, b = len(s) - b, len(s) - a
            reads.append(stored)
            v.append((i, a, b, st))
        return Case(name, reads, view_arrays(v), (sp27, [ec.B] * len(sp27), True, 0.1, MIN_OVERLAP))
    if name == "O":      # round 1 takes the reverse orientation of a strand-1 view
        reads, v = [], []
        for i in range(200):
            f = sw.mutate(rng, sp5[i % len(sp5)], 0.05)
            b = sw.mutate(rng, sp27[i % len(sp27)], 0.05)
            body = sw.rand_seq(rng, 150 + i % 200)
            oriented = f + revcomp(body + b) if i % 3 else f + body + b
            lf, rf = sw.rand_seq(rng, 10 + i % 7), sw.rand_seq(rng, 5 + i % 11)
            reads.append(lf + revcomp(oriented) + rf)
            v.append((i, len(lf), len(lf) + len(oriented), 1))
        return Case(name, reads, view_arrays(v), r0, r1)
    if name == "E":      # ^A, XA then A$, AX on views strictly inside their reads
        a0 = [sw.rand_seq(rng, 24) for _ in range(3)]
        a1 = [sw.rand_seq(rng, 20) for _ in range(3)]
        e0 = (a0, [ec.PREFIX, ec.FRONTX, ec.F], True, 0.1, MIN_OVERLAP)
        e1 = (a1, [ec.SUFFIX, ec.BACKX, ec.B], True, 0.1, MIN_OVERLAP)
        reads, v = [], []
        for i in range(180):
            x, y = a0[i % 3], a1[(i // 3) % 3]
            if i % 5 == 1:
                x = sw.mutate(rng, x, 0.08)
            if i % 7 == 2:
                y = sw.mutate(rng, y, 0.08)
            cut0 = (0, 0, 5, 9)[i % 4]     # the view starts inside the 5' copy (XA: a partial one)
            cut1 = (0, 4, 0, 7)[(i // 2) % 4]
            inner = x + sw.rand_seq(rng, 150 + i % 90) + y
            lf, rf = sw.rand_seq(rng, 30 + i % 13), sw.rand_seq(rng, 40 + i % 9)
            s = lf + inner + rf
            a, b = len(lf) + cut0, len(lf) + len(inner) - cut1
            st = i % 2
            stored = revcomp(s) if st else s
            if st:
                a, b = len(s) - b, len(s) - a
            reads.append(stored)
            v.append((i, a, b, st))
        return Case(name, reads, view_arrays(v), e0, e1)
    if name == "G":      # 5,000 views: more than one scan block, across a 2048-task sort group
        reads = demux_reads(rng, 2500, sp5, sp27, 150, 400)
        return Case(name, reads, view_arrays(_rand_views(rng, reads, 5000, shuffle=False)), r0, r1)
    if name == "N":      # no views: a valid run with no results
        reads = demux_reads(rng, 50, sp5, sp27)
        return Case(name, reads, view_arrays([]), r0, r1)
    if name == "R":      # one random IUPAC panel of the sweep generator (the first it accepts)
        for k in range(40):
            prng = np.random.default_rng([SEED, 900 + k])
            pan = sw.random_panel(prng)
            if len(pan) >= 4 and lib.panel_reach(pan, lib.DMX_FRONT | lib.DMX_RC, 0.1, 3)[0] == 0:
                break
        reads = sw.reads_for(rng, pan, 400, maxlen=600, plant_lo=1)
        reads = [s if len(s) >= 150 else s + sw.rand_seq(rng, 150 - len(s)) for s in reads]
        return Case(name, reads, view_arrays(_rand_views(rng, reads, 600)),
                    (pan, [ec.F] * len(pan), True, 0.1, 3))
    raise KeyError(name)


def differing(got, exp):
    assert got.dtype.itemsize == exp.dtype.itemsize == 40
    g = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), 40)
    e = np.ascontiguousarray(exp).view(np.uint8).reshape(len(exp), 40)
    return np.nonzero((g != e).any(axis=1))[0]


def run_views(ctx, c: Case):
    """(results, counts, flags) of the view run of case c on ctx."""
    c.set_panels(ctx)
    ctx.load(c.packed())
    ctx.set_views(*c.views)
    ctx.exec()
    return ctx.fetch(), ctx.counts(), ctx.stats()["flags"]


def run_merged(ctx, c: Case):
    """(b): the view strings packed as reads of their own, run whole."""
    c.set_panels(ctx)
    strs = c.strings()
    if not strs:
        return np.zeros(0, dtype=lib.RESULT_DTYPE)
    return ctx.run(lib.pack(*oracle.pack_ascii(strs)))


def main():
    out = {"lib": os.path.basename(lib.LIB_PATH), "cases": {}}
    with lib.Context(0) as ctx:
        for name in ("M", "B", "E"):
            c = case(name)
            try:
                got, _, flags = run_views(ctx, c)
                out["cases"][name] = [int(len(differing(got, c.expected()))), len(got), flags, ""]
            except lib.DmxError as e:
                out["cases"][name] = [-1, 0, 0, str(e)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
