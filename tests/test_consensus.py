"""sorter.consensus (create_consensus of amplicon_sorter.py:358-428 on dmx_groupalign; DESIGN.md
§8g) against an in-test model of the whole loop, whose alignment step is the model of
groupalign_cases.py: rows as lists, a tally per column in row order, Python's stable sorts."""
import functools

import numpy as np
import pytest

import groupalign_cases as gc
import pairdist_cases as pc
from dmx import lib, sorter


def model_homopolymer(cols):
    out, run = [], [cols[0]]
    for x in cols[1:]:
        if x[0][0] == run[0][0][0]:
            run.append(x)
        else:
            run.sort(key=lambda e: int(e[0][1]), reverse=True)
            out += run
            run = [x]
    return out + run          # the last run is not sorted


def model_consensus(reads):
    reads = sorted((r.decode() for r in reads), key=len, reverse=True)
    everyone = list(reads)
    cons, rest = reads[0], reads[1:]
    for thr in (0.45, 0.15, 0.5):
        rows, _, _ = gc.model_alignment(cons, rest)
        c = len(rows)
        cols = []
        for y in range(len(rows[0])):
            tally = {}
            for z in rows:
                if z[y] != "-":
                    tally[z[y]] = tally.get(z[y], 0) + 1
            ranked = sorted(tally.items(), key=lambda kv: int(kv[1]), reverse=True)
            if ranked and ranked[0][1] > c * 0.10:
                cols.append(ranked[:2])
        cols = model_homopolymer(cols)
        cons = "".join(x[0][0] for x in cols if x[0][1] > c * thr)
        rest = everyone
    out, b = [], 1
    for n, x in enumerate(cols):
        sym, cnt = x[0]
        before = cols[n - 1][0]
        if sym == before[0]:
            if sym in ("A", "T"):
                if (cnt > c * 0.2) if b >= 4 else (cnt > c * thr):
                    out.append(sym)
                    b += 1
            elif sym in ("C", "G"):
                if (before[1] * 0.5 < cnt > c * 0.2) if b >= 3 else (cnt > c * thr):
                    out.append(sym)
                    b += 1
        elif cnt > c * thr:
            out.append(sym)
            b = 1
    return "".join(out)


def family(rng, n):
    """A sequence of about n nt with homopolymer runs of 3..8 every 10..30 nt, no N."""
    out = bytearray()
    while len(out) < n:
        out += pc.rand_seq(rng, int(rng.integers(10, 31)), p_n=0.0)
        out += bytes([b"ACGT"[rng.integers(4)]]) * int(rng.integers(3, 9))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def cases():
    """Six groups of 5..12 reads of 150..400 nt from two families, a group of four reads with
    a column where the two top symbols tie, and five error-free copies.  Returns (reads, groups,
    the model's consensus per group)."""
    rng = np.random.default_rng(91)
    fam = [family(rng, 400), family(rng, 260)]
    reads, groups = [], []
    for k in range(6):
        f = fam[k % 2]
        cut = f[:int(rng.integers(150, len(f) + 1))]
        g = []
        for _ in range(int(rng.integers(5, 13))):
            g.append(len(reads))
            reads.append(pc.mutate(rng, cut, float(rng.uniform(0.03, 0.12)))[:400])
        groups.append(g)
    # the tie: T, C, C, T in one column of four reads of one length.  Cycle 1 counts T twice
    # (row 0 and the last read) and C twice; T was seen first, so it seeds cycle 2 and wins
    x, y = pc.rand_seq(rng, 40, p_n=0.0), pc.rand_seq(rng, 40, p_n=0.0)
    groups.append(list(range(len(reads), len(reads) + 4)))
    reads += [x + b"T" + y, x + b"C" + y, x + b"C" + y, x + b"T" + y]
    groups.append(list(range(len(reads), len(reads) + 5)))
    reads += [fam[1]] * 5
    return reads, groups, [model_consensus([reads[i] for i in g]) for g in groups]


def test_consensus_on_the_host_reference_equals_the_model():
    reads, groups, exp = cases()
    got = sorter.consensus(None, reads, groups)
    assert got == exp
    tie = reads[groups[6][0]].decode()
    assert got[6] == tie and tie[40] == "T"        # first occurrence decided, not the symbol order
    assert got[7] == reads[groups[7][0]].decode()  # error-free copies: the sequence itself
    assert sorter.consensus(None, reads, []) == []
    # str input, one group, one thread
    assert sorter.consensus(None, [r.decode() for r in reads], groups[:1], n_threads=1) == exp[:1]


def test_consensus_refusals():
    reads, groups, _ = cases()
    with pytest.raises(lib.DmxError, match="-amb"):
        sorter.consensus(None, reads, groups, ambiguous=True)
    with pytest.raises(lib.DmxError, match="group 1 has no reads"):
        sorter.consensus(None, reads, [groups[0], []])
    with pytest.raises(lib.DmxError, match="outside ACGTN"):
        sorter.consensus(None, [b"ACGR", b"ACGT"], [[0, 1]])


@pytest.mark.gpu
def test_consensus_on_the_gpu_equals_the_model(ctx):
    reads, groups, exp = cases()
    assert sorter.consensus(ctx, reads, groups) == exp
    st = ctx.groupalign_stats()
    assert st["rounds"] == max(len(g) for g in groups) and st["merge"] > 0
