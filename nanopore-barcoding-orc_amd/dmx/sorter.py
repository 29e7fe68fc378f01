"""The similarity pass of the amplicon-sorting stage (scripts/03_amplicon_sorter.sh:163-167,
`amplicon_sorter.py -ar -np N`) on the GPU: read selection, pair generation and the pairwise
identity lines, restated from scripts/auxiliary_code/amplicon_sorter.py (:550-623 selection,
:648-716 pairs, :225-235 + :777-808 identities) on top of dmx_pairdist (include/dmx.h).

Clustering, species grouping and consensus building are NOT replaced: this module stops at the
similarity lines (`i:j:iden`, `i:j:iden:reverse`) the reference's later steps read.  The random
selection modes (-ra, -a) are out of scope.  Alphabet: A, C, G, T, N (a read with any other
byte is refused; the reference would compare such bytes literally).

gapped() restates one iteration of create_alignment (:340-355) on a path of dmx_pairalign: the
two gapped rows a read and a fresh, ungapped consensus get.  The loop over the reads of a group
is NOT restated: the reference aligns read k against a consensus list that has already
received the '-' gaps of reads 0..k-1 (`z.insert(i, '-')` edits the target in place, it is
alignlist[0]), so a group's alignments are sequential and their targets hold a symbol that is
not in the packed batch.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import lib
from .lib import DmxError

GROUP = 1000   # reads per comparison group (amplicon_sorter.py:571, :615-622)


def usable(lengths, minlength: int = 300, maxlength=None) -> np.ndarray:
    """Indices of the reads that pass the length filter (:550-555), in input order."""
    ln = np.asarray(lengths, dtype=np.int64)
    keep = ln >= int(minlength)
    if maxlength is not None:
        keep &= ln <= int(maxlength)
    return np.flatnonzero(keep)


def select_groups(lengths, minlength: int = 300, maxlength=None, maxreads: int = 10000,
                  allreads: bool = False) -> list:
    """The non-random read selection (:550-623): groups of indices into the length-filtered
    list.  Fewer than 1000 usable reads: one group of all of them; otherwise the first
    `maxreads` usable reads in consecutive groups of 1000, the remainder last.  With `allreads`,
    maxreads becomes the number of usable reads when that is at most maxreads."""
    total = len(usable(lengths, minlength, maxlength))
    if total < 5:
        raise DmxError("number of usable sequences is lower than 5")
    maxreads = int(maxreads)
    if allreads and total <= maxreads:
        maxreads = total
    if total < GROUP:
        return [np.arange(total, dtype=np.int64)]
    take = max(0, min(maxreads, total))
    return [np.arange(n, min(n + GROUP, take), dtype=np.int64) for n in range(0, take, GROUP)]


def pairs(groups, lengths):
    """Every compared pair, in the reference's order (:669-683): within each group a stable
    sort by length, then every ordered pair (shorter first) except where
    len(short) * 1.05 < len(long) in double arithmetic.  `lengths` are those of the
    length-filtered list the groups index.  Returns (short, long) index arrays."""
    ln = np.asarray(lengths, dtype=np.int64)
    qs, ts = [], []
    for g in groups:
        g = np.asarray(g, dtype=np.int64)
        order = g[np.argsort(ln[g], kind="stable")]
        sl = ln[order].astype(np.float64)
        # the lengths are ascending, so the partners of position p are p + 1 .. end[p] - 1:
        # those whose length is <= sl[p] * 1.05, the same double product the reference forms
        end = np.searchsorted(sl, sl * 1.05, side="right")
        pos = np.arange(len(order))
        cnt = np.maximum(end - (pos + 1), 0)
        tot = int(cnt.sum())
        if not tot:
            continue
        first = np.repeat(pos, cnt)
        start = np.cumsum(cnt) - cnt
        second = np.arange(tot) - np.repeat(start, cnt) + first + 1
        qs.append(order[first])
        ts.append(order[second])
    if not qs:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(qs), np.concatenate(ts)


def identity(d: int, length: int) -> float:
    """distance()'s identity (:234): Python's round, not numpy's."""
    return round(1 - d / length, 3)


def identity_cap(length: int, threshold: float) -> int:
    """The largest edit distance d whose identity(d, length) is still >= threshold (-1: none).
    The identity never grows with d, so one estimate and a short walk find it."""
    length = int(length)
    if not identity(0, length) >= threshold:
        return -1
    d = min(max(int(length * (1 - threshold)), 0), length)
    while d > 0 and not identity(d, length) >= threshold:
        d -= 1
    while d < length and identity(d + 1, length) >= threshold:
        d += 1
    return d


def gapped(query, target, ops):
    """One iteration of create_alignment (:340-355) for a fresh, ungapped consensus `target`
    and the read `query`, from the path `ops` of query against target (lib.pairalign): the
    consensus row with a '-' wherever the read inserts (I), and the read's row with a '-'
    wherever it deletes (D).  Both rows have len(ops) columns.  Returns (target_row,
    query_row) as str."""
    q = query.decode("ascii") if isinstance(query, (bytes, bytearray)) else str(query)
    t = target.decode("ascii") if isinstance(target, (bytes, bytearray)) else str(target)
    a = np.asarray(ops, dtype=np.uint8)
    takes_q = a != lib.PA_DELETE
    takes_t = a != lib.PA_INSERT
    if int(takes_q.sum()) != len(q) or int(takes_t.sum()) != len(t):
        raise DmxError("gapped: the path does not span the query and the target")
    qi = np.cumsum(takes_q) - 1
    ti = np.cumsum(takes_t) - 1
    qrow = np.where(takes_q, np.frombuffer((q or "-").encode(), dtype=np.uint8)[np.maximum(qi, 0)],
                    ord("-")).astype(np.uint8)
    trow = np.where(takes_t, np.frombuffer((t or "-").encode(), dtype=np.uint8)[np.maximum(ti, 0)],
                    ord("-")).astype(np.uint8)
    return trow.tobytes().decode(), qrow.tobytes().decode()


def _clean(reads) -> list:
    out = []
    for i, r in enumerate(reads):
        b = r.encode("ascii", "replace") if isinstance(r, str) else bytes(r)
        b = b.upper()
        if b.translate(None, b"ACGTN"):
            raise DmxError(f"read {i} has a byte outside ACGTN (the similarity pass supports "
                           "A, C, G, T and N only)")
        out.append(b)
    return out


def similarity(ctx, reads, similar_genes: float = 80.0, minlength: int = 300, maxlength=None,
               maxreads: int = 10000, allreads: bool = False, out=None) -> list:
    """The similarity pass (:777-808) over `reads` (str or bytes): the lines `i:j:iden` for
    pairs whose forward identity is >= similar_genes / 100, and `i:j:iden:reverse` for pairs
    whose forward identity is below 0.5 and whose identity against the reverse complement of
    the longer read is >= similar_genes / 100; i, j index the length-filtered reads, shorter
    first.  Lines come in pair-generation order (the reference's workers interleave theirs) and
    are written to `out` (a path) when given."""
    seqs = _clean(reads)
    idx = usable([len(s) for s in seqs], minlength, maxlength)
    groups = select_groups([len(s) for s in seqs], minlength, maxlength, maxreads, allreads)
    seqs = [seqs[i] for i in idx]
    ln = np.array([len(s) for s in seqs], dtype=np.int64)
    if len(ln) and int(ln.max()) > lib.PD_MAX_LEN:
        raise DmxError(f"a read is longer than {lib.PD_MAX_LEN} nt (pass maxlength)")
    q, t = pairs(groups, ln)
    lines = []
    if len(q):
        sg = similar_genes / 100
        # the two caps once per distinct length of the longer read, by the reference's own
        # expression; the decisions below are integer comparisons against them
        cap_half = np.full(int(ln.max()) + 1, -1, dtype=np.int64)
        cap_sg = np.full(int(ln.max()) + 1, -1, dtype=np.int64)
        for L in np.unique(ln[t]):
            cap_half[L] = identity_cap(int(L), 0.5)
            cap_sg[L] = identity_cap(int(L), sg)
        blob = np.frombuffer(b"".join(seqs), dtype=np.uint8)
        offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
        ctx.load(lib.pack(blob, offs, ln.astype(np.uint32)))
        lt = ln[t]
        # the exact distance is needed wherever the identity is >= 0.5 or >= sg
        fcap = np.maximum(np.maximum(cap_half[lt], cap_sg[lt]), 0).astype(np.uint32)
        df = ctx.pairdist(q, t, lib.PD_NW, caps=fcap).astype(np.int64)
        plain = df <= cap_sg[lt]
        need_rc = ~plain & (df > cap_half[lt]) & (cap_sg[lt] >= 0)
        rcs = np.flatnonzero(need_rc)
        dr = np.zeros(0, dtype=np.int64)
        if len(rcs):
            dr = ctx.pairdist(q[rcs], t[rcs], lib.PD_NW,
                              flags=np.full(len(rcs), lib.PD_RC, dtype=np.uint8),
                              caps=cap_sg[lt[rcs]].astype(np.uint32)).astype(np.int64)
        rev = np.zeros(len(q), dtype=bool)
        dist = df.copy()
        hit = dr <= cap_sg[lt[rcs]]
        rev[rcs[hit]] = True
        dist[rcs[hit]] = dr[hit]
        for k in np.flatnonzero(plain | rev):
            iden = identity(int(dist[k]), int(lt[k]))
            lines.append(f"{q[k]}:{t[k]}:{iden}" + (":reverse" if rev[k] else ""))
    if out is not None:
        with open(out, "w") as f:
            f.write("".join(x + "\n" for x in lines))
    return lines


def read_sequences(path: str) -> list:
    """Every record's sequence of a FASTQ/FASTA(.gz) file, through the native reader."""
    from . import nio
    seqs = []
    with nio.Reader(path) as rd:
        for b in rd:
            seqs.extend(b.sequence(i) for i in range(len(b)))
            b.free()
    return seqs


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(
        prog="dmx-similarity",
        description="The similarity pass of amplicon_sorter.py (pairwise identities of one "
                    "bin's reads) on the GPU; clustering and consensus stay with the reference.")
    ap.add_argument("-i", "--input", required=True, help="bin in FASTQ/FASTA, optionally .gz")
    ap.add_argument("-o", "--output", required=True, help="similarity lines (i:j:iden[:reverse])")
    ap.add_argument("-min", "--minlength", type=int, default=300)
    ap.add_argument("-max", "--maxlength", type=int, default=None)
    ap.add_argument("-maxr", "--maxreads", type=int, default=10000)
    ap.add_argument("-ar", "--allreads", action="store_true")
    ap.add_argument("-sg", "--similar_genes", type=float, default=80.0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        reads = read_sequences(a.input)
        with lib.Context(a.device) as ctx:
            lines = similarity(ctx, reads, a.similar_genes, a.minlength, a.maxlength, a.maxreads,
                               a.allreads, out=a.output)
    except (DmxError, OSError, ValueError) as e:
        print(f"dmx-similarity: {e}", file=sys.stderr)
        return 1
    print(f"dmx-similarity: {len(reads)} reads, {len(lines)} similarity lines -> {a.output}",
          file=sys.stderr)
    return 0
