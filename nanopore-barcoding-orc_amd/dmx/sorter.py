"""The similarity pass of the amplicon-sorting stage (scripts/03_amplicon_sorter.sh:163-167,
`amplicon_sorter.py -ar -np N`) on the GPU: read selection, pair generation and the pairwise
identity lines, restated from scripts/auxiliary_code/amplicon_sorter.py (:550-623 selection,
:648-716 pairs, :225-235 + :777-808 identities) on top of dmx_pairdist (include/dmx.h).

similarity() stops at the similarity lines (`i:j:iden`, `i:j:iden:reverse`); gene_groups() goes
on to what update_list (:983-1034) and merge_groups (:1058-1087) make of them, the gene groups,
on dmx_pairhits / dmx_hitgroups, without forming the lines.
comp_consensus_groups() and compare_consensus() restate the two merge loops (:1231-1334,
:1857-1958) on dmx_rowhits (consensus against consensus, HW, both strands), with
the first reads of a group in index order where the reference samples at random.
estimate_ssg() and species_groups() restate SSG (:810-836) and the first half of read_indexes
(:1363-1411) on dmx_hithist / dmx_pairhits_cross / dmx_hitgroups_within.
assign_best() is one pass of process_consensuslist / similarity_species / update_groups
(:1628-1755) as one dmx_rowassign call (pairs, decision and best line per read
inside the call), rest_reads() the loop around it (:1962-2014), species_consensuses() the second
half of read_indexes (:1431-1456), and sort_species() runs them per gene group.  NOT replaced:
that random sampling and the .group / results files.  finetune() restates finetune (:838-965)
with the first reads in order where the reference samples; it runs as rest_reads'
hook when asked for (dmx-similarity --finetune) and stays with the reference otherwise.  The
random selection modes (-ra, -a) are out of scope.  Alphabet: A, C, G, T, N (a read with any other byte is refused;
the reference would compare such bytes literally).

consensus() restates create_consensus (:358-428) for many groups at once on top of
dmx_groupalign, which runs create_alignment's loop (:324-356) in lock-step
over the groups and returns per-column symbol counts, all the consensus reads of an alignment.
alignment_rows() rebuilds the gapped rows themselves from the returned paths (the -aln output,
and the tests).  orient() restates consensus_direction (:1826-1838) on dmx_pairdist, and
make_consensus() is make_consensus (:1089-1105): orient(), then consensus() with every read's
strand passed to dmx_groupalign_strands, so that gene groups, which mix both orientations, go
straight into the alignment on one resident batch.  Out of scope: -amb (ambiguity, degenerate)
and the callers' random sampling.
"""
from __future__ import annotations

import argparse
import functools
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
    query_row) as str.  The loop over a group's reads, where read k meets a row that already
    carries the gaps of reads 0..k-1, is alignment_rows() on the paths of lib.groupalign."""
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


def alignment_rows(seed, reads, ops) -> list:
    """The gapped rows of create_alignment (:324-356): row 0 is `seed` (str or bytes, '-' and
    IUPAC allowed), row k + 1 is reads[k]; ops[k] is read k's path against row 0 as it stood
    (a slice of groupalign's ops).  A DELETE puts '-' into the read's row; every INSERT column
    becomes a '-' column of row 0 and of every earlier row.  Returns the rows as str, all of
    the last path's length."""
    def raw(x):
        return np.frombuffer(x.encode("ascii") if isinstance(x, str) else bytes(x), dtype=np.uint8)
    if len(reads) != len(ops):
        raise DmxError("alignment_rows: one path per read")
    rows = [raw(seed).copy()]
    for r, path in zip(reads, ops):
        a = np.asarray(path, dtype=np.uint8)
        q = raw(r)
        takes_q = a != lib.PA_DELETE
        takes_t = a != lib.PA_INSERT
        if int(takes_q.sum()) != len(q) or int(takes_t.sum()) != len(rows[0]):
            raise DmxError("alignment_rows: a path does not span its read and the row it met")
        for k, old in enumerate(rows):
            new = np.full(len(a), ord("-"), dtype=np.uint8)
            new[takes_t] = old
            rows[k] = new
        new = np.full(len(a), ord("-"), dtype=np.uint8)
        new[takes_q] = q
        rows.append(new)
    return [x.tobytes().decode() for x in rows]


THRESHOLDS = (0.45, 0.15, 0.5)   # create_consensus's three cycles (:365)
_SYMS = "ACGTN"


def _column_tops(res, g, n_rows):
    """The kept columns of group g's alignment (:372-384): for every column whose most frequent
    symbol is shown by more than 10 % of the rows, that symbol and its count (and the runner-up's,
    which only -amb reads).  Row 0's own symbol counts, before any member's; ties go to the
    symbol seen first down the rows (the reference's stable sort over dict insertion order)."""
    lo, hi = int(res["col_off"][g]), int(res["col_off"][g + 1])
    cnt = res["count"][lo:hi].astype(np.int64)
    rank = res["first"][lo:hi].astype(np.int64)
    rank[cnt == 0] = 1 << 30
    mask = res["mask"][lo:hi]
    for c in range(5):   # row 0 shows a symbol where its mask is that symbol's bit alone
        own = mask == (1 << c)
        cnt[own, c] += 1
        rank[own, c] = 0
    # falling count, then rising first occurrence (places are below 65536)
    order = np.argsort(-cnt * 65536 + np.minimum(rank, 65535), axis=1, kind="stable")
    top = order[:, 0]
    top_n = np.take_along_axis(cnt, order[:, :1], axis=1)[:, 0]
    keep = (top_n > 0) & (top_n > n_rows * 0.10)
    return top[keep], top_n[keep]


def _homopolymer_sort(top, top_n):
    """homopolymersort (:244-257): within every run of columns with the same top symbol, the
    columns by falling count (stable); the last run stays as it is, as in the reference."""
    if not len(top):
        raise DmxError("consensus: no column of the alignment is kept")
    run = np.concatenate([[0], np.cumsum(top[1:] != top[:-1])])
    key = np.where(run == run[-1], 0, -top_n)
    order = np.lexsort((key, run))
    return top[order], top_n[order]


def _final_correction(top, top_n, c, treshold):
    """The homopolymer correction of :394-428, literally (the entry before the first is the
    last one; `treshold` is still the last cycle's)."""
    out = []
    b = 1
    n_cols = len(top)
    for n in range(n_cols):
        sym, cnt = _SYMS[top[n]], int(top_n[n])
        prev = (n - 1) % n_cols
        if top[n] == top[prev]:
            if sym in "AT":
                if b >= 4:
                    if cnt > c * 0.2:
                        out.append(sym)
                        b += 1
                elif cnt > c * treshold:
                    out.append(sym)
                    b += 1
            elif sym in "CG":
                if b >= 3:
                    if int(top_n[prev]) * 0.5 < cnt > c * 0.2:
                        out.append(sym)
                        b += 1
                elif cnt > c * treshold:
                    out.append(sym)
                    b += 1
        elif cnt > c * treshold:
            out.append(sym)
            b = 1
    return "".join(out)


_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(seq: bytes) -> bytes:
    """compl_reverse (:237-242) over A/C/G/T/N: backwards, complemented, N stays."""
    return seq[::-1].translate(_RC)


_NOT_ACGT = bytes(c for c in range(256) if c not in b"ACGT")


class Operands:
    """Reads that are already on the GPU: operands of the batch resident in `ctx` (DESIGN.md
    §3.18), to be passed wherever the functions here take `reads`.  The functions then skip
    clean, pack and load: they select by the operands' lengths, set the selected operands as the
    context's table and run on the resident batch, with the results they return for the list of
    the operands' sequences.
    Operands(ctx, seqs_source) takes the context's current table (Context.result_operands or
    set_operands); a slice is the operands of that range, so with bin_first of result_operands
    `ops.bin(bin_first, b)` is well b and indices are local to it.  seqs_source is the host copy
    of the batch: read r's bases are seqs_source[r] (str or bytes), or seqs_source(r) for a
    callable.  len() is the number of operands; ops[k] the cleaned sequence of operand k (bytes
    over A/C/G/T/N as the packed batch holds it, the sub-range, reverse-complemented on strand
    1), materialised on first use: orient()'s duplicate test and the consensus text need it."""

    def __init__(self, ctx, seqs_source, table=None):
        if ctx is None:
            raise DmxError("Operands need a Context: the host twins run on packed sequences")
        self.ctx, self.source = ctx, seqs_source
        t = ctx.operands() if table is None else table
        self.read = np.ascontiguousarray(t[0], dtype=np.uint32)
        self.start = np.ascontiguousarray(t[1], dtype=np.int32)
        self.stop = np.ascontiguousarray(t[2], dtype=np.int32)
        self.strand = np.ascontiguousarray(t[3], dtype=np.uint8)
        self.lengths = (self.stop - self.start).astype(np.int64)
        self._gen = getattr(ctx, "_load_gen", 0)
        self._seqs = {}

    def __len__(self):
        return len(self.read)

    def subset(self, idx):
        """The operands idx (an index array or a slice), as Operands of their own."""
        sub = Operands(self.ctx, self.source, (self.read[idx], self.start[idx], self.stop[idx],
                                               self.strand[idx]))
        sub._gen = self._gen   # of the batch these operands were made on, not of today's
        return sub

    def bin(self, bin_first, b):
        """Bin b of a table made by Context.result_operands, which returned bin_first."""
        return self.subset(slice(int(bin_first[b]), int(bin_first[b + 1])))

    def __getitem__(self, k):
        if isinstance(k, slice):
            return self.subset(k)
        k = int(k)
        if k < 0:
            k += len(self)
        if k not in self._seqs:
            r = int(self.read[k])
            raw = self.source(r) if callable(self.source) else self.source[r]
            b = raw.encode("ascii", "replace") if isinstance(raw, str) else bytes(raw)
            b = b[int(self.start[k]):int(self.stop[k])].upper()
            b = b.translate(bytes.maketrans(_NOT_ACGT, b"N" * len(_NOT_ACGT)))
            self._seqs[k] = revcomp(b) if self.strand[k] else b
        return self._seqs[k]

    def activate(self):
        """These operands become the context's table: index k of a sorting call is operand k."""
        ctx = self.ctx
        if getattr(ctx, "_load_gen", 0) != self._gen:
            raise DmxError("Operands: another batch was loaded since these operands were made")
        if getattr(ctx, "_resident", None) is not self:
            ctx.set_operands(self.read, self.start, self.stop, self.strand)
            ctx._resident = self   # a list's batch is not resident: its next pass loads again


def _load(ctx, p):
    """The plan's batch into ctx: a packed batch is loaded, Operands become the table."""
    if isinstance(p, Operands):
        p.activate()
    else:
        ctx.load(p)


def _pack_reads(ctx, reads):
    """The cleaned reads, their lengths and their batch, packed once and loaded into ctx (when
    there is one): what orient(), consensus() and make_consensus() run on.  Operands are
    resident: no clean, no pack, no load; their sequences come on demand."""
    if isinstance(reads, Operands):
        if len(reads) and int(reads.lengths.max()) > lib.PD_MAX_LEN:
            raise DmxError(f"a read is longer than {lib.PD_MAX_LEN} nt")
        if ctx is not reads.ctx:
            raise DmxError("Operands run on the Context they were made with")
        reads.activate()
        return reads, reads.lengths, None
    seqs = _clean(reads)
    ln = np.array([len(s) for s in seqs], dtype=np.int64)
    if len(ln) and int(ln.max()) > lib.PD_MAX_LEN:
        raise DmxError(f"a read is longer than {lib.PD_MAX_LEN} nt")
    p = None
    if len(seqs):
        blob = np.frombuffer(b"".join(seqs), dtype=np.uint8)
        offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
        p = lib.pack(blob, offs, ln.astype(np.uint32))
        if ctx is not None:
            ctx.load(p)
    return seqs, ln, p


def _orient(ctx, p, seqs, ln, groups, n_threads):
    """orient() on a batch that is packed (p) and, with a ctx, resident."""
    orders, q, t = [], [], []
    for k, g in enumerate(groups):
        g = np.asarray(g, dtype=np.int64).reshape(-1)
        if len(g) and (int(g.min()) < 0 or int(g.max()) >= len(seqs)):
            raise DmxError(f"orient: group {k} names a read outside the reads")
        o = g[np.argsort(ln[g], kind="stable")] if len(g) else g
        orders.append(o)
        q.append(np.full(max(len(o) - 1, 0), o[0] if len(o) else 0, dtype=np.int64))
        t.append(o[1:])
    q = np.concatenate(q + [np.zeros(0, dtype=np.int64)])
    t = np.concatenate(t + [np.zeros(0, dtype=np.int64)])
    d = np.zeros(0, dtype=np.int64)
    if len(q):   # one call: every (anchor, other) pair forward, then reverse-complemented
        flags = np.concatenate([np.zeros(len(q), dtype=np.uint8),
                                np.full(len(q), lib.PD_RC, dtype=np.uint8)])
        q2, t2 = np.concatenate([q, q]), np.concatenate([t, t])
        d = (ctx.pairdist(q2, t2, lib.PD_NW, flags=flags) if ctx is not None
             else lib.pairdist_host(p, q2, t2, lib.PD_NW, flags=flags, n_threads=n_threads))
        d = d.astype(np.int64)
    members, strands, at = [], [], 0
    for k, o in enumerate(orders):
        mem, st, seen = [], [], set()
        for x, y in enumerate(o):
            turned = 0
            if x:   # distance() divides by the longer read's length: y's (rising lengths)
                iden = identity(int(d[at + x - 1]), int(ln[y]))
                iden_r = identity(int(d[len(q) + at + x - 1]), int(ln[y]))
                turned = 0 if iden > iden_r else 1
            s = revcomp(seqs[y]) if turned else seqs[y]
            if s not in seen and len(o) > 1:   # the anchor enters the set with the first other
                seen.add(s)
                mem.append(int(y))
                st.append(turned)
        at += max(len(o) - 1, 0)
        if len(mem) < 2:
            raise DmxError(f"orient: group {k} has {len(mem)} distinct oriented reads (2 at "
                           "least make a consensus)")
        members.append(np.array(mem, dtype=np.int64))
        strands.append(np.array(st, dtype=np.uint8))
    return members, strands


def orient(ctx, reads, groups, n_threads: int = 16):
    """consensus_direction (:1826-1838) as make_consensus (:1089-1105) calls it, for many groups
    at once.  Per group (indices into `reads`): a stable sort by rising length; the first read
    is the anchor x and stays forward; every other read y stays forward iff
    identity(d(x, y), len(y)) > identity(d(x, rc(y)), len(y)), so a tie turns it round (a
    palindromic read is always turned, into itself).  The distances are one pairdist call over
    all groups (NW, half the pairs with PD_RC); ctx: a Context, or None for lib.pairdist_host.
    The reference collects the oriented sequences in a set: equal oriented byte strings
    collapse here to the first one.  Parity finding: the reference's resulting order is
    Python's string-hash order of that set, which differs from run to run; here it is first
    appearance in the length-sorted list.  A group left with fewer than 2 reads is refused (in
    the reference a one-read group leaves the set empty and create_consensus fails on pop(0)).
    Returns (members, strands): per group the kept read indices and, parallel, 0 = forward,
    1 = reverse-complemented."""
    seqs, ln, p = _pack_reads(ctx, reads)
    return _orient(ctx, p, seqs, ln, groups, n_threads)


def consensus(ctx, reads, groups, ambiguous: bool = False, n_threads: int = 16,
              strands=None) -> list:
    """create_consensus (:358-428) for many groups at once: `groups` are lists of indices into
    `reads` (str or bytes over A/C/G/T/N, already oriented).  Per group: a stable sort by
    falling length, the longest read seeds cycle 1 and the others are aligned against it;
    cycles 2 and 3 align every read, the seed included, against the previous cycle's
    consensus.  Every group of the call goes into each of the three groupalign calls.  ctx: a
    Context, or None to run on the host reference (lib.groupalign_host, n_threads).
    strands: None, or parallel to groups, 0 / 1 per read as orient() returns them: a read
    marked 1 enters reverse-complemented (groupalign's strands; no read is turned on the host
    but a cycle-1 seed).  Returns the consensus strings, one per group."""
    if ambiguous:
        raise DmxError("consensus: -amb (ambiguity, degenerate) is not supported")
    seqs, ln, p = _pack_reads(ctx, reads)
    return _consensus(ctx, p, seqs, ln, groups, strands, n_threads)


def make_consensus(ctx, reads, groups, n_threads: int = 16) -> list:
    """make_consensus (:1089-1105) for many groups at once: orient(), then consensus()'s three
    cycles with the strands passed through to groupalign.  The batch is packed and loaded
    once; the orientation distances and the alignments both run on it, and no read is turned
    round on the host.  Not restated: the random sampling of comp_consensus_groups, which picks
    the reads before this is called."""
    seqs, ln, p = _pack_reads(ctx, reads)
    members, strands = _orient(ctx, p, seqs, ln, groups, n_threads)
    return _consensus(ctx, p, seqs, ln, members, strands, n_threads)


def _consensus(ctx, p, seqs, ln, groups, strands, n_threads):
    """consensus() on a batch that is packed (p) and, with a ctx, resident."""
    if strands is not None and len(strands) != len(groups):
        raise DmxError("consensus: strands must be parallel to groups")
    orders, sorders = [], None if strands is None else []
    for k, g in enumerate(groups):
        g = np.asarray(g, dtype=np.int64).reshape(-1)
        if not len(g):
            raise DmxError(f"consensus: group {k} has no reads")
        by_len = np.argsort(-ln[g], kind="stable")
        orders.append(g[by_len])
        if strands is not None:
            s = np.asarray(strands[k], dtype=np.uint8).reshape(-1)
            if len(s) != len(g) or (len(s) and int(s.max()) > 1):
                raise DmxError(f"consensus: group {k}: strands are 0 or 1, one per read")
            sorders.append(s[by_len])
    if not orders:
        return []
    seeds = [seqs[o[0]] for o in orders]
    members = [o[1:] for o in orders]
    mstr = None
    if strands is not None:   # a reversed longest read seeds cycle 1 as its reverse complement
        seeds = [revcomp(s) if so[0] else s for s, so in zip(seeds, sorders)]
        mstr = [so[1:] for so in sorders]
    tops = []
    for treshold in THRESHOLDS:
        res = (ctx.groupalign(seeds, members, strands=mstr) if ctx is not None
               else lib.groupalign_host(p, seeds, members, n_threads=n_threads, strands=mstr))
        tops, seeds = [], []
        for k, mem in enumerate(members):
            c = len(mem) + 1
            top, top_n = _homopolymer_sort(*_column_tops(res, k, c))
            tops.append((top, top_n, c))
            seeds.append("".join(_SYMS[x] for x in top[top_n > c * treshold]))
            if not seeds[-1]:
                raise DmxError(f"consensus: group {k}: no column passes the threshold")
        members, mstr = orders, sorders   # the full list from the second cycle on
    return [_final_correction(top, top_n, c, THRESHOLDS[-1]) for top, top_n, c in tops]


def assign(ctx, reads, unassigned, consensuses, similar: float, n_threads: int = 16,
           chunk: int = 2_000_000, max_chunks: int = 100):
    """One pass of process_consensuslist (:1628-1691) + similarity_species (:1693-1716) + the
    best-hit filter of update_groups (:1730-1755) on top of dmx_rowdist.
    `reads` are the bin's reads (str or bytes over A/C/G/T/N), `unassigned` the indices of those
    not yet in a group, `consensuses` the groups' consensus sequences (group = list index),
    `similar` the pass's threshold as a fraction.  ctx: a Context, or None to run on the host
    reference (lib.rowdist_host, n_threads).

    Pairs: every read of `unassigned`, in the given order, against every consensus in index
    order, except where len(a) * 1.05 < len(b) or len(b) * 1.05 < len(a) in double arithmetic
    (:1664); generation stops after the read at whose end `max_chunks` full chunks of `chunk`
    comparisons have been made (:1669-1676, tested once per read).
    Lines: iden = round(1 - d / len(longer), 3); `read:group:iden` when iden >= similar - 0.01,
    else, when iden < 0.5, the same line form with the identity against the reverse-complemented
    consensus if that passes (no `:reverse` tag here, as in the reference).
    Best hit: one survivor per read; a later line replaces the kept one iff its identity is >=
    the kept one's, so among equal identities the last line wins.  The lines come in
    pair-generation order, read-major and consensus ascending; the reference's own order is its
    workers' interleaving, so its tie winner is whichever worker wrote last.

    Returns (lines, best, added): best has one (read, group, iden) per read that has a line, in
    first-appearance order; added are the entries of best with iden >= similar.  The outer
    rest_reads loop, the sampling above 200 reads, finetune and compare_consensus are the
    caller's (consensus_direction is orient())."""
    seqs = _clean(reads)
    cons = _clean(consensuses, "consensus")
    for g, s in enumerate(cons):
        if not s:
            raise DmxError(f"assign: consensus {g} is empty")
    un = np.asarray(unassigned, dtype=np.int64).reshape(-1)
    if len(un) and (int(un.min()) < 0 or int(un.max()) >= len(seqs)):
        raise DmxError("assign: an unassigned index is outside the reads")
    ln = np.array([len(s) for s in seqs], dtype=np.int64)
    lc = np.array([len(s) for s in cons], dtype=np.int64)
    if (len(ln) and int(ln.max()) > lib.PD_MAX_LEN) or (len(lc) and int(lc.max()) > lib.PD_MAX_LEN):
        raise DmxError(f"a read or a consensus is longer than {lib.PD_MAX_LEN} nt")
    if not len(un) or not len(cons):
        return [], [], []
    # the pairs: the 5 % rule in both directions with the reference's double products, then the
    # stop, tested after each read's consensuses as the reference does (k == 100, :1675)
    la = ln[un].astype(np.float64)[:, None]
    lb = lc.astype(np.float64)[None, :]
    keep = ~((la * 1.05 < lb) | (lb * 1.05 < la))
    full = np.cumsum(keep.sum(axis=1)) // int(chunk)   # todo files written by the end of a read
    stop = np.flatnonzero(full == int(max_chunks))
    if len(stop):
        keep[stop[0] + 1:] = False
    xi, g = np.nonzero(keep)            # row-major: read-major, consensus ascending
    if not len(xi):
        return [], [], []
    q = un[xi]
    lt = np.maximum(ln[q], lc[g])       # distance() divides by the longer one's length
    thr = similar - 0.01
    top = int(lt.max()) + 1
    cap_half = np.full(top, -1, dtype=np.int64)
    cap_thr = np.full(top, -1, dtype=np.int64)
    for L in np.unique(lt):
        cap_half[L] = identity_cap(int(L), 0.5)
        cap_thr[L] = identity_cap(int(L), thr)
    rows = [lib.mask_row(s) for s in cons]
    p = None
    if ctx is None or getattr(ctx, "_resident", None) is not reads:
        blob = np.frombuffer(b"".join(seqs), dtype=np.uint8)
        offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
        p = lib.pack(blob, offs, ln.astype(np.uint32))
        if ctx is not None:
            ctx.load(p)
            ctx._resident = reads      # the next pass over the same list finds its batch loaded

    def dist(rws, qq, rr, caps):
        if ctx is not None:
            return ctx.rowdist(rws, qq, rr, caps).astype(np.int64)
        return lib.rowdist_host(p, rws, qq, rr, caps, n_threads=n_threads).astype(np.int64)

    # the exact distance is needed wherever the identity is >= 0.5 or >= similar - 0.01
    fcap = np.maximum(np.maximum(cap_half[lt], cap_thr[lt]), 0).astype(np.uint32)
    df = dist(rows, q, g, fcap)
    plain = df <= cap_thr[lt]
    rcs = np.flatnonzero(~plain & (df > cap_half[lt]) & (cap_thr[lt] >= 0))
    hit = np.zeros(len(q), dtype=bool)
    d = df.copy()
    if len(rcs):
        # the reverse-complemented consensuses the second call needs, as rows of their own
        gs, inv = np.unique(g[rcs], return_inverse=True)
        dr = dist([lib.mask_rc(rows[k]) for k in gs], q[rcs], inv,
                  cap_thr[lt[rcs]].astype(np.uint32))
        ok = dr <= cap_thr[lt[rcs]]
        hit[rcs[ok]] = True
        d[rcs[ok]] = dr[ok]
    lines, best = [], {}
    for k in np.flatnonzero(plain | hit):
        rd, grp = int(q[k]), int(g[k])
        iden = identity(int(d[k]), int(lt[k]))
        lines.append(f"{rd}:{grp}:{iden}")
        if rd not in best or iden >= best[rd][2]:
            best[rd] = (rd, grp, iden)
    best = list(best.values())
    return lines, best, [b for b in best if b[2] >= similar]


def _assign_tables(lengths, similar):
    """dmx_rowassign's three tables, indexed by the longer length of a pair: for every distinct
    length L among `lengths`, cap_hit[L] = identity_cap(L, similar - 0.01), cap_half[L] =
    identity_cap(L, 0.5) and a row of cap_hit[L] + 1 identity classes (thousandths, by
    identity() itself, as _identity_table makes them).  Returns (cap_hit, cap_half, bin_off,
    bins)."""
    thr = similar - 0.01
    top = (int(max(lengths)) + 1) if len(lengths) else 0
    cap_hit = np.full(top, -1, dtype=np.int32)
    cap_half = np.full(top, -1, dtype=np.int32)
    bin_off = np.zeros(top, dtype=np.uint32)
    rows, at = [], 0
    for L in sorted({int(x) for x in lengths}):
        if L < 1:
            continue
        cap_half[L] = identity_cap(L, 0.5)
        cap_hit[L] = cap = identity_cap(L, thr)
        bin_off[L] = at
        n = max(cap, 0) + 1
        rows.append(np.array([int(round(identity(d, L) * 1000)) for d in range(n)],
                             dtype=np.uint16))
        at += n
    return cap_hit, cap_half, bin_off, np.concatenate(rows + [np.zeros(1, dtype=np.uint16)])


def assign_best(ctx, reads, unassigned, consensuses, similar: float, n_threads: int = 16,
                chunk: int = 2_000_000, max_chunks: int = 100):
    """assign() without the lines: the same pass (process_consensuslist :1628-1691,
    similarity_species :1693-1716, the best-hit filter of update_groups :1730-1755) as one
    dmx_rowassign call: the pairs are generated, decided and reduced inside the
    call, and one record per read comes back.  Arguments as assign()'s; ctx: a Context, or None
    for the host twin (lib.rowassign_host, n_threads).  The tables are built once per distinct
    length among the reads and the consensuses (_assign_tables).
    Returns (best, added): exactly assign()'s second and third return values for the same
    arguments, the same tuples (read, group, iden) with iden = class / 1000, in the same order.
    The batch of an unchanged `reads` list stays resident (ctx._resident), as in assign()."""
    ops = reads if isinstance(reads, Operands) else None
    if ops is not None and ctx is not ops.ctx:
        raise DmxError("Operands run on the Context they were made with")
    seqs = ops if ops is not None else _clean(reads)
    cons = _clean(consensuses, "consensus")
    for g, s in enumerate(cons):
        if not s:
            raise DmxError(f"assign_best: consensus {g} is empty")
    un = np.asarray(unassigned, dtype=np.int64).reshape(-1)
    if len(un) and (int(un.min()) < 0 or int(un.max()) >= len(seqs)):
        raise DmxError("assign_best: an unassigned index is outside the reads")
    ln = ops.lengths if ops is not None else np.array([len(s) for s in seqs], dtype=np.int64)
    lc = np.array([len(s) for s in cons], dtype=np.int64)
    if (len(ln) and int(ln.max()) > lib.PD_MAX_LEN) or (len(lc) and int(lc.max()) > lib.PD_MAX_LEN):
        raise DmxError(f"a read or a consensus is longer than {lib.PD_MAX_LEN} nt")
    if not len(un) or not len(cons):
        return [], []
    tables = _assign_tables(np.concatenate([ln[un], lc]), similar)
    rows = [lib.mask_row(s) for s in cons]
    p = None
    if ops is not None:
        ops.activate()
    elif ctx is None or getattr(ctx, "_resident", None) is not reads:
        blob = np.frombuffer(b"".join(seqs), dtype=np.uint8)
        offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
        p = lib.pack(blob, offs, ln.astype(np.uint32))
        if ctx is not None:
            ctx.load(p)
            ctx._resident = reads
    if ctx is not None:
        row, _, cls, _, _ = ctx.rowassign(rows, un, *tables, chunk=chunk, max_chunks=max_chunks)
    else:
        row, _, cls, _, _ = lib.rowassign_host(p, rows, un, *tables, chunk=chunk,
                                               max_chunks=max_chunks, n_threads=n_threads)
    # one entry per read in first-appearance order; a read named twice keeps its later place's
    # line iff that identity is >= the kept one's, as a later line of the same read would
    best = {}
    for k in np.flatnonzero(row != lib.LG_NONE):
        rd, iden = int(un[k]), int(cls[k]) / 1000
        if rd not in best or iden >= best[rd][2]:
            best[rd] = (rd, int(row[k]), iden)
    best = list(best.values())
    return best, [b for b in best if b[2] >= similar]


def species_consensuses(ctx, reads, species, sample: int = 100, n_threads: int = 16) -> list:
    """The second half of read_indexes (:1431-1456): a consensus per species group
    (make_consensus) of its first `sample` reads in index order; the reference takes 100 at
    random from a larger group (:1434-1435).  species: index arrays into reads.  Returns the
    consensus strings, one per group."""
    if not len(species):
        return []
    return _group_consensuses(ctx, reads, species, sample, n_threads)


def rest_reads(ctx, reads, indexes, groups, consensuses, similar_species: float = 85.0,
               similar_consensus: float = 96.0, length_diff: float = 8.0, start: float = 0.95,
               finetune=None, n_threads: int = 16):
    """rest_reads (:1962-2014), restated literally: the reads of a gene group that are in no
    species group yet are compared with the groups' consensuses at `similar` = start, lowered in
    steps of 0.01 down to similar_species / 100, up to three passes per step.
    reads: the reads the indices name; indexes: the gene group's reads; groups: its species
    groups (index arrays) with their `consensuses`.  State: the groups and their consensuses,
    the kept best list of the last pass (the reference's temp file, read back as `templist`) and
    `templist2`, its entries with iden >= similar.
      process + update   one assign_best at the current similar over the reads of `indexes` in
                         no group, ascending (:1648-1657), then update.
      update alone       (:2008-2011) thresholds the kept best list at the lowered similar
                         without comparing again, as the reference reads its temp file again.
      update             every entry of templist2 appends its read to its group; every group
                         that received a read gets a fresh consensus (make_consensus) of its
                         first 200 reads in index order.  The reference samples 200 at random
                         (:1791-1792); index order is this project's standing stand-in for the
                         reference's random samples.
    compare_consensus is sorter.compare_consensus with length_diff = 8.0 inside the loop (:1980,
    :1991: the literal 1.08) and the caller's length_diff at the end (:2014).  The k / similar
    state machine is the reference's, similar = round(similar - 0.01, 2) included; an update
    alone after a pass that added reads appends them a second time, as the reference does (a
    merge or a consensus does not count a read twice).
    finetune: at similar in [0.94, 0.88] the reference runs finetune (:1997-2000), which draws
    random samples at every step and has no value to pin.  Here it is a callable
    (groups, consensuses) -> (groups, consensuses) run at that point, empty groups dropped
    afterwards; None skips the call.  Either way the process step of :2000 runs (its kept list
    replaces the previous one), which is the difference from the reference with finetune=None.
    ctx: a Context, or None for the host twins.  Returns (groups, consensuses)."""
    groups = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
    cons = [c.decode("ascii") if isinstance(c, (bytes, bytearray)) else str(c)
            for c in consensuses]
    if len(groups) != len(cons):
        raise ValueError("rest_reads: one consensus per group")
    indexes = np.unique(np.asarray(indexes, dtype=np.int64).reshape(-1))
    similar = start
    min_similar = similar_species / 100
    state = {"kept": [], "groups": groups, "cons": cons}

    def tag():   # make_consensus loaded this very list, packed as assign_best packs it
        if ctx is not None and not isinstance(reads, Operands):   # (Operands tag themselves)
            ctx._resident = reads

    def process():
        inside = (np.concatenate(state["groups"]) if state["groups"]
                  else np.zeros(0, dtype=np.int64))
        un = indexes[~np.isin(indexes, inside)]
        state["kept"] = assign_best(ctx, reads, un, state["cons"], similar,
                                    n_threads=n_threads)[0]

    def update():
        templist = state["kept"]
        templist2 = [b for b in templist if b[2] >= similar]
        if templist2:
            grown = {}
            for rd, g, _ in templist2:
                grown.setdefault(g, []).append(rd)
            for g, more in grown.items():
                state["groups"][g] = np.concatenate([state["groups"][g],
                                                     np.array(more, dtype=np.int64)])
            order = sorted(grown)
            fresh = _group_consensuses(ctx, reads, [state["groups"][g] for g in order], 200,
                                       n_threads)
            tag()
            for g, c in zip(order, fresh):
                state["cons"][g] = c
        return templist, templist2

    def compare(ld):
        made = len(state["groups"]) > 1   # compare_consensus then makes consensuses of `reads`
        state["groups"], state["cons"] = compare_consensus(
            ctx, reads, state["groups"], state["cons"], similar_consensus, ld, 200, n_threads)
        if made:
            tag()

    k = 0
    process()
    templist, templist2 = update()
    if len(templist2) > 200:
        compare(8.0)
    k += 1
    while similar > min_similar:
        while k <= 2:
            if len(templist2) > 0:
                process()
                templist, templist2 = update()
                if len(templist2) > 0 and k < 2:
                    if len(state["groups"]) > 1:
                        compare(8.0)
                k += 1
            else:
                k = 3
        else:
            k = 0
            if similar in [0.94, 0.88]:
                if finetune is not None:
                    g2, c2 = finetune(state["groups"], state["cons"])
                    keep = [i for i, g in enumerate(g2) if len(g) > 0]
                    state["groups"] = [np.asarray(g2[i], dtype=np.int64).reshape(-1)
                                       for i in keep]
                    state["cons"] = [str(c2[i]) for i in keep]
                process()
            similar = round(similar - 0.01, 2)
            if len(templist) == 0:
                process()
                templist, templist2 = update()
                k += 1
            else:
                templist, templist2 = update()
                k += 1
    if len(state["groups"]) > 1:
        compare(length_diff)
    return state["groups"], state["cons"]


def _ft_select(rl, track, ln, row_len):
    """The host half of check_consensus (:866-872) on a group's readlist `rl` (entries [read,
    strand, iden, d1, d2]): every entry's identity against the track's consensus from the
    distance the lock-step call left in x[3 + track], the in-place stable string sort, then the
    reads at > 0.94 (the last 20 when those are fewer than 20), of which the last 50 make the
    consensus.  Returns those entries."""
    for x in rl:
        x[2] = identity(int(x[3 + track]), max(int(ln[x[0]]), row_len))
    rl.sort(key=lambda x: str(x[2]))
    sel = [x for x in rl if x[2] > 0.94]
    if len(sel) < 20:
        sel = rl[-20:]
    return sel[-50:]


def finetune(ctx, reads, groups, consensuses, n_threads: int = 16, max_cycles: int = 10):
    """finetune (:838-965) for all species groups of a gene group at once, restated literally
    per group and run in lock-step over the groups.  reads: a list of reads or
    Operands; groups: index arrays into them; consensuses: one string per group, ignored but
    where a group comes back unchanged (the reference strips them, :882-883).
    functools.partial(finetune, ctx, reads) is rest_reads' hook.  Per group:
      orientation   reads_direction (:854-862): the first read x anchors; read y is turned iff
                    identity(d(x, y)) < identity(d(x, rc(y))), a tie keeps it.  A turned read
                    enters every later step turned: as strand 1 of the consensus calls and
                    against mask_rc of the row in the distance calls; none is turned on the host.
      S1            where the reference draws random.sample(readlist, 100) (:889-892): the
                    first min(100, n) entries.  Read 0 of them against the others, stable sort
                    by identity, the start sequences at int(len // 1.25) and int(len // 5).
      the loop      (:903-912) check_consensus (:864-875) for track 1, then for track 2 on the
                    order track 1's sort left, then iden3 of the two new consensuses; until
                    iden1 and iden2 are both 1, max_cycles cycles at most (the reference's 10).
      S2            where the reference draws random.sample(seqlist, 150): seqlist[:150] in the
                    order seqlist has at that point.
      outcomes      iden3 == 1: the reads at >= 0.95 (of track 2's last check) stay, in the
                    group's order, with a fresh consensus; fewer than 5: the group is empty.
                    Otherwise group B, the reads at >= 0.95 in readlist order with their
                    consensus, or the original group and consensus when fewer than 5; then,
                    when more than 5 reads are left, check_consensus against consensus1 and
                    group A of the reads at >= 0.95, appended after all groups.  (That last
                    check_consensus builds a consensus nothing reads; it is not built here.)
    distance_finetune (:840-852, HW) is dead code in the reference and has no part here.  A
    group of fewer than 2 reads is returned unchanged (the reference fails on scorelist[0]).
    Schedule: one pairdist call for every group's orientation and scorelist; per cycle one
    rowdist call for both tracks of every group still in its loop, the selections on the host,
    one consensus call, one rowpairdist call; one rowdist and one consensus call for the
    outcomes.  ctx: a Context, or None for the host twins.  The batch of an unchanged list
    stays resident, as in assign_best().  Returns (groups, consensuses); an emptied group is an
    empty array with consensus ''."""
    if int(max_cycles) < 1:
        raise ValueError("finetune: max_cycles must be at least 1")
    gin = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
    cin = [c.decode("ascii") if isinstance(c, (bytes, bytearray)) else str(c)
           for c in consensuses]
    if len(gin) != len(cin):
        raise ValueError("finetune: one consensus per group")
    if (ctx is None or isinstance(reads, Operands)
            or getattr(ctx, "_resident", None) is not reads):
        seqs, ln, p = _pack_reads(ctx, reads)
        if ctx is not None and not isinstance(reads, Operands) and p is not None:
            ctx._resident = reads
    else:   # the list's batch is loaded: the distances and alignments run on it as it lies
        seqs, p = _clean(reads), None
        ln = np.array([len(s) for s in seqs], dtype=np.int64)
    for k, g in enumerate(gin):
        if len(g) and (int(g.min()) < 0 or int(g.max()) >= len(seqs)):
            raise DmxError(f"finetune: group {k} names a read outside the reads")
    out_g, out_c, added = list(gin), list(cin), []
    live = [i for i, g in enumerate(gin) if len(g) >= 2]
    if not live:
        return out_g, out_c

    def rowdist(rows, q, r):
        if ctx is not None:
            return ctx.rowdist(rows, q, r).astype(np.int64)
        return lib.rowdist_host(p, rows, q, r, n_threads=n_threads).astype(np.int64)

    def track_rows(rows, row, rl):
        """The row of a track's consensus, and its reverse complement where a read is turned:
        per entry of rl the read and the index of the row it goes against."""
        sd = np.array([x[1] for x in rl], dtype=np.int64)
        base = len(rows)
        rows.append(row)
        if sd.any():
            rows.append(lib.mask_rc(row))
        return np.array([x[0] for x in rl], dtype=np.int64), base + sd

    # 1. orientation and S1: the first read against every other one, forward and turned
    q = np.concatenate([np.full(len(gin[i]) - 1, gin[i][0], dtype=np.int64) for i in live])
    t = np.concatenate([gin[i][1:] for i in live])
    swap = ln[q] > ln[t]                       # distance(): the shorter one is the query
    q, t = np.where(swap, t, q), np.where(swap, q, t)
    fl = np.concatenate([np.zeros(len(q), dtype=np.uint8),
                         np.full(len(q), lib.PD_RC, dtype=np.uint8)])
    q2, t2 = np.concatenate([q, q]), np.concatenate([t, t])
    d = (ctx.pairdist(q2, t2, lib.PD_NW, flags=fl) if ctx is not None
         else lib.pairdist_host(p, q2, t2, lib.PD_NW, flags=fl, n_threads=n_threads))
    d = d.astype(np.int64)
    state, at = {}, 0
    for i in live:
        g = gin[i]
        rl, score = [[int(g[0]), 0, "", 0, 0]], []
        for k, y in enumerate(g[1:]):
            L = int(ln[t[at + k]])
            iden, iden_r = identity(int(d[at + k]), L), identity(int(d[len(q) + at + k]), L)
            rl.append([int(y), int(iden < iden_r), "", 0, 0])
            score.append(iden_r if iden < iden_r else iden)
        at += len(g) - 1
        m = min(100, len(rl)) - 1              # readlist2[1:100] of the first 100 entries
        order = sorted(range(m), key=lambda k: score[k])
        starts = [rl[1 + order[int(m // 1.25)]], rl[1 + order[int(m // 5)]]]
        rows = [lib.mask_row(seqs[x[0]]) for x in starts]
        state[i] = {"rl": rl, "row": [lib.mask_rc(r) if x[1] else r
                                      for r, x in zip(rows, starts)],
                    "iden3": 0, "cycles": 0}

    # 2. the loop, all groups still in it advancing together
    active = list(live)
    while active:
        rows, qs, rs = [], [], []
        for i in active:
            st = state[i]
            for tr in (0, 1):
                a, b = track_rows(rows, st["row"][tr], st["rl"])
                qs.append(a)
                rs.append(b)
        d = rowdist(rows, np.concatenate(qs), np.concatenate(rs))
        at, picks = 0, []
        for i in active:
            rl = state[i]["rl"]
            for tr in (0, 1):                  # the entries as they stood when the call was made
                for k, x in enumerate(rl):
                    x[3 + tr] = d[at + k]
                at += len(rl)
            for tr in (0, 1):                  # track 2 starts from the order track 1 left
                picks.append(_ft_select(rl, tr, ln, len(state[i]["row"][tr])))
        fresh = _consensus(ctx, p, seqs, ln, [[x[0] for x in s] for s in picks],
                           [[x[1] for x in s] for s in picks], n_threads)
        rows, pq, pt = [], [], []
        for k, i in enumerate(active):
            b = len(rows)
            rows += [state[i]["row"][0], lib.mask_row(fresh[2 * k]),
                     state[i]["row"][1], lib.mask_row(fresh[2 * k + 1])]
            pq += [b + 1, b + 3, b + 1]        # new 1 : old 1, new 2 : old 2, new 1 : new 2
            pt += [b, b + 2, b + 3]
        d = (ctx.rowpairdist(rows, pq, pt, lib.PD_NW) if ctx is not None
             else lib.rowpairdist_host(rows, pq, pt, lib.PD_NW, n_threads=n_threads))
        still = []
        for k, i in enumerate(active):
            st = state[i]
            iden = [identity(int(d[3 * k + j]), max(len(rows[pq[3 * k + j]]),
                                                    len(rows[pt[3 * k + j]]))) for j in range(3)]
            st["row"] = [rows[4 * k + 1], rows[4 * k + 3]]
            st["iden3"] = iden[2]
            st["cycles"] += 1
            if (iden[0] < 1 or iden[1] < 1) and st["cycles"] < int(max_cycles):
                still.append(i)
        active = still

    # 3. the outcomes
    jobs, rest_of = [], {}
    for i in live:
        rl = state[i]["rl"]
        keep = [x for x in rl if x[2] >= 0.95]
        if state[i]["iden3"] == 1:
            if len(keep) >= 5:
                grp = [int(x) for x in gin[i]]
                for x in rl:
                    if x[2] < 0.95:
                        grp.remove(x[0])
                out_g[i] = np.array(grp, dtype=np.int64)
                jobs.append((i, False, keep[:150]))
            else:
                out_g[i], out_c[i] = np.zeros(0, dtype=np.int64), ""
            continue
        rest = rl
        if len(keep) >= 5:                     # group B; fewer: the original group stays
            out_g[i] = np.array([x[0] for x in keep], dtype=np.int64)
            jobs.append((i, False, keep[:150]))
            rest = [x for x in rl if x[2] < 0.95]
        if len(rest) > 5:
            rest_of[i] = rest
    if rest_of:                                # group A: the rest against consensus1
        rows, qs, rs = [], [], []
        for i, rest in rest_of.items():
            a, b = track_rows(rows, state[i]["row"][0], rest)
            qs.append(a)
            rs.append(b)
        d = rowdist(rows, np.concatenate(qs), np.concatenate(rs))
        at = 0
        for i, rest in rest_of.items():
            for k, x in enumerate(rest):
                x[3] = d[at + k]
            at += len(rest)
            _ft_select(rest, 0, ln, len(state[i]["row"][0]))
            keep = [x for x in rest if x[2] >= 0.95]
            if len(keep) >= 5:
                jobs.append((i, True, keep[:150]))
                added.append(np.array([x[0] for x in keep], dtype=np.int64))
    if jobs:
        fresh = _consensus(ctx, p, seqs, ln, [[x[0] for x in s] for _, _, s in jobs],
                           [[x[1] for x in s] for _, _, s in jobs], n_threads)
        extra = []
        for (i, is_a, _), c in zip(jobs, fresh):
            if is_a:
                extra.append(c)
            else:
                out_c[i] = c
        return out_g + added, out_c + extra
    return out_g, out_c


def compare_consensuses(ctx, consensuses, length_diff: float = 8.0, threshold: float = 0.60,
                        n_threads: int = 16) -> list:
    """The pair loop of comp_consensus_groups / compare_consensus (:1276-1296, :1869-1889) with
    iden_consensus (:1140-1159) on dmx_rowhits: the lines (y, z, iden) of the
    consensus pairs whose larger identity over both strands is >= threshold, in pair-generation
    order (y-major, z ascending; the reference's order is its workers' interleaving).
    consensuses: A/C/G/T/N strings or bytes, or uint8 mask rows (lib.mask_row: gap and IUPAC
    columns allowed; two columns are equal iff their masks intersect).
    Pairs: y < z, dropped where len(A1) * ldc < len(A2) or len(A2) * ldc < len(A1) with
    ldc = length_diff / 100 + 1 in double arithmetic.  The query is the shorter consensus (y's
    on equal lengths), the target the longer; HW; the other strand is the target's reverse
    complement (the reference turns z's consensus, which gives the same distance).
    iden = round(1 - d / len(longer), 3) with d the smaller distance, decided as
    d <= identity_cap(len(longer), threshold).  ctx: a Context, or None for lib.rowhits_host."""
    rows = [np.ascontiguousarray(c, dtype=np.uint8).reshape(-1) if isinstance(c, np.ndarray)
            else lib.mask_row(_clean([c], "consensus")[0]) for c in consensuses]
    ln = np.array([len(r) for r in rows], dtype=np.int64)
    if len(ln) and (int(ln.min()) < 1 or int(ln.max()) > lib.PD_MAX_LEN):
        raise DmxError(f"compare_consensuses: consensuses of 1..{lib.PD_MAX_LEN} columns")
    n = len(rows)
    if n < 2:
        return []
    ldc = length_diff / 100 + 1
    y, z = np.triu_indices(n, 1)               # y-major, z ascending
    la, lb = ln[y].astype(np.float64), ln[z].astype(np.float64)
    keep = ~((la * ldc < lb) | (lb * ldc < la))
    y, z = y[keep], z[keep]
    if not len(y):
        return []
    swap = ln[y] > ln[z]                       # the query is the shorter, y's on equal lengths
    q, t = np.where(swap, z, y), np.where(swap, y, z)
    lt = ln[t]
    caps = {int(L): identity_cap(int(L), threshold) for L in np.unique(lt)}
    cap = np.array([caps[int(L)] for L in lt], dtype=np.int32)
    if ctx is not None:
        pair, d, _ = ctx.rowhits(rows, q, t, cap, lib.PD_HW)
    else:
        pair, d, _ = lib.rowhits_host(rows, q, t, cap, lib.PD_HW, n_threads=n_threads)
    return [(int(y[k]), int(z[k]), identity(int(dk), int(lt[k]))) for k, dk in zip(pair, d)]


def merge_by_consensus(groups, consensuses, lines, threshold: float) -> list:
    """What comp_consensus_groups (:1305-1330) and compare_consensus (:1898-1914) make of the
    lines, then merge_groups (:1058-1087), restated literally.  Group k is the set of its read
    tokens (the decimal strings of groups[k]) plus its consensus string.  Per line (y, z, iden)
    with iden >= threshold, in the order given: y is followed while its set has exactly one
    element (that element is a pointer "=k"); S[y] |= S[z]; S[z] = {"=y"}.  z is not followed:
    a z that is already a pointer hands its pointer token to y (the reference does the same, and
    the two groups then meet through that token in the merge below).  Then the sets of at most
    one element are dropped and sets that share any element (a read, a pointer token, an equal
    consensus string) are merged, pass after pass in the reference's double loop, until a pass
    merges nothing; a surviving group stands at its earliest position.  Only the read indices
    are kept.  Returns ascending int64 index arrays.  A group without reads is a ValueError.
    The result depends on the order of the lines where the reference's does: ours is
    pair-generation order, the reference's the interleaving of its workers."""
    if len(groups) != len(consensuses):
        raise ValueError("merge_by_consensus: one consensus per group")
    sets = []
    for k, (g, c) in enumerate(zip(groups, consensuses)):
        g = np.asarray(g, dtype=np.int64).reshape(-1)
        if not len(g):
            raise ValueError(f"merge_by_consensus: group {k} has no reads")
        c = c.decode("ascii") if isinstance(c, (bytes, bytearray)) else str(c)
        sets.append({str(int(x)) for x in g} | {c})
    for y, z, iden in lines:
        if not float(iden) >= threshold:
            continue
        y, z = int(y), int(z)
        while len(sets[y]) == 1:
            y = int(next(iter(sets[y])).replace("=", ""))
        sets[y].update(sets[z])
        sets[z] = {"=" + str(y)}
    sets = [s for s in sets if len(s) > 1]
    a1, a2 = len(sets) + 1, len(sets)
    while a1 > a2:
        a1 = len(sets)
        for i in range(len(sets) - 1):
            for j in range(i + 1, len(sets)):
                if not sets[i].isdisjoint(sets[j]):
                    sets[i] = sets[i] | sets[j]
                    sets[j].clear()
        sets = [s for s in sets if s]
        a2 = len(sets)
    return [np.array(sorted(int(x) for x in s if x.isdigit()), dtype=np.int64) for s in sets]


def _group_consensuses(ctx, reads, groups, sample, n_threads):
    """make_consensus of every group's first `sample` reads in index order."""
    return [c for c in make_consensus(ctx, reads, [np.sort(np.asarray(g, dtype=np.int64))[:sample]
                                                   for g in groups], n_threads=n_threads)]


def comp_consensus_groups(ctx, reads, groups, length_diff: float = 8.0, sample: int = 50,
                          min_reads: int = 6, n_threads: int = 16) -> list:
    """The merge loop of comp_consensus_groups (:1231-1334): while the number of groups falls,
    a consensus per group (make_consensus of its first `sample` reads in index order; the
    reference samples that many at random, the difference documented for --consensus),
    compare_consensuses at 0.60, and merge_by_consensus with threshold 0.80 when
    length_diff / 100 + 1 > 1.08 and 0.60 otherwise.  Then the groups with at least min_reads
    reads are kept (:1334).  groups: index arrays into reads.  ctx: a Context, or None for the
    host twins.  Returns ascending index arrays."""
    groups = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
    ldc = length_diff / 100 + 1
    a1, a2 = len(groups), 0
    while a1 > a2:
        a1 = len(groups)
        if not a1:
            break
        cons = _group_consensuses(ctx, reads, groups, sample, n_threads)
        lines = compare_consensuses(ctx, cons, length_diff, 0.60, n_threads)
        groups = merge_by_consensus(groups, cons, lines, 0.80 if ldc > 1.08 else 0.60)
        a2 = len(groups)
    return [g for g in groups if len(g) >= min_reads]


def compare_consensus(ctx, reads, groups, consensuses, similar_consensus: float = 96.0,
                      length_diff: float = 8.0, sample: int = 200, n_threads: int = 16):
    """The loop of compare_consensus (:1857-1958): at most 3 cycles, while the number of groups
    falls; a cycle compares the consensuses (lines at 0.60), merges at similar_consensus / 100
    and makes fresh consensuses of every group's first `sample` reads in index order (random in
    the reference).  Returns (groups, consensuses)."""
    groups = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
    cons = [c.decode("ascii") if isinstance(c, (bytes, bytearray)) else str(c)
            for c in consensuses]
    if len(groups) != len(cons):
        raise ValueError("compare_consensus: one consensus per group")
    if len(groups) > 1:
        a1, a2, b = len(groups), 0, 0
        while a1 > a2 and b < 3:
            a1 = len(groups)
            lines = compare_consensuses(ctx, cons, length_diff, 0.60, n_threads)
            groups = merge_by_consensus(groups, cons, lines, similar_consensus / 100)
            cons = _group_consensuses(ctx, reads, groups, sample, n_threads)
            a2 = len(groups)
            b += 1
    return groups, cons


def _clean(reads, what: str = "read") -> list:
    out = []
    for i, r in enumerate(reads):
        b = r.encode("ascii", "replace") if isinstance(r, str) else bytes(r)
        b = b.upper()
        if b.translate(None, b"ACGTN"):
            raise DmxError(f"{what} {i} has a byte outside ACGTN (the similarity pass supports "
                           "A, C, G, T and N only)")
        out.append(b)
    return out


def _similarity_plan(reads, similar_genes, minlength, maxlength, maxreads, allreads):
    """What similarity() and gene_groups() compare: the length-filtered reads packed, their
    lengths, the pairs (shorter, longer) and, per pair, the largest distance whose identity is
    still >= similar_genes / 100 and >= 0.5 (-1: none).  p is None when there is no pair."""
    ops = reads if isinstance(reads, Operands) else None
    seqs = None if ops is not None else _clean(reads)
    all_ln = [int(x) for x in ops.lengths] if ops is not None else [len(s) for s in seqs]
    idx = usable(all_ln, minlength, maxlength)
    groups = select_groups(all_ln, minlength, maxlength, maxreads, allreads)
    ln = np.array([all_ln[i] for i in idx], dtype=np.int64)
    if len(ln) and int(ln.max()) > lib.PD_MAX_LEN:
        raise DmxError(f"a read is longer than {lib.PD_MAX_LEN} nt (pass maxlength)")
    q, t = pairs(groups, ln)
    if not len(q):
        return None, ln, q, t, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    sg = similar_genes / 100
    # the two caps once per distinct length of the longer read, by the reference's own
    # expression; the decisions are integer comparisons against them
    cap_half = np.full(int(ln.max()) + 1, -1, dtype=np.int64)
    cap_sg = np.full(int(ln.max()) + 1, -1, dtype=np.int64)
    for L in np.unique(ln[t]):
        cap_half[L] = identity_cap(int(L), 0.5)
        cap_sg[L] = identity_cap(int(L), sg)
    if ops is not None:   # resident: the selected operands stand for the packed batch
        return (ops.subset(np.asarray(idx, dtype=np.int64)), ln, q, t, cap_sg[ln[t]],
                cap_half[ln[t]])
    blob = np.frombuffer(b"".join(seqs[i] for i in idx), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(ln[:-1])]).astype(np.uint64)
    p = lib.pack(blob, offs, ln.astype(np.uint32))
    return p, ln, q, t, cap_sg[ln[t]], cap_half[ln[t]]


def similarity(ctx, reads, similar_genes: float = 80.0, minlength: int = 300, maxlength=None,
               maxreads: int = 10000, allreads: bool = False, out=None) -> list:
    """The similarity pass (:777-808) over `reads` (str or bytes): the lines `i:j:iden` for
    pairs whose forward identity is >= similar_genes / 100, and `i:j:iden:reverse` for pairs
    whose forward identity is below 0.5 and whose identity against the reverse complement of
    the longer read is >= similar_genes / 100; i, j index the length-filtered reads, shorter
    first.  Lines come in pair-generation order (the reference's workers interleave theirs) and
    are written to `out` (a path) when given."""
    p, ln, q, t, cap_sg, cap_half = _similarity_plan(reads, similar_genes, minlength, maxlength,
                                                     maxreads, allreads)
    lines = []
    if len(q):
        _load(ctx, p)
        lt = ln[t]
        # the exact distance is needed wherever the identity is >= 0.5 or >= sg
        fcap = np.maximum(np.maximum(cap_half, cap_sg), 0).astype(np.uint32)
        df = ctx.pairdist(q, t, lib.PD_NW, caps=fcap).astype(np.int64)
        plain = df <= cap_sg
        need_rc = ~plain & (df > cap_half) & (cap_sg >= 0)
        rcs = np.flatnonzero(need_rc)
        dr = np.zeros(0, dtype=np.int64)
        if len(rcs):
            dr = ctx.pairdist(q[rcs], t[rcs], lib.PD_NW,
                              flags=np.full(len(rcs), lib.PD_RC, dtype=np.uint8),
                              caps=cap_sg[rcs].astype(np.uint32)).astype(np.int64)
        rev = np.zeros(len(q), dtype=bool)
        dist = df.copy()
        hit = dr <= cap_sg[rcs]
        rev[rcs[hit]] = True
        dist[rcs[hit]] = dr[hit]
        for k in np.flatnonzero(plain | rev):
            iden = identity(int(dist[k]), int(lt[k]))
            lines.append(f"{q[k]}:{t[k]}:{iden}" + (":reverse" if rev[k] else ""))
    if out is not None:
        with open(out, "w") as f:
            f.write("".join(x + "\n" for x in lines))
    return lines


def identity_tie(d: int, length: int) -> int:
    """The largest distance whose identity(., length) equals identity(d, length): lines of one
    longer read whose distances differ but round to the same identity tie in update_list.  Below
    1000 nt the step 1 / length is above the rounding's 0.001 and this is d itself."""
    d, length = int(d), int(length)
    iden = identity(d, length)
    while d < length and identity(d + 1, length) == iden:
        d += 1
    return d


def gene_groups(ctx, reads, similar_genes: float = 80.0, minlength: int = 300, maxlength=None,
                maxreads: int = 10000, allreads: bool = False, n_threads: int = 16) -> list:
    """The gene groups update_list (:983-1034) and merge_groups (:1058-1087) make of the
    similarity lines, without the lines: similarity()'s selection, pairs and caps, the hit
    decisions on the device (dmx_pairhits), per longer read the hits of the largest identity
    with every tie, and the connected components of those links (dmx_hitgroups).
    Returns the groups as ascending index arrays into the length-filtered reads, ordered as the
    reference's grouplist: by falling (best identity in the group, largest longer read among the
    links with that identity).  Reads on no kept link are in no group.  ctx: a Context, or None
    to run the host twins (lib.pairhits_host, lib.hitgroups_host; n_threads)."""
    p, ln, q, t, cap_sg, cap_half = _similarity_plan(reads, similar_genes, minlength, maxlength,
                                                     maxreads, allreads)
    if not len(q):
        return []
    if isinstance(p, Operands) and ctx is not p.ctx:
        raise DmxError("Operands run on the Context they were made with")
    if ctx is not None:
        _load(ctx, p)
        best, _ = ctx.pairhits(q, t, cap_sg, cap_half)
    else:
        hits = lib.pairhits_host(p, q, t, cap_sg, cap_half, n_threads=n_threads)
        best = hits.best
    has = np.flatnonzero(best != lib.LG_NONE)
    tie = np.full(len(ln), lib.LG_NONE, dtype=np.uint32)
    for r in has:
        tie[r] = identity_tie(int(best[r]), int(ln[r]))
    labels = ctx.hitgroups(tie) if ctx is not None else lib.hitgroups_host(hits, tie)
    # a group stands where its first link does in the list sorted by (iden, j), reverse=True;
    # every kept link of j has the identity of best[j]
    first = {}
    for r in has:
        key = (identity(int(best[r]), int(ln[r])), int(r))
        g = int(labels[r])
        if g not in first or key > first[g]:
            first[g] = key
    members = {g: [] for g in first}
    for r in np.flatnonzero(labels != lib.LG_NONE):
        members[int(labels[r])].append(int(r))
    order = sorted(first, key=lambda g: first[g], reverse=True)
    return [np.array(members[g], dtype=np.int64) for g in order]


N_CLASSES = 1001   # identity classes of the histogram: thousandths, 0.000 .. 1.000


def _run_pairhits(ctx, p, q, t, cap_sg, cap_half, n_threads):
    """pairhits on the plan's batch: (best, hits) with hits the host state, or None on a ctx."""
    if isinstance(p, Operands) and ctx is not p.ctx:
        raise DmxError("Operands run on the Context they were made with")
    if ctx is not None:
        _load(ctx, p)
        return ctx.pairhits(q, t, cap_sg, cap_half)[0], None
    hits = lib.pairhits_host(p, q, t, cap_sg, cap_half, n_threads=n_threads)
    return hits.best, hits


def _identity_table(ln, t, cap_sg):
    """dmx_hithist's table: per distinct length L of a longer read one row of cap + 1 entries,
    row[d] = the identity of distance d at L in thousandths, by identity() itself (cap = the
    hit cap at L: no hit has a larger distance).  Returns (bin_off per read, bins)."""
    bin_off = np.zeros(len(ln), dtype=np.uint32)
    rows, at = [], 0
    lens, first = np.unique(ln[t], return_index=True)
    for L, k in zip(lens, first):
        cap = int(cap_sg[k])
        if cap < 0:
            continue
        rows.append(np.array([int(round(identity(d, int(L)) * 1000)) for d in range(cap + 1)],
                             dtype=np.uint16))
        bin_off[ln == L] = at
        at += cap + 1
    return bin_off, np.concatenate(rows + [np.zeros(0, dtype=np.uint16)])


def identity_histogram(ctx, reads, similar_genes: float = 80.0, minlength: int = 300,
                       maxlength=None, maxreads: int = 10000, allreads: bool = False,
                       n_threads: int = 16) -> np.ndarray:
    """How many similarity lines (forward and reverse) of similarity()'s pass carry each
    identity: hist[k] = the lines with iden == k / 1000, k = 0 .. 1000 (uint64), without the
    lines: dmx_pairhits, then dmx_hithist over a table of identity() per (length, distance)
    (DESIGN.md §8k).  ctx: a Context, or None for the host twins."""
    p, ln, q, t, cap_sg, cap_half = _similarity_plan(reads, similar_genes, minlength, maxlength,
                                                     maxreads, allreads)
    if not len(q):
        return np.zeros(N_CLASSES, dtype=np.uint64)
    _, hits = _run_pairhits(ctx, p, q, t, cap_sg, cap_half, n_threads)
    bin_off, bins = _identity_table(ln, t, cap_sg)
    if ctx is not None:
        return ctx.hithist(bin_off, bins, N_CLASSES)
    return lib.hithist_host(hits, bin_off, bins, N_CLASSES)


def ssg_from_histogram(hist) -> int:
    """SSG (:810-836) on the histogram of identities in thousandths, in integers: the total
    T = sum k * c_k stands for totalsimil = T / 1000, b = int(totalsimil * 0.06) is
    T * 6 // 100000, and the walk down the identities that occur stops at the first k whose
    running sum of k * c_k reaches 1000 * b.  Returns int(k / 1000 * 100) in double, as the
    reference evaluates int(x * 100) (k / 1000 is the double the reference parses from the
    line).  No line at all (the reference returns None and fails later) raises DmxError."""
    c = [int(x) for x in np.asarray(hist).reshape(-1)]
    if not any(c):
        raise DmxError("estimate_ssg: no similarity line, nothing to estimate the ssg from")
    total = sum(k * n for k, n in enumerate(c))
    b = total * 6 // 100000
    run = 0
    for k in range(len(c) - 1, -1, -1):
        if c[k]:
            run += k * c[k]
            if run >= 1000 * b:
                return int((k / 1000) * 100)
    raise DmxError("estimate_ssg: the histogram's walk did not end")   # run ends at total >= 1000 b


def estimate_ssg(ctx, reads, similar_genes: float = 80.0, minlength: int = 300, maxlength=None,
                 maxreads: int = 10000, allreads: bool = False, n_threads: int = 16) -> int:
    """The species threshold the reference estimates when -ssg is not given (SSG, :810-836,
    'N6'): identity_histogram(), then ssg_from_histogram() in exact integer arithmetic.  The
    reference adds the identities as doubles in the order its workers wrote the lines, so at a
    razor edge (totalsimil * 0.06 within rounding of an integer, or the running sum within
    rounding of b) its answer depends on that order and there is no single reference value;
    away from such an edge both agree.  ctx: a Context, or None for the host twins."""
    return ssg_from_histogram(identity_histogram(ctx, reads, similar_genes, minlength, maxlength,
                                                 maxreads, allreads, n_threads))


def species_groups(ctx, reads, groups, ssg, similar_genes: float = 80.0, minlength: int = 300,
                   maxlength=None, maxreads: int = 10000, allreads: bool = False,
                   n_threads: int = 16) -> list:
    """The species groups of every gene group: the first half of read_indexes (:1363-1411) for
    all groups at once.  `groups` are gene groups as gene_groups() /
    comp_consensus_groups() return them (index arrays into the length-filtered reads, disjoint);
    `ssg` the species threshold in percent.  Per gene group g the reference takes the similarity
    lines with iden >= ssg / 100 and at least one read in g, keeps per longer read the best
    ones (ties kept, as in gene_groups), groups them and keeps the groups of more than 3 reads.
    Here: one pairhits call; the lines inside a group are filtered and joined on the device
    (dmx_hitgroups_within), the few lines that leave a group (dmx_pairhits_cross) are filtered
    in numpy, and a read pulled into a foreign group g enters the graph as a clone node (g, read),
    so that one components run gives every group's graph.  Returns per gene group the list of
    its species groups as ascending index arrays, by falling best identity, then smallest
    member.  No group (the reference's nogroup file) gives no species group.  ctx: a Context, or
    None for the host twins."""
    p, ln, q, t, cap_sg, cap_half = _similarity_plan(reads, similar_genes, minlength, maxlength,
                                                     maxreads, allreads)
    NONE = lib.LG_NONE
    n = len(ln)
    label = np.full(n, NONE, dtype=np.uint32)
    for k, g in enumerate(groups):
        g = np.asarray(g, dtype=np.int64).reshape(-1)
        if len(g) and (int(g.min()) < 0 or int(g.max()) >= n):
            raise DmxError(f"species_groups: group {k} names a read outside the reads")
        if (label[g] != NONE).any() or len(np.unique(g)) != len(g):
            raise DmxError(f"species_groups: group {k} shares a read with another group")
        label[g] = k
    out = [[] for _ in groups]
    if not len(q) or not len(groups):
        return out
    best, hits = _run_pairhits(ctx, p, q, t, cap_sg, cap_half, n_threads)
    thr = float(ssg) / 100
    cap_of = {int(L): identity_cap(int(L), thr) for L in np.unique(ln)}
    cap2 = np.array([cap_of[int(L)] for L in ln], dtype=np.int32)
    # 1. inside its own group a longer read keeps the lines of its global best identity
    tie2 = np.full(n, NONE, dtype=np.uint32)
    for r in np.flatnonzero((best != NONE) & (best.astype(np.int64) <= cap2)):
        tie2[r] = identity_tie(int(best[r]), int(ln[r]))
    # 2. the lines that leave a group
    pair, d, _ = (ctx.pairhits_cross(label, cap2) if ctx is not None
                  else lib.pairhits_cross_host(hits, label, cap2))
    d = d.astype(np.int64)
    cq, ct = q[pair].astype(np.int64), t[pair].astype(np.int64)
    # 3. per line and per valid group of its two reads: (group, read inside, read outside, kept)
    # the longer read inside: its best is the global one
    a = label[ct] != NONE
    keep_a = a & (tie2[ct] != NONE) & (d <= tie2[ct].astype(np.int64))
    # the longer read outside: its best among the lines whose shorter read is in that group
    b = np.flatnonzero(label[cq] != NONE)
    key = label[cq[b]].astype(np.int64) * n + ct[b]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    least = np.full(len(first), np.iinfo(np.int64).max)
    np.minimum.at(least, inv, d[b])
    tie_b = np.array([identity_tie(int(least[i]), int(ln[ct[b[first[i]]]]))
                      for i in range(len(first))], dtype=np.int64)
    keep_b = b[d[b] <= tie_b[inv]]
    ka = np.flatnonzero(keep_a)
    grp = np.concatenate([label[ct[ka]], label[cq[keep_b]]]).astype(np.int64)
    inside = np.concatenate([ct[ka], cq[keep_b]])
    outside = np.concatenate([cq[ka], ct[keep_b]])
    line_d = np.concatenate([d[ka], d[keep_b]])
    line_t = np.concatenate([ct[ka], ct[keep_b]])
    # 4. one clone node per distinct (group, read outside it)
    ckey, cidx = np.unique(grp * n + outside, return_inverse=True)
    clone_read = ckey % n
    n_nodes = n + len(ckey)
    xa, xb = inside.astype(np.uint32), (n + cidx).astype(np.uint32)
    # 5. one components run
    labels = (ctx.hitgroups_within(tie2, label, xa, xb, n_nodes) if ctx is not None
              else lib.hitgroups_within_host(hits, tie2, label, xa, xb, n_nodes))
    node_read = np.concatenate([np.arange(n, dtype=np.int64), clone_read])
    # the identity a node's kept lines carry (a longer read's lines all carry one identity)
    iden = np.full(n_nodes, -1.0)
    for r in np.flatnonzero(tie2 != NONE):
        iden[r] = identity(int(best[r]), int(ln[r]))
    for k in range(len(line_d)):
        node = int(line_t[k]) if label[line_t[k]] == grp[k] else int(n + cidx[k])
        iden[node] = max(iden[node], identity(int(line_d[k]), int(ln[line_t[k]])))
    comps = {}
    for v in np.flatnonzero(labels != NONE):
        comps.setdefault(int(labels[v]), []).append(int(v))
    found = [[] for _ in groups]
    for root, nodes in comps.items():
        # a component's smallest node is a read of the group: a clone hangs on one
        members = np.unique(node_read[nodes])
        if len(members) > 3:
            found[int(label[root])].append((-float(iden[nodes].max()), int(members[0]), members))
    for k, f in enumerate(found):
        out[k] = [m for _, _, m in sorted(f, key=lambda x: x[:2])]
    return out


def sort_species(ctx, reads, gene_groups, species, similar_species: float = 85.0,
                 similar_consensus: float = 96.0, length_diff: float = 8.0, finetune=None,
                 n_threads: int = 16, log=None) -> list:
    """What the stage is run for: per gene group with at least one species group (the others
    are the reference's 'Nothing to do', :2124-2127, reported through `log`),
    species_consensuses() and then rest_reads() over the gene group's reads.  gene_groups and
    species as gene_groups() / comp_consensus_groups() and species_groups() return them (index
    arrays into `reads`, the length-filtered list).  Returns a list of (gene group index, final
    species groups, their consensuses)."""
    out = []
    for k, (g, sp) in enumerate(zip(gene_groups, species)):
        if not len(sp):
            if log is not None:
                log(f"gene group {k}: no species group, nothing to do")
            continue
        cons = species_consensuses(ctx, reads, sp, n_threads=n_threads)
        groups, cons = rest_reads(ctx, reads, g, sp, cons, similar_species, similar_consensus,
                                  length_diff, finetune=finetune, n_threads=n_threads)
        out.append((k, groups, cons))
    return out


def write_assigned(path: str, sorted_species, similar_species: float, similar_consensus: float,
                   length_diff: float):
    """sort_species()'s result as two files: `path`, a first line '# ss N sc N ldc N' and per
    final species group a line '<gene group>.<k>: ' and its read indices; `path`.fasta, a record
    '>consensus_<gene group>_<k>(<n reads>)' per group, the reference's header shape (:1568)."""
    with open(path, "w") as f:
        f.write(f"# ss {similar_species:g} sc {similar_consensus:g} ldc {length_diff:g}\n")
        for k, groups, _ in sorted_species:
            for j, g in enumerate(groups):
                f.write(f"{k}.{j}: " + " ".join(str(int(x)) for x in g) + "\n")
    with open(path + ".fasta", "w") as f:
        for k, groups, cons in sorted_species:
            for j, (g, c) in enumerate(zip(groups, cons)):
                f.write(f">consensus_{k}_{j}({len(g)})\n{c}\n")


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
                    "bin's reads) on the GPU, and with --groups the gene groups of its best "
                    "hits, with --consensus a consensus per gene group, and with "
                    "--merged-groups the groups after comp_consensus_groups' merge loop "
                    "(consensuses compared on the GPU, dmx_rowhits), and with "
                    "--species-groups the species groups of every group at the estimated or "
                    "given ssg, and with --assigned the species group every read ends up in "
                    "(the rest_reads loop, reads assigned on the GPU, dmx_rowassign), with "
                    "--finetune the finetune pass inside that loop (first reads in order "
                    "where the reference samples at random); the random sampling, the .group / "
                    "results files and, without --finetune, finetune stay with the reference.")
    ap.add_argument("-i", "--input", required=True, help="bin in FASTQ/FASTA, optionally .gz")
    ap.add_argument("-o", "--output", default=None,
                    help="similarity lines (i:j:iden[:reverse]); optional with --groups")
    ap.add_argument("--groups", default=None, metavar="FILE",
                    help="gene groups, one per line: space-separated read indices, in the "
                         "reference's group order")
    ap.add_argument("--consensus", default=None, metavar="FILE",
                    help="with --groups: FASTA, one '>group_<k>(<n reads>)' record per gene "
                         "group, the consensus of the group's first --consensus-reads reads in "
                         "index order, oriented and aligned on the GPU (make_consensus); the "
                         "reference samples that many reads at random (comp_consensus_groups)")
    ap.add_argument("--consensus-reads", type=int, default=50, metavar="N",
                    help="reads per group that make its consensus (default 50, the reference's "
                         "sample size)")
    ap.add_argument("--merged-groups", default=None, metavar="FILE",
                    help="with --groups: the groups after comp_consensus_groups' merge loop "
                         "(consensus of the first --consensus-reads reads of every group, "
                         "consensuses compared in HW mode on both strands, groups merged, "
                         "repeated while their number falls; groups of fewer than 6 reads "
                         "dropped), one per line like --groups")
    ap.add_argument("--species-groups", default=None, metavar="FILE",
                    help="with --groups: the species groups (more than 3 reads) of every "
                         "merged group when --merged-groups is given, else of every gene group; "
                         "first line '# ssg N estimated' or '# ssg N given', then one line per "
                         "species group: '<group index>:' and the space-separated read indices")
    ap.add_argument("-ssg", "--similar_species_groups", type=float, default=None, metavar="N",
                    help="species threshold in percent for --species-groups (default: "
                         "estimated from the identities of all similarity lines, as the "
                         "reference's 'Estimate')")
    ap.add_argument("--assigned", default=None, metavar="FILE",
                    help="with --species-groups: the species group every read ends up in.  Per "
                         "gene group with a species group: a consensus per species group, then "
                         "the rest_reads loop (the other reads against the consensuses at a "
                         "similarity lowered from 0.95 to -ss, reads assigned on the GPU, "
                         "dmx_rowassign; consensuses compared and groups merged at -sc); first "
                         "line '# ss N sc N ldc N', then '<gene group>.<k>: ' and the read "
                         "indices per final group; FILE.fasta gets a "
                         "'>consensus_<gene group>_<k>(<n reads>)' record per group.  finetune "
                         "is run only with --finetune")
    ap.add_argument("--finetune", action="store_true",
                    help="with --assigned: run finetune (amplicon_sorter.py:838-965) where the "
                         "reference does, at similarities 0.94 and 0.88 of the rest_reads loop: "
                         "reads below 0.95 against their group's consensus leave the group, a "
                         "group of two species is split.  Where the reference samples reads at "
                         "random, the first in order are taken (the first 100 of a group for the "
                         "start sequences, the first 150 for a consensus); a group of fewer than "
                         "2 reads is left as it is.  Without the flag finetune is not run")
    ap.add_argument("-ss", "--similar_species", type=float, default=85.0, metavar="N",
                    help="lowest similarity (%%) at which a read joins a species group "
                         "(default 85.0)")
    ap.add_argument("-sc", "--similar_consensus", type=float, default=96.0, metavar="N",
                    help="similarity (%%) at which two species groups' consensuses merge them "
                         "(default 96.0)")
    ap.add_argument("-ldc", "--length_diff_consensus", type=float, default=8.0,
                    help="length difference (%%) allowed between two compared consensuses "
                         "(default 8.0)")
    ap.add_argument("-min", "--minlength", type=int, default=300)
    ap.add_argument("-max", "--maxlength", type=int, default=None)
    ap.add_argument("-maxr", "--maxreads", type=int, default=10000)
    ap.add_argument("-ar", "--allreads", action="store_true")
    ap.add_argument("-sg", "--similar_genes", type=float, default=80.0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.output is None and a.groups is None:
        ap.error("the following arguments are required: -o/--output")
    if a.consensus is not None and a.groups is None:
        ap.error("--consensus needs --groups")
    if a.merged_groups is not None and a.groups is None:
        ap.error("--merged-groups needs --groups")
    if a.species_groups is not None and a.groups is None:
        ap.error("--species-groups needs --groups")
    if a.assigned is not None and a.species_groups is None:
        ap.error("--assigned needs --species-groups")
    if a.finetune and a.assigned is None:
        ap.error("--finetune needs --assigned")
    if a.consensus_reads < 2:
        ap.error("--consensus-reads must be at least 2")
    try:
        reads = read_sequences(a.input)
        with lib.Context(a.device) as ctx:
            if a.output is not None:
                lines = similarity(ctx, reads, a.similar_genes, a.minlength, a.maxlength,
                                   a.maxreads, a.allreads, out=a.output)
                print(f"dmx-similarity: {len(reads)} reads, {len(lines)} similarity lines -> "
                      f"{a.output}", file=sys.stderr)
            if a.groups is not None:
                groups = gene_groups(ctx, reads, a.similar_genes, a.minlength, a.maxlength,
                                     a.maxreads, a.allreads)
                with open(a.groups, "w") as f:
                    f.write("".join(" ".join(str(int(x)) for x in g) + "\n" for g in groups))
                print(f"dmx-similarity: {len(reads)} reads, {len(groups)} gene groups -> "
                      f"{a.groups}", file=sys.stderr)
                if a.consensus is not None:
                    # the groups index the length-filtered reads
                    kept = [reads[i] for i in usable([len(s) for s in reads], a.minlength,
                                                     a.maxlength)]
                    cons = make_consensus(ctx, kept, [g[:a.consensus_reads] for g in groups])
                    with open(a.consensus, "w") as f:
                        f.write("".join(f">group_{k}({len(g)})\n{c}\n"
                                        for k, (g, c) in enumerate(zip(groups, cons))))
                    print(f"dmx-similarity: {len(cons)} consensus sequences -> {a.consensus}",
                          file=sys.stderr)
                if a.merged_groups is not None:
                    kept = [reads[i] for i in usable([len(s) for s in reads], a.minlength,
                                                     a.maxlength)]
                    merged = comp_consensus_groups(ctx, kept, groups, a.length_diff_consensus,
                                                   sample=a.consensus_reads)
                    with open(a.merged_groups, "w") as f:
                        f.write("".join(" ".join(str(int(x)) for x in g) + "\n" for g in merged))
                    print(f"dmx-similarity: {len(merged)} merged groups -> {a.merged_groups}",
                          file=sys.stderr)
                if a.species_groups is not None:
                    plan = (a.similar_genes, a.minlength, a.maxlength, a.maxreads, a.allreads)
                    ssg, how = a.similar_species_groups, "given"
                    if ssg is None:
                        ssg, how = estimate_ssg(ctx, reads, *plan), "estimated"
                        print(f"estimated ssg = {ssg}", file=sys.stderr)
                    of = merged if a.merged_groups is not None else groups
                    species = species_groups(ctx, reads, of, ssg, *plan)
                    with open(a.species_groups, "w") as f:
                        f.write(f"# ssg {ssg:g} {how}\n")
                        f.write("".join(f"{k}: " + " ".join(str(int(x)) for x in m) + "\n"
                                        for k, sp in enumerate(species) for m in sp))
                    print(f"dmx-similarity: {sum(len(sp) for sp in species)} species groups -> "
                          f"{a.species_groups}", file=sys.stderr)
                    if a.assigned is not None:
                        kept = [reads[i] for i in usable([len(s) for s in reads], a.minlength,
                                                         a.maxlength)]
                        done = sort_species(
                            ctx, kept, of, species, a.similar_species, a.similar_consensus,
                            a.length_diff_consensus,
                            finetune=(functools.partial(finetune, ctx, kept) if a.finetune
                                      else None),
                            log=lambda m: print(f"dmx-similarity: {m}", file=sys.stderr))
                        write_assigned(a.assigned, done, a.similar_species, a.similar_consensus,
                                       a.length_diff_consensus)
                        print(f"dmx-similarity: {sum(len(g) for _, g, _ in done)} final species "
                              f"groups -> {a.assigned}, {a.assigned}.fasta", file=sys.stderr)
    except (DmxError, OSError, ValueError) as e:
        print(f"dmx-similarity: {e}", file=sys.stderr)
        return 1
    return 0
