"""Shared inputs and the numpy oracle of the row-distance tests (test_rowdist_host.py and
test_assign.py on the CPU, test_rowdist.py on the GPU).  The oracle is written from the contract
alone (include/dmx.h dmx_rowdist): a full-matrix NW DP whose equality is (mask[j] >> symbol) & 1,
so a gap column equals nothing and an IUPAC column equals each of its symbols."""
import functools

import numpy as np

import groupalign_cases as gc
import pairdist_cases as pc
from dmx import lib

# the reverse complement over a row's whole alphabet
COMP_ROW = bytes.maketrans(b"ACGTNRYMKSW-", b"TGCANYRKMSW-")
SYM = np.full(256, 255, dtype=np.uint8)
for _k, _ch in enumerate(b"ACGTN"):
    SYM[_ch] = _k


def revcomp_row(s: str) -> str:
    return s.encode().translate(COMP_ROW)[::-1].decode()


def np_rowdist(queries, rows):
    """NW distances of queries[b] (bytes over ACGTN) against rows[b] (uint8 masks), all pairs at
    once, row by row; the in-row insertion chain is resolved by minimum.accumulate."""
    B = len(queries)
    if B == 0:
        return np.zeros(0, dtype=np.int64)
    ml = np.array([len(x) for x in queries])
    nl = np.array([len(x) for x in rows])
    M, N = int(ml.max()), int(nl.max())
    Q = np.zeros((B, M), dtype=np.uint8)
    T = np.zeros((B, N), dtype=np.uint8)          # padding: mask 0 equals nothing
    for b in range(B):
        Q[b, :ml[b]] = SYM[np.frombuffer(queries[b], dtype=np.uint8)]
        T[b, :nl[b]] = rows[b]
    assert int(Q.max()) < 5
    ar = np.arange(N + 1, dtype=np.int32)
    prev = np.tile(ar, (B, 1))
    res = np.zeros(B, dtype=np.int64)
    c = np.empty((B, N + 1), dtype=np.int32)
    for i in range(1, M + 1):
        neq = ((T >> Q[:, i - 1:i]) & 1) == 0
        c[:, 0] = i
        np.minimum(prev[:, 1:] + 1, prev[:, :-1] + neq, out=c[:, 1:])
        cur = np.minimum.accumulate(c - ar, axis=1) + ar
        sel = np.flatnonzero(ml == i)
        res[sel] = cur[sel, nl[sel]]
        prev = cur
    return res


@functools.lru_cache(maxsize=None)
def host_set(seed=81):
    """The CPU set: 40 reads of 1..300 nt with N, 12 rows (mutated copies with gap, IUPAC and N
    columns planted, an unrelated one, a row of 1 column, an all-gap row), and 300 pairs in no
    particular order: row 3 serves many of them, the first and the last row are used, pairs
    repeat.  Returns (reads, rows as str, q, r, numpy distances)."""
    rng = np.random.default_rng(seed)
    reads = [pc.rand_seq(rng, int(n), p_n=0.08)
             for n in [1, 2, 63, 64, 65, 300] + list(rng.integers(1, 301, 34))]
    rows = []
    for k in range(9):
        src = reads[int(rng.integers(len(reads)))]
        rows.append(gc.plant(rng, pc.mutate(rng, src, float(rng.uniform(0.02, 0.3))), 0.15))
    rows += [pc.rand_seq(rng, 120, p_n=0.2).decode(), "R", "-" * 17]
    n = 300
    q = rng.integers(0, len(reads), n).astype(np.uint32)
    r = rng.integers(0, len(rows), n).astype(np.uint32)
    r[rng.random(n) < 0.3] = 3
    r[:2] = [0, len(rows) - 1]
    q[10:14] = q[9]
    r[10:14] = r[9]
    exp = np_rowdist([reads[i] for i in q], [lib.mask_row(rows[j]) for j in r])
    return reads, rows, q, r, exp


def planted_row(rng, s: bytes, rate=0.06) -> str:
    """A mutated copy of s with gap, IUPAC and N columns."""
    return gc.plant(rng, pc.mutate(rng, s, rate), 0.05)


@functools.lru_cache(maxsize=None)
def boundary_case():
    """The GPU set.  Query lengths 1, 63, 64, 65, 127, 128, 129 and 64 G - 1, 64 G, 64 G + 1 for
    every group size, each against a planted copy of itself (a 500-column piece above 1,400 nt);
    a query of 4,200 nt (two stripes: the scratch row) against rows of 1,200 and 4,150 columns;
    rows of 1, 15, 16, 17, 31, 32, 33 columns against a 24-nt and a 1,200-nt read, and one of
    1,200; a 1-nt query on the 1,200-column row and the long query on the 1-column row.
    Returns (reads, rows as str, q, r)."""
    rng = np.random.default_rng(82)
    qlens = {1, 63, 64, 65, 127, 128, 129}
    for g in lib.pairdist_group_sizes():
        qlens |= {64 * g - 1, 64 * g, 64 * g + 1}
    reads, rows, q, r = [], [], [], []
    for m in sorted(qlens):
        a = pc.rand_seq(rng, m)
        piece = a if m <= 1400 else a[m // 3:m // 3 + 500]
        q.append(len(reads)), r.append(len(rows))
        reads.append(a), rows.append(planted_row(rng, piece))
    big = pc.rand_seq(rng, 4200)
    ibig = len(reads)
    reads.append(big)
    for piece in (big[1500:2700], big[:4150]):
        q.append(ibig), r.append(len(rows))
        rows.append(planted_row(rng, piece))
    short, long_ = pc.rand_seq(rng, 24), pc.rand_seq(rng, 1200)
    ishort, ilong = len(reads), len(reads) + 1
    reads += [short, long_]
    for n in (1, 15, 16, 17, 31, 32, 33):
        k = len(rows)
        rows.append(planted_row(rng, (short + long_)[:n], 0.1)[:n].ljust(n, "-"))
        q += [ishort, ilong]
        r += [k, k]
    k1200 = len(rows)
    rows.append(planted_row(rng, long_)[:1200].ljust(1200, "N"))
    one = len(reads)
    reads.append(b"G")
    q += [ilong, ishort, one, ibig]
    r += [k1200, k1200, k1200, k1200 - 7]     # rows[k1200 - 7] is the 1-column row
    assert len(rows[k1200 - 7]) == 1 and len(rows[k1200]) == 1200
    return reads, rows, np.array(q, dtype=np.uint32), np.array(r, dtype=np.uint32)


def mixed_pick(q, lens, seed=5):
    """Indices into a pair list: 151 draws of the short pairs, every pair forwards and
    backwards, a triple: short and long pairs, duplicates, no order, and a count that fills no
    wave evenly."""
    rng = np.random.default_rng(seed)
    short = np.flatnonzero(lens[q] <= 600)
    pick = np.concatenate([rng.choice(short, 151), np.arange(len(q)), np.arange(len(q))[::-1],
                           [3, 3, 3]])
    rng.shuffle(pick)
    assert len(pick) % 64 and len(pick) % 21 and len(pick) % 3
    return pick
