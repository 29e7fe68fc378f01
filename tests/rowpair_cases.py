"""Shared inputs and the numpy oracle of the row-pair tests (test_rowpair_host.py and
test_merge_consensus.py on the CPU, test_rowpair.py and test_merge_consensus_gpu.py on the GPU).
The oracle is written from the contract alone (include/dmx.h dmx_rowpairdist): a full-matrix DP,
NW or HW, whose equality is "the two masks intersect", so a gap column equals nothing on either
side and an IUPAC column equals each of its letters."""
import functools

import numpy as np

import pairdist_cases as pc
import rowdist_cases as rc
from dmx import lib


def np_rowpair(qrows, trows, mode):
    """Distances of qrows[b] against trows[b] (uint8 masks), all pairs at once, row by row; the
    in-row insertion chain is resolved by minimum.accumulate.  HW: row 0 is free and the result
    is the least of the last row within the target."""
    B = len(qrows)
    if B == 0:
        return np.zeros(0, dtype=np.int64)
    ml = np.array([len(x) for x in qrows])
    nl = np.array([len(x) for x in trows])
    M, N = int(ml.max()), int(nl.max())
    Q = np.zeros((B, M), dtype=np.uint8)
    T = np.zeros((B, N), dtype=np.uint8)          # padding: mask 0 equals nothing
    for b in range(B):
        Q[b, :ml[b]] = qrows[b]
        T[b, :nl[b]] = trows[b]
    ar = np.arange(N + 1, dtype=np.int32)
    prev = np.tile(ar, (B, 1)) if mode == lib.PD_NW else np.zeros((B, N + 1), dtype=np.int32)
    inside = ar[None, :] <= nl[:, None]
    res = np.zeros(B, dtype=np.int64)
    c = np.empty((B, N + 1), dtype=np.int32)
    for i in range(1, M + 1):
        neq = (Q[:, i - 1:i] & T) == 0
        c[:, 0] = i
        np.minimum(prev[:, 1:] + 1, prev[:, :-1] + neq, out=c[:, 1:])
        cur = np.minimum.accumulate(c - ar, axis=1) + ar
        sel = np.flatnonzero(ml == i)
        if len(sel):
            if mode == lib.PD_NW:
                res[sel] = cur[sel, nl[sel]]
            else:
                res[sel] = np.where(inside[sel], cur[sel], np.iinfo(np.int32).max).min(axis=1)
        prev = cur
    return res


def rand_row(rng, n, p_other=0.15) -> str:
    """A row over the whole alphabet: mostly A/C/G/T, some N, gap and IUPAC columns."""
    s = rng.choice(list("ACGT"), n)
    other = rng.random(n) < p_other
    s[other] = rng.choice(list("N-RYMKSW"), int(other.sum()))
    return "".join(s)


def expected(rows, q, t, flags, mode):
    """The oracle's distances of a pair list over rows given as str."""
    masks = [lib.mask_row(x) for x in rows]
    ts = [lib.mask_rc(masks[j]) if f else masks[j] for j, f in zip(t, flags)]
    return np_rowpair([masks[i] for i in q], ts, mode)


@functools.lru_cache(maxsize=None)
def host_set(seed=91):
    """The CPU set: rows of 1..70 columns and one of 1,200 over the whole alphabet (gap, IUPAC and
    N columns on either side), planted copies of each other and of reverse complements so that
    both strands see related rows; 260 pairs in no order with a random RC flag, pairs whose query
    is longer than the target, repeats.  Returns (rows as str, q, t, flags)."""
    rng = np.random.default_rng(seed)
    rows = [rand_row(rng, int(n)) for n in [1, 2, 15, 16, 17, 63, 64, 65, 70] +
            list(rng.integers(1, 71, 21))]
    for k in range(12):
        src = rows[int(rng.integers(len(rows)))]
        cp = rc.planted_row(rng, src.replace("-", "A").encode().translate(
            bytes.maketrans(b"RYMKSW", b"AGCTCA")), 0.1)
        rows.append(rc.revcomp_row(cp) if k % 2 else cp)
    big = pc.rand_seq(rng, 1200)
    rows += [rc.planted_row(rng, big)[:1200].ljust(1200, "N"), rc.planted_row(rng, big[300:360]),
             "-" * 9, "N" * 5]
    n = 260
    q = rng.integers(0, len(rows), n).astype(np.uint32)
    t = rng.integers(0, len(rows), n).astype(np.uint32)
    ibig = len(rows) - 4
    q[:4], t[:4] = [ibig + 1, ibig, ibig, 0], [ibig, ibig + 1, ibig, ibig]
    q[10:13], t[10:13] = q[9], t[9]
    flags = (rng.random(n) < 0.5).astype(np.uint8)
    flags[:4] = [0, 1, 1, 0]
    return rows, q, t, flags


@functools.lru_cache(maxsize=None)
def boundary_case():
    """The GPU set.  Query rows of 1, 63, 64, 65, 127, 128, 129 and 64 G - 1, 64 G, 64 G + 1
    columns for every group size, and of 4,095, 4,096, 4,097 and 4,200 (stripes: the scratch
    row), each against a planted copy of itself (a 500-column piece above 1,400) and against the
    reverse complement of one; target rows of 1, 15, 16, 17, 31, 32, 33, 63, 64, 65 and 1,200
    columns against a 24-column and a 1,200-column query.  Gap, IUPAC and N columns on both
    sides.  Returns (rows as str, q, t, flags)."""
    rng = np.random.default_rng(92)
    qlens = {1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4200}
    for g in lib.pairdist_group_sizes():
        qlens |= {64 * g - 1, 64 * g, 64 * g + 1}
    rows, q, t, f = [], [], [], []
    for m in sorted(qlens):
        a = pc.rand_seq(rng, m)
        piece = a if m <= 1400 else a[m // 3:m // 3 + 500]
        k = len(rows)
        rows += [rc.planted_row(rng, a, 0.03)[:m].ljust(m, "N"), rc.planted_row(rng, piece),
                 rc.revcomp_row(rc.planted_row(rng, piece))]
        q += [k, k, k, k]
        t += [k + 1, k + 1, k + 2, k + 2]
        f += [0, 1, 1, 0]
    short, long_ = pc.rand_seq(rng, 24), pc.rand_seq(rng, 1200)
    ishort, ilong = len(rows), len(rows) + 1
    rows += [rc.planted_row(rng, short, 0.1)[:24].ljust(24, "R"),
             rc.planted_row(rng, long_)[:1200].ljust(1200, "N")]
    for n in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1200):
        k = len(rows)
        rows.append(rc.planted_row(rng, (short + long_)[:n], 0.1)[:n].ljust(n, "-"))
        q += [ishort, ilong, ishort, ilong]
        t += [k, k, k, k]
        f += [0, 0, 1, 1]
    return (rows, np.array(q, dtype=np.uint32), np.array(t, dtype=np.uint32),
            np.array(f, dtype=np.uint8))


def mixed_pick(rows, q, seed=6):
    """Indices into a pair list: 152 draws of the short pairs, every pair forwards and backwards,
    a triple: short and long pairs, duplicates, no order, a count that fills no wave evenly."""
    rng = np.random.default_rng(seed)
    ql = np.array([len(rows[i]) for i in q])
    short = np.flatnonzero(ql <= 600)
    pick = np.concatenate([rng.choice(short, 152), np.arange(len(q)), np.arange(len(q))[::-1],
                           [3, 3, 3]])
    rng.shuffle(pick)
    assert len(pick) % 64 and len(pick) % 21 and len(pick) % 3
    return pick


@functools.lru_cache(maxsize=None)
def split_bin(seed=93):
    """A small synthetic bin: 3 unrelated families of ~120 nt, 16 reads each (3 % errors), the
    third family's reads reverse-complemented in its second half-group; every family is split
    into 2 groups of 8.  Returns (reads, groups, family of each group)."""
    rng = np.random.default_rng(seed)
    reads, groups, fam = [], [], []
    for k in range(3):
        src = pc.rand_seq(rng, int(rng.integers(115, 126)), p_n=0.0)
        for half in range(2):
            g = []
            for _ in range(8):
                r = pc.mutate(rng, src, 0.03).replace(b"N", b"A")
                if k == 2 and half == 1:
                    r = pc.revcomp(r)
                g.append(len(reads))
                reads.append(r)
            groups.append(np.array(g, dtype=np.int64))
            fam.append(k)
    return reads, groups, fam
