"""Shared inputs and the in-test oracle of the dmx_rowassign tests (test_rowassign_host.py on the
CPU, test_rowassign.py on the GPU).  The oracle is written from the contract alone (include/dmx.h
dmx_rowassign): rowdist_cases.np_rowdist for the distances, then a literal Python loop for the
pair rule, the stop, the decision, the retry and the best line per place."""
import functools

import numpy as np

import groupalign_cases as gc
import pairdist_cases as pc
import rowdist_cases as rc
from dmx import lib, sorter

NONE, REV = lib.LG_NONE, lib.LG_REV
THRESHOLD = 0.85          # the hit threshold of the realistic part of the tables


def tables(lengths, threshold=THRESHOLD, overrides=None):
    """cap_hit, cap_half, bin_off, bins over 0 .. max(lengths): per distinct length the two caps
    by sorter.identity_cap and a row of cap_hit + 1 classes (thousandths of sorter.identity).
    overrides: {L: (cap_hit or None, cap_half or None)} replaces a length's caps (the tables are
    the caller's: any value >= -1 is a valid cap)."""
    overrides = overrides or {}
    top = int(max(lengths)) + 1
    cap_hit = np.full(top, -1, dtype=np.int32)
    cap_half = np.full(top, -1, dtype=np.int32)
    bin_off = np.zeros(top, dtype=np.uint32)
    rows, at = [], 0
    for L in sorted({int(x) for x in lengths}):
        ch, cf = sorter.identity_cap(L, threshold), sorter.identity_cap(L, 0.5)
        o = overrides.get(L, (None, None))
        ch = ch if o[0] is None else o[0]
        cf = cf if o[1] is None else o[1]
        cap_hit[L], cap_half[L], bin_off[L] = ch, cf, at
        n = max(ch, 0) + 1
        rows.append([int(round(sorter.identity(min(d, L), L) * 1000)) for d in range(n)])
        at += n
    return cap_hit, cap_half, bin_off, np.array(sum(rows, []), dtype=np.uint16)


def distances(queries, rows):
    """np_rowdist, the short pairs and the long ones apart (the DP is padded to the longest)."""
    out = np.zeros(len(queries), dtype=np.int64)
    long_ = np.array([len(a) > 400 or len(b) > 400 for a, b in zip(queries, rows)], dtype=bool)
    for sel in (np.flatnonzero(long_), np.flatnonzero(~long_)):
        if len(sel):
            out[sel] = rc.np_rowdist([queries[i] for i in sel], [rows[i] for i in sel])
    return out


def oracle(reads, rows, sel, cap_hit, cap_half, bin_off, bins, chunk=2_000_000, max_chunks=100):
    """The contract, literally.  rows are str.  Returns a dict: best_row, best_d, best_class,
    n_pairs, n_lines, and `pairs`: per compared pair (k, g, L, df, dr or None, line 'f'/'r'/None,
    d, class)."""
    pairs, made, stopped_at = [], 0, None
    for k, r in enumerate(sel):
        la = len(reads[r])
        for g, row in enumerate(rows):
            lb = len(row)
            if la * 1.05 < lb or lb * 1.05 < la:
                continue
            pairs.append((k, g))
            made += 1
        if made // chunk == max_chunks:
            stopped_at = k
            break
    L = [max(len(reads[sel[k]]), len(rows[g])) for k, g in pairs]
    fcap = [max(int(cap_hit[x]), int(cap_half[x]), 0) for x in L]
    df = distances([reads[sel[k]] for k, _ in pairs], [lib.mask_row(rows[g]) for _, g in pairs])
    df = [min(int(d), c + 1) for d, c in zip(df, fcap)]
    again = [i for i, d in enumerate(df)
             if not d <= cap_hit[L[i]] and cap_hit[L[i]] >= 0 and d > cap_half[L[i]]]
    dr = dict(zip(again, distances([reads[sel[pairs[i][0]]] for i in again],
                                   [lib.mask_row(rc.revcomp_row(rows[pairs[i][1]]))
                                    for i in again])))
    n = len(sel)
    best_row = np.full(n, NONE, dtype=np.uint32)
    best_d = np.full(n, NONE, dtype=np.uint32)
    best_class = np.zeros(n, dtype=np.uint16)
    rec, lines = [], 0
    for i, (k, g) in enumerate(pairs):
        ch = int(cap_hit[L[i]])
        kind, d, r = None, df[i], None
        if df[i] <= ch:
            kind = "f"
        elif i in dr:
            r = min(int(dr[i]), ch + 1)
            if r <= ch:
                kind, d = "r", r
        cls = None
        if kind:
            lines += 1
            cls = int(bins[int(bin_off[L[i]]) + d])
            if best_row[k] == NONE or cls >= best_class[k]:   # the last of equal classes wins
                best_row[k], best_class[k] = g, cls
                best_d[k] = d | (REV if kind == "r" else 0)
        rec.append((k, g, L[i], df[i], r, kind, d, cls))
    return dict(best_row=best_row, best_d=best_d, best_class=best_class, n_pairs=len(pairs),
                n_lines=lines, pairs=rec, stopped_at=stopped_at)


def _subs(rng, s: bytes, count: int) -> bytes:
    """s with `count` substitutions at distinct, well separated places."""
    out = bytearray(s)
    for pos in rng.choice(len(s) // 3, count, replace=False) * 3:
        out[pos] = ord("ACGT"[("ACGTN".index(chr(out[pos])) + 1) % 4])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def host_set(seed=91):
    """The CPU set.  41 reads: 1, 2, 63, 64, 65 and 300 nt, 24 mutated copies (2-20 %, every
    fourth reverse-complemented) of two founders of 200 and 204 nt, three unrelated ones of
    211-213 nt, random ones of 1..300 nt, and
    one of 1,200 nt.  14 rows: planted copies of the founders (gap, IUPAC and N columns), reverse
    complements of mutated copies, an unrelated row of 202 columns, a copy of the 64-nt read,
    one of 290 columns, two identical rows, and two rows of 1,200 columns whose distances to the
    long read differ by one and share an identity class.  The read list names read 8 twice.
    The caps of five lengths are then set from the oracle's own forward distances so that the
    edges of both comparisons occur (see coverage()).  Returns (reads, rows as str, sel, tables,
    oracle result)."""
    rng = np.random.default_rng(seed)
    f0, f1 = pc.rand_seq(rng, 200, p_n=0.0), pc.rand_seq(rng, 204, p_n=0.0)
    reads = [pc.rand_seq(rng, n, p_n=0.05) for n in (1, 2, 63, 64, 65, 300)]
    for k in range(24):
        s = pc.mutate(rng, (f0, f1)[k % 2], float(rng.uniform(0.02, 0.2)))
        reads.append(pc.revcomp(s) if k % 4 == 3 else s)
    reads += [pc.rand_seq(rng, n, p_n=0.02) for n in (211, 212, 213)]     # unrelated to every row
    reads += [pc.rand_seq(rng, int(n), p_n=0.05) for n in rng.integers(1, 301, 7)]
    long_ = pc.rand_seq(rng, 1200, p_n=0.0)
    reads.append(long_)
    # two distances at 1,200 nt that round to one class: the step 1 / 1200 is below 0.001
    d_tie = next(d for d in range(5, 60)
                 if sorter.identity(d, 1200) == sorter.identity(d + 1, 1200))
    twin = rc.planted_row(rng, f0, 0.03)
    rows = [rc.planted_row(rng, f0, 0.04), rc.planted_row(rng, f1, 0.05),
            rc.revcomp_row(pc.mutate(rng, f0, 0.03).decode()),
            rc.revcomp_row(rc.planted_row(rng, f1, 0.04)),
            pc.rand_seq(rng, 202, p_n=0.02).decode(),
            twin, pc.mutate(rng, f1, 0.10).decode(), twin,
            gc.plant(rng, pc.mutate(rng, reads[3], 0.05), 0.05),
            pc.mutate(rng, reads[5], 0.04).decode()[:290],
            pc.mutate(rng, f0, 0.15).decode(), pc.mutate(rng, f1, 0.01).decode(),
            _subs(rng, long_, d_tie).decode(), _subs(rng, long_, d_tie + 1).decode()]
    assert rows[5] == rows[7] and len(rows[12]) == len(rows[13]) == 1200
    sel = np.array(list(range(len(reads))) + [8], dtype=np.uint32)
    lengths = sorted({max(len(reads[r]), len(row)) for r in sel for row in rows
                      if not (len(reads[r]) * 1.05 < len(row) or len(row) * 1.05 < len(reads[r]))}
                     | {len(x) for x in reads} | {len(x) for x in rows})
    base = oracle(reads, rows, sel, *tables(lengths, overrides={L: (len(reads[5]), len(reads[5]))
                                                                for L in lengths}))
    # with caps as wide as a length every forward distance is exact: pick the pairs whose
    # length's caps are then moved onto them
    by_len = {}
    for k, g, L, df, _, _, _, _ in base["pairs"]:
        by_len.setdefault(L, []).append((df, k, g))
    far = sorted(L for L, v in by_len.items() if min(x[0] for x in v) > 0.3 * L and L > 40)
    near = sorted(L for L, v in by_len.items()
                  if 2 <= min(x[0] for x in v) <= 0.12 * L and L not in far and L != 1200)
    assert len(far) >= 3 and len(near) >= 2, (far, near)
    over = {far[0]: (None, min(x[0] for x in by_len[far[0]])),          # df == cap_half: no retry
            far[1]: (None, min(x[0] for x in by_len[far[1]]) - 1),      # df == cap_half + 1
            far[2]: (-1, None),                                         # a length without hits
            near[0]: (min(x[0] for x in by_len[near[0]]), None),        # d == cap_hit
            near[1]: (min(x[0] for x in by_len[near[1]]) - 1, None)}    # d == cap_hit + 1
    tb = tables(lengths, overrides=over)
    return reads, rows, sel, tb, oracle(reads, rows, sel, *tb), over


def coverage(case):
    """What the CPU set must show, from the oracle's answers alone."""
    reads, rows, sel, (cap_hit, cap_half, bin_off, bins), exp, over = case
    P = exp["pairs"]
    assert 38 <= len(reads) <= 44 and 12 <= len(rows) <= 14
    assert any(kind == "f" for *_, kind, _, _ in P)
    assert any(kind == "r" for *_, kind, _, _ in P)
    assert any(kind is None and r is not None for _, _, _, _, r, kind, _, _ in P)
    assert any(df == cap_half[L] and r is None and kind is None for _, _, L, df, r, kind, _, _ in P)
    assert any(df == cap_half[L] + 1 and r is not None for _, _, L, df, r, kind, _, _ in P)
    assert any(kind and d == cap_hit[L] for _, _, L, _, _, kind, d, _ in P)
    assert any(kind is None and r is None and df == cap_hit[L] + 1 and cap_hit[L] >= 0
               for _, _, L, df, r, kind, _, _ in P)
    assert any(cap_hit[L] == -1 for _, _, L, *_ in P)
    # a pair dropped by each side of the 5 % rule
    la = [len(reads[r]) for r in sel]
    lb = [len(x) for x in rows]
    assert any(a * 1.05 < b for a in la for b in lb) and any(b * 1.05 < a for a in la for b in lb)
    # a place decided by the row index alone: the two identical rows, the larger index wins
    twins = [k for k in range(len(sel)) if exp["best_row"][k] == 7
             and any(p[:2] == (k, 5) and p[5] and p[7] == exp["best_class"][k] for p in P)]
    assert twins and not (exp["best_row"] == 5).any()
    # a place whose two best lines differ in distance and share a class (1,200 nt)
    k = len(reads) - 1
    top = [p for p in P if p[0] == k and p[5] and p[7] == exp["best_class"][k]]
    assert len(top) == 2 and top[0][6] != top[1][6] and exp["best_row"][k] == top[1][1] == 13
    assert int(exp["best_d"][k]) == top[1][6] > top[0][6]      # not the least distance
    # a read named twice: both places, the same answer
    assert sel[-1] == sel[8] and exp["best_row"][-1] == exp["best_row"][8] != NONE
    assert (exp["best_row"] == NONE).any() and exp["n_lines"] > len(sel) // 2


def same(got, exp, what=""):
    row, d, cls, n_pairs, n_lines = got
    np.testing.assert_array_equal(row, exp["best_row"], err_msg=what + " best_row")
    np.testing.assert_array_equal(d, exp["best_d"], err_msg=what + " best_d")
    np.testing.assert_array_equal(cls, exp["best_class"], err_msg=what + " best_class")
    assert (n_pairs, n_lines) == (exp["n_pairs"], exp["n_lines"]), what


@functools.lru_cache(maxsize=None)
def boundary_set(seed=92):
    """The GPU boundary set: reads of 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097 and 4200 nt
    (group sizes +-1, one and two stripes), each with 3-4 rows made from it that the 5 % rule
    keeps: a planted copy, the reverse complement of a mutated copy, a copy trimmed or padded so
    that the short ones' rows end around multiples of 16 columns, and for every second read an
    unrelated row of the read's length.  Returns (reads, rows as str, sel, tables)."""
    rng = np.random.default_rng(seed)
    reads, rows = [], []
    for j, m in enumerate((1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4200)):
        a = pc.rand_seq(rng, m, p_n=0.02 if m > 1 else 0.0)
        reads.append(a)
        if m == 1:
            rows += [a.decode(), rc.revcomp_row(a.decode()), "N"]
            continue
        rate = 0.04 if m < 200 else 0.02
        rows.append(rc.planted_row(rng, a, rate))
        rows.append(rc.revcomp_row(pc.mutate(rng, a, rate).decode()))
        cut = pc.mutate(rng, a, rate).decode()
        edge = (m + 8) // 16 * 16 + (j % 3 - 1)      # 16 x - 1, 16 x, 16 x + 1 columns
        rows.append((cut + a.decode())[:edge] if m < 200 else cut)
        if j % 2:
            rows.append(pc.rand_seq(rng, m, p_n=0.02).decode())
    sel = np.arange(len(reads), dtype=np.uint32)
    lengths = {len(x) for x in reads} | {len(x) for x in rows}
    lengths |= {max(len(a), len(b)) for a in reads for b in rows}
    return reads, rows, sel, tables(sorted(lengths))
