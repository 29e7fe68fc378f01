"""The call sequence of test_rowset_sequence.py: nine calls of the three row forms (dmx_rowassign,
dmx_rowdist, dmx_rowpairdist / dmx_rowhits) on one context, each on a row set of its own, so that
what a call leaves on the device (the rows, their reverse complements, whether those were
written) is what the next call must not rely on.  Every step's expectation is its host twin's.

Rows of 1, 15, 16, 17, 63, 64 and 65 columns (the 16-column pad: one short, exact, one over; the
word of 64 rows likewise); reads of 15..70 nt made from the rows so that dmx_rowassign's 5 % rule
pairs them; every step a few dozen pairs, run with DMX_PD_CHUNK=7: several launches each."""
import functools

import numpy as np

import operands_cases as oc
import pairdist_cases as pc
import rowassign_cases as ra
import rowdist_cases as rc
from dmx import lib

CHUNK = "7"
ROW_LENGTHS = (1, 15, 16, 17, 63, 64, 65)


def _fit(rng, s: bytes, n: int) -> bytes:
    """A mutated copy of s, cut or padded to n nt."""
    m = pc.mutate(rng, s, 0.06)
    return (m + pc.rand_seq(rng, n, p_n=0.0))[:n]


@functools.lru_cache(maxsize=None)
def case(seed=4107):
    """reads (bytes), their packed batch, the operand table of step 3 with its repacked batch,
    and the steps: (name, call, args).  The founders of the rows are f[L]; rows(tag) makes a
    fresh set of planted copies (gap, IUPAC and N columns) trimmed to the seven lengths."""
    rng = np.random.default_rng(seed)
    f = {L: pc.rand_seq(rng, L, p_n=0.0) for L in ROW_LENGTHS}

    def rows(lengths, flip=()):
        out = []
        for L in lengths:
            s = (rc.planted_row(rng, f[L], 0.05) + f[L].decode())[:L]
            out.append(rc.revcomp_row(s) if L in flip else s)
        return out

    # reads: per founder of 15 nt and more, copies of the founder's length (the short ones) or
    # within 5 % of it, every third one reverse-complemented: its only line is the retry's
    reads = []
    for L in ROW_LENGTHS[1:]:
        for k in range(6):
            n = L if L < 20 else L + (k % 5) - 2
            s = _fit(rng, f[L], n)
            reads.append(pc.revcomp(s) if k % 3 == 2 else s)
    reads += [pc.rand_seq(rng, n, p_n=0.05) for n in (15, 33, 70)]
    assert {len(x) for x in reads} >= {15, 16, 17, 61, 63, 64, 65, 67, 70}
    assert all(15 <= len(x) <= 70 for x in reads)
    sel = np.arange(len(reads), dtype=np.uint32)

    def tables(rws, no_retry):
        ln = sorted({len(x) for x in reads} | {len(x) for x in rws} |
                    {max(len(a), len(b)) for a in reads for b in rws})
        # a cap_half as wide as the length: no distance is above it, so nothing retries; a third
        # of the length: every pair that is not a near copy does
        return ra.tables(ln, threshold=0.8,
                         overrides={L: (None, L if no_retry else L // 3) for L in ln})

    rows1 = rows(ROW_LENGTHS)
    rows2 = rows((64, 16, 65), flip=(16,))
    # operands: sub-ranges of the reads on alternating strands; the strand-1 ones read the copies
    ops = [(k, 1, len(reads[k]) - (k % 3), (k // 4) % 2) for k in range(0, len(reads), 4)]
    tab = oc.table_arrays(ops)
    n_ops = len(ops)
    rows3 = rows((17, 1, 65, 15, 63), flip=(65,))
    q3 = np.repeat(np.arange(n_ops, dtype=np.uint32), len(rows3))
    r3 = np.tile(np.arange(len(rows3), dtype=np.uint32), n_ops)
    rows4 = rows((16, 64, 1))
    q4 = np.repeat(sel[::3], len(rows4))
    r4 = np.tile(np.arange(len(rows4), dtype=np.uint32), len(sel[::3]))
    rows5 = rows(ROW_LENGTHS[::-1], flip=(63, 15)) + rows((64, 65))
    n5 = len(rows5)
    pairs5 = np.array([(i, j) for i in range(n5) for j in range(n5) if i != j][::2], np.uint32)
    flags5 = (rng.random(len(pairs5)) < 0.5).astype(np.uint8) * lib.PD_RC
    rows6 = rows(ROW_LENGTHS) + rows(ROW_LENGTHS, flip=ROW_LENGTHS) + rows((65, 64, 63))
    n6 = len(rows6)
    pairs6 = np.array([(i, (i * 5 + k) % n6) for i in range(n6) for k in (1, 2, 3)], np.uint32)
    rows7 = rows((63, 64, 65, 15, 16, 17, 1), flip=(64, 17)) + rows((63, 65), flip=(63,))
    n7 = len(rows7)
    pairs7 = np.array([(i, j) for i in range(n7) for j in range(i + 1, n7)], np.uint32)
    cap7 = np.array([max(len(rows7[i]), len(rows7[j])) // 4 if (i + j) % 5 else -1
                     for i, j in pairs7], np.int32)
    rows8 = rows((65, 17, 63, 15, 64, 16), flip=(17, 64))
    rows9 = rows((64, 15, 1, 63, 16), flip=(15, 63))
    q9 = np.repeat(np.arange(n_ops, dtype=np.uint32), len(rows9))
    r9 = np.tile(np.arange(len(rows9), dtype=np.uint32), n_ops)
    steps = [
        ("1 rowassign, some pair retries", "rowassign", (rows1, sel, *tables(rows1, False))),
        ("2 rowassign, none retries, smaller row set", "rowassign",
         (rows2, sel, *tables(rows2, True))),
        ("3 rowdist on operands, strand-1 queries", "rowdist", (rows3, q3, r3)),
        ("4 rowdist, operands cleared", "rowdist", (rows4, q4, r4)),
        ("5 rowpairdist with PD_RC flags", "rowpairdist",
         (rows5, pairs5[:, 0], pairs5[:, 1], lib.PD_HW, flags5)),
        ("6 rowpairdist without flags, larger row set", "rowpairdist",
         (rows6, pairs6[:, 0], pairs6[:, 1], lib.PD_NW, None)),
        ("7 rowhits", "rowhits", (rows7, pairs7[:, 0], pairs7[:, 1], cap7, lib.PD_HW)),
        # every form keeps a PdRows of its own: the two read forms once more, on other rows, so
        # that each of them needs fresh copies after a call of its own that wrote none
        ("8 rowassign again, some pair retries", "rowassign", (rows8, sel, *tables(rows8, False))),
        ("9 rowdist on operands again", "rowdist", (rows9, q9, r9)),
    ]
    for _, call, args in steps:
        assert 24 <= len(args[1]) <= 100       # a few dozen pairs (rowassign: places)
    assert (tab[3] == 1).any() and (tab[3] == 0).any()
    return dict(reads=reads, packed=pc.pack_reads(reads), tab=tab, steps=steps,
                repacked=oc.pack(oc.extract([x.decode() for x in reads], tab)))


def expected(c, k):
    """Step k by its host twin, as a list of arrays."""
    name, call, args = c["steps"][k]
    if call == "rowassign":
        row, d, cls, n_pairs, n_lines = lib.rowassign_host(c["packed"], *args, n_threads=8)
        return [row, d, cls, np.array([n_pairs, n_lines])]
    if call == "rowdist":
        p = c["repacked"] if "on operands" in name else c["packed"]
        return [lib.rowdist_host(p, *args, n_threads=8)]
    if call == "rowpairdist":
        return [lib.rowpairdist_host(*args, n_threads=8)]
    return list(lib.rowhits_host(*args, n_threads=8))


def run(ctx, c, k):
    """Step k on the context; the first step loads the batch, the operand table is set for the
    steps on operands alone."""
    name, call, args = c["steps"][k]
    if k == 0:
        ctx.load(c["packed"])
    if "on operands" in name:
        ctx.set_operands(*c["tab"])
    try:
        got = getattr(ctx, call)(*args)
    finally:
        if "on operands" in name:
            ctx.clear_operands()
    if call == "rowassign":
        return [got[0], got[1], got[2], np.array(got[3:])]
    return list(got) if isinstance(got, tuple) else [got]


def check_coverage(c, exp):
    """What the sequence must show, from the host twins' answers alone."""
    REV, NONE = lib.LG_REV, lib.LG_NONE
    d1, d2 = exp[0][1], exp[1][1]
    assert ((d1 != NONE) & ((d1 & REV) != 0)).any()          # step 1: a retry made a line
    assert ((d1 != NONE) & ((d1 & REV) == 0)).any()
    assert ((exp[7][1] != NONE) & ((exp[7][1] & REV) != 0)).any()   # step 8 likewise
    assert (d2 != NONE).any() and not ((d2 != NONE) & ((d2 & REV) != 0)).any()
    assert exp[0][3][0] >= 30 and exp[1][3][0] >= 24         # pairs: several launches of 7
    flags5 = c["steps"][4][2][4]
    assert (flags5 != 0).any() and (flags5 == 0).any()
    pair, d, rev = exp[6]
    assert (rev == 1).any() and (rev == 0).any() and len(pair) < len(c["steps"][6][2][1])
