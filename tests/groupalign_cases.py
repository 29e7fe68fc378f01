"""The in-test model of dmx_groupalign and shared inputs of its tests (test_groupalign_host.py and
test_consensus.py on the CPU, test_groupalign.py on the GPU).  The model is written from the
contract alone: a numpy full-matrix DP with the mask equality, the walk back
by the tie rule up / left / diagonal, Python lists with insert() for the rows, and per-column
counting with first occurrence down the rows."""
import numpy as np

import pairdist_cases as pc
from dmx import lib

SYMS = "ACGTN"
# what a row symbol equals among the query's symbols
EQUALS = {"A": "A", "C": "C", "G": "G", "T": "T", "N": "N", "-": "", "R": "AG", "Y": "CT",
          "M": "AC", "K": "GT", "S": "GC", "W": "AT"}
M, I, D, X = lib.PA_MATCH, lib.PA_INSERT, lib.PA_DELETE, lib.PA_MISMATCH


def model_path(q: str, row: list):
    """(distance, ops in forward order) of query q against the row's symbols."""
    m, n = len(q), len(row)
    eq = np.zeros((m, n), dtype=bool)
    for j, ch in enumerate(row):
        for s in EQUALS[ch]:
            eq[:, j] |= np.frombuffer(q.encode(), dtype=np.uint8) == ord(s)
    ar = np.arange(n + 1, dtype=np.int64)
    Dm = np.zeros((m + 1, n + 1), dtype=np.int64)
    Dm[0] = ar
    c = np.empty(n + 1, dtype=np.int64)
    for i in range(1, m + 1):
        c[0] = i
        np.minimum(Dm[i - 1, 1:] + 1, Dm[i - 1, :-1] + ~eq[i - 1], out=c[1:])
        Dm[i] = np.minimum.accumulate(c - ar) + ar
    ops, i, j = [], m, n
    while i > 0 or j > 0:
        if j == 0:
            ops.append(I), (i := i - 1)
        elif i == 0:
            ops.append(D), (j := j - 1)
        elif Dm[i - 1, j] + 1 == Dm[i, j]:
            ops.append(I), (i := i - 1)
        elif Dm[i, j - 1] + 1 == Dm[i, j]:
            ops.append(D), (j := j - 1)
        else:
            ops.append(M if eq[i - 1, j - 1] else X)
            i, j = i - 1, j - 1
    return int(Dm[m, n]), ops[::-1]


def model_alignment(seed: str, reads):
    """create_alignment by the contract: (rows as lists of symbols, distances, paths)."""
    rows = [list(seed)]
    dists, paths = [], []
    for r in reads:
        r = r.decode() if isinstance(r, bytes) else r
        d, ops = model_path(r, rows[0])
        q = list(r)
        inserts = []
        for col, op in enumerate(ops):
            if op == I:
                inserts.append(col)
            if op == D:
                q.insert(col, "-")
        for col in inserts:
            for z in rows:
                z.insert(col, "-")
        rows.append(q)
        dists.append(d)
        paths.append(ops)
    assert len({len(z) for z in rows}) == 1
    return rows, dists, paths


def model_columns(rows):
    """mask of row 0, count and first over the member rows 1.., as dmx_groupalign reports them."""
    n = len(rows[0])
    mask = np.array([sum(1 << SYMS.index(s) for s in EQUALS[ch]) for ch in rows[0]],
                    dtype=np.uint8).reshape(n)
    count = np.zeros((n, 5), dtype=np.uint16)
    first = np.zeros((n, 5), dtype=np.uint16)
    for k, z in enumerate(rows[1:], 1):
        for y, ch in enumerate(z):
            if ch != "-":
                c = SYMS.index(ch)
                if count[y, c] == 0:
                    first[y, c] = k
                count[y, c] += 1
    return mask, count, first


def group_slices(res, g):
    """Group g of a groupalign result: (mask, count, first, dist, [paths])."""
    lo, hi = int(res["col_off"][g]), int(res["col_off"][g + 1])
    m0, m1 = int(res["member_off"][g]), int(res["member_off"][g + 1])
    paths = None
    if "ops" in res:
        paths = [res["ops"][int(res["op_off"][x]):int(res["op_off"][x + 1])] for x in range(m0, m1)]
    return res["mask"][lo:hi], res["count"][lo:hi], res["first"][lo:hi], res["dist"][m0:m1], paths


def same_result(got, exp):
    for name in ("col_off", "mask", "count", "first", "dist", "op_off", "ops"):
        assert (name in got) == (name in exp), name
        if name in exp:
            g, e = got[name], exp[name]
            assert g.dtype == e.dtype and g.shape == e.shape, (name, g.shape, e.shape)
            bad = np.argwhere(g != e)
            assert len(bad) == 0, (name, bad[:10].tolist())


def plant(rng, s: bytes, rate=0.05) -> str:
    """A seed row: s with '-' and IUPAC columns planted."""
    a = list(s.decode())
    for k in range(len(a)):
        if rng.random() < rate:
            a[k] = "-RYMKSW"[rng.integers(7)]
    return "".join(a)


def boundary_case():
    """GPU case (a): members of 1, 63, 64, 65, 128, 129 nt and 64 G - 1, 64 G, 64 G + 1 for every
    group size, two per group (mutated copies of the group's seed, so round 2 meets a gapped
    row); the seeds are 5 or 11 columns short of a multiple of 16, so the rows cross one when
    the first member inserts.  Returns (reads, seeds, groups)."""
    rng = np.random.default_rng(71)
    lens = {1, 63, 64, 65, 128, 129}
    for g in lib.pairdist_group_sizes():
        lens |= {64 * g - 1, 64 * g, 64 * g + 1}
    reads, seeds, groups = [], [], []
    for k, m in enumerate(sorted(lens)):
        n = max(((m + 15) // 16) * 16 - (5 if k % 2 else 11), 3)
        base = pc.rand_seq(rng, n)
        a = (pc.mutate(rng, base, 0.08) + pc.rand_seq(rng, m))[:m]
        b = pc.mutate(rng, a, 0.08)
        seeds.append(base.decode())
        groups.append([len(reads), len(reads) + 1])
        reads += [a, b]
    return reads, seeds, groups
