"""dmx_pairalign_host (include/dmx.h) against a full-matrix DP and traceback
written here: the distance, the path op for op, and the properties every NW path has.  Hand cases
pin the tie rule (up, then left, then the diagonal).  lib.cigar and sorter.gapped on the same
cases.  No GPU."""
import functools
import re

import numpy as np
import pytest

import pairdist_cases as pc
from dmx import lib, sorter


def dp_path(a: bytes, b: bytes):
    """(distance, ops) of query a (rows) against target b (columns): the whole matrix, then the
    walk back from (m, n) by the contract's rule."""
    m, n = len(a), len(b)
    A = np.frombuffer(a, dtype=np.uint8)
    B = np.frombuffer(b, dtype=np.uint8)
    D = np.zeros((m + 1, n + 1), dtype=np.int32)
    D[0] = np.arange(n + 1)
    ar = np.arange(n + 1)
    for i in range(1, m + 1):
        c = np.empty(n + 1, dtype=np.int32)
        c[0] = i
        c[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (A[i - 1] != B))
        D[i] = np.minimum.accumulate(c - ar) + ar
    ops = []
    i, j = m, n
    while i or j:
        if j == 0:
            ops.append(lib.PA_INSERT)
            i -= 1
        elif i == 0:
            ops.append(lib.PA_DELETE)
            j -= 1
        elif D[i - 1, j] + 1 == D[i, j]:
            ops.append(lib.PA_INSERT)
            i -= 1
        elif D[i, j - 1] + 1 == D[i, j]:
            ops.append(lib.PA_DELETE)
            j -= 1
        else:
            ops.append(lib.PA_MATCH if a[i - 1] == b[j - 1] else lib.PA_MISMATCH)
            i -= 1
            j -= 1
    return int(D[m, n]), ops[::-1]


def replay(a: bytes, b: bytes, ops):
    """Walk the ops over both sequences: (query consumed, target consumed, MATCH only on equal
    symbols and MISMATCH only on different ones)."""
    i = j = 0
    ok = True
    for op in ops:
        if op in (lib.PA_MATCH, lib.PA_MISMATCH):
            if i >= len(a) or j >= len(b):
                return i, j, False
            ok &= (a[i] == b[j]) == (op == lib.PA_MATCH)
            i += 1
            j += 1
        elif op == lib.PA_INSERT:
            i += 1
        elif op == lib.PA_DELETE:
            j += 1
        else:
            ok = False
    return i, j, ok


@functools.lru_cache(maxsize=None)
def small_set():
    """300 random ACGTN pairs of 1..120 nt, unrelated and mutated, a random RC flag each, and
    their (distance, ops) by dp_path: computed once, shared."""
    reads, q, t, flags, _ = pc.random_set(n_pairs=300, max_len=120, seed=5)
    exp = [dp_path(reads[a], pc.revcomp(reads[b]) if f else reads[b])
           for a, b, f in zip(q, t, flags)]
    return reads, q, t, flags, exp


def paths(off, ops):
    return [ops[int(off[i]):int(off[i + 1])].tolist() for i in range(len(off) - 1)]


def test_random_pairs_equal_the_numpy_dp_and_replay():
    reads, q, t, flags, exp = small_set()
    p = pc.pack_reads(reads)
    dist, off, ops = lib.pairalign_host(p, q, t, flags, n_threads=4)
    assert off[0] == 0 and len(off) == len(q) + 1 and off[-1] == len(ops)
    nw = lib.pairdist_host(p, q, t, lib.PD_NW, flags)
    got = paths(off, ops)
    for k in range(len(q)):
        a = reads[q[k]]
        b = pc.revcomp(reads[t[k]]) if flags[k] else reads[t[k]]
        assert replay(a, b, got[k]) == (len(a), len(b), True), k
        assert sum(op != lib.PA_MATCH for op in got[k]) == dist[k] == nw[k] == exp[k][0], k
        assert got[k] == exp[k][1], k
    # one thread and no flags: the same calls, pair by pair
    d1, o1, p1 = lib.pairalign_host(p, q, t, flags, n_threads=1)
    assert (d1 == dist).all() and (o1 == off).all() and (p1 == ops).all()
    d0, o0, p0 = lib.pairalign_host(p, q[:40], t[:40])
    for k, path in enumerate(paths(o0, p0)):
        assert (int(d0[k]), path) == dp_path(reads[q[k]], reads[t[k]]), k


M, I, D, X = lib.PA_MATCH, lib.PA_INSERT, lib.PA_DELETE, lib.PA_MISMATCH
HAND = [
    # query, target, distance, ops, cigar, extended cigar, (target row, query row)
    # homopolymers: the surplus is taken last (up / left are tried before the diagonal at
    # (m, n)), so it comes at the END of the forward path
    (b"AAAA", b"AAA", 1, [M, M, M, I], "3M1I", "3=1I", ("AAA-", "AAAA")),
    (b"AAA", b"AAAA", 1, [M, M, M, D], "3M1D", "3=1D", ("AAAA", "AAA-")),
    (b"AAAAAA", b"AA", 4, [M, M, I, I, I, I], "2M4I", "2=4I", ("AA----", "AAAAAA")),
    (b"AAAA", b"CCCC", 4, [X, X, X, X], "4M", "4X", ("CCCC", "AAAA")),
    (b"AAA", b"CC", 3, [X, X, I], "2M1I", "2X1I", ("CC-", "AAA")),
    (b"A", b"CCAC", 3, [D, D, M, D], "2D1M1D", "2D1=1D", ("CCAC", "--A-")),
    (b"CCAC", b"A", 3, [I, I, M, I], "2I1M1I", "2I1=1I", ("--A-", "CCAC")),
    (b"G", b"T", 1, [X], "1M", "1X", ("T", "G")),
    (b"N", b"N", 0, [M], "1M", "1=", ("N", "N")),
    (b"N", b"A", 1, [X], "1M", "1X", ("A", "N")),
    (b"ANA", b"AAA", 1, [M, X, M], "3M", "1=1X1=", ("AAA", "ANA")),
    # a tie between a gap early and a gap late: up is preferred at the end of the walk back,
    # so the insert sits as late as the distance allows
    (b"ACGT", b"AGT", 1, [M, I, M, M], "1M1I2M", "1=1I2=", ("A-GT", "ACGT")),
    (b"AGT", b"ACGT", 1, [M, D, M, M], "1M1D2M", "1=1D2=", ("ACGT", "A-GT")),
]


@pytest.mark.parametrize("case", HAND, ids=[f"{c[0].decode()}-{c[1].decode()}" for c in HAND])
def test_hand_cases_pin_the_tie_rule(case):
    a, b, d, ops, cg, cgx, rows = case
    assert dp_path(a, b) == (d, ops)          # the test's own DP agrees with the hand path
    p = pc.pack_reads([a, b])
    dist, off, got = lib.pairalign_host(p, [0], [1])
    assert dist.tolist() == [d] and off.tolist() == [0, len(ops)] and got.tolist() == ops
    assert lib.cigar(got) == cg
    assert lib.cigar(got, extended=True) == cgx
    assert sorter.gapped(a, b, got) == rows
    assert sorter.gapped(a.decode(), b.decode(), got) == rows


def test_rc_flag_reads_the_target_backwards():
    p = pc.pack_reads([b"AACGN", b"NCGTA"])            # revcomp(NCGTA) = TACGN
    dist, off, ops = lib.pairalign_host(p, [0], [1], flags=[lib.PD_RC])
    assert (int(dist[0]), ops.tolist()) == dp_path(b"AACGN", b"TACGN") == (1, [X, M, M, M, M])


def test_cigar_and_gapped_edges():
    assert lib.cigar([]) == "" and lib.cigar(np.zeros(0, dtype=np.uint8), True) == ""
    assert lib.cigar([M, X, X, I, I, D, M]) == "3M2I1D1M"
    assert lib.cigar([M, X, X, I, I, D, M], extended=True) == "1=2X2I1D1="
    with pytest.raises(lib.DmxError):
        lib.cigar([0, 4])
    with pytest.raises(lib.DmxError):
        sorter.gapped(b"ACG", b"AC", [M, M])            # a path that leaves a query symbol over
    # the rows are what create_alignment's list edits make (amplicon_sorter.py:340-355)
    q, t, ops = "ACGGT", "CGTT", [I, M, M, X, M]
    tl, ql, ins = list(t), list(q), []
    scorelist = []
    for cnt, y in re.findall(r"(\d+)(\D)", lib.cigar(ops, extended=True)):
        scorelist += int(cnt) * [y]
    assert scorelist == ["I", "=", "=", "X", "="]
    for i, y in enumerate(scorelist):
        if y == "I":
            ins.append(i)
        if y == "D":
            ql.insert(i, "-")
    for i in ins:
        tl.insert(i, "-")
    assert sorter.gapped(q, t, ops) == ("".join(tl), "".join(ql)) == ("-CGTT", "ACGGT")


def test_refusals():
    reads = [b"ACGT" * 5, b"", b"ACGTT" * 4]
    p = pc.pack_reads(reads)
    dist, off, ops = lib.pairalign_host(p, [0], [2])
    assert int(dist[0]) == dp_path(reads[0], reads[2])[0] and off[-1] == len(ops)
    with pytest.raises(lib.DmxError, match=r"\(-1\).*ops_cap"):
        lib.pairalign_host(p, [0, 0], [2, 2], ops_cap=79)     # 2 x (20 + 20) needed
    lib.pairalign_host(p, [0, 0], [2, 2], ops_cap=80)
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        lib.pairalign_host(p, [0, 3], [2, 2])                 # an index >= n_reads
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        lib.pairalign_host(p, [0], [2], flags=[2])            # an unknown flag
    with pytest.raises(lib.DmxError, match=r"\(-4\)"):
        lib.pairalign_host(p, [0, 1], [2, 2])                 # a zero-length read
    d, off, ops = lib.pairalign_host(p, [], [])
    assert len(d) == 0 and off.tolist() == [0] and len(ops) == 0


def test_cigars_equal_edlib_where_it_is_installed():
    """The standing pin of the tie rule against edlib itself (not installed everywhere)."""
    edlib = pytest.importorskip("edlib")
    reads, q, t, flags, _ = small_set()
    p = pc.pack_reads(reads)
    dist, off, ops = lib.pairalign_host(p, q, t, flags, n_threads=4)
    for k, path in enumerate(paths(off, ops)):
        a = reads[q[k]].decode()
        b = (pc.revcomp(reads[t[k]]) if flags[k] else reads[t[k]]).decode()
        r = edlib.align(a, b, mode="NW", task="path")
        assert r["editDistance"] == dist[k], k
        assert r["cigar"] == lib.cigar(np.array(path, dtype=np.uint8), extended=True), k
