"""Anchored and non-internal adapters on the host (no GPU).

dmx_ends_host, the full-matrix twin of the end-window stage, against a demux oracle written in
ends_cases.py from oracle.locate with cutadapt's EndSkip flags (^A: QUERY_STOP, XA: REF_START |
QUERY_STOP, A$: QUERY_START, AX: QUERY_START | REF_END), best_match and --rc.  oracle.locate
keeps one column and Ukkonen's cut-off as _align.pyx does; it is itself checked here against an
independent full-matrix DP in numpy.  cutadapt is not installed: parity with it is unpinned."""

import numpy as np
import pytest

import ends_cases as ec
import oracle
from dmx import lib


def numpy_locate(ref: str, query: str, rate: float, flags: int, min_overlap: int):
    """Aligner.locate by a full (m + 1) x (n + 1) matrix over every column of the read: no column
    range, no cut-off.  Restricted to what the four flag sets need; returns locate's tuple."""
    sr, sq, er, eq = bool(flags & 1), bool(flags & 2), bool(flags & 4), bool(flags & 8)
    m, n = len(ref), len(query)
    k = int(rate * m)
    wild = not set(ref) <= set("ACGT")
    iupac = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3,
             "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}
    acgt = {"A": 1, "C": 2, "G": 4, "T": 8}
    ncount = np.concatenate([[0], np.cumsum([c == "N" for c in ref])])
    eff_all = m - int(ncount[m]) if wild else m
    min_n, max_n = 0, n   # locate's own range is [max(0, n - m - k), n] or [0, min(n, m + k)]
    cost = np.zeros((m + 1, n + 1), dtype=np.int64)
    score = np.zeros_like(cost)
    orig = np.zeros_like(cost)
    for i in range(m + 1):
        if not sr and not sq:
            cost[i, min_n], score[i, min_n], orig[i, min_n] = max(i, min_n), -2 * max(i, min_n), 0
        elif sr and not sq:
            cost[i, min_n], score[i, min_n], orig[i, min_n] = min_n, 0, min(0, min_n - i)
        elif sq and not sr:
            cost[i, min_n], score[i, min_n], orig[i, min_n] = i, -2 * i, max(0, min_n - i)
        else:
            cost[i, min_n], score[i, min_n], orig[i, min_n] = min(i, min_n), 0, min_n - i
    best = None

    def offer(i, j):
        nonlocal best
        length = i + min(int(orig[i, j]), 0)
        eff = length
        if wild:
            eff = length - int(ncount[max(length, 0)]) if length < m else eff_all
        if length < min_overlap or float(cost[i, j]) > eff * rate:
            return
        if best is None or score[i, j] > best[0] or (score[i, j] == best[0] and cost[i, j] < best[1]):
            best = (int(score[i, j]), int(cost[i, j]), int(orig[i, j]), i, j)

    for j in range(min_n + 1, max_n + 1):
        if sq:
            cost[0, j], score[0, j], orig[0, j] = cost[0, j - 1], score[0, j - 1], j
        else:
            cost[0, j], score[0, j], orig[0, j] = j, -2 * j, orig[0, j - 1]
        for i in range(1, m + 1):
            if wild:
                same = bool(iupac[ref[i - 1]] & acgt.get(query[j - 1], 0))
            else:
                same = ref[i - 1] == query[j - 1]
            d, u, l = (i - 1, j - 1), (i - 1, j), (i, j - 1)
            if same:
                cost[i, j], score[i, j], orig[i, j] = cost[d], score[d] + 1, orig[d]
            elif cost[d] <= cost[l] and cost[d] <= cost[u]:
                cost[i, j], score[i, j], orig[i, j] = cost[d] + 1, score[d] - 1, orig[d]
            elif cost[u] <= cost[l]:
                cost[i, j], score[i, j], orig[i, j] = cost[u] + 1, score[u] - 2, orig[u]
            else:
                cost[i, j], score[i, j], orig[i, j] = cost[l] + 1, score[l] - 2, orig[l]
        if eq:
            offer(m, j)
    if max_n == n:
        for i in range(0 if er else m, m + 1):
            offer(i, n)
    if best is None:
        return None
    s, c, o, i, j = best
    return (0 if o >= 0 else -o, i, o if o >= 0 else 0, j, s, c)


@pytest.mark.parametrize("where", ec.RESTRICTED)
def test_oracle_locate_equals_full_matrix_dp(where):
    """oracle.locate with each restricted flag set against the numpy full-matrix DP on 300 random
    (adapter, read) pairs: planted copies with substitutions and indels, cut-off copies, short
    and empty reads, N in reads and adapters, rates 0 .. 0.4."""
    rng = np.random.default_rng(1000 + where)
    flags = ec.FLAGS[where]
    hits = 0
    for it in range(300):
        m = int(rng.integers(1, 26))
        ad = ec._rand(rng, m, "ACGT" * 6 + "N" if it % 5 == 0 else "ACGT")
        if set(ad) == {"N"}:
            ad = "A" + ad[1:]
        rate = float(rng.choice([0.0, 0.1, 0.2, 0.25, 0.4]))
        mo = m if where & ec.ANCH else int(rng.integers(1, 6))
        piece = ad.replace("N", "C")
        if where & ec.NONI and rng.random() < 0.5:
            c = int(rng.integers(0, m))
            piece = piece[c:] if where & ec.F else piece[:m - c]
        if len(piece) > 1:
            piece = ec._sub(rng, piece, int(rng.integers(0, min(3, len(piece)))))
        if piece and rng.random() < 0.3:
            i = int(rng.integers(len(piece)))
            piece = piece[:i] + piece[i + 1:] if rng.random() < 0.5 else piece[:i] + "G" + piece[i:]
        read = ec._place(where, piece, ec._rand(rng, int(rng.integers(0, 50)), "ACGT" * 8 + "N"))
        if rng.random() < 0.15:
            read = ec._rand(rng, int(rng.integers(0, 4)))
        exp = numpy_locate(ad, read, rate, flags, mo)
        got = oracle.locate(ad, read, rate, flags, mo)
        assert got == exp, (ad, read, rate, mo)
        hits += exp is not None
    assert 60 <= hits <= 290, hits


def test_case_set_covers_every_stratum():
    cov = ec.coverage(ec.groups())
    missing = ec.required_coverage() - cov
    assert not missing, sorted(map(str, missing))


def test_ends_host_equals_the_demux_oracle():
    """All 40 bytes of every record, every group of the case set."""
    n = 0
    for g in ec.groups():
        got = lib.ends_host(g.seqs, g.wheres, g.packed(), g.rc, g.e, g.overlap)
        exp = g.expected()
        bad = np.nonzero(got.view(np.uint8).reshape(len(got), -1) !=
                         exp.view(np.uint8).reshape(len(exp), -1))[0]
        assert len(bad) == 0, (g.name, g.labels[bad[0]], g.reads[bad[0]], got[bad[0]], exp[bad[0]])
        n += len(got)
    assert n > 1500


def test_ends_host_per_adapter_min_overlap():
    """min_overlaps[a] replaces -O for adapter a; an anchored adapter ignores both."""
    ad = "ACGTTGCAAGGCTTAACCGA"
    reads = [ad[-4:] + "TTTTTTTTTTTTTTTT", ad + "TTTT"]
    blob, offs, lens = oracle.pack_ascii(reads)
    p = lib.pack(blob, offs, lens)
    for mo, hit in ((4, True), (5, False)):
        got = lib.ends_host([ad], [ec.FRONTX], p, False, 0.1, 9, [mo])
        assert (got["bin1"][0] == 0) == hit
        assert got["bin1"][1] == 0
    got = lib.ends_host([ad], [ec.PREFIX], p, False, 0.1, 3, [4])
    assert got["bin1"].tolist() == [-1, 0]


def test_abi_has_the_new_entry_points_and_refuses_bad_bits():
    L = lib.load()
    assert hasattr(L, "dmx_set_panel_ex") and hasattr(L, "dmx_ends_host")
    assert (lib.DMX_ANCHORED, lib.DMX_NONINTERNAL) == (0x04, 0x08)
    blob, offs, lens = oracle.pack_ascii(["ACGT"])
    p = lib.pack(blob, offs, lens)
    for wh in (lib.DMX_FRONT | lib.DMX_ANCHORED | lib.DMX_NONINTERNAL, lib.DMX_ANCHORED,
               lib.DMX_FRONT | lib.DMX_BACK | lib.DMX_ANCHORED, 0x20 | lib.DMX_FRONT):
        with pytest.raises(lib.DmxError, match=r"\(-1\)"):
            lib.ends_host(["ACGT"], [wh], p, False)
    # the reach of a panel is that of its unrestricted adapters; restricted ones add nothing
    seqs = ["ACGTACGTACGTAAGGTTCC", "TTGACCATGACCATGGATCA"]
    rc0, r0 = lib.panel_reach(seqs[:1], lib.DMX_FRONT | lib.DMX_RC, 0.1, 3)
    rc1, r1 = lib.panel_reach(seqs, lib.DMX_RC, 0.1, 3, wheres=[lib.DMX_FRONT, ec.SUFFIX])
    rc2, r2 = lib.panel_reach(seqs, lib.DMX_RC, 0.1, 3, wheres=[ec.PREFIX, ec.BACKX])
    assert (rc0, rc1, rc2) == (0, 0, 0)
    assert r1 == r0 and r2["need_pre"] <= r2["guard"] and r2["need_post"] <= r2["guard"]
