"""Near-start 5' cells inside the shared suffix (`DevPanel::near_shared`): the
panel flag on the host, and the argument behind it by brute force.

A last-row cell (m_a, j) with j <= jS = |S| - max kk lies, with every alignment of cost <= kk that
ends there, inside the shared suffix S, so its cost, score and aligned length are the same for
every adapter; where the acceptance tables agree on lengths <= |S| the adapters accept it alike.
No GPU: `dmx_panel_near_shared` builds the panel on the host.
"""
import numpy as np
import pytest

from dmx import lib, synth

ACGT = list("ACGT")
PRE, SUF = 10, 12


def _dna(rng, n):
    return "".join(rng.choice(ACGT, size=n)) if n > 0 else ""


def _pis(rng, ls, pre=PRE, suf=SUF):
    """P + I_a + S with index blocks of the given lengths, distinct in their first and last nt
    (so that neither P nor S grows by a common nt of the blocks)."""
    P, S = _dna(rng, pre), _dna(rng, suf)
    out = []
    for i, l in enumerate(ls):
        b = list(_dna(rng, l))
        b[0] = ACGT[i % 4]
        b[-1] = ACGT[(i + (0 if l == 1 else 1)) % 4]
        out.append(P + "".join(b) + S)
    assert len(set(out)) == len(out)
    return out


def _tables(m, rate, min_overlap=3):
    """acc[L] (the largest accepted cost of an alignment of L adapter chars: cost <= L * rate in
    IEEE double, -1 below min_overlap) and its prefix maximum pacc, as cutadapt accepts matches."""
    acc, pacc, kk = [], [], -1
    for L in range(m + 1):
        a = -1
        if L >= min_overlap:
            a = 0
            while float(a + 1) <= L * rate:
                a += 1
        acc.append(a)
        kk = max(kk, a)
        pacc.append(kk)
    return acc, pacc


def _info(seqs, flags, e=0.1, wheres=None):
    rc, info = lib.panel_near_shared(seqs, flags, e, 3, wheres)
    assert rc == 0
    return info


def test_sp5_panel_flag():
    """The synthetic 24 x 24 SP5 panel at -e 0.1: S of 17 nt, 5 errors at most, jsplit as the
    index screen has it (m - pre_len + kk = 59 - 25 + 5)."""
    sp5 = synth.generate("c2x24", n=10)["sp5"]
    assert len(sp5) == 24 and {len(s) for s in sp5} == {59}
    info = _info(sp5, lib.DMX_FRONT | lib.DMX_RC)
    assert info == {"near_shared": 12, "filter_len": 17, "jsplit": 39, "kk": 5}
    assert _info(sp5, lib.DMX_FRONT)["near_shared"] == 12       # without --rc too


def test_switch_forces_every_adapter(monkeypatch):
    sp5 = synth.generate("c2x24", n=10)["sp5"]
    monkeypatch.setenv("DMX_NEAR_ALL", "1")
    info = _info(sp5, lib.DMX_FRONT | lib.DMX_RC)
    assert info == {"near_shared": -1, "filter_len": 17, "jsplit": 39, "kk": 5}


def test_unequal_lengths_keep_the_flag():
    """Index blocks of 1 and 32 nt: m = 23 and 54, 2 and 5 errors at most.  The tables differ
    above |S| (54 rows accept more) and agree on 0..|S|, which is all the flag needs."""
    rng = np.random.default_rng(11)
    pan = _pis(rng, [1, 32, 1, 32, 32, 1])
    ms = sorted({len(s) for s in pan})
    assert ms == [PRE + 1 + SUF, PRE + 32 + SUF]
    t = [_tables(m, 0.1) for m in ms]
    for x in range(SUF + 1):
        assert t[0][0][x] == t[1][0][x] and t[0][1][x] == t[1][1][x]
    assert t[0][1][-1] == 2 and t[1][1][-1] == 5
    info = _info(pan, lib.DMX_FRONT | lib.DMX_RC)
    assert info["filter_len"] == SUF and info["kk"] == 5
    assert info["near_shared"] == SUF - 5
    assert info["jsplit"] == 32 + SUF + 5
    # an absolute error count gives each length its own rate: 2 / 23 accepts one error in 12
    # rows, 2 / 54 none, so the tables differ inside S
    a, b = _tables(ms[0], 2.0 / ms[0]), _tables(ms[1], 2.0 / ms[1])
    assert a[0][SUF] != b[0][SUF]
    assert _info(pan, lib.DMX_FRONT | lib.DMX_RC, e=2.0)["near_shared"] == -1


def test_panels_without_the_flag():
    rng = np.random.default_rng(12)
    pan = _pis(rng, [8] * 6)                                   # m = 30
    assert _info(pan, lib.DMX_FRONT | lib.DMX_RC)["near_shared"] == SUF - 3
    # a 3' panel
    back = _info(pan, lib.DMX_BACK | lib.DMX_RC)
    assert back["filter_len"] == SUF and back["near_shared"] == -1
    # a mixed panel
    wh = [lib.DMX_FRONT, lib.DMX_BACK] * 3
    assert _info(pan, lib.DMX_RC, wheres=wh)["near_shared"] == -1
    assert _info(pan, lib.DMX_RC, wheres=[lib.DMX_FRONT] * 6)["near_shared"] == SUF - 3
    # |S| <= kk: at -e 0.45 a 30-nt adapter takes 13 errors, more than S has rows
    hi = _info(pan, lib.DMX_FRONT | lib.DMX_RC, e=0.45)
    assert hi["kk"] == 13 and hi["filter_len"] <= hi["kk"] and hi["near_shared"] == -1
    # an error rate that leaves jS = |S| - kk = 0: -e 0.4 takes 12 errors; one less, jS = 1
    zero = _info(pan, lib.DMX_FRONT | lib.DMX_RC, e=0.4)
    assert zero["kk"] == SUF and zero["near_shared"] == -1
    one = _info(pan, lib.DMX_FRONT | lib.DMX_RC, e=0.39)
    assert one["kk"] == SUF - 1 and one["filter_len"] == SUF and one["near_shared"] == 1
    # no shared suffix block at all (the filter is off)
    loose = [_dna(rng, 30) for _ in range(6)]
    off = _info(loose, lib.DMX_FRONT | lib.DMX_RC)
    assert off["filter_len"] == 0 and off["near_shared"] == -1


def _last_row(ad, read, jmax, rate, min_overlap=3):
    """The 5' DP of cutadapt's Aligner.locate as oracle/pyref.py restates it (column 0 free:
    cost 0, score 0, origin -i; equal characters take the diagonal; else a mismatch if it costs
    no more than either indel, else the insertion if it costs no more than the deletion; +1 / -1
    / -2).  Returns, per column j = 1..jmax, the last-row cell as (cost, score, aligned rows) if
    cutadapt accepts it, else None."""
    m = len(ad)
    col = [(0, 0, -i) for i in range(m + 1)]
    out = []
    for j in range(1, jmax + 1):
        new = [(0, 0, j)]
        c = read[j - 1]
        for i in range(1, m + 1):
            d, up, left = col[i - 1], new[i - 1], col[i]
            if ad[i - 1] == c:
                new.append((d[0], d[1] + 1, d[2]))
            elif d[0] <= left[0] and d[0] <= up[0]:
                new.append((d[0] + 1, d[1] - 1, d[2]))
            elif up[0] <= left[0]:
                new.append((up[0] + 1, up[1] - 2, up[2]))
            else:
                new.append((left[0] + 1, left[1] - 2, left[2]))
        col = new
        cost, score, origin = col[m]
        lr = m + min(origin, 0)
        out.append((cost, score, lr) if lr >= min_overlap and cost <= lr * rate else None)
    return out


def _start_reads(rng, pan, suf, n):
    """20-nt read prefixes: random ones, and tails of S (or of an adapter, a few rows past S)
    with 0..2 edits in front of random bases, where near cells are accepted."""
    reads = [_dna(rng, 20) for _ in range(n // 4)]
    while len(reads) < n:
        a = pan[int(rng.integers(len(pan)))]
        s = list(a[-int(rng.integers(3, suf + 4)):])
        for _ in range(int(rng.integers(0, 3))):
            p = int(rng.integers(len(s)))
            u = rng.random()
            if u < 0.6:
                s[p] = ACGT[int(rng.integers(4))]
            elif u < 0.8:
                del s[p]
            else:
                s.insert(p, ACGT[int(rng.integers(4))])
        reads.append(("".join(s) + _dna(rng, 20))[:20])
    return reads


@pytest.mark.parametrize("case", ["sp5", "l8", "l17", "l1_32", "suf20"])
def test_near_cells_are_the_same_for_every_adapter(case):
    """For every column j <= near_shared and every read prefix the accepted last-row cell (cost,
    score, aligned rows; or its rejection) is the same for every adapter of the panel, and the
    same as that of the adapter's last r rows alone, r = 4..20, wherever r >= j + kk: the cell
    sees nothing above those rows."""
    rng = np.random.default_rng({"sp5": 1, "l8": 2, "l17": 3, "l1_32": 4, "suf20": 5}[case])
    if case == "sp5":
        pan = synth.generate("c2x24", n=10)["sp5"]
    elif case == "l8":
        pan = _pis(rng, [8] * 6)
    elif case == "l17":
        pan = _pis(rng, [17] * 6)
    elif case == "l1_32":
        pan = _pis(rng, [1, 32, 32, 1, 17])
    else:
        pan = _pis(rng, [20] * 5, pre=12, suf=20)               # m = 52: 5 errors, jS = 15
    info = _info(pan, lib.DMX_FRONT | lib.DMX_RC)
    jS, sl, kk = info["near_shared"], info["filter_len"], info["kk"]
    assert jS == sl - kk and jS >= 1
    reads = _start_reads(rng, pan, sl, 24)
    accepted = 0
    for rd in reads:
        cells = [_last_row(ad, rd, jS, 0.1) for ad in pan]
        for c in cells[1:]:
            assert c == cells[0], (rd, cells[0], c)
        accepted += sum(x is not None for x in cells[0])
        # rows of S alone are one string for the whole panel; longer suffixes per adapter
        for r in range(4, 21):
            tails = {ad[-r:] for ad in pan} if r > sl else {pan[0][-r:]}
            for t in tails:
                if len(t) < r:
                    continue
                got = _last_row(t, rd, min(jS, r - kk), 0.1)
                assert got == cells[0][:len(got)], (rd, r, got)
    assert accepted > 0   # the reads do reach accepted near cells
