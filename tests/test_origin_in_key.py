"""The winner key of a band-mode round carries its origin.

A band-mode round publishes, with the one 64-bit atomicMin that picks a slot's winner, the path's
start diagonal against the end cell's own: delta = origin - (j - iend), |delta| <= cost <= kk <= 7,
stored as delta + 8 in the 4 bits below the scan position.  finalize rebuilds the origin from the
end cell the key already names.  In a Match that is

    delta = (rstart - astart) - (rstop - astop)

(an alignment with c inserted read bases ends c columns right of its start diagonal: delta = -c;
with c deleted ones, delta = +c).  Every case below is built so that the ORACLE's winners take
every delta in [-kk, kk] for each panel; that is asserted first, on the CPU (test_inputs_cover_*
also runs without a GPU).  Then the GPU's results are compared with the oracle's: every field of
every read, the per-bin counts, and flags == 0 — once in band mode (origin from the key) and once
in ring mode (DMX_RESOLVE=ring: origin from the per-slot array), so the per-round flag is shown
to pick the right decode.
"""
import functools
import os

import numpy as np
import pytest

import oracle
from dmx import lib, panel, synth

_COMP = str.maketrans("ACGTN", "TGCAN")


def _rc(s):
    return s.translate(_COMP)[::-1]


def _dna(rng, n):
    return "".join(rng.choice(list("ACGT"), size=int(n)))


def _indel_copy(rng, a, c, kind, lo, hi, gap=4):
    """A copy of adapter `a` with exactly c inserted (kind 'ins') or c deleted ('del') bases at
    positions in [lo, hi) that are at least `gap` apart, so the cheapest alignment is the c
    indels."""
    if c == 0:
        return a
    while True:
        pos = np.sort(rng.choice(np.arange(lo, hi), size=c, replace=False))
        if c == 1 or np.diff(pos).min() >= gap:
            break
    out = list(a)
    for p in pos[::-1]:
        p = int(p)
        if kind == "del":
            del out[p]
        else:   # a base that differs from both neighbours: no cheaper mismatch reading
            b = [x for x in "ACGT" if x != a[p - 1] and x != a[p]]
            out.insert(p, b[int(rng.integers(len(b)))])
    return "".join(out)


def _shape(rng, kk, short):
    """(c, kind, partial): exact copies, c = 1..kk indels of one kind, a third of them partial."""
    c = int(rng.integers(0, kk + 1))
    kind = "ins" if rng.random() < 0.5 else "del"
    return c, kind, (rng.random() < 0.33 and not short)


def _two_round_reads(rng, sp5, sp27, kk, n, margin):
    """[flank] + SP5 copy + body + SP27 copy + [flank], each copy with its own indels; partial
    copies lose 1..3 characters off the read's start (FRONT: origin < 0) or end (BACK: a
    last-column cell, t > len); half the reads are reverse-complemented; a few carry nothing."""
    seqs = []
    for _ in range(n):
        if rng.random() < 0.03:
            seqs.append(_dna(rng, rng.integers(0, 300)))
            continue
        a5 = sp5[int(rng.integers(len(sp5)))]
        a27 = sp27[int(rng.integers(len(sp27)))]
        c1, k1, part1 = _shape(rng, kk, False)
        c2, k2, part2 = _shape(rng, kk, False)
        # a partial copy keeps its indels away from the cut end (they stay interior edits)
        f = _indel_copy(rng, a5, c1, k1, margin + (4 if part1 else 0), len(a5) - margin)
        b = _indel_copy(rng, a27, c2, k2, margin, len(a27) - margin - (4 if part2 else 0))
        left = "" if part1 else _dna(rng, rng.integers(0, 50))
        right = "" if part2 else _dna(rng, rng.integers(0, 50))
        if part1:
            f = f[int(rng.integers(1, 4)):]
        if part2:
            b = b[:len(b) - int(rng.integers(1, 4))]
        s = left + f + _dna(rng, rng.integers(40, 200)) + b + right
        seqs.append(_rc(s) if rng.random() < 0.5 else s)
    return seqs


def _short_reads(rng, p1, p2, kk, n):
    """9-nt adapters at -e 3 -O 2: an accepted match may score <= 0 (a copy with 3 deleted bases
    scores 9 - 3 - 6 = 0), so the round keeps one winner slot per orientation.  Such a match wins
    only where nothing scores above 0, so most reads are the two copies and at most two bases
    before, between and after them; the indels are strictly inside the copies."""
    seqs = []
    for i in range(n):
        parts = []
        for pn in (p1, p2):
            a = pn[int(rng.integers(len(pn)))]
            c = int(rng.integers(0, kk + 1))
            kind = "ins" if rng.random() < 0.5 else "del"
            parts.append(_indel_copy(rng, a, c, kind, 2, len(a) - 2, gap=2))
        flank = i % 4 == 0   # some with random sequence around the copies
        if i % 4 == 1:       # and some with the first panel's copy alone
            parts[1] = ""
        s = (_dna(rng, rng.integers(0, 12 if flank else 3)) + parts[0] +
             _dna(rng, rng.integers(0, 12 if flank else 3)) + parts[1] +
             _dna(rng, rng.integers(0, 12 if flank else 3)))
        seqs.append(_rc(s) if rng.random() < 0.5 else s)
    return seqs


_IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT",
          "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


def _linked_reads(rng, pairs, kk, n):
    """F + body + R amplicons of the COI primer pairs (`-g F...R`), IUPAC codes resolved, each
    primer with c = 0..kk indels in its interior; some primers cut at the read's end."""
    seqs = []
    for _ in range(n):
        f, r = pairs[int(rng.integers(len(pairs)))]
        out = []
        for x, (pr, front) in enumerate(((f, True), (r, False))):
            a = "".join(_IUPAC[ch][int(rng.integers(len(_IUPAC[ch])))] for ch in pr)
            c, kind, part = _shape(rng, kk, False)
            a = _indel_copy(rng, a, c, kind, 5 + (4 if part and front else 0),
                            len(a) - 5 - (4 if part and not front else 0))
            if part:
                a = a[int(rng.integers(1, 3)):] if front else a[:len(a) - int(rng.integers(1, 3))]
            out.append((a, part))
        (fs, pf), (rs, pr_) = out
        seqs.append(("" if pf else _dna(rng, rng.integers(0, 30))) + fs +
                    _dna(rng, rng.integers(60, 300)) + rs +
                    ("" if pr_ else _dna(rng, rng.integers(0, 30))))
    return seqs


# name -> (mode, kk, max_errors, min_overlap, rc)
CASES = {
    "e0.1_kk5": (lib.MODE_TWO_ROUND, 5, 0.1, 3, True),       # 59 / 57 nt: int(0.1 m) = 5
    "e0.125_kk7": (lib.MODE_TWO_ROUND, 7, 0.125, 3, True),   # int(0.125 m) = 7: band_wide
    "nonpos_kk3": (lib.MODE_TWO_ROUND, 3, 3, 2, True),       # one slot per orientation
    "linked_coi_kk2": (lib.MODE_LINKED, 2, 0.1, 3, False),   # 22..26 counted characters
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(panel 0, panel 1, blob, offsets, lengths, the oracle's results): computed once."""
    mode, kk, e, mo, rc = CASES[name]
    rng = np.random.default_rng({"e0.1_kk5": 501, "e0.125_kk7": 701, "nonpos_kk3": 303,
                                 "linked_coi_kk2": 201}[name])
    if name == "nonpos_kk3":
        p0 = ["".join(rng.choice(list("ACGT"), size=9)) for _ in range(2)]
        p1 = ["".join(rng.choice(list("ACGT"), size=9)) for _ in range(2)]
        seqs = _short_reads(rng, p0, p1, kk, 4000)
    elif mode == lib.MODE_LINKED:
        fa = os.path.join(os.path.dirname(panel.SP5_FASTA), "COI_primers.fa")
        pairs = [(f, r) for _, f, r in panel.primer_pairs(fa)]
        p0, p1 = [p[0] for p in pairs], [p[1] for p in pairs]
        seqs = _linked_reads(rng, pairs, kk, 3000)
    else:
        d = synth.generate("c2x24", n=8)
        p0, p1 = list(d["sp5"]), list(d["sp27"])
        seqs = _two_round_reads(rng, p0, p1, kk, 4000, 8)
    seqs += ["", "A", p0[0], p1[0], p0[0] + p1[0]]
    blob, offs, lens = oracle.pack_ascii(seqs)
    exp = oracle.run_batch(oracle.Panel(p0, oracle.FRONT, max_errors=e, min_overlap=mo),
                           oracle.Panel(p1, oracle.BACK, max_errors=e, min_overlap=mo),
                           blob, offs, lens, mode=2 if mode == lib.MODE_LINKED else 1,
                           use_rc=rc, threads=8)
    exp.setflags(write=False)
    return p0, p1, blob, offs, lens, exp


def _deltas(exp, m, binf):
    """delta of the oracle's winner of one round, for the reads that have one."""
    has = exp[binf] >= 0
    f = {k: exp[f"{m}_{k}"][has].astype(np.int64) for k in ("rstart", "astart", "rstop", "astop")}
    return (f["rstart"] - f["astart"]) - (f["rstop"] - f["astop"]), exp[f"{m}_errors"][has]


def _assert_inputs_cover(name):
    """The condition on the inputs: each panel's winners take every delta in [-kk, kk], among
    them FRONT partials (origin < 0) and BACK last-column cells with a nonzero delta, and both
    orientations."""
    mode, kk, _, _, rc = CASES[name]
    _, p1, _, _, lens, exp = _case(name)
    for m, binf in (("m1", "bin1"), ("m2", "bin2")):
        dl, err = _deltas(exp, m, binf)
        assert np.all(np.abs(dl) <= err) and err.max() == kk, (name, m)
        missing = sorted(set(range(-kk, kk + 1)) - set(dl.tolist()))
        assert not missing, f"{name} {m}: no winner with delta {missing}"
    if name == "nonpos_kk3":
        assert (exp["m1_score"][exp["bin1"] >= 0] <= 0).any()
        return
    d1, _ = _deltas(exp, "m1", "bin1")
    neg = exp["m1_astart"][exp["bin1"] >= 0] > 0               # FRONT partial: origin < 0
    assert (d1[neg] > 0).any() and (d1[neg] < 0).any(), name
    d2, _ = _deltas(exp, "m2", "bin2")
    m2 = np.array([len(s) for s in p1])[exp["bin2"][exp["bin2"] >= 0]]
    cut = exp["m2_astop"][exp["bin2"] >= 0] < m2                # BACK last-column cell
    assert (d2[cut] > 0).any() and (d2[cut] < 0).any(), name
    if rc:
        assert exp["rc1"].any() and not exp["rc1"].all()


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_cover_every_delta(name):
    _assert_inputs_cover(name)


def _expected_counts(name, exp, a0, a1):
    mode = CASES[name][0]
    n = (a0 + 1) * (a1 + 1)
    c = np.zeros(n + 2, dtype=np.uint64)
    if mode == lib.MODE_LINKED:   # pair a in bin (a + 1, a + 1), untrimmed reads in bin 0
        b = exp["bin1"].astype(np.int64) + 1
        np.add.at(c, b * (a0 + 1) + b, 1)
        return c
    b = (exp["bin1"].astype(np.int64) + 1) * (a1 + 1) + exp["bin2"].astype(np.int64) + 1
    c[:n] = np.bincount(b, minlength=n)
    c[n] = int(exp["rc1"].sum())
    c[n + 1] = int(exp["rc2"].sum())
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("resolve", ["band", "ring"])
@pytest.mark.parametrize("name", list(CASES))
def test_origin_from_key_matches_oracle(name, resolve, monkeypatch):
    _assert_inputs_cover(name)
    mode, _, e, mo, rc = CASES[name]
    p0, p1, blob, offs, lens, exp = _case(name)
    if resolve == "ring":
        monkeypatch.setenv("DMX_RESOLVE", "ring")
    f = lib.DMX_RC if rc else 0
    with lib.Context(0) as c:
        c.set_panel(0, p0, lib.DMX_FRONT | f, e, mo)
        c.set_panel(1, p1, lib.DMX_BACK | f, e, mo)
        c.set_mode(mode)
        got = c.run(lib.pack(blob, offs, lens)).view(oracle.RESULT_DTYPE)
        counts = c.counts()
        flags = c.stats()["flags"]
    for fld in oracle.RESULT_DTYPE.names:
        bad = np.nonzero(got[fld] != exp[fld])[0]
        assert len(bad) == 0, f"{fld}: {len(bad)} reads differ, first {bad[:10]}"
    assert got.tobytes() == exp.tobytes()
    assert np.array_equal(counts, _expected_counts(name, exp, len(p0), len(p1)))
    assert flags == 0
