"""GPU parity of the piece screen against the oracle.

Adversarial reads: every adapter of the 24 x 24 panels with exactly K edits, one in each of K of
its K + 1 pieces (so exactly one piece survives as an exact copy), for every surviving piece, in
both read orientations, at the read start, middle and end; partial adapters at both read ends;
N inside and around the pieces.  The flat scan (dmx_pack layouts, permuted read order, reads
that overlap in the packed batch), the per-part screen (DMX_NO_FLAT=1) and the full filter pass
(DMX_NO_PIECES=1) must all equal the oracle on every result byte.  The seam tests at the end
place the surviving piece on the part boundaries of the per-part screen and on the lane and
superblock seams of the flat scan (pieces_seam_cases.py).
"""
import numpy as np
import pytest

import oracle
from dmx import lib, synth
from test_pieces_host import (SEAM_PANELS, _flank_cases, _seam_case, full_k, mutate, pieces_of,
                              revcomp)
import pieces_seam_cases as sc

pytestmark = pytest.mark.gpu


def _assert_same(got, exp):
    got = got.view(np.uint8).reshape(len(got), -1)
    exp = exp.view(np.uint8).reshape(len(exp), -1)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} reads differ, first {bad[:10]}"


def _rand(rng, n, alphabet="ACGT", p=None):
    return "".join(rng.choice(list(alphabet), size=int(n), p=p))


def adversarial_reads(rng, panel, where, rate=0.1):
    """Reads holding one adapter copy with K edits (one surviving piece), plus partial copies at
    the read ends (a FRONT adapter's suffix at the start, a BACK adapter's prefix at the end)."""
    seqs = []
    for ad in panel:
        K = full_k(len(ad), rate)
        pcs = pieces_of(len(ad), K)
        for survive in range(K + 1):
            for place in ("start", "middle", "end"):
                copy = mutate(rng, ad, pcs, survive)
                L = int(rng.integers(150, 900))
                flank = int(rng.integers(0, 9))
                if place == "start":
                    s = _rand(rng, flank) + copy + _rand(rng, L)
                elif place == "end":
                    s = _rand(rng, L) + copy + _rand(rng, flank)
                else:
                    s = _rand(rng, L // 2) + copy + _rand(rng, L // 2)
                seqs.append(revcomp(s) if rng.random() < 0.5 else s)
        for _ in range(3):   # partial copies at the ends, with up to acc errors of their own
            cut = int(rng.integers(3, len(ad)))
            part = ad[len(ad) - cut:] if where == oracle.FRONT else ad[:cut]
            part = "".join(c if rng.random() > 0.05 else _rand(rng, 1) for c in part)
            s = part + _rand(rng, 300) if where == oracle.FRONT else _rand(rng, 300) + part
            seqs.append(revcomp(s) if rng.random() < 0.5 else s)
    # N inside and around the pieces of otherwise exact copies
    for _ in range(60):
        ad = panel[int(rng.integers(len(panel)))]
        s = list(_rand(rng, 200) + ad + _rand(rng, 200))
        for _ in range(int(rng.integers(1, 4))):
            s[200 + int(rng.integers(-8, len(ad) + 8))] = "N"
        s = "".join(s)
        seqs.append(revcomp(s) if rng.random() < 0.5 else s)
    return seqs + ["", "A", ad[:7], ad[-7:]]


def overlapping(seqs):
    """seqs plus, per read of >= 12 nt, the read without its first 3 and last 4 nt: packed as a
    view into the read's own nt (_run), so the batch holds reads that share nt."""
    return seqs + [s[3:len(s) - 4] for s in seqs if len(s) >= 12]


def _run(seqs, panel, where, layout="sorted", env=None, monkeypatch=None):
    perm = None
    if layout == "overlap":   # results for overlapping(seqs): the sub-reads point into their reads
        blob, offs, lens = oracle.pack_ascii(seqs)
        p = lib.pack(blob, offs, lens)
        src = [i for i in range(len(seqs)) if lens[i] >= 12]
        offs2 = np.concatenate([p.offsets, p.offsets[src] + 3]).astype(p.offsets.dtype)
        lens2 = np.concatenate([p.lengths, p.lengths[src] - 7]).astype(p.lengths.dtype)
        p = lib.Packed(p.seq2b, p.nmask, offs2, lens2)
    else:
        blob, offs, lens = oracle.pack_ascii(seqs)
        p = lib.pack(blob, offs, lens)
    if layout == "permuted":
        perm = np.random.default_rng(1).permutation(p.n_reads)
        p = lib.Packed(p.seq2b, p.nmask, p.offsets[perm].copy(), p.lengths[perm].copy())
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    f = lib.DMX_FRONT if where == oracle.FRONT else lib.DMX_BACK
    with lib.Context(0) as c:
        c.set_panel(0, panel, f | lib.DMX_RC)
        c.set_mode(lib.MODE_SINGLE)
        got = c.run(p)
        tasks = c.stats()["filter_tasks"]
    for k in (env or {}):
        monkeypatch.delenv(k)
    if perm is not None:
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        got = got[inv]
    return got, tasks


@pytest.mark.parametrize("rnd", [0, 1])
@pytest.mark.parametrize("variant", ["flat", "permuted", "overlap", "no_flat", "no_pieces"])
def test_one_surviving_piece(rnd, variant, monkeypatch):
    n1, s5, n2, s27 = synth.panels(24, 24)
    panel, where = (s5, oracle.FRONT) if rnd == 0 else (s27, oracle.BACK)
    rng = np.random.default_rng(100 + rnd)
    seqs = adversarial_reads(rng, panel, where)
    blob, offs, lens = oracle.pack_ascii(overlapping(seqs) if variant == "overlap" else seqs)
    exp = oracle.run_batch(oracle.Panel(panel, where), None, blob, offs, lens, mode=0,
                           use_rc=True, threads=8)
    assert (exp["bin1"] >= 0).mean() > 0.7
    layout = variant if variant in ("permuted", "overlap") else "sorted"
    env = {"no_flat": {"DMX_NO_FLAT": "1"}, "no_pieces": {"DMX_NO_PIECES": "1"}}.get(variant)
    got, tasks = _run(seqs, panel, where, layout, env, monkeypatch)
    _assert_same(got, exp)
    if variant == "no_pieces":
        assert tasks[0] == 0
    else:
        assert tasks[0] > 0   # the piece screen ran


def test_two_round_adversarial(ctx):
    """Both rounds on one batch: SP5 copies with one surviving piece at the read start, SP27rc
    copies with one surviving piece at the end, orientations mixed."""
    n1, s5, n2, s27 = synth.panels(24, 24)
    rng = np.random.default_rng(7)
    seqs = []
    for i in range(3000):
        a, b = s5[i % 24], s27[(i * 7) % 24]
        ka, kb = full_k(len(a), 0.1), full_k(len(b), 0.1)
        ca = mutate(rng, a, pieces_of(len(a), ka), int(rng.integers(ka + 1)))
        cb = mutate(rng, b, pieces_of(len(b), kb), int(rng.integers(kb + 1)))
        s = _rand(rng, rng.integers(0, 9)) + ca + _rand(rng, rng.integers(100, 1500)) + cb + \
            _rand(rng, rng.integers(0, 9))
        seqs.append(revcomp(s) if rng.random() < 0.3 else s)
    blob, offs, lens = oracle.pack_ascii(seqs)
    exp = oracle.run_batch(oracle.Panel(s5, oracle.FRONT), oracle.Panel(s27, oracle.BACK), blob,
                           offs, lens, mode=1, threads=8)
    assert (exp["bin2"] >= 0).mean() > 0.7
    ctx.set_panel(0, s5, lib.DMX_FRONT | lib.DMX_RC)
    ctx.set_panel(1, s27, lib.DMX_BACK | lib.DMX_RC)
    ctx.set_mode(lib.MODE_TWO_ROUND)
    got = ctx.run(lib.pack(blob, offs, lens))
    _assert_same(got, exp)
    assert all(t > 0 for t in ctx.stats()["filter_tasks"])


def test_iupac_panel_falls_back_to_the_full_filter(ctx):
    """A panel with a wildcard builds no pieces: the full filter pass runs (no filter tasks)."""
    rng = np.random.default_rng(9)
    suffix = _rand(rng, 20)
    panel = [_rand(rng, 20) + "N" + _rand(rng, 15) + suffix for _ in range(6)]
    seqs = []
    for _ in range(1500):
        ad = panel[int(rng.integers(6))].replace("N", "ACGT"[int(rng.integers(4))])
        s = _rand(rng, rng.integers(0, 300)) + ad + _rand(rng, rng.integers(0, 300))
        seqs.append(revcomp(s) if rng.random() < 0.5 else s)
    blob, offs, lens = oracle.pack_ascii(seqs)
    exp = oracle.run_batch(oracle.Panel(panel, oracle.BACK), None, blob, offs, lens, mode=0,
                           use_rc=True, threads=8)
    ctx.set_panel(0, panel, lib.DMX_BACK | lib.DMX_RC)
    ctx.set_mode(lib.MODE_SINGLE)
    got = ctx.run(lib.pack(blob, offs, lens))
    _assert_same(got, exp)
    assert ctx.stats()["filter_tasks"][0] == 0


@pytest.mark.parametrize("case", ["iupac_round1", "no_flat"])
def test_two_round_mixed_screens(case, monkeypatch):
    """Round 1 on the full filter pass (a wildcard panel) while round 2 takes the flat scan (its
    marks come from the one scan launched ahead of round 1), and both rounds on the per-part
    screen (DMX_NO_FLAT=1)."""
    n1, s5, n2, s27 = synth.panels(24, 24)
    rng = np.random.default_rng(11)
    p1 = [a[:10] + "N" + a[11:] for a in s5] if case == "iupac_round1" else s5
    seqs = []
    for i in range(2000):
        a = p1[i % 24].replace("N", "ACGT"[int(rng.integers(4))])
        b = s27[(i * 5) % 24]
        kb = full_k(len(b), 0.1)
        cb = mutate(rng, b, pieces_of(len(b), kb), int(rng.integers(kb + 1)))
        s = _rand(rng, rng.integers(0, 9)) + a + _rand(rng, rng.integers(100, 1200)) + cb
        seqs.append(revcomp(s) if rng.random() < 0.4 else s)
    blob, offs, lens = oracle.pack_ascii(seqs)
    exp = oracle.run_batch(oracle.Panel(p1, oracle.FRONT), oracle.Panel(s27, oracle.BACK), blob,
                           offs, lens, mode=1, threads=8)
    assert (exp["bin2"] >= 0).mean() > 0.6
    if case == "no_flat":
        monkeypatch.setenv("DMX_NO_FLAT", "1")
    with lib.Context(0) as c:
        c.set_panel(0, p1, lib.DMX_FRONT | lib.DMX_RC)
        c.set_panel(1, s27, lib.DMX_BACK | lib.DMX_RC)
        c.set_mode(lib.MODE_TWO_ROUND)
        got = c.run(lib.pack(blob, offs, lens))
        tasks = c.stats()["filter_tasks"]
    _assert_same(got, exp)
    assert tasks[1] > 0 and (tasks[0] == 0) == (case == "iupac_round1")


@pytest.mark.parametrize("variant", ["flat", "no_flat"])
@pytest.mark.parametrize("name,panel,where,rate", _flank_cases())
def test_shared_flank_panels(name, panel, where, rate, variant, monkeypatch):
    """Panels whose adapters share a constant prefix and suffix: pieces that straddle a shared
    block sample a window past offset 0 (the tools/parity_sweep.py seed-56 mismatches, when
    offsets 4 .. 8 overflowed the entries' 2-bit field)."""
    w = oracle.FRONT if where == lib.DMX_FRONT else oracle.BACK
    rng = np.random.default_rng(200 + len(name))
    seqs = adversarial_reads(rng, panel, w, rate)
    for ad in panel:   # exact copies at every start modulo the sampling stride
        for shift in range(4):
            s = _rand(rng, 40 + shift) + ad + _rand(rng, 60)
            seqs.append(revcomp(s) if rng.random() < 0.5 else s)
    blob, offs, lens = oracle.pack_ascii(seqs)
    exp = oracle.run_batch(oracle.Panel(panel, w, max_errors=rate), None, blob, offs, lens,
                           mode=0, use_rc=True, threads=8)
    assert (exp["bin1"] >= 0).mean() > 0.5
    if variant == "no_flat":
        monkeypatch.setenv("DMX_NO_FLAT", "1")
    with lib.Context(0) as c:
        c.set_panel(0, panel, where | lib.DMX_RC, rate)
        c.set_mode(lib.MODE_SINGLE)
        got = c.run(lib.pack(blob, offs, lens))
        tasks = c.stats()["filter_tasks"]
    _assert_same(got, exp)
    assert tasks[0] > 0


# ---------------------------------------------------------------------------------------------
# Seams: the surviving piece on a part boundary of the per-part screen, on a lane or superblock
# seam of the flat scan, and block steps of the per-part screen with many items and parts
# ---------------------------------------------------------------------------------------------
def _run_checked(seqs, panel, where, rate, rc, use_perm=False):
    """(results in read order, filter tasks) of one single-round run in a context of its own; the
    pipeline flags show neither a cell outside a part's mask (16) nor a full list (4)."""
    blob, offs, lens = oracle.pack_ascii(seqs)
    p = lib.pack(blob, offs, lens)
    perm = None
    if use_perm:
        perm = np.random.default_rng(2).permutation(p.n_reads)
        p = lib.Packed(p.seq2b, p.nmask, p.offsets[perm].copy(), p.lengths[perm].copy())
    with lib.Context(0) as c:
        c.set_panel(0, list(panel), where | (lib.DMX_RC if rc else 0), rate)
        c.set_mode(lib.MODE_SINGLE)
        got = c.run(p)
        tasks = c.stats()["filter_tasks"]
        flags = int(c.debug_fetch(lib.DBG_FLAGS, 0)[0])
    assert flags & (16 | 4) == 0, flags
    if perm is not None:
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        got = got[inv]
    return got, tasks


def _oracle(seqs, panel, where, rate, rc):
    blob, offs, lens = oracle.pack_ascii(seqs)
    w = oracle.FRONT if where == lib.DMX_FRONT else oracle.BACK
    return oracle.run_batch(oracle.Panel(list(panel), w, max_errors=rate), None, blob, offs, lens,
                            mode=0, use_rc=rc, threads=8)


@pytest.mark.parametrize("part", [64, 0])
@pytest.mark.parametrize("variant", ["no_flat", "one_orientation"])
@pytest.mark.parametrize("name", SEAM_PANELS)
def test_part_seams(name, variant, part, monkeypatch):
    """The seam reads of pieces_seam_cases.py (the surviving piece starts at b - 3 .. b + 1 of
    the first and last interior part boundary b, both strands) through the per-part screen: with
    both orientations (DMX_NO_FLAT=1) and as a one-orientation panel, which always takes it; with
    64-position parts in reads of 160 nt and with the table's own parts in reads of 2.5 parts."""
    rc = variant == "no_flat"
    panel, where, rate = sc.panel(name)
    seqs = _seam_case(name, rc, part, monkeypatch)[0]   # (sets DMX_PIECE_PART)
    exp = _oracle(seqs, panel, where, rate, rc)
    assert (exp["bin1"] >= 0).mean() > 0.7
    if rc:
        monkeypatch.setenv("DMX_NO_FLAT", "1")
    got, tasks = _run_checked(seqs, panel, where, rate, rc)
    _assert_same(got, exp)
    assert tasks[0] > 0


@pytest.mark.parametrize("where", [lib.DMX_FRONT, lib.DMX_BACK])
def test_many_parts_per_block(where, monkeypatch):
    """Per-part screen with 64-position parts over 1500 reads of 0 .. 1000 nt: a block step holds
    512 items and thousands of (item, part) tasks (the prefix search, the task loop), views of
    0 parts (an empty FRONT view), of 1 part (an empty BACK view: its last-column window; reads
    of 1 .. 64 nt) and of up to 16; the adapter copy (one surviving piece) in a random part."""
    n1, s5, n2, s27 = synth.panels(24, 24)
    panel = s5 if where == lib.DMX_FRONT else s27
    rng = np.random.default_rng(300 + where)
    seqs = []
    for i in range(1500):
        ad = panel[i % 24]
        K = full_k(len(ad), 0.1)
        copy = mutate(rng, ad, pieces_of(len(ad), K), int(rng.integers(K + 1)))
        n = int(rng.integers(0, 1001))
        if n < len(copy) + 2:
            s = _rand(rng, n)
        else:
            left = int(rng.integers(0, n - len(copy) + 1))
            s = _rand(rng, left) + copy + _rand(rng, n - left - len(copy))
        seqs.append(revcomp(s) if rng.random() < 0.5 else s)
    seqs[0], seqs[1], seqs[700], seqs[701], seqs[-2], seqs[-1] = "", "G", "", "T", "C", ""
    assert sum(sc.part_len(len(s), 64) and -(-len(s) // sc.part_len(len(s), 64))
               for s in seqs[:512]) > 8 * 256
    exp = _oracle(seqs, panel, where, 0.1, True)
    assert (exp["bin1"] >= 0).mean() > 0.7
    monkeypatch.setenv("DMX_NO_FLAT", "1")
    monkeypatch.setenv("DMX_PIECE_PART", "64")
    got, tasks = _run_checked(seqs, panel, where, 0.1, True)
    _assert_same(got, exp)
    assert tasks[0] > 0


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("name", ["sp5", "flank3"])
def test_flat_scan_seams(name, flip):
    """The flat scan with the surviving piece's copy starting at batch nt 64 j + d (lane seams:
    the neighbour's words come by shuffles) and 4096 s + d (superblock seams: the LDS copy's 4
    words before and after), d = -19 .. 3, on both strands; a copy starting at the first read's
    first nt and one ending at the last read's last nt.  The permuted batch reads the same marks
    by batch nt."""
    panel, where, rate = sc.panel(name)
    seqs, meta = sc.flat_seam_reads(np.random.default_rng(400 + flip), panel, rate, flip)
    for kind in ("lane", "superblock"):
        assert {(d, s) for k, _, d, s in meta if k == kind} == \
            {(d, s) for d in sc.FLAT_D for s in (0, 1)}
    blob, offs, lens = oracle.pack_ascii(seqs)
    p = lib.pack(blob, offs, lens)
    for (kind, nt, d, s), o, n in zip(meta, p.offsets.tolist(), p.lengths.tolist()):
        assert o <= nt - min(d, 0) < o + n     # the seam lies in the read that holds the copy
        assert (nt - d) % (4096 if kind == "superblock" else 64 if kind == "lane" else 1) == 0
    assert meta[0][1] == p.offsets[0] and meta[-1][1] == p.offsets[-1] + p.lengths[-1] - 1
    exp = _oracle(seqs, panel, where, rate, True)
    assert (exp["bin1"] >= 0).mean() > 0.7
    for use_perm in (False, True):
        got, tasks = _run_checked(seqs, panel, where, rate, True, use_perm)
        _assert_same(got, exp)
        assert tasks[0] > 0
