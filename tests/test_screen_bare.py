"""The packed index screen with bare groups: warm-up columns run without the
cost update and the running minimum, and the cost comes back from the vertical deltas before the
first counted group.  P + I + S panels with index blocks of 1, 8, 16, 17 and 32 nt, 5' and 3',
both orientations, against the oracle, the one-lane-per-adapter screen and no screen.

The reads put the first counted column of a lane on every offset 0..15 of a 16-column chunk and
give lanes of 1 to 5 chunks (checked from the verified windows, with the kernel's own column
arithmetic); 3' adapters cut at the read end run the partial-I rows behind bare chunks; N falls in
warm-up and in counted columns; 5' adapters cut by leading bases behind a short flank make near
pieces.
"""
import numpy as np
import pytest

import oracle
from dmx import lib, synth

pytestmark = pytest.mark.gpu

PRE, SUF = 10, 12
ACGT = list("ACGT")


def _dna(rng, n):
    return "".join(rng.choice(ACGT, size=n)) if n > 0 else ""


def _rc(s):
    import pyref
    return pyref.revcomp(s)


def _panel(rng, l):
    """P + I_a + S with index blocks of exactly l nt (all four 1-nt blocks for l = 1)."""
    P, S = _dna(rng, PRE), _dna(rng, SUF)
    if l == 1:
        return [P + c + S for c in ACGT]
    blocks = set()
    while len(blocks) < 10:   # 4 + 4 + 2: a partial quad
        blocks.add(_dna(rng, l))
    blocks = sorted(blocks)
    assert len({b[0] for b in blocks}) > 1 and len({b[-1] for b in blocks}) > 1
    return [P + b + S for b in blocks]


def _edit(rng, a, k):
    """k edits (substitution, deletion or insertion) at random places of a."""
    a = list(a)
    for _ in range(k):
        if not a:
            break
        p = int(rng.integers(len(a)))
        u = rng.random()
        if u < 0.6:
            a[p] = ACGT[int(rng.integers(4))]
        elif u < 0.8:
            del a[p]
        else:
            a.insert(p, ACGT[int(rng.integers(4))])
    return "".join(a)


def _with_n(rng, s, lo, hi):
    """One or two N within s[lo:hi]."""
    s = list(s)
    for _ in range(int(rng.integers(1, 3))):
        if hi > lo:
            s[int(rng.integers(max(0, lo), min(len(s), hi)))] = "N"
    return "".join(s)


def _reads(rng, pan, front, n, other):
    """n reads around copies of pan's adapters; 3' reads start with an adapter of the round-1
    panel `other`, so that round 2 runs on them."""
    m = len(pan[0])
    K = int(0.1 * m)
    seqs = []
    for i in range(n):
        a = pan[int(rng.integers(len(pan)))]
        a = _edit(rng, a, int(rng.integers(0, K + 2)))
        second = ""
        if rng.random() < 0.4:   # a second copy 0..40 nt on: wider windows, more chunks
            b = _edit(rng, pan[int(rng.integers(len(pan)))], int(rng.integers(0, K + 1)))
            second = _dna(rng, int(rng.integers(0, 41))) + b
        body = _dna(rng, int(rng.integers(20, 70)))
        if front:
            flank = int(rng.integers(0, m + 26))
            if rng.random() < 0.3:   # cut by leading bases behind a short flank: near pieces
                a = a[int(rng.integers(0, m)):]
                flank = int(rng.integers(0, m + 6))
            s = _dna(rng, flank) + a + second + body
            pos = flank
        else:
            tail = int(rng.integers(0, 26)) if rng.random() < 0.7 else 0
            if tail == 0 and rng.random() < 0.6:   # cut at the read end: partial-I rows
                a = a[:int(rng.integers(1, len(a) + 1))]
                second = ""
            head = other[int(rng.integers(len(other)))] if rng.random() < 0.85 else ""
            s = head + body + a + second + _dna(rng, tail if not second else 0)
            pos = len(head) + len(body)
        if rng.random() < 0.3:   # N before the adapter (warm-up columns) and inside it
            s = _with_n(rng, s, pos - 25, pos + m)
        if i % 2:
            s = _rc(s)
        assert len(s) <= 300
        seqs.append(s)
    return seqs + ["", "A", pan[0], pan[-1][:PRE + 1], pan[1][PRE:]]


def _lane_shapes(w, l, m, front):
    """(chunks, offset of the first counted column in its chunk) of every scanning lane, as
    iscreen4_kernel computes them (all blocks l nt, so every quad of a window has one shape)."""
    pl, sl, kk = PRE, SUF, int(0.1 * m)
    kf = kk
    jsplit = l + sl + kk if front else 0
    j1, j2 = w["j1"].astype(np.int64), w["j2"].astype(np.int64)
    ln = w["len"].astype(np.int64)
    bm = w["bmin"].astype(np.int64)
    dP = (w["info"] & 255).astype(np.int64)
    lastc = (w["lastcol"] != 0) & (not front)
    jr = np.maximum(j1, jsplit)
    rows = (bm != 255) & (jr <= j2) & (kk - bm - dP >= 0)
    big = np.int64(1 << 30)
    x1 = np.where(rows, jr - l - sl - kf, big)
    x1 = np.where(lastc, np.minimum(x1, ln - (m - 1 - pl) - kf), x1)
    xe = np.where(lastc, ln, np.minimum(j2 - sl + kf, ln))
    xq = np.minimum(np.where(rows, jr - sl - kf, big), np.where(lastc, ln - sl + 1 - kf, big))
    need = (rows | lastc) & (ln > 0)
    nch = (xe - x1 + 15) >> 4
    jb = xe - 16 * nch
    ok = need & (nch > 0)
    return nch[ok], (xq[ok] - jb[ok] - 1) % 16


def _same(got, exp):
    got = got.view(np.uint8).reshape(len(got), -1)
    exp = exp.view(np.uint8).reshape(len(exp), -1)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} reads differ, first {bad[:10]}"


def _sorted_tasks(t):
    """The task set: every field but the item number and the slot tag above the view's offset
    (both depend on the order in which earlier kernels appended their lists)."""
    cols = [t["off"] & np.uint64((1 << 36) - 1)] + [t[f].astype(np.uint64) for f in
            ("o", "lastcol", "strand", "bmin", "j1", "j2", "n", "start", "len", "info")]
    b = np.stack(cols, axis=1)
    return b[np.lexsort(b.T[::-1])]


@pytest.mark.parametrize("where", ["front", "back"])
@pytest.mark.parametrize("l", [1, 8, 16, 17, 32])
def test_bare_groups(l, where, monkeypatch):
    """Results byte-equal to the oracle with the packed screen, the one-lane-per-adapter screen
    and no screen, no pipeline flag set.  Where every block fits a 16-bit half the packed screen
    emits the one-lane-per-adapter screen's task set and the window scan finds the same number of
    candidate cells (so it does on the parent commit; the band DP count is left out, it depends on
    the order in which winners become known).  Longer blocks are cut to 16 rows: never fewer
    tasks."""
    front = where == "front"
    rng = np.random.default_rng(7000 + 10 * l + front)
    pan = _panel(rng, l)
    m = len(pan[0])
    d = synth.generate("c2", n=300, seed=l)
    seqs = _reads(rng, pan, front, 6000, d["sp5"]) + [s[:300] for s in synth.to_strings(d)]
    blob, offs, lens = oracle.pack_ascii(seqs)
    p1, p2 = (pan, d["sp27"]) if front else (d["sp5"], pan)
    r = 0 if front else 1
    exp = oracle.run_batch(oracle.Panel(p1, oracle.FRONT), oracle.Panel(p2, oracle.BACK), blob,
                           offs, lens, mode=1, threads=8)
    packed = lib.pack(blob, offs, lens)
    stats, tasks = {}, {}
    for variant in ("packed", "v1", "none"):
        monkeypatch.delenv("DMX_SCREEN_V1", raising=False)
        monkeypatch.delenv("DMX_NO_SCREEN", raising=False)
        if variant == "v1":
            monkeypatch.setenv("DMX_SCREEN_V1", "1")
        if variant == "none":
            monkeypatch.setenv("DMX_NO_SCREEN", "1")
        with lib.Context(0) as c:
            c.set_panel(0, p1, lib.DMX_FRONT | lib.DMX_RC)
            c.set_panel(1, p2, lib.DMX_BACK | lib.DMX_RC)
            c.load(packed)
            if front and variant != "none":   # the window and task lists belong to the last round
                c.set_mode(lib.MODE_SINGLE)
                c.exec()
                c.sync()
                tasks[variant] = _sorted_tasks(c.debug_fetch(lib.DBG_TASKS, 0))
                if variant == "packed":
                    nch, off = _lane_shapes(c.debug_fetch(lib.DBG_VERIFIED, 0), l, m, True)
            c.set_mode(lib.MODE_TWO_ROUND)
            c.exec()
            _same(c.fetch(), exp)
            stats[variant] = c.stats()
            if not front and variant != "none":
                tasks[variant] = _sorted_tasks(c.debug_fetch(lib.DBG_TASKS, 1))
                if variant == "packed":
                    nch, off = _lane_shapes(c.debug_fetch(lib.DBG_VERIFIED, 1), l, m, False)
        assert stats[variant]["flags"] == 0   # no capacity overflow, no window violation
    print(f"l={l} {where}: chunks {sorted(set(nch.tolist()))} offsets {sorted(set(off.tolist()))}")
    for k in ("tasks", "resolved", "traces", "windows"):
        print(f"  {k}: " + " ".join(f"{v} {stats[v][k]}" for v in stats))
    print(f"  task lists equal: {np.array_equal(tasks['packed'], tasks['v1'])}")
    # the inputs do what they are built for: every chunk offset, and lanes from the fewest chunks
    # a block of l rows can have (l + 2 kf + 1 columns at least) up to 5 (3 for 1-nt blocks)
    assert set(off.tolist()) == set(range(16))
    lo = 1 if l <= 8 else 2 if l <= 17 else 3
    assert set(range(lo, 4 if l == 1 else 6)) <= set(nch.tolist())
    assert stats["packed"]["windows"] == stats["v1"]["windows"]
    if l <= 16:
        # blocks that fit a 16-bit half: the packed screen scans the same rows from the same
        # column as the one-lane-per-adapter screen, and (on the parent too) passes the same
        # tasks, which give the same candidate cells
        assert np.array_equal(tasks["packed"], tasks["v1"])
        for k in ("tasks", "resolved"):
            assert stats["packed"][k][r] == stats["v1"][k][r], k
    else:   # cut to the last 16 rows: a lower bound, so never fewer tasks
        assert stats["v1"]["tasks"][r] <= stats["packed"]["tasks"][r]
