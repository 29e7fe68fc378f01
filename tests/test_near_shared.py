"""Near pieces inside the shared suffix (`DevPanel::near_shared`): a 5' window
piece before jsplit keeps every adapter, but its columns j <= jS = |S| - max kk hold the same cell
for every adapter, so only adapter 0 scans them.  P + I + S panels (PRE 10, SUF 12, 10 adapters:
a partial last quad) with index blocks of 8, 17 and of 1 and 32 nt mixed, -e 0.1 --rc, against the
oracle field by field: by default, with every adapter kept (DMX_NEAR_ALL=1), with the
one-lane-per-adapter screen and with no screen.

The reads start with the last 3..|S|+3 nt of an adapter (and jsplit - 2..jsplit + 1 nt, so that
windows end on both sides of jS and straddle jsplit), with 0..2 edits and sometimes an N; some go
on with a whole adapter 1..5 nt later (near and far piece in one window), some with adapter 0's
index block or all of adapter 0 further on (adapter 0 as near winner and far candidate); every
read comes reverse-complemented too.
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


def _panel(rng, ls):
    P, S = _dna(rng, PRE), _dna(rng, SUF)
    out = []
    for i, l in enumerate(ls):
        b = list(_dna(rng, l))
        b[0] = ACGT[i % 4]
        b[-1] = ACGT[(i + (0 if l == 1 else 1)) % 4]
        out.append(P + "".join(b) + S)
    assert len(set(out)) == len(out)
    return out


def _edit(rng, a, k):
    a = list(a)
    for _ in range(k):
        p = int(rng.integers(len(a)))
        u = rng.random()
        if u < 0.6:
            a[p] = ACGT[int(rng.integers(4))]
        elif u < 0.8 and len(a) > 1:
            del a[p]
        else:
            a.insert(p, ACGT[int(rng.integers(4))])
    return "".join(a)


def _reads(rng, pan, jS, jsplit):
    """(reads, index of a read that starts with S's last 6 nt and holds no other adapter, index of
    a read whose start is followed by a whole copy of adapter 1)."""
    starts = list(range(3, SUF + 4)) + [jsplit - 2, jsplit - 1, jsplit, jsplit + 1]
    assert {jS - 1, jS, jS + 1} <= set(starts)
    seqs = []
    for s in starts:
        for k in (0, 0, 1, 2):
            for kind in range(5):
                a = pan[int(rng.integers(len(pan)))]
                st = _edit(rng, a[-min(s, len(a)):], k)
                if kind == 1 and len(st) > 2:                   # one N inside the start
                    p = int(rng.integers(len(st)))
                    st = st[:p] + "N" + st[p + 1:]
                rest = ""
                if kind == 2:                                   # a whole adapter 1..5 nt later
                    b = pan[int(rng.integers(len(pan)))]
                    rest = _dna(rng, int(rng.integers(1, 6))) + _edit(rng, b, int(rng.integers(0, 3)))
                if kind == 3:                                   # adapter 0's index block later
                    rest = _dna(rng, int(rng.integers(2, 30))) + pan[0][PRE:len(pan[0]) - SUF]
                if kind == 4:                                   # all of adapter 0 later
                    rest = _dna(rng, int(rng.integers(6, 40))) + _edit(rng, pan[0], int(rng.integers(0, 2)))
                head = st + rest
                seqs.append(head + _dna(rng, int(rng.integers(max(60, len(head) + 20), 200)) - len(head)))
    i_near = len(seqs)
    seqs.append(pan[0][-6:] + _dna(rng, 80))
    i_far = len(seqs)
    seqs.append(pan[0][-6:] + _dna(rng, 3) + pan[1] + _dna(rng, 70))
    seqs += [_rc(s) for s in seqs]
    assert all(60 <= len(s) <= 200 for s in seqs)
    return seqs, i_near, i_far


def _same(got, exp, what):
    for f in exp.dtype.names:
        bad = np.nonzero(got[f] != exp[f])[0]
        assert len(bad) == 0, f"{what}: {len(bad)} reads differ in {f}, first {bad[:10]}"


VARIANTS = {"default": {}, "near_all": {"DMX_NEAR_ALL": "1"}, "v1": {"DMX_SCREEN_V1": "1"},
            "none": {"DMX_NO_SCREEN": "1"}}


@pytest.mark.parametrize("case", ["l8", "l17", "l1_32"])
def test_near_shared(case, monkeypatch):
    rng = np.random.default_rng({"l8": 81, "l17": 171, "l1_32": 132}[case])
    ls = {"l8": [8] * 10, "l17": [17] * 10, "l1_32": [1, 32, 32, 1, 32, 1, 1, 32, 32, 32]}[case]
    pan = _panel(rng, ls)
    rc, info = lib.panel_near_shared(pan, lib.DMX_FRONT | lib.DMX_RC, 0.1)
    kk = int(0.1 * max(len(a) for a in pan))
    jsplit = max(len(a) - PRE + int(0.1 * len(a)) for a in pan)
    assert rc == 0 and info == {"near_shared": SUF - kk, "filter_len": SUF, "jsplit": jsplit,
                                "kk": kk}
    jS = info["near_shared"]
    d = synth.generate("c2", n=50, seed=3)
    seqs, i_near, i_far = _reads(rng, pan, jS, jsplit)
    seqs += [s[:200] for s in synth.to_strings(d)]
    blob, offs, lens = oracle.pack_ascii(seqs)
    exp = oracle.run_batch(oracle.Panel(pan, oracle.FRONT), oracle.Panel(d["sp27"], oracle.BACK),
                           blob, offs, lens, mode=1, threads=8)
    # the lowest index wins the cell every adapter shares, and a far match of another adapter
    # beats it
    assert exp["bin1"][i_near] == 0 and exp["m1_rstop"][i_near] == 6 and exp["rc1"][i_near] == 0
    assert exp["bin1"][i_far] == 1 and exp["m1_rstop"][i_far] == 9 + len(pan[1]) > jsplit
    near0 = (exp["bin1"] == 0) & (exp["m1_rstop"] <= jS) & (exp["m1_rstop"] > 0)
    print(f"{case}: {len(seqs)} reads, jS {jS}, jsplit {jsplit}, adapter 0 wins a cell at "
          f"j <= jS in {int(near0.sum())}, other bins {int((exp['bin1'] > 0).sum())}, "
          f"unknown {int((exp['bin1'] < 0).sum())}")
    assert near0.sum() >= 20
    packed = lib.pack(blob, offs, lens)
    stats = {}
    for v, env in VARIANTS.items():
        for k in ("DMX_NEAR_ALL", "DMX_SCREEN_V1", "DMX_NO_SCREEN"):
            monkeypatch.delenv(k, raising=False)
        for k, x in env.items():
            monkeypatch.setenv(k, x)
        with lib.Context(0) as c:
            c.set_panel(0, pan, lib.DMX_FRONT | lib.DMX_RC)
            c.set_panel(1, d["sp27"], lib.DMX_BACK | lib.DMX_RC)
            c.set_mode(lib.MODE_TWO_ROUND)
            c.load(packed)
            c.exec()
            _same(c.fetch(), exp, v)
            stats[v] = c.stats()
        assert stats[v]["flags"] == 0
    for k in ("tasks", "resolved", "traces", "windows", "windows_raw"):
        print(f"  {k}: " + " ".join(f"{v} {stats[v][k]}" for v in stats))
    for v in ("near_all", "v1"):
        for k in ("windows", "windows_raw", "filter_tasks"):
            assert stats["default"][k] == stats[v][k], (v, k)
        for k in ("tasks", "resolved"):                         # round 2 is untouched
            assert stats["default"][k][1] == stats[v][k][1], (v, k)
    # the path ran: fewer tasks and fewer candidate cells in round 1 than with every adapter
    assert stats["default"]["tasks"][0] < stats["near_all"]["tasks"][0]
    assert stats["default"]["resolved"][0] < stats["near_all"]["resolved"][0]
    if max(ls) <= 16:   # both screens scan the same rows: the same tasks, the same cells
        assert stats["default"]["tasks"][0] == stats["v1"]["tasks"][0]
        assert stats["default"]["resolved"][0] == stats["v1"]["resolved"][0]
