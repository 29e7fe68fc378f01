"""Shared material of tests/test_finetune_host.py (no GPU) and tests/test_finetune.py (GPU):
dmx.sorter.finetune against a model that transcribes finetune of
scripts/auxiliary_code/amplicon_sorter.py (:838-965) literally over lists [index, string, iden],
with three replacements:
  random.sample      the stand-ins S1 (readlist[:100]) and S2 (seqlist[:150]);
  distance           (:225-235) on a plain numpy NW DP instead of edlib;
  create_consensus   sorter.consensus(None, ...), which tests/test_consensus.py pins.
and one stated difference: a group of fewer than 2 reads comes back unchanged (the reference
raises IndexError on scorelist[0] of an empty list).

The cases are synthetic amplicons of 300-420 nt with about 3 % noise (substitutions, insertions
and deletions), some reads noisier where a case needs reads that miss 0.95, a good third of
them stored reverse-complemented.  All cases share one list of reads; a case is one group of it.
Every case states which branch of finetune its group must take and asserts it from the model's
trace (check_coverage), so that a change of the generator cannot silently move a case off its
branch.  The seeds were chosen, with the model alone, so that the branch table is hit and every
loop but `stop`'s converges within 4 cycles."""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from dmx import sorter  # noqa: E402

COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s: str) -> str:
    return s.translate(COMP)[::-1]


def rand_seq(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=int(n)))


def mutate(rng, s: str, rate: float) -> str:
    """s with a substitution, an insertion or a deletion at about `rate` of its positions."""
    out = []
    for ch in s:
        if rng.random() < rate:
            kind = int(rng.integers(3))
            if kind == 0:
                out.append("ACGT".replace(ch, "")[int(rng.integers(3))])
            elif kind == 1:
                out.append(ch + "ACGT"[int(rng.integers(4))])
        else:
            out.append(ch)
    return "".join(out)


# ---- the model ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def nw(a: str, b: str) -> int:
    """The Levenshtein distance of a and b, row by row over the full matrix."""
    x = np.frombuffer(a.encode(), dtype=np.uint8)
    y = np.frombuffer(b.encode(), dtype=np.uint8)
    ar = np.arange(len(y) + 1, dtype=np.int64)
    prev = ar.copy()
    for i in range(1, len(x) + 1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (y != x[i - 1]))
        prev = np.minimum.accumulate(cur - ar) + ar   # the step from the left, all at once
    return int(prev[-1])


def distance(X1: str, X2: str) -> float:
    """distance (:225-235)."""
    if len(X1) > len(X2):
        A2, A1 = X1, X2
    else:
        A1, A2 = X1, X2
    return round(1 - nw(A1, A2) / len(A2), 3)


def create_consensus(seqlist) -> str:
    return sorter.consensus(None, list(seqlist), [np.arange(len(seqlist))])[0]


def model(reads, groups, consensuses, max_cycles: int = 10):
    """finetune (:838-965) over `groups` (lists of indices into reads) with their consensus
    strings.  Returns (groups, consensuses, trace): the groups as lists of int, group A's
    appended after all others, and per input group a dict: branch ('small', 'one', 'gone',
    'split', 'thin'), cycles, converged (the loop ended on iden1 == iden2 == 1), turned,
    removed (reads of the group that are in no group it left), group_a (A was appended) and
    tie_at_cut (some check_consensus cut seqlist[-50:] between two reads of equal str(iden))."""
    reads = [r.decode() if isinstance(r, (bytes, bytearray)) else str(r) for r in reads]
    grouplist = [[int(n) for n in g] for g in groups]
    conslist = [str(c) for c in consensuses]
    addlist, addcons, trace = [], [], []

    def reads_direction(readlist):
        x = readlist[0][1]
        for i, y in enumerate(readlist):
            iden = distance(x, y[1])
            idenR = distance(x, revcomp(y[1]))
            if iden < idenR:
                readlist[i][1] = revcomp(y[1])
        return readlist

    def check_consensus(consensus, readlist, t):
        for i, x in enumerate(readlist):
            iden = distance(consensus, x[1])
            readlist[i][2] = iden
        readlist.sort(key=lambda x: str(x[2]))
        seqlist = [x[1] for x in readlist if x[2] > 0.94]
        if len(seqlist) > 50:
            cut = [x for x in readlist if x[2] > 0.94]
            t["tie_at_cut"] |= str(cut[-51][2]) == str(cut[-50][2])
        if len(seqlist) < 20:
            seqlist = [x[1] for x in readlist[-20:]]
        consensus1 = create_consensus(seqlist[-50:])
        iden = distance(consensus1, consensus)
        return iden, consensus1, readlist

    for i, group in enumerate(grouplist):
        group2 = group[:]
        t = {"branch": None, "cycles": 0, "converged": False, "turned": 0, "removed": 0,
             "group_a": False, "tie_at_cut": False}
        trace.append(t)
        if len(group) < 2:                      # the stated difference: unchanged
            t["branch"] = "small"
            continue
        readlist = [[n, reads[n], ""] for n in group]
        readlist = reads_direction(readlist)
        t["turned"] = sum(x[1] != reads[x[0]] for x in readlist)
        readlist2 = readlist[:100]                                    # S1
        for x in readlist2[0:1]:
            scorelist = []
            for y in readlist2[1:100]:
                iden = distance(x[1], y[1])
                scorelist.append([iden, y[1]])
        scorelist.sort(key=lambda x: x[0])
        consensus1 = scorelist[int(len(scorelist) // 1.25)][1]
        consensus2 = scorelist[int(len(scorelist) // 5)][1]

        p = 1
        iden1 = iden2 = 0
        while iden1 < 1 or iden2 < 1:
            iden1, consensus1, readlist = check_consensus(consensus1, readlist, t)
            iden2, consensus2, readlist = check_consensus(consensus2, readlist, t)
            iden3 = distance(consensus1, consensus2)
            p += 1
            if p == max_cycles + 1:
                break
        t["cycles"] = p - 1
        t["converged"] = not (iden1 < 1 or iden2 < 1)

        left = set()
        if iden3 == 1:
            seqlist = [x[1] for x in readlist if x[2] >= 0.95]
            if len(seqlist) >= 5:
                t["branch"] = "one"
                sample = seqlist[:150]                                # S2
                conslist[i] = create_consensus(sample)
                for x in readlist:
                    if x[2] < 0.95:
                        grouplist[i].remove(x[0])
                left |= set(grouplist[i])
            else:
                t["branch"] = "gone"
                grouplist[i] = []
                conslist[i] = ""
        else:
            t["branch"] = "split"
            grouplist[i] = []
            seqlist = [x[1] for x in readlist if x[2] >= 0.95]
            if len(seqlist) >= 5:
                sample = seqlist[:150]                                # S2
                consensus = create_consensus(sample)
                for j, x in enumerate(readlist):
                    if x[2] >= 0.95:
                        grouplist[i].append(x[0])
                        readlist[j] = []
                conslist[i] = consensus
            if len(grouplist[i]) == 0:
                t["branch"] = "thin"             # 'finetune did not improve it'
                grouplist[i] = group2
            left |= set(grouplist[i])
            readlist = [x for x in readlist if len(x) > 0]
            if len(readlist) > 5:
                iden1, consensus1, readlist = check_consensus(consensus1, readlist, t)
                seqlist = [x[1] for x in readlist if x[2] >= 0.95]
                templist = []
                if len(seqlist) >= 5:
                    sample = seqlist[:150]                            # S2
                    consensus = create_consensus(sample)
                    for _, x in enumerate(readlist):
                        if x[2] >= 0.95:
                            templist.append(x[0])
                    addlist.append(templist)
                    addcons.append(consensus)
                    t["group_a"] = True
                    left |= set(templist)
        t["removed"] = len(set(group2) - left)
    return grouplist + addlist, conslist + addcons, trace


# ---- the cases ----------------------------------------------------------------------------------

def _reads_of(rng, template, rates):
    """One read per rate: the template mutated, a good third stored reverse-complemented (the
    first one never: it anchors the group's orientation, and the second always, so that every
    group has both strands)."""
    out = []
    for k, r in enumerate(rates):
        s = mutate(rng, template, r)
        out.append(revcomp(s) if k == 1 or (k > 1 and rng.random() < 0.4) else s)
    return out


def _with_runs(rng, s, runs):
    """s with `runs` stretches of 5..8 nt overwritten by one base: homopolymers, where a
    consensus depends most on the reads it is made of."""
    s = list(s)
    for _ in range(runs):
        at, n = int(rng.integers(10, len(s) - 20)), int(rng.integers(5, 9))
        s[at:at + n] = "ACGT"[int(rng.integers(4))] * n
    return "".join(s)


def _species_pair(rng, n, away, runs=0):
    """Two templates of n nt about `away` apart: substitutions and a 2 nt deletion."""
    a = _with_runs(rng, rand_seq(rng, n), runs)
    b = list(a)
    for k in rng.choice(n, size=int(round(n * away)), replace=False):
        b[k] = "ACGT".replace(b[k], "")[int(rng.integers(3))]
    cut = int(rng.integers(20, n - 20))
    b = "".join(b)
    return a, b[:cut] + b[cut + 2:]             # and a 2 nt deletion


def make_one(seed):
    rng = np.random.default_rng([seed, 1])
    return _reads_of(rng, rand_seq(rng, 384), [0.03] * 26 + [0.08] * 4)


def make_mixed(seed):
    rng = np.random.default_rng([seed, 2])
    a, b = _species_pair(rng, 400, 0.06, runs=6)
    first = _reads_of(rng, a, [0.03] * 14 + [0.045] * 8 + [0.09] * 2)
    return first + _reads_of(rng, b, [0.03] * 16)


def make_thin(seed):
    rng = np.random.default_rng([seed, 3])
    a, b = _species_pair(rng, 360, 0.06)
    first = _reads_of(rng, a, [0.03] * 10)
    return first + _reads_of(rng, b, [0.07] * 14)


def make_gone(seed):
    rng = np.random.default_rng([seed, 4])
    return _reads_of(rng, rand_seq(rng, 330), [0.07] * 12)


def make_small(seed):
    rng = np.random.default_rng([seed, 5])
    return [rand_seq(rng, 420)]


def make_ties(seed):
    rng = np.random.default_rng([seed, 6])
    return _reads_of(rng, rand_seq(rng, 300), [0.03] * 56)


MAKERS = {"one": make_one, "mixed": make_mixed, "thin": make_thin, "gone": make_gone,
          "small": make_small, "ties": make_ties}
SEEDS = {"one": 1, "mixed": 4, "thin": 1, "gone": 1, "small": 1, "ties": 10}
# what the model must do, per case: (branch, group A appended)
EXPECT = {"one": ("one", False), "mixed": ("split", True), "thin": ("thin", None),
          "gone": ("gone", False), "small": ("small", False), "ties": ("one", False)}
ORDER = ("one", "mixed", "thin", "gone", "small", "ties")


@functools.lru_cache(maxsize=None)
def bin_reads():
    """(reads, {case: its group}): all cases' reads in one list, ORDER after each other."""
    reads, groups = [], {}
    for name in ORDER:
        mine = MAKERS[name](SEEDS[name])
        groups[name] = np.arange(len(reads), len(reads) + len(mine), dtype=np.int64)
        reads += mine
    return reads, groups


def old_consensus(k: int) -> str:
    """The consensus a group brings along: finetune ignores it, and gives it back only with a
    group that it leaves unchanged."""
    return "ACGT" * (20 + k)


def case(name: str):
    """(reads, [group], [consensus], max_cycles) of one case; `stop` is `mixed` at 2 cycles."""
    reads, groups = bin_reads()
    src = "mixed" if name == "stop" else name
    return reads, [groups[src]], [old_consensus(ORDER.index(src))], 2 if name == "stop" else 10


def mixed_extra(n: int = 8):
    """n more reads of each of `mixed`'s two species (first n: the first species), from the
    same templates: the reads a rest_reads bin holds unassigned beside the mixed group."""
    rng = np.random.default_rng([SEEDS["mixed"], 2])
    a, b = _species_pair(rng, 400, 0.06, runs=6)
    rng = np.random.default_rng([SEEDS["mixed"], 7])
    return _reads_of(rng, a, [0.03] * n) + _reads_of(rng, b, [0.03] * n)


@functools.lru_cache(maxsize=None)
def rest_bin():
    """A gene group for rest_reads: `mixed`'s 40 reads as its one species group (first 24 the
    first species), then 8 unassigned reads of each species.  Returns (reads, indexes, groups,
    the first species' reads, the second species' reads)."""
    reads = make_mixed(SEEDS["mixed"]) + mixed_extra(8)
    first = list(range(24)) + list(range(40, 48))
    second = list(range(24, 40)) + list(range(48, 56))
    return (reads, np.arange(len(reads), dtype=np.int64), [np.arange(40, dtype=np.int64)],
            first, second)


def all_cases():
    """(reads, groups, consensuses): every case of ORDER as one call's groups."""
    reads, groups = bin_reads()
    return reads, [groups[n] for n in ORDER], [old_consensus(k) for k in range(len(ORDER))]


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """The model's (groups, consensuses, trace) of a case, computed once."""
    reads, groups, cons, cycles = case(name)
    return model(reads, groups, cons, cycles)


def check_coverage(name: str):
    """The case does what its row of the table says, by the model's own trace."""
    groups, cons, trace = expected(name)
    t = trace[0]
    reads, gin, cin, _ = case(name)
    n = len(gin[0])
    if name == "stop":
        assert t["cycles"] == 2 and not t["converged"], t
        assert expected("mixed")[2][0]["cycles"] > 2
        return
    branch, group_a = EXPECT[name]
    assert t["branch"] == branch, t
    if group_a is not None:
        assert t["group_a"] == group_a, t
    if name == "small":
        assert n == 1 and [list(g) for g in groups] == [gin[0].tolist()] and cons == cin
        return
    assert t["converged"] and 1 <= t["cycles"] <= 4, t
    assert 1 <= t["turned"] < n, t
    if name == "one":
        assert n == 30 and 1 <= t["removed"] <= 6 and len(groups) == 1, t
        assert len(groups[0]) == n - t["removed"]
    elif name == "mixed":
        assert n == 40 and len(groups) == 2 and t["removed"] >= 1, t
        first = set(gin[0][:24].tolist())       # B is the second species, A the first
        assert len(groups[0]) >= 12 and not set(groups[0]) & first
        assert len(groups[1]) >= 18 and set(groups[1]) <= first
    elif name == "thin":
        assert groups[0] == gin[0].tolist() and cons[0] == cin[0], t
    elif name == "gone":
        assert groups == [[]] and cons == [""] and t["removed"] == n, t
    elif name == "ties":
        assert n == 56 and t["tie_at_cut"], t
        assert all(295 <= len(r) <= 305 for r in (reads[k] for k in gin[0]))
