"""dmx.sorter.assign (one pass of process_consensuslist + similarity_species + the best-hit filter
of update_groups) against a literal restatement of amplicon_sorter.py:1660-1676, :1698-1708 and
:1730-1755 in plain Python lists, on the numpy DP of pairdist_cases.py and the built-in round.
On the host reference here (ctx=None) and on the GPU (marked gpu)."""
import numpy as np
import pytest

import pairdist_cases as pc
from dmx import lib, sorter, synth

SIMILAR = 0.93
LENGTHS = (308, 362, 420, 365)


def family(k, n, mutate):
    return synth.amplicon_bin(n, families=1, length=(LENGTHS[k], LENGTHS[k]), mutate=mutate,
                              rc_frac=0.25, n_reads_with_n=2, seed=90 + k)


def make_bin():
    """~100 reads of four amplicon families of 300-420 nt, copies mutated 3-12 %, a quarter
    reverse-complemented, some with N; six consensuses: the families 0, 1, 2 themselves
    (family 3 has none), family 0 a second time, a 2 % mutated family 1, and family 2 with an N."""
    reads = []
    for k in range(4):
        reads += family(k, 25, (0.03, 0.12))
    rng = np.random.default_rng(3)
    rng.shuffle(reads)
    # the same seed and no mutation: the family's own sequence
    fam = [synth.amplicon_bin(1, families=1, length=(LENGTHS[k], LENGTHS[k]), mutate=(0.0, 0.0),
                              rc_frac=0.0, seed=90 + k)[0] for k in range(3)]
    near1 = pc.mutate(rng, fam[1].encode(), 0.02).decode().replace("N", "A")
    with_n = fam[2][:200] + "N" + fam[2][201:]
    cons = [fam[0], fam[1], with_n, fam[0], near1, fam[2]]
    unassigned = [i for i in range(len(reads)) if i % 10 != 7]   # some reads are in groups already
    return reads, unassigned, cons


def compl_reverse(s):
    return pc.revcomp(s.encode()).decode()


def restated(reads, unassigned, cons, similar, chunk=2000000, max_chunks=100):
    """The reference's lines of code, with its names.  Returns (lines, templist, templist2,
    facts about the branches taken)."""
    comparelist4 = [[None, reads[i].upper(), None, i] for i in unassigned]
    consensuslist = [[x, y] for x, y in enumerate(cons)]
    todo, todolist = [], []
    facts = dict(drop_a=0, drop_b=0, forward=0, reverse_only=0)
    k = 0
    for x in range(0, len(comparelist4)):                       # :1660-1676
        for y in range(0, len(consensuslist)):
            A1 = comparelist4[x]
            A2 = consensuslist[y]
            if len(A1[1]) * 1.05 < len(A2[1]) or len(A2[1]) * 1.05 < len(A1[1]):
                facts["drop_a" if len(A1[1]) * 1.05 < len(A2[1]) else "drop_b"] += 1
            else:
                todolist.append([A1, A2])
                if len(todolist) == chunk:
                    todo += todolist
                    todolist = []
                    k += 1
        if k == max_chunks:
            break
    todo += todolist

    def distances(pairs):   # distance() (:225-235): the shorter one is the query
        xs = [(a.encode(), b.encode()) if len(a) <= len(b) else (b.encode(), a.encode())
              for a, b in pairs]
        d = pc.np_dist([a for a, _ in xs], [b for _, b in xs], lib.PD_NW)
        return [round(1 - int(e) / len(b), 3) for e, (_, b) in zip(d, xs)]

    fwd = distances([(A1[1], A2[1]) for A1, A2 in todo])
    again = [n for n, iden in enumerate(fwd) if not iden >= similar - 0.01 and iden < 0.5]
    rev = dict(zip(again, distances([(todo[n][0][1], compl_reverse(todo[n][1][1]))
                                     for n in again])))
    templist = []
    for n, (A1, A2) in enumerate(todo):                          # :1698-1708
        iden = fwd[n]
        if iden >= similar - 0.01:
            templist.append((str(A1[3]) + ':' + str(A2[0]) + ':' + str(iden)))
            facts["forward"] += 1
        elif iden < 0.5:
            iden = rev[n]
            if iden >= similar - 0.01:
                templist.append((str(A1[3]) + ':' + str(A2[0]) + ':' + str(iden)))
                facts["reverse_only"] += 1
    lines = templist
    templist, tempdict = [], {}
    for line in lines:                                           # :1730-1755
        e = line.strip().split(':')
        a = e[0]
        if a in tempdict:
            tempdict[a].append(e)
            tempdict[a].sort(key=lambda x: (int(x[0]), float(x[2])))
            for i, j in enumerate(tempdict[a][:-1]):
                if j[0] == tempdict[a][i + 1][0]:
                    if j[2] <= tempdict[a][i + 1][2]:
                        j[0] = ''
            tempdict[a] = [i for i in tempdict[a] if i[0] != '']
        else:
            tempdict[a] = [e]
    templist.extend(tempdict.values())
    templist = [x for sublist in templist for x in sublist]
    templist2 = [i for i in templist if float(i[2]) >= similar]
    facts["n_todo"] = len(todo)
    facts["last_read"] = todo[-1][0][3] if todo else None
    as_tuples = lambda t: [(int(a), int(b), float(c)) for a, b, c in t]   # noqa: E731
    return lines, as_tuples(templist), as_tuples(templist2), facts


@pytest.fixture(scope="module")
def case():
    reads, unassigned, cons = make_bin()
    return reads, unassigned, cons, restated(reads, unassigned, cons, SIMILAR)


def test_the_inputs_take_every_branch(case):
    """On the restatement alone."""
    reads, unassigned, cons, (lines, best, added, facts) = case
    assert 90 <= len(reads) <= 110 and len(cons) == 6 and cons[0] == cons[3]
    assert any("N" in r for r in reads)
    assert facts["forward"] > 0 and facts["reverse_only"] > 0
    assert facts["drop_a"] > 0 and facts["drop_b"] > 0
    with_line = {b[0] for b in best}
    assert len(best) == len(with_line) < len(unassigned)         # a read with no line at all
    assert any(SIMILAR - 0.01 <= b[2] < SIMILAR for b in best)   # a line, but not added
    assert 0 < len(added) < len(best)
    # a tie between the identical consensuses 0 and 3 goes to the later one
    tied = [b for b in best if f"{b[0]}:0:{b[2]}" in lines and f"{b[0]}:3:{b[2]}" in lines]
    assert tied and all(b[1] == 3 for b in tied)
    assert not any(b[1] == 0 for b in best)


def check(ctx, case):
    reads, unassigned, cons, (lines, best, added, facts) = case
    got = sorter.assign(ctx, reads, unassigned, cons, SIMILAR)
    assert got[0] == lines
    assert got[1] == best
    assert got[2] == added
    # lower case and bytes in, the same out
    again = sorter.assign(ctx, [r.lower().encode() for r in reads], unassigned, cons, SIMILAR)
    assert again == got
    # the stop after max_chunks full chunks, tested once per read
    lines2, best2, added2, facts2 = restated(reads, unassigned, cons, SIMILAR, 50, 2)
    assert 100 <= facts2["n_todo"] < facts["n_todo"]
    got2 = sorter.assign(ctx, reads, unassigned, cons, SIMILAR, chunk=50, max_chunks=2)
    assert got2 == (lines2, best2, added2)
    assert lines2 and facts2["last_read"] != facts["last_read"]
    # a threshold at which no reverse complement is tried, and one nothing passes
    for similar in (0.45, 1.01):
        exp = restated(reads, unassigned, cons, similar)[:3]
        assert sorter.assign(ctx, reads, unassigned, cons, similar) == exp


def test_assign_on_the_host_reference(case):
    check(None, case)


@pytest.mark.gpu
def test_assign_on_the_gpu(ctx, case):
    check(ctx, case)
    reads, unassigned, cons, _ = case
    assert ctx.rowdist_ms() >= 0.0
    # the batch of an unchanged list stays resident; another load in between is noticed
    assert ctx._resident is reads
    ctx.load(pc.pack_reads([b"ACGT"]))
    assert sorter.assign(ctx, reads, unassigned, cons, SIMILAR)[1] == case[3][1]


def test_refusals():
    with pytest.raises(lib.DmxError, match="read 1 has a byte outside ACGTN"):
        sorter.assign(None, ["ACGT", "ACGR"], [0], ["ACGT"], 0.9)
    with pytest.raises(lib.DmxError, match="consensus 0 has a byte outside ACGTN"):
        sorter.assign(None, ["ACGT"], [0], ["AC-T"], 0.9)
    with pytest.raises(lib.DmxError, match="consensus 1 is empty"):
        sorter.assign(None, ["ACGT"], [0], ["ACGT", ""], 0.9)
    with pytest.raises(lib.DmxError, match="outside the reads"):
        sorter.assign(None, ["ACGT"], [1], ["ACGT"], 0.9)
    assert sorter.assign(None, ["ACGT"], [], ["ACGT"], 0.9) == ([], [], [])
    assert sorter.assign(None, ["ACGT"], [0], [], 0.9) == ([], [], [])
    assert sorter.assign(None, ["ACGT"], [0], ["ACGT"], 0.9) == (["0:0:1.0"], [(0, 0, 1.0)],
                                                                [(0, 0, 1.0)])
