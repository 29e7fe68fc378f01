"""dmx.sorter.assign_best (one dmx_rowassign call) against dmx.sorter.assign (the same pass with
every distance on the host), and dmx.sorter.rest_reads against a literal restatement of
amplicon_sorter.py:1962-2014 (with update_groups :1718-1824) over Python lists of strings, with
assign() as its pass, the same index-order sampling and finetune skipped.  On the host twins here
(ctx=None); test_rest_reads_gpu.py runs the same inputs through a Context."""
import functools

import numpy as np
import pytest

import pairdist_cases as pc
import test_assign as ta
from dmx import sorter


@pytest.fixture(scope="module")
def bin_():
    return ta.make_bin()


@pytest.mark.parametrize("similar", [0.95, 0.90, 0.85])
def test_assign_best_is_assign_without_the_lines(bin_, similar):
    reads, unassigned, cons = bin_
    lines, best, added = sorter.assign(None, reads, unassigned, cons, similar)
    assert lines and best and added
    assert sorter.assign_best(None, reads, unassigned, cons, similar) == (best, added)
    # lower case and bytes in, the same out
    assert sorter.assign_best(None, [r.lower().encode() for r in reads], unassigned, cons,
                              similar) == (best, added)


def test_assign_best_stop_and_empty(bin_):
    reads, unassigned, cons = bin_
    full = sorter.assign(None, reads, unassigned, cons, 0.93)
    cut = sorter.assign(None, reads, unassigned, cons, 0.93, chunk=50, max_chunks=2)
    assert 0 < len(cut[1]) < len(full[1])
    assert sorter.assign_best(None, reads, unassigned, cons, 0.93, chunk=50,
                              max_chunks=2) == cut[1:]
    assert sorter.assign_best(None, reads, [], cons, 0.93) == ([], [])
    assert sorter.assign_best(None, reads, unassigned, [], 0.93) == ([], [])
    # a threshold at which no reverse complement is tried, and one nothing passes
    for similar in (0.45, 1.01):
        assert sorter.assign_best(None, reads, unassigned, cons, similar) == \
            sorter.assign(None, reads, unassigned, cons, similar)[1:]
    with pytest.raises(sorter.DmxError, match="consensus 1 is empty"):
        sorter.assign_best(None, ["ACGT"], [0], ["ACGT", ""], 0.9)
    with pytest.raises(sorter.DmxError, match="outside the reads"):
        sorter.assign_best(None, ["ACGT"], [1], ["ACGT"], 0.9)


@functools.lru_cache(maxsize=None)
def species_bin(seed=95, per=30):
    """Three planted species of `per` (about 30) reads of about 400 nt: five reads at 1 % from the
    founder (the species group to start from), the others mutated 2-14 %, so that they reach
    their consensus at different steps of `similar`; every fourth read reverse-complemented.
    Species 0 starts as two groups (a merge for compare_consensus).  Two reads mutated 30 % never
    reach -ss.  Returns (reads as str, indexes, starting groups as index arrays)."""
    rng = np.random.default_rng(seed)
    reads, groups = [], []
    for s in range(3):
        founder = pc.rand_seq(rng, 396 + 4 * s, p_n=0.0)
        first = len(reads)
        for k in range(per):
            rate = 0.01 if k < 10 else float(rng.uniform(0.02, 0.14))
            r = pc.mutate(rng, founder, rate)
            reads.append((pc.revcomp(r) if k % 4 == 3 else r).decode().replace("N", "A"))
        if s == 0:
            groups += [np.arange(first, first + 5), np.arange(first + 5, first + 10)]
        else:
            groups.append(np.arange(first, first + 5))
    for s in range(2):
        reads.append(pc.mutate(rng, pc.rand_seq(rng, 400, p_n=0.0), 0.3).decode().replace("N", "A"))
    order = rng.permutation(len(reads))          # the species interleaved in index order
    where = np.argsort(order)
    reads = [reads[i] for i in order]
    groups = [np.sort(where[g]) for g in groups]
    return reads, np.arange(len(reads)), groups


def restated(reads, indexes, groups, consensuses, similar_species=85.0, similar_consensus=96.0,
             length_diff=8.0):
    """The reference's lines with its names.  grouplist: lists of read tokens (decimal strings)
    with the consensus last.  Returns (groups, consensuses, facts)."""
    facts = dict(process=0, update_alone=0, merges=0, similar=[])
    indexes = {str(int(i)) for i in indexes}
    st = dict(grouplist=[[str(int(x)) for x in g] + [c] for g, c in zip(groups, consensuses)],
              tempfile=None, similar=0.95)

    def process_consensuslist():                                      # :1628-1691
        facts["process"] += 1
        indexes2 = indexes.copy()
        for x in st["grouplist"]:
            for y in x:
                if y.isdigit():
                    indexes2.discard(y)
        consensuslist = [y[-1] for y in st["grouplist"]]
        comparelist4 = [i for i in range(len(reads)) if str(i) in indexes2]
        lines = sorter.assign(None, reads, comparelist4, consensuslist, st["similar"])[0]
        st["tempfile"] = lines if lines else None                    # no line: no file

    def update_groups():                                              # :1718-1824
        similar = st["similar"]
        grouplist = st["grouplist"]
        templist, tempdict = [], {}
        if st["tempfile"] is not None:
            for line in st["tempfile"]:
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
        if len(templist2) > 0:
            for x in templist2:
                grouplist[int(x[1])].append(x[0])
            for i, x in enumerate(grouplist):
                if x[-1].isdigit():
                    grouplist[i] = [y for y in x if y.isdigit()]
            todo = [i for i, x in enumerate(grouplist) if x[-1].isdigit()]
            # the first 200 reads in index order where the reference samples 200 at random
            made = sorter.make_consensus(None, reads, [sorted(int(y) for y in grouplist[i])[:200]
                                                       for i in todo])
            for i, c in zip(todo, made):
                grouplist[i].append(c)
        return templist, templist2

    def compare_consensus(length_diff_percent):                       # :1840-1960
        grouplist = st["grouplist"]
        g, c = sorter.compare_consensus(None, reads, [[int(y) for y in x[:-1]] for x in grouplist],
                                        [x[-1] for x in grouplist], similar_consensus,
                                        length_diff_percent, 200)
        facts["merges"] += len(grouplist) - len(g)
        st["grouplist"] = [[str(int(y)) for y in a] + [b] for a, b in zip(g, c)]

    k = 0
    min_similar = similar_species / 100
    process_consensuslist()                                           # :1974
    templist, templist2 = update_groups()
    if len(templist2) > 200:
        compare_consensus(8.0)
    k += 1
    while st["similar"] > min_similar:                                # :1982
        while k <= 2:
            if len(templist2) > 0:
                process_consensuslist()
                templist, templist2 = update_groups()
                if len(templist2) > 0 and k < 2:
                    if len(st["grouplist"]) > 1:
                        compare_consensus(8.0)
                k += 1
            else:
                k = 3
        else:
            k = 0
            if st["similar"] in [0.94, 0.88]:                         # finetune skipped
                process_consensuslist()
            st["similar"] = round(st["similar"] - 0.01, 2)
            facts["similar"].append(st["similar"])
            if len(templist) == 0:
                process_consensuslist()
                templist, templist2 = update_groups()
                k += 1
            else:
                facts["update_alone"] += 1
                templist, templist2 = update_groups()
                k += 1
    if len(st["grouplist"]) > 1:                                      # :2012-2014
        compare_consensus(length_diff)
    return ([[int(y) for y in x[:-1]] for x in st["grouplist"]],
            [x[-1] for x in st["grouplist"]], facts)


@functools.lru_cache(maxsize=None)
def rest_case():
    """The bin, its starting consensuses and the restatement's answer (computed once)."""
    reads, indexes, groups = species_bin()
    cons = sorter.species_consensuses(None, reads, groups)
    return reads, indexes, groups, cons, restated(reads, indexes, groups, cons)


def test_the_restatement_takes_every_branch():
    reads, indexes, groups, cons, (g, c, facts) = rest_case()
    assert len(groups) == 4 and len(cons) == 4 and 85 <= len(reads) <= 95
    assert facts["process"] > 3 and facts["update_alone"] > 0 and facts["merges"] > 0
    assert facts["similar"] == [round(0.95 - 0.01 * k, 2) for k in range(1, 11)]
    assert len(g) == 3 and sorted(len(x) for x in g) == [30, 30, 30]
    left = set(indexes.tolist()) - {i for x in g for i in x}
    assert len(left) == 2                        # the two reads that never reach -ss
    # the reads joined at several steps, not all at once
    start = {int(i) for x in groups for i in x}
    assert len(start) == 20


def test_rest_reads_equals_the_restatement():
    reads, indexes, groups, cons, (g, c, _) = rest_case()
    got_g, got_c = sorter.rest_reads(None, reads, indexes, groups, cons)
    assert [x.tolist() for x in got_g] == g
    assert got_c == c


def test_finetune_runs_at_094_and_088(monkeypatch):
    reads, indexes, groups, cons, _ = rest_case()
    seen, pending = [], []
    real = sorter.assign_best

    def spy(ctx, rds, un, cs, similar, **kw):
        if pending:                              # the process step of :2000, right after finetune
            seen.append(similar)
            pending.clear()
        return real(ctx, rds, un, cs, similar, **kw)

    def finetune(g, c):
        pending.append(1)
        assert len(g) == len(c) and all(len(x) for x in g)
        return g, c

    monkeypatch.setattr(sorter, "assign_best", spy)
    got = sorter.rest_reads(None, reads, indexes, groups, cons, finetune=finetune)
    assert seen == [0.94, 0.88]
    # a finetune that changes nothing: the answer of finetune=None
    monkeypatch.setattr(sorter, "assign_best", real)
    plain = sorter.rest_reads(None, reads, indexes, groups, cons)
    assert [x.tolist() for x in got[0]] == [x.tolist() for x in plain[0]] and got[1] == plain[1]


def test_species_consensuses_takes_the_first_reads_in_index_order():
    reads, indexes, groups, cons, _ = rest_case()
    assert cons == sorter.make_consensus(None, reads, [np.sort(g)[:100] for g in groups])
    assert sorter.species_consensuses(None, reads, []) == []
    shuffled = [g[::-1] for g in groups]
    assert sorter.species_consensuses(None, reads, shuffled, sample=3) == \
        sorter.make_consensus(None, reads, [np.sort(g)[:3] for g in groups])


def test_assigned_needs_species_groups(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        sorter.main(["-i", str(tmp_path / "none.fastq"), "--groups", str(tmp_path / "g.txt"),
                     "--assigned", str(tmp_path / "a.txt")])
    assert e.value.code == 2
    assert "--assigned needs --species-groups" in capsys.readouterr().err


def test_write_assigned_shapes_both_files(tmp_path):
    done = [(0, [np.array([3, 1]), np.array([7])], ["ACGT", "GG"]), (2, [np.array([5])], ["TT"])]
    sorter.write_assigned(str(tmp_path / "a.txt"), done, 85.0, 96.0, 8.0)
    assert (tmp_path / "a.txt").read_text() == "# ss 85 sc 96 ldc 8\n0.0: 3 1\n0.1: 7\n2.0: 5\n"
    assert (tmp_path / "a.txt.fasta").read_text() == (
        ">consensus_0_0(2)\nACGT\n>consensus_0_1(1)\nGG\n>consensus_2_0(1)\nTT\n")


def test_sort_species_skips_a_gene_group_without_species_groups():
    reads, indexes, groups, cons, (g, c, _) = rest_case()
    said = []
    done = sorter.sort_species(None, reads, [np.array([0, 1, 2]), indexes], [[], groups],
                               log=said.append)
    assert said == ["gene group 0: no species group, nothing to do"]
    assert len(done) == 1 and done[0][0] == 1
    assert [x.tolist() for x in done[0][1]] == g and done[0][2] == c
