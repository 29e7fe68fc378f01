"""sorter.compare_consensuses, merge_by_consensus and comp_consensus_groups on
the host twins, against in-test restatements of the contract: the pair loop and iden_consensus
with a numpy DP, and the merge as sets of strings."""
import numpy as np
import pytest

import pairdist_cases as pc
import rowpair_cases as rp
from dmx import lib, sorter


def restated_lines(cons, length_diff=8.0, threshold=0.60):
    """The pair loop and iden_consensus from the contract: every y < z that passes the length
    rule, HW distance of the shorter in the longer (y's on equal lengths) and against the reverse
    complement of z's, the larger identity, a line when it is >= threshold."""
    ldc = length_diff / 100 + 1
    out = []
    for y in range(len(cons) - 1):
        for z in range(y + 1, len(cons)):
            a1, a2 = cons[y], cons[z]
            if len(a1) * ldc < len(a2) or len(a2) * ldc < len(a1):
                continue
            idens = []
            for b in (a2, pc.revcomp(a2)):
                s, l = (b, a1) if len(a1) > len(b) else (a1, b)
                d = int(pc.np_dist([s], [l], lib.PD_HW)[0])
                idens.append(round(1 - d / len(l), 3))
            if max(idens) >= threshold:
                out.append((y, z, max(idens)))
    return out


def test_compare_consensuses_length_rule_strands_and_threshold():
    rng = np.random.default_rng(5)
    base = pc.rand_seq(rng, 125, p_n=0.0)
    # 100 * 1.08 == 108.0 and 125 * 1.08 == 135.0 in double arithmetic: the product lands exactly
    # on 108 / 135 (compared), just under 109 / 136 (dropped) and just over 107 (compared)
    cons = [base[:100], base[:108], base[:109], base, (base + base)[:135], (base + base)[:136],
            pc.revcomp(pc.mutate(rng, base, 0.05)), pc.mutate(rng, base, 0.04)[:125].ljust(125, b"A"),
            pc.rand_seq(rng, 125, p_n=0.0), base[:107]]
    assert 100 * (8.0 / 100 + 1) == 108.0 and 125 * (8.0 / 100 + 1) == 135.0
    exp = restated_lines(cons)
    got = sorter.compare_consensuses(None, cons, n_threads=4)
    assert got == exp
    pairs = {(y, z) for y, z, _ in got}
    assert (0, 1) in pairs and (0, 2) not in pairs and (3, 4) in pairs and (3, 5) not in pairs
    assert (0, 9) in pairs
    assert (3, 6) in pairs and (3, 7) in pairs            # the reversed family, equal lengths
    assert sorter.compare_consensuses(None, [c.decode() for c in cons], n_threads=4) == exp
    assert sorter.compare_consensuses(None, [lib.mask_row(c) for c in cons], n_threads=4) == exp
    # other parameters
    assert sorter.compare_consensuses(None, cons, 30.0, 0.80, 4) == restated_lines(cons, 30.0, 0.80)
    assert sorter.compare_consensuses(None, cons[:1]) == [] and sorter.compare_consensuses(None, []) == []


def test_identity_exactly_at_the_threshold():
    # 10 columns, 4 of them wrong whatever the shift: identity 0.6 exactly; 5 wrong: 0.5
    a, b, c = b"AAAAAAAAAA", b"AAAAAACCCC", b"AAAAACCCCC"
    exp = restated_lines([a, b, c])
    assert (0, 1, 0.6) in exp and not any(y == 0 and z == 2 for y, z, _ in exp)
    assert sorter.compare_consensuses(None, [a, b, c]) == exp


def restated_merge(groups, cons, lines, threshold):
    """The merge as the contract states it, on sets of strings."""
    S = [set(str(int(x)) for x in g) | {c} for g, c in zip(groups, cons)]
    for y, z, iden in lines:
        if iden >= threshold:
            while len(S[y]) == 1:
                y = int(list(S[y])[0].replace("=", ""))
            S[y].update(S[z])
            S[z] = {"=" + str(y)}
    S = [s for s in S if len(s) > 1]
    moved = True
    while moved:
        moved = False
        for i in range(len(S) - 1):
            for j in range(i + 1, len(S)):
                if S[i] & S[j]:
                    S[i] |= S[j]
                    S[j] = set()
                    moved = True
        S = [s for s in S if s]
    return [sorted(int(x) for x in s if x.isdigit()) for s in S]


def as_lists(groups):
    return [[int(x) for x in g] for g in groups]


def test_merge_by_consensus_on_hand_built_lines():
    groups = [[0, 1], [2, 3], [4, 5], [6], [7, 8], [9, 10], [11]]
    cons = ["AAAA", "CCCC", "GGGG", "TTTT", "ACAC", "ACAC", "GTGT"]
    cases = {
        # 1 -> 0, 2 -> 1 (a pointer: chased to 0), 3 -> 2 (two hops: 2 -> 1 -> 0)
        "two hops": [(0, 1, 0.9), (1, 2, 0.9), (2, 3, 0.9)],
        # z = 1 is already a pointer to 0: group 2 takes the token '=0' and never group 0's reads
        "z is a pointer": [(0, 1, 0.9), (2, 1, 0.9)],
        # the same, and then 3 is given 2's set: 2 and 3 stay apart from 0 (no shared token)
        "token handed on": [(0, 1, 0.9), (2, 1, 0.9), (3, 2, 0.9)],
        # 1 and 3 both point to 0; 2 takes 1's token and 4 takes 3's: 2 and 4 hold '=0' and meet
        # through it alone, apart from group 0 itself
        "meet through the token": [(0, 1, 0.9), (0, 3, 0.9), (2, 1, 0.9), (4, 3, 0.9)],
        "threshold": [(0, 1, 0.79), (2, 3, 0.8), (4, 6, 0.95), (0, 2, 0.5)],
        "no lines": [],
    }
    for name, lines in cases.items():
        got = as_lists(sorter.merge_by_consensus(groups, cons, lines, 0.8))
        assert got == restated_merge(groups, cons, lines, 0.8), name
    got = {n: as_lists(sorter.merge_by_consensus(groups, cons, l, 0.8)) for n, l in cases.items()}
    assert got["two hops"][0] == [0, 1, 2, 3, 4, 5, 6]
    # identical consensus strings join groups 4 and 5 without any line
    assert [7, 8, 9, 10] in got["no lines"] and len(got["no lines"]) == 6
    assert got["z is a pointer"] == [[0, 1, 2, 3], [4, 5], [6], [7, 8, 9, 10], [11]]
    # (and the equal consensus strings of groups 4 and 5 bring 5 along)
    assert got["meet through the token"] == [[0, 1, 2, 3, 6], [4, 5, 7, 8, 9, 10], [11]]
    assert got["threshold"] == [[0, 1], [2, 3], [4, 5, 6], [7, 8, 9, 10, 11]]
    # the result depends on the order of the lines, as the reference's does
    a = as_lists(sorter.merge_by_consensus(groups, cons, [(0, 1, 0.9), (2, 1, 0.9)], 0.8))
    b = as_lists(sorter.merge_by_consensus(groups, cons, [(2, 1, 0.9), (0, 1, 0.9)], 0.8))
    assert a != b
    with pytest.raises(ValueError, match="group 1 has no reads"):
        sorter.merge_by_consensus([[0], []], ["A", "C"], [], 0.8)
    for g in sorter.merge_by_consensus(groups, cons, cases["two hops"], 0.8):
        assert g.dtype == np.int64 and (np.diff(g) > 0).all()


def test_comp_consensus_groups_rejoins_the_split_families():
    reads, groups, fam = rp.split_bin()
    assert len(groups) == 6 and all(len(g) == 8 for g in groups)
    got = sorter.comp_consensus_groups(None, reads, groups, n_threads=8)
    exp = [sorted(int(x) for k, g in enumerate(groups) if fam[k] == f for x in g) for f in range(3)]
    assert as_lists(got) == exp
    # one cycle by hand: consensuses, lines, merge
    cons = sorter.make_consensus(None, reads, groups, n_threads=8)
    lines = sorter.compare_consensuses(None, cons, n_threads=8)
    assert lines == restated_lines([c.encode() for c in cons])
    assert {(y, z) for y, z, _ in lines} == {(0, 1), (2, 3), (4, 5)}
    assert as_lists(sorter.merge_by_consensus(groups, cons, lines, 0.60)) == exp
    # min_reads drops small groups at the end; nothing to merge ends after one cycle
    assert sorter.comp_consensus_groups(None, reads, groups, min_reads=17, n_threads=8) == []
    assert as_lists(sorter.comp_consensus_groups(None, reads, groups[:1] + groups[2:3],
                                                 n_threads=8)) == as_lists(groups[:1] + groups[2:3])
    # compare_consensus: the same merge in at most 3 cycles, with fresh consensuses
    g2, c2 = sorter.compare_consensus(None, reads, groups, cons, similar_consensus=90.0, n_threads=8)
    assert as_lists(g2) == exp and len(c2) == 3
    assert c2 == sorter.make_consensus(None, reads, exp, n_threads=8)


def test_merged_groups_without_groups_is_refused(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        sorter.main(["-i", str(tmp_path / "none.fastq"), "-o", str(tmp_path / "sim.txt"),
                     "--merged-groups", str(tmp_path / "m.txt")])
    assert e.value.code == 2
    assert "--merged-groups needs --groups" in capsys.readouterr().err
