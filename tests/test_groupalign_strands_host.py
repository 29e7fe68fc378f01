"""dmx_groupalign_strands_host (a strand per member) against the unflagged host
path on physically turned reads, and sorter.orient / sorter.make_consensus (consensus_direction
and make_consensus of amplicon_sorter.py:1826-1838, :1089-1105) against in-test restatements.
No GPU."""
import functools

import numpy as np
import pytest

import groupalign_cases as gc
import groupalign_strand_cases as sc
import pairdist_cases as pc
import test_consensus as tc
from dmx import lib, sorter


@pytest.mark.parametrize("name,kind", sc.RUNS)
def test_flagged_members_equal_turned_reads(name, kind):
    case, exp = sc.expected(name)
    _, seeds, groups, strands = case
    p = sc.packed(case, kind)
    got = lib.groupalign_host(p, seeds, groups, strands=strands, paths=True, n_threads=16)
    gc.same_result(got, exp)
    plain = lib.groupalign_host(p, seeds, groups, strands=strands, n_threads=16)
    assert "ops" not in plain
    for key in ("col_off", "mask", "count", "first", "dist"):
        np.testing.assert_array_equal(plain[key], exp[key])


def test_the_cases_reverse_what_they_claim():
    (reads, _, groups, strands), _ = sc.expected("lengths")
    rev = {len(reads[r]) for g, s in zip(groups, strands) for r, f in zip(g, s) if f}
    assert rev == set(sc.LENGTHS)
    assert strands[0][0] == 1 and groups[0][0] == 0 and len(reads[0]) == 1    # read 0
    assert groups[0][-1] == len(reads) - 1 and strands[0][-1] == 1           # the last read
    assert all(reads[k][0:1] == b"N" and reads[k][-1:] == b"N" for k in range(len(sc.LENGTHS)))
    assert reads[sc.LENGTHS.index(129)][63:65] == b"NN"
    (reads, _, groups, strands), _ = sc.expected("stripes")
    assert len(reads[0]) > 64 * 64 and len(reads[2]) == 2 * 4096 + 70 and strands[0][0] == 1
    (_, _, groups, strands), _ = sc.expected("both")
    uses = {(r, f) for g, s in zip(groups, strands) for r, f in zip(g, s)}
    assert (0, 0) in uses and (0, 1) in uses
    (_, _, groups, strands), _ = sc.expected("uneven")
    assert [len(g) for g in groups] == [0, 1, 2, 7]
    assert all(0 < sum(s) < len(s) for s in strands[2:])


def test_no_strands_is_todays_call():
    reads, seeds, groups, _ = sc.CASES["uneven"]()
    p = pc.pack_reads(reads)
    today = lib.groupalign_host(p, seeds, groups, paths=True)
    zeros = [[0] * len(g) for g in groups]
    gc.same_result(lib.groupalign_host(p, seeds, groups, paths=True, strands=None), today)
    gc.same_result(lib.groupalign_host(p, seeds, groups, paths=True, strands=zeros), today)


def test_an_unknown_flag_is_refused_naming_group_and_member():
    reads, seeds, groups, strands = sc.CASES["uneven"]()
    p = pc.pack_reads(reads)
    bad = [list(s) for s in strands]
    bad[3][4] = 3
    with pytest.raises(lib.DmxError, match=r"\(-1\).*group 3.*member 4.*flag"):
        lib.groupalign_host(p, seeds, groups, strands=bad)
    bad[3][4] = 0x80
    with pytest.raises(lib.DmxError, match=r"\(-1\).*group 3.*member 4.*flag"):
        lib.groupalign_host(p, seeds, groups, strands=bad)
    with pytest.raises(lib.DmxError, match="parallel to groups"):
        lib.groupalign_host(p, seeds, groups, strands=strands[:-1])
    with pytest.raises(lib.DmxError, match="parallel to groups"):
        lib.groupalign_host(p, seeds, groups, strands=[[], [1], [0], [1] * 7])


# ---- sorter.orient against consensus_direction, literally ------------------------------------

def ref_distance(x1: bytes, x2: bytes) -> float:
    """distance() (:225-235) on pc.np_dist."""
    a1, a2 = (x2, x1) if len(x1) > len(x2) else (x1, x2)
    d = int(pc.np_dist([a1], [a2], lib.PD_NW)[0])
    return round(1 - d / len(a2), 3)


def ref_direction(consensuslist):
    """consensus_direction (:1826-1838), with the set kept in first-insertion order (the
    reference's own order is the string hash's)."""
    out = {}
    for x in consensuslist[0:1]:
        for y in consensuslist[1:]:
            iden = ref_distance(x, y)
            iden_r = ref_distance(x, pc.revcomp(y))
            for s in ([x, y] if iden > iden_r else [x, pc.revcomp(y)]):
                out.setdefault(s, None)
    return list(out)


def ref_make_consensus_list(reads, group):
    """make_consensus's list (:1097-1103): the group's reads by rising length, then oriented."""
    lst = [reads[i] for i in group]
    lst.sort(key=lambda s: len(s))
    return ref_direction(lst)


def oriented(reads, members, strands):
    return [pc.revcomp(reads[i]) if f else reads[i] for i, f in zip(members, strands)]


def test_orient_equals_consensus_direction():
    rng = np.random.default_rng(181)
    fam = pc.rand_seq(rng, 120, p_n=0.02)
    pal = b"ACGTTGCAACGT" + b"ACGTTGCAACGT"      # its own reverse complement
    assert pc.revcomp(pal) == pal
    reads = [pc.mutate(rng, fam, 0.08) for _ in range(9)]
    for k in (1, 4, 5, 8):
        reads[k] = pc.revcomp(reads[k])
    groups = [list(range(9))]
    # a palindrome ties with itself and is turned; the unrelated anchor keeps it a tie as well
    reads += [b"ACGTTGCAAC", pal, pal + b"A"]
    groups.append([9, 10, 11])
    # duplicates: two equal reads, and a forward read equal to another's reverse complement
    a = pc.rand_seq(rng, 60, p_n=0.0)
    b = pc.mutate(rng, a, 0.05) + b"ACG"
    reads += [a, b, b, pc.revcomp(b), pc.mutate(rng, a, 0.1) + b"ACGTA"]
    groups.append([12, 13, 14, 15, 16])
    members, strands = sorter.orient(None, reads, groups, n_threads=4)
    for g, m, s in zip(groups, members, strands):
        assert oriented(reads, m, s) == ref_make_consensus_list(reads, g)
        assert s[0] == 0                               # the anchor stays forward
    assert sorted(strands[0].tolist()) == [0] * 5 + [1] * 4 or \
        sorted(strands[0].tolist()) == [0] * 4 + [1] * 5      # one family, two orientations
    assert 10 in members[1] and strands[1][members[1].tolist().index(10)] == 1   # the tie
    assert len(members[2]) == 3                         # b, b and rc(rc(b)) collapse to one
    # str input gives the same
    m2, s2 = sorter.orient(None, [r.decode() for r in reads], groups)
    assert [x.tolist() for x in m2] == [x.tolist() for x in members]
    assert [x.tolist() for x in s2] == [x.tolist() for x in strands]


def test_orient_refuses_a_group_of_fewer_than_two_reads():
    reads = [b"ACGTACGTAC", b"ACGTACGTAA", b"TTGTACGTAC"]
    with pytest.raises(lib.DmxError, match="group 1 has 0"):
        sorter.orient(None, reads, [[0, 1], [2]])
    with pytest.raises(lib.DmxError, match="group 0 has 0"):
        sorter.orient(None, reads, [[]])
    # equal reads collapse to one
    with pytest.raises(lib.DmxError, match="group 1 has 1"):
        sorter.orient(None, reads + [pc.revcomp(reads[2])], [[0, 1], [2, 3]])


# ---- sorter.make_consensus against the model of test_consensus.py ---------------------------

@functools.lru_cache(maxsize=None)
def mixed_bin():
    """test_consensus.cases() with a seeded half of the reads turned round.  Returns (reads,
    groups that keep two distinct reads, the group of equal copies)."""
    reads, groups, _ = tc.cases()
    rng = np.random.default_rng(182)
    flip = rng.random(len(reads)) < 0.5
    reads = [pc.revcomp(r) if f else r for r, f in zip(reads, flip)]
    return reads, groups[:7], groups[7], flip


def test_make_consensus_on_the_host_reference_equals_the_model():
    reads, groups, copies, flip = mixed_bin()
    members, strands = sorter.orient(None, reads, groups)
    exp = [tc.model_consensus(oriented(reads, m, s)) for m, s in zip(members, strands)]
    got = sorter.make_consensus(None, reads, groups)
    assert got == exp
    # consensus() with the strands passed in is the same route
    assert sorter.consensus(None, reads, members, strands=strands) == exp
    # the generator's own properties: a reversed anchor (the shortest read was turned in the
    # bin, so the consensus is the family's reverse complement) and a reversed longest read
    ln = np.array([len(r) for r in reads])
    rev_anchor = [bool(flip[m[0]]) for m in members]
    assert any(rev_anchor) and not all(rev_anchor)
    longest = [int(s[np.argsort(-ln[m], kind="stable")[0]]) for m, s in zip(members, strands)]
    assert any(longest)
    # the oriented reads are the family's own where the anchor was left forward in the bin, and
    # their reverse complements otherwise: the consensus is the model's of exactly those
    orig, _, _ = tc.cases()
    for k, (m, s) in enumerate(zip(members, strands)):
        want = {pc.revcomp(orig[i]) if rev_anchor[k] else orig[i] for i in groups[k]}
        assert set(oriented(reads, m, s)) == want
    # error-free copies collapse to one read: refused, naming the group
    with pytest.raises(lib.DmxError, match="group 1 has 1"):
        sorter.make_consensus(None, reads, [groups[0], copies])
