"""dmx.sorter.finetune on the host twins (ctx=None) against the literal model of
tests/finetune_cases.py: the groups, their order and contents, and the consensus strings of
every case; the lock-step over several groups against the groups one by one; and the same groups
from the same reads all turned round."""
import functools

import numpy as np
import pytest

import finetune_cases as fc
from dmx import lib, sorter

CASES = fc.ORDER + ("stop",)


def as_lists(groups):
    return [[int(x) for x in g] for g in groups]


@pytest.mark.parametrize("name", CASES)
def test_case_takes_its_branch(name):
    fc.check_coverage(name)


def test_reads_are_what_the_cases_promise():
    reads, groups = fc.bin_reads()
    lens = {len(r) for r in reads}
    # templates of 300..420 nt; the noise's insertions and deletions move a read's length a little
    assert {383, 384, 385} <= lens and min(lens) >= 290 and max(lens) <= 430
    assert all(set(r) <= set("ACGT") for r in reads)


@pytest.mark.parametrize("name", CASES)
def test_finetune_equals_the_model(name):
    reads, groups, cons, cycles = fc.case(name)
    exp_g, exp_c, _ = fc.expected(name)
    got_g, got_c = sorter.finetune(None, reads, groups, cons, max_cycles=cycles)
    assert as_lists(got_g) == exp_g
    assert list(got_c) == exp_c
    assert all(isinstance(g, np.ndarray) and g.dtype == np.int64 for g in got_g)


@pytest.mark.parametrize("cycles", [10, 2])
def test_all_cases_in_one_call_equal_the_cases_one_by_one(cycles):
    reads, groups, cons = fc.all_cases()
    got_g, got_c = sorter.finetune(None, reads, groups, cons, max_cycles=cycles)
    exp_g, exp_c, add_g, add_c = [], [], [], []
    for g, c in zip(groups, cons):
        one_g, one_c = sorter.finetune(None, reads, [g], [c], max_cycles=cycles)
        exp_g.append(one_g[0])
        exp_c.append(one_c[0])
        add_g += one_g[1:]                      # group A's come after all the groups
        add_c += one_c[1:]
    assert as_lists(got_g) == as_lists(exp_g + add_g)
    assert list(got_c) == exp_c + add_c
    assert len(add_g) >= 1
    if cycles == 10:                            # and so the whole call equals the model's
        mod_g, mod_c, _ = fc.model(reads, groups, cons)
        assert as_lists(got_g) == mod_g and list(got_c) == mod_c


def test_every_read_turned_round_gives_the_same_groups():
    """The same groups in the same places, each with the same reads.  Every distance is that of
    the mirrored pair, so the orientation and the start sequences are the same reads; the
    consensuses are not mirror images of each other (create_consensus' homopolymer correction
    looks at the column before), so a read's identity can move by a thousandth and with it the
    order group B and group A list their reads in, which is readlist's sort order."""
    reads, groups, cons = fc.all_cases()
    got_g, _ = sorter.finetune(None, reads, groups, cons)
    rev_g, _ = sorter.finetune(None, [fc.revcomp(r) for r in reads], groups, cons)
    assert [sorted(g) for g in as_lists(rev_g)] == [sorted(g) for g in as_lists(got_g)]
    assert len(got_g) == len(groups) + 1


def test_bytes_reads_and_the_hook_form():
    reads, groups, cons = fc.all_cases()
    hook = functools.partial(sorter.finetune, None, [r.encode() for r in reads])
    got_g, got_c = hook(groups, cons)
    exp_g, exp_c = sorter.finetune(None, reads, groups, cons)
    assert as_lists(got_g) == as_lists(exp_g) and got_c == exp_c


def test_refusals():
    reads, groups, cons = fc.all_cases()
    with pytest.raises(ValueError, match="one consensus per group"):
        sorter.finetune(None, reads, groups, cons[:-1])
    with pytest.raises(ValueError, match="max_cycles"):
        sorter.finetune(None, reads, groups, cons, max_cycles=0)
    with pytest.raises(lib.DmxError, match="outside the reads"):
        sorter.finetune(None, reads, [np.array([0, len(reads)])], ["ACGT"])
    assert sorter.finetune(None, reads, [], []) == ([], [])
    got_g, got_c = sorter.finetune(None, reads, [np.zeros(0, np.int64), np.array([3])], ["", "AC"])
    assert as_lists(got_g) == [[], [3]] and got_c == ["", "AC"]


@functools.lru_cache(maxsize=None)
def rest_expected():
    """rest_reads over fc.rest_bin() on the host twins, with and without the hook (once)."""
    reads, indexes, groups, _, _ = fc.rest_bin()
    cons = sorter.species_consensuses(None, reads, groups)
    hook = functools.partial(sorter.finetune, None, reads)
    return (sorter.rest_reads(None, reads, indexes, groups, cons, finetune=hook),
            sorter.rest_reads(None, reads, indexes, groups, cons), cons)


def test_rest_reads_with_the_hook_splits_the_mixed_group():
    """Without finetune the bin stays one blended group; with it the two species part, the
    second one as group B in the group's place, the first one as group A behind it, and the
    unassigned reads of either species join their own."""
    _, _, _, first, second = fc.rest_bin()
    (got_g, got_c), (plain_g, _), _ = rest_expected()
    assert len(plain_g) == 1
    assert len(got_g) == 2 and len(got_c) == 2 and got_c[0] != got_c[1]
    b, a = set(got_g[0].tolist()), set(got_g[1].tolist())
    assert b <= set(second) and a <= set(first)
    assert len(b & set(range(48, 56))) >= 6 and len(a & set(range(40, 48))) >= 6
