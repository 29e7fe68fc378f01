"""dmx.sorter on resident operands (sorter.Operands): given the Operands of a
bin, every function returns what it returns for the list of those sequences.  The bin's reads lie
as oriented sub-ranges inside longer raw reads, behind another bin in the table, so that the
bin's local indices are not the table's."""
import functools

import numpy as np
import pytest

import operands_cases as oc
import species_cases as sc
from dmx import lib, sorter

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def resident_bin():
    """The species bin's reads as operands: (raw reads, table, bin_first, the bin's sequences)."""
    rng = np.random.default_rng(31803)
    seqs = [r if isinstance(r, str) else bytes(r).decode() for r in sc.species_bin()[0]]
    raw, ops = [], []
    for k in range(7):   # bin 0: seven operands that are not the bin's
        raw.append(oc.rand_seq(rng, 90))
        ops.append((k, 5, 80, k & 1))
    for k, s in enumerate(seqs):
        strand = int(rng.integers(2))
        left, right = oc.rand_seq(rng, rng.integers(0, 40)), oc.rand_seq(rng, rng.integers(0, 40))
        if k % 2 == 0:   # every other pair of operands shares a raw read
            raw.append("")
        a = len(raw[-1]) + len(left)
        raw[-1] += left + (oc.revcomp(s) if strand else s) + right
        ops.append((len(raw) - 1, a, a + len(s), strand))
    first = np.array([0, 7, len(ops)], np.uint64)
    return raw, oc.table_arrays(ops), first, [s.encode() for s in seqs]


@pytest.fixture(scope="module")
def both():
    """(a context for the lists, the bin's Operands on a context of their own, the sequences)."""
    raw, tab, first, seqs = resident_bin()
    with lib.Context(0) as c_list, lib.Context(0) as c_ops:
        c_ops.load(oc.pack(raw))
        c_ops.set_operands(*tab)
        ops = sorter.Operands(c_ops, raw).bin(first, 1)
        yield c_list, ops, seqs


def _same_groups(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_operands_are_the_sequences(both):
    _, ops, seqs = both
    assert len(ops) == len(seqs) and [ops[k] for k in range(len(ops))] == seqs
    assert ops[-1] == seqs[-1] and len(ops[3:9]) == 6 and ops[3:9][2] == seqs[5]
    assert set(ops.strand.tolist()) == {0, 1} and ops.lengths.tolist() == [len(s) for s in seqs]


def test_similarity_and_groups(both):
    c, ops, seqs = both
    assert sorter.similarity(ops.ctx, ops, minlength=0) == sorter.similarity(c, seqs, minlength=0)
    # the length filter selects among the operands as it does among the list's reads
    lo = int(np.median([len(s) for s in seqs]))
    assert sorter.similarity(ops.ctx, ops, minlength=lo) == sorter.similarity(c, seqs, minlength=lo)
    _same_groups(sorter.gene_groups(ops.ctx, ops, minlength=lo),
                 sorter.gene_groups(c, seqs, minlength=lo))
    groups = sorter.gene_groups(c, seqs, minlength=0)
    _same_groups(sorter.gene_groups(ops.ctx, ops, minlength=0), groups)
    assert len(groups) >= 1
    assert sorter.estimate_ssg(ops.ctx, ops, minlength=0) == sorter.estimate_ssg(c, seqs, minlength=0)
    got = sorter.species_groups(ops.ctx, ops, groups, sc.SSG, minlength=0)
    exp = sorter.species_groups(c, seqs, groups, sc.SSG, minlength=0)
    assert len(got) == len(exp) and sum(len(x) for x in exp) >= 2
    for g, e in zip(got, exp):
        _same_groups(g, e)


def test_consensus_assign_and_rest_reads(both):
    c, ops, seqs = both
    groups = sorter.gene_groups(c, seqs, minlength=0)
    species = sorter.species_groups(c, seqs, groups, sc.SSG, minlength=0)
    k = int(np.argmax([len(s) for s in species]))
    sp = [g[:12] for g in species[k]]
    cons = sorter.make_consensus(c, seqs, sp)
    assert sorter.make_consensus(ops.ctx, ops, sp) == cons
    inside = np.concatenate(species[k])
    un = np.setdiff1d(groups[k], inside)
    un = un if len(un) else groups[k][:10]
    exp = sorter.assign_best(c, seqs, un, cons, 0.9)
    got = sorter.assign_best(ops.ctx, ops, un, cons, 0.9)
    assert got == exp and len(exp[0]) >= 1
    exp = sorter.rest_reads(c, seqs, groups[k], species[k], cons, similar_species=93.0)
    got = sorter.rest_reads(ops.ctx, ops, groups[k], species[k], cons, similar_species=93.0)
    _same_groups(got[0], exp[0])
    assert got[1] == exp[1]


def test_operands_of_a_replaced_batch_are_refused(both):
    _, ops, _ = both
    raw = resident_bin()[0]
    ops.ctx.load(oc.pack(raw))   # the same bases, but no longer the batch the operands were made on
    with pytest.raises(lib.DmxError, match="another batch"):
        sorter.gene_groups(ops.ctx, ops, minlength=0)
