"""The species groups on the CPU: the host twins dmx_hithist_host,
dmx_pairhits_cross_host and dmx_hitgroups_within_host against numpy, and sorter.estimate_ssg /
sorter.species_groups with ctx=None against the literal restatement of SSG and read_indexes
(species_cases).  No GPU."""
import numpy as np
import pytest

import genegroups_cases as gc
import species_cases as sc
from dmx import lib, sorter
from dmx.lib import DmxError

NONE = lib.LG_NONE


def bin_tables():
    """The bin's plan, host state, identity table, labels, second caps and ties."""
    reads, role, groups = sc.species_bin()
    p, ln, q, t, cap_sg, cap_half, hits = sc.species_plan()
    bin_off, bins = sorter._identity_table(ln, t, cap_sg)
    label = np.full(len(ln), NONE, dtype=np.uint32)
    for k, g in enumerate(groups):
        label[g] = k
    cap2 = np.array([sorter.identity_cap(int(L), sc.SSG / 100) for L in ln], dtype=np.int32)
    tie2 = np.where((hits.best != NONE) & (hits.best.astype(np.int64) <= cap2),
                    [sorter.identity_tie(int(b), int(L)) if b != NONE else 0
                     for b, L in zip(hits.best, ln)], NONE).astype(np.uint32)
    return ln, q, t, hits, bin_off, bins, label, cap2, tie2


def test_the_bin_has_its_features():
    sc.species_oracle()      # asserts them


def test_hithist_host_against_bincount_and_the_lines():
    ln, q, t, hits, bin_off, bins, *_ = bin_tables()
    pair, d, rev = hits.fetch()
    got = lib.hithist_host(hits, bin_off, bins, sorter.N_CLASSES)
    gc.assert_same(got, sc.np_hithist(hits.t, pair, d, bin_off, bins, sorter.N_CLASSES), "hist")
    lines = sc.species_oracle()[0]
    exp = np.bincount([int(round(x * 1000)) for x in sc.line_simils(lines)],
                      minlength=sorter.N_CLASSES)
    gc.assert_same(got, exp.astype(np.uint64), "hist against the restated lines")
    assert rev.any() and int(got.sum()) == len(lines)


def test_hithist_host_adds_and_refuses():
    ln, q, t, hits, bin_off, bins, *_ = bin_tables()
    L = lib.load()
    hist = np.full(sorter.N_CLASSES, 7, dtype=np.uint64)

    def call(off, b, n_classes):
        return L.dmx_hithist_host(hits.t.ctypes.data, hits.outcome.ctypes.data, len(hits.t),
                                  hits.n_reads, off.ctypes.data, b.ctypes.data, len(b), n_classes,
                                  hist.ctypes.data)

    assert call(bin_off, bins, sorter.N_CLASSES) == 0
    gc.assert_same(hist - np.uint64(7), lib.hithist_host(hits, bin_off, bins, sorter.N_CLASSES),
                   "the call adds to hist")
    before = hist.copy()
    pair, d, _ = hits.fetch()
    top = int((bin_off[hits.t[pair]].astype(np.int64) + d).max())
    assert call(bin_off, bins[:top + 1], sorter.N_CLASSES) == 0        # the last entry is read
    hist[:] = before
    assert call(bin_off, bins[:top], sorter.N_CLASSES) == -1           # one short: refused
    assert b"table index" in L.dmx_last_error(None)
    assert call(bin_off, bins, int(bins[bin_off[hits.t[pair]] + d].max())) == -1
    assert b"class" in L.dmx_last_error(None)
    assert call(bin_off, bins, 1025) == -1
    gc.assert_same(hist, before, "a refused call leaves hist untouched")
    with pytest.raises(DmxError, match="table index"):
        lib.hithist_host(hits, bin_off, bins[:top], sorter.N_CLASSES)


def test_cross_host_against_numpy():
    ln, q, t, hits, bin_off, bins, label, cap2, tie2 = bin_tables()
    pair, d, rev = hits.fetch()
    alt = (np.arange(len(ln)) % 2).astype(np.uint32)
    for lab, c2 in ((label, cap2), (alt, cap2), (alt, np.full(len(ln), -1, dtype=np.int32)),
                    (np.zeros(len(ln), dtype=np.uint32), cap2),
                    (np.full(len(ln), NONE, dtype=np.uint32), cap2)):
        keep = sc.np_cross(hits.q, hits.t, pair, d, lab, c2)
        gp, gd, gr = lib.pairhits_cross_host(hits, lab, c2)
        gc.assert_same(gp, pair[keep], "pair")
        gc.assert_same(gd, d[keep], "d")
        gc.assert_same(gr, rev[keep], "rev")
    assert sc.np_cross(hits.q, hits.t, pair, d, label, cap2).sum() > 0
    assert not len(lib.pairhits_cross_host(hits, np.zeros(len(ln), dtype=np.uint32), cap2)[0])


def test_within_host_against_union_find():
    ln, q, t, hits, bin_off, bins, label, cap2, tie2 = bin_tables()
    pair, d, _ = hits.fetch()
    n = len(ln)
    same = np.zeros(n, dtype=np.uint32)
    # all labels equal, no extra edge: dmx_hitgroups itself
    best_tie = np.where(hits.best != NONE, hits.best, NONE).astype(np.uint32)
    gc.assert_same(lib.hitgroups_within_host(hits, best_tie, same),
                   lib.hitgroups_host(hits, best_tie), "within == hitgroups")
    for lab, tie, xa, xb, nn in ((label, tie2, [], [], n),
                                 (label, tie2, [0, 3, n + 1], [n, n, 5], n + 2),
                                 (label, np.full(n, NONE, dtype=np.uint32), [1], [n], n + 1)):
        got = lib.hitgroups_within_host(hits, tie, lab, xa, xb, nn)
        gc.assert_same(got, sc.np_within(hits.q, hits.t, pair, d, tie, lab, xa, xb, nn), "labels")
    # tie2 = NONE is no edge, not a huge distance
    got = lib.hitgroups_within_host(hits, np.full(n, NONE, dtype=np.uint32), same)
    assert (got == NONE).all()


def test_within_host_refusals():
    ln, q, t, hits, bin_off, bins, label, cap2, tie2 = bin_tables()
    n = len(ln)
    with pytest.raises(DmxError, match="outside"):
        lib.hitgroups_within_host(hits, tie2, label, [0], [n + 1], n + 1)
    with pytest.raises(DmxError, match="nodes for"):
        lib.hitgroups_within_host(hits, tie2, label, [], [], n - 1)


def test_estimate_ssg_on_the_bin():
    reads = sc.species_bin()[0]
    lines = sc.species_oracle()[0]
    exp, margin = sc.ssg_float(sc.line_simils(lines))
    assert margin > sc.EDGE
    assert sorter.estimate_ssg(None, reads, minlength=0) == exp


def test_ssg_on_random_histograms():
    cases = sc.random_histograms()
    assert len(cases) >= 300 and len({s for _, s in cases}) > 20
    for hist, exp in cases:
        assert sorter.ssg_from_histogram(hist) == exp


def test_ssg_without_a_line_is_an_error():
    with pytest.raises(DmxError, match="no similarity line"):
        sorter.ssg_from_histogram(np.zeros(sorter.N_CLASSES, dtype=np.uint64))
    with pytest.raises(DmxError, match="no similarity line"):
        sorter.estimate_ssg(None, gc.quiet_bin(), minlength=0)


def test_species_groups_against_the_restatement():
    reads, role, groups = sc.species_bin()
    exp = sc.species_oracle()[2]
    got = sorter.species_groups(None, reads, groups, sc.SSG, minlength=0)
    assert len(got) == len(groups)
    for k, (sp, e) in enumerate(zip(got, exp)):
        assert {frozenset(m.tolist()) for m in sp} == e, k
        assert all((np.diff(m) > 0).all() for m in sp)
    # the read foreign to two groups is in a species group of each, and they stay apart
    x = int(np.flatnonzero(role == "X")[0])
    in_a = [m for m in got[0] if x in m]
    in_b = [m for m in got[1] if x in m]
    assert len(in_a) == 1 and len(in_b) == 1
    assert set(role[in_a[0]]) == {"A1", "X"} and set(role[in_b[0]]) == {"B1", "X"}
    # the dropped 3-read species, and the pulled-in reads of the small group
    assert not any((role[m] == "A3").any() for sp in got for m in sp)
    assert any(set(role[m]) == {"A2", "S"} for m in got[0])


def test_species_groups_order_and_nogroup():
    reads, role, groups = sc.species_bin()
    p, ln, *_ = sc.species_plan()
    got = sorter.species_groups(None, reads, groups, sc.SSG, minlength=0)
    assert [int(m[0]) for m in got[2]] == sorted(int(m[0]) for m in got[2])
    # no gene group at all (the reference's nogroup file): nothing
    assert sorter.species_groups(None, reads, [], sc.SSG, minlength=0) == []
    # at a threshold nothing reaches: every group is empty
    assert sorter.species_groups(None, reads, groups, 101, minlength=0) == [[], [], []]
    with pytest.raises(DmxError, match="shares a read"):
        sorter.species_groups(None, reads, [groups[0], groups[0][:2]], sc.SSG, minlength=0)
    with pytest.raises(DmxError, match="outside the reads"):
        sorter.species_groups(None, reads, [[len(ln)]], sc.SSG, minlength=0)


def test_cli_needs_groups(capsys):
    with pytest.raises(SystemExit):
        sorter.main(["-i", "x.fq", "-o", "o.txt", "--species-groups", "s.txt"])
    assert "--species-groups needs --groups" in capsys.readouterr().err
