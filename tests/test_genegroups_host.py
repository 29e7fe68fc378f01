"""Gene groups on the host (include/dmx.h dmx_edgegroups_host, dmx_pairhits_host,
dmx_hitgroups_host; dmx.sorter.gene_groups(None, ...)) against a literal
restatement of amplicon_sorter.py update_list (:983-1034) and merge_groups (:1058-1087).  No GPU."""
import numpy as np
import pytest

import genegroups_cases as gc
import pairdist_cases as pc
from dmx import lib, sorter


def reference_components(a, b, n):
    """The restatement's groups for the edge list: one line per edge, all of one identity, so
    that its filter keeps every line; as labels."""
    lines = [f"{x}:{y}:0.9" for x, y in zip(a, b)]
    _, grouplist = gc.update_list(lines)
    labels = np.full(n, gc.NONE, dtype=np.uint32)
    for g in gc.as_index_groups(grouplist):
        labels[g] = g[0]
    return labels


@pytest.mark.parametrize("name", sorted(gc.small_graphs()))
def test_edgegroups_host_equals_the_restatement(name):
    a, b, n = gc.small_graphs()[name]
    got = lib.edgegroups_host(a, b, n)
    np.testing.assert_array_equal(got, gc.components(list(zip(a, b)), n))
    if not any(x == y for x, y in zip(a, b)):   # the reference never sees a read against itself
        np.testing.assert_array_equal(got, reference_components(a, b, n))


def test_isolated_nodes_and_self_loops():
    a, b, n = gc.small_graphs()["star"]
    got = lib.edgegroups_host(a, b, n)
    assert got[17] == lib.LG_NONE and (np.delete(got, 17) == 0).all()
    assert lib.edgegroups_host([3], [3], 5).tolist() == [lib.LG_NONE] * 3 + [3, lib.LG_NONE]
    assert len(lib.edgegroups_host([], [], 0)) == 0


def test_the_bin_holds_what_it_is_meant_to():
    """Every property the bin is built for is there, so that it cannot quietly stop testing it."""
    reads, fam = gc.gene_bin()
    lines, hits, templist, groups = gc.gene_bin_oracle()
    ln = np.array([len(r) for r in reads])
    for f in range(3):
        assert 13 <= (fam == f).sum() <= 17 and ((ln[fam == f] >= 120) & (ln[fam == f] <= 200)).all()
    assert (fam == 3).sum() == 8 and ((ln[fam == 3] >= 1100) & (ln[fam == 3] <= 2100)).all()
    kept = {(int(x[0]), int(x[1])): x[2] for x in templist}
    d_of = {(a, b): (d, r) for a, b, d, r in hits}
    # reverse hits form edges
    assert sum(1 for e in kept if d_of[e][1]) >= 1
    # the filter matters: with every line an edge, families A and B merge; the bridge read is
    # hit by both, and only its hits from B are best hits
    n = len(reads)
    unfiltered = gc.groups_of(gc.components([(a, b) for a, b, _, _ in hits], n))
    assert unfiltered != sorted(groups)
    bridge = int(np.flatnonzero(ln == 167)[0])
    assert {fam[a] for a, b, _, _ in hits if b == bridge} == {0, 1}
    assert {fam[a] for (a, b) in kept if b == bridge} == {1}
    assert sorted(sorted(set(fam[g].tolist())) for g in groups) == [[0], [1], [2], [3]]
    # some longer read keeps two lines of different distances and one identity ...
    per_j = {}
    for (a, b), iden in kept.items():
        per_j.setdefault(b, []).append((d_of[(a, b)][0], iden))
    assert any(len({d for d, _ in v}) > 1 and len({i for _, i in v}) == 1 and ln[j] > 1000
               for j, v in per_j.items())
    # ... and some longer read keeps two lines of one distance
    assert any(len(v) > len({d for d, _ in v}) for v in per_j.values())
    # reads with no hit at all
    on_a_line = {a for a, _, _, _ in hits} | {b for _, b, _, _ in hits}
    assert set(np.flatnonzero(fam >= 4)) and not (set(np.flatnonzero(fam >= 4)) & on_a_line)


def test_gene_groups_host_equals_the_restatement():
    reads, _ = gc.gene_bin()
    _, _, _, groups = gc.gene_bin_oracle()
    got = sorter.gene_groups(None, reads, minlength=0)
    assert [g.tolist() for g in got] == groups          # the partition and the groups' order
    assert all(g.dtype == np.int64 and (np.diff(g) > 0).all() for g in got)
    # lower case in, the same groups out
    assert [g.tolist() for g in sorter.gene_groups(None, [r.lower() for r in reads], minlength=0)] \
        == groups


def test_a_bin_where_nothing_hits_has_no_groups():
    assert gc.update_list(gc.restated_lines(gc.quiet_bin())[0])[1] == []
    assert sorter.gene_groups(None, gc.quiet_bin(), minlength=0) == []


def test_pairhits_host_equals_the_restated_lines():
    reads, _ = gc.gene_bin()
    _, hits, _, _ = gc.gene_bin_oracle()
    p, ln, q, t, cap_hit, cap_half = gc.bin_plan(reads)
    st = lib.pairhits_host(p, q, t, cap_hit, cap_half, n_threads=8)
    pair, d, rev = st.fetch()
    assert [(int(q[k]), int(t[k]), int(dd), bool(r)) for k, dd, r in zip(pair, d, rev)] == hits
    best = np.full(len(reads), lib.LG_NONE, dtype=np.uint32)
    np.minimum.at(best, t[pair], d)
    np.testing.assert_array_equal(st.best, best)


def test_the_tie_table_is_the_reference_rounding():
    for L in (120, 999, 1000, 1001, 1500, 2100):
        for d in range(0, L // 4, 7):
            hi = sorter.identity_tie(d, L)
            assert hi >= d and round(1 - hi / L, 3) == round(1 - d / L, 3)
            assert hi == L or round(1 - (hi + 1) / L, 3) != round(1 - d / L, 3)
    assert sorter.identity_tie(31, 1500) == 32 and sorter.identity_tie(30, 165) == 30


def test_update_list_can_keep_a_line_below_the_best():
    """What the restatement shows about the reference and DESIGN.md §8i writes down: its filter
    runs after every line and drops a line only when the next one in the sorted list is better,
    so of two equal lines followed by a better one the first stays until another line for that
    read arrives.  Which lines survive that way depends on the order of the lines (the
    reference's workers interleave theirs).  gene_groups keeps the best lines and their ties
    only; on the bin every such leftover joins two reads of one group, so the groups agree."""
    kept, _ = gc.update_list(["1:9:0.9", "2:9:0.9", "3:9:0.95"])
    assert [x[0] for x in kept] == ["3", "1"]
    kept, _ = gc.update_list(["1:9:0.9", "2:9:0.9", "3:9:0.95", "4:9:0.8"])
    assert [x[0] for x in kept] == ["3"]
    lines, _, templist, groups = gc.gene_bin_oracle()
    left = {(int(x[0]), int(x[1])) for x in templist} - gc.best_lines(lines)
    where = {v: k for k, g in enumerate(groups) for v in g}
    assert all(where[a] == where[b] for a, b in left)
    assert gc.best_lines(lines) <= {(int(x[0]), int(x[1])) for x in templist}


# ---- pair lists of many blocks and tiles (genegroups_cases.scale_case) ---------------------------

@pytest.mark.parametrize("layout", gc.SCALE_LAYOUTS)
def test_host_twins_equal_the_numpy_oracle_at_scale(layout):
    """The twins the GPU tests compare with, against numpy arithmetic on the distinct pairs'
    distances: outcomes, hits, best, and the labels for both tie tables."""
    c = gc.scale_case(layout, gc.SCALE_HOST_N)
    host = c.host
    gc.assert_same(host.outcome, c.outcome, "outcome")
    pair, d, rev = host.fetch()
    gc.assert_same(pair, c.pair, "pair")
    gc.assert_same(d, c.d, "d")
    gc.assert_same(rev, c.rev, "rev")
    gc.assert_same(host.best, c.best, "best")
    for name, tie in c.ties().items():
        gc.assert_same(lib.hitgroups_host(host, tie), c.labels(tie), f"labels, tie = {name}")


def test_the_scale_lists_hold_what_they_are_meant_to():
    """Conditions on the generator, not on code under test: a weak list cannot hide a failure."""
    n = gc.SCALE_TOP
    assert sorted(set(gc.scale_cases())) == sorted(
        [(name, n) for name in gc.SCALE_LAYOUTS] +
        [(name, k) for name in ("all_forward", "mixed")
         for k in (255, 256, 257, 16384, 16385, 65536, 65537)])
    reads, p, d_fwd, d_rev = gc.scale_reads()
    assert len(reads) == 64 and p.lengths.max() <= 64     # one 64-row word per read

    def per_block(c):
        return np.add.reduceat(c.hit.astype(np.int64), np.arange(0, c.n, 256))

    mixed = gc.scale_case("mixed", n)
    assert (np.bincount(mixed.cls, minlength=4) >= n // 8).all()
    assert mixed.rev.any() and not mixed.rev.all()
    for name, tie in mixed.ties().items():                # the tie filter removes and keeps
        assert 0 < mixed.edges(tie).sum() < mixed.n_hits, name
    assert mixed.edges(mixed.ties()["best"]).sum() < mixed.edges(mixed.ties()["best+1"]).sum()
    labels = mixed.labels(mixed.best)
    assert len(gc.groups_of(labels)) >= 4 and (labels == gc.NONE).any()

    c = gc.scale_case("all_forward", n)
    assert c.n_hits == n and (per_block(c)[:-1] == 256).all() and per_block(c)[-1] == n % 256
    c = gc.scale_case("none", n)
    assert c.n_hits == 0 and abs(int((c.cap_hit == -1).sum()) - n // 2) <= 1
    assert ((c.cap_hit >= 0) & (c.cap_half >= c.d_fwd)).any()
    c = gc.scale_case("every_257th", n)
    assert sorted(set((c.pair % 256).tolist())) == list(range(256))   # every place in a block
    assert set(per_block(c).tolist()) == {0, 1}
    c = gc.scale_case("block_stripes", n)
    assert {0, 256} <= set(per_block(c).tolist())
    c = gc.scale_case("tile_heads", n)
    tiles = per_block(c)[:256 * (len(per_block(c)) // 256)].reshape(-1, 256).sum(axis=1)
    assert (tiles == 1).any() and c.hit[-1] and c.pair.tolist() == [0, 65536, 131072, n - 1]
    c = gc.scale_case("last_only", n)
    assert c.pair.tolist() == [n - 1] and c.rev.tolist() == [1]
    c = gc.scale_case("one_target", n)
    assert len(set(c.t.tolist())) == 3
    assert np.bincount(c.t[c.pair], minlength=c.n_reads).max() > 10000
    assert (np.bincount(c.cls, minlength=4) >= n // 8).all()
    # both sides of every comparison of the rule, at the boundary
    assert (mixed.d_fwd == mixed.cap_hit).any() and (mixed.d_fwd == mixed.cap_hit + 1).any()
    assert (mixed.d_fwd == mixed.cap_half).any() and (mixed.d_fwd == mixed.cap_half + 1).any()
    tried = (mixed.cls == gc.R) | (mixed.cls == gc.X)
    assert (mixed.d_rev == mixed.cap_hit)[tried].any()
    assert (mixed.d_rev == mixed.cap_hit + 1)[tried].any()


def test_argument_checks():
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        lib.edgegroups_host([0, 5], [1, 2], 5)            # an endpoint out of range
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        lib.hitgroups_host(None, np.zeros(3, dtype=np.uint32))   # hitgroups before pairhits
    rng = np.random.default_rng(8)
    a = pc.rand_seq(rng, 90, p_n=0.0)
    reads = [a, pc.mutate(rng, a, 0.02), pc.revcomp(a), pc.rand_seq(rng, 90, p_n=0.0)]
    p = pc.pack_reads(reads)
    q, t = [0, 0, 0], [1, 2, 3]
    # caps of -1: no hit threshold means no hit and no reverse try, whatever the distance
    st = lib.pairhits_host(p, q, t, [-1, -1, -1], [-1, 40, -1])
    assert (st.outcome == lib.LG_NONE).all() and (st.best == lib.LG_NONE).all()
    # cap_half of -1 with a hit cap: every forward miss is tried reversed
    st = lib.pairhits_host(p, q, t, [18, 18, 18], [-1, -1, -1])
    pair, d, rev = st.fetch()
    assert pair.tolist() == [0, 1] and rev.tolist() == [0, 1] and d[1] == 0
    labels = lib.hitgroups_host(st, np.array([0, 18, 18, 0], dtype=np.uint32))
    assert labels.tolist() == [0, 0, 0, lib.LG_NONE]
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        lib.pairhits_host(p, q, t, [-2, 0, 0], [0, 0, 0])
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        lib.pairhits_host(p, [0], [4], [5], [5])           # a read outside the batch
