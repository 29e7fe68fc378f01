"""dmx_result_operands on the GPU past one tile per block, and operand_of beyond the benchmark's
shape (csrc/dmx_operands.hip).  The oracle is the host twin
lib.result_operands_host on ctx.fetch()'s results (tied to a string model in
tests/test_operands_host.py); every comparison is exact equality of bin_first and of the four
table arrays."""
import functools

import numpy as np
import pytest

import operands_cases as oc
import operands_scale_cases as sc
import views_cases as vc
from dmx import lib

pytestmark = pytest.mark.gpu
F, B = oc.F, oc.B
TWO, SINGLE = lib.MODE_TWO_ROUND, lib.MODE_SINGLE
SEED = 31806
N = 3 * sc.BLOCK + 1   # the item count of section "operand_of": four blocks of one tile


@pytest.fixture(scope="module")
def ctx():
    with lib.Context(0) as c:
        yield c


def _panels(ctx, mode, p0, p1=None):
    """p0, p1: (adapters, DMX_FRONT or DMX_BACK); the benchmark's error rate and overlap."""
    ctx.set_panel(0, p0[0], p0[1] | lib.DMX_RC, 0.1, 3)
    if p1 is not None:
        ctx.set_panel(1, p1[0], p1[1] | lib.DMX_RC, 0.1, 3)
    ctx.set_mode(mode)
    return [p0[1]] * len(p0[0]), ([p1[1]] * len(p1[0]) if p1 is not None else None)


def _check(ctx, res, lens, mode, w0, w1, views, keep, min_len):
    """One build against the host twin and against item_records; returns (table, bin_first,
    item_records' answer)."""
    exp, efirst = lib.result_operands_host(res, lens, mode, w0, w1, views=views, keep=keep,
                                           min_len=min_len)
    first = ctx.result_operands(keep, min_len)
    np.testing.assert_array_equal(first, efirst)
    got = ctx.operands()
    assert len(got[0]) == int(first[-1])
    for g, e, name in zip(got, exp, ("read", "start", "stop", "strand")):
        np.testing.assert_array_equal(g, e, err_msg=name)
    rec = sc.item_records(res, lens, views, mode, w0, w1, keep, min_len)
    for g, e, name in zip(got, sc.expected_table(rec)[0], ("read", "start", "stop", "strand")):
        np.testing.assert_array_equal(g, e, err_msg=name + " (item_records)")
    return got, first, rec


def _exec(ctx, reads, views):
    ctx.load(oc.pack(reads))
    if views is not None:
        ctx.set_views(*views)
    ctx.exec_checked()
    return ctx.fetch(), [len(r) for r in reads]


# ---- 1. more than one tile per block ------------------------------------------------------------

@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_builder_at_scale(ctx, shape):
    reads, sp5, sp27 = sc.bench_reads()
    views = sc.views_of(shape)
    n = sc.SHAPES[shape]
    tiles, n_blocks, span = sc.launch_shape(n)   # dmx_result_operands' arithmetic
    assert n_blocks == 256 and span // 256 == {"two_tiles": 2, "three_tiles": 3, "one_tile": 1}[shape]
    assert (sc.empty_blocks(n) > 0) == (shape != "one_tile")
    w0, w1 = _panels(ctx, TWO, (sp5, F), (sp27, B))
    res, lens = _exec(ctx, reads, views)
    assert len(res) == n
    n_bins = (len(sp5) + 1) * (len(sp27) + 1)
    # keep all ones is not the loop's: the unknown bins' records are their views, each its own
    for keep in (None, sc.loop_keep(len(sp5), len(sp27)), np.ones(n_bins, np.uint8)):
        tab, first, rec = _check(ctx, res, lens, TWO, w0, w1, views, keep, 1)
        src, unique = sc.sources(tab, first, rec)
        assert sc.strictly_increasing_inside_bins(src, first)
        assert len(src) > n // 3
        if keep is not None and keep.all():
            assert len(src) == n and unique > 0.15
        two, second_only = sc.tile_facts(rec, n)
        assert two == second_only == (shape != "one_tile")


def test_builder_all_items_in_one_bin(ctx):
    reads, sp5, sp27 = sc.one_pair_reads()
    views = sc.views_of("two_tiles", True)
    n = sc.SHAPES["two_tiles"]
    w0, w1 = _panels(ctx, TWO, (sp5, F), (sp27, B))
    res, lens = _exec(ctx, reads, views)
    the_bin = (1 + 1) * (len(sp27) + 1) + (2 + 1)
    tab, first, rec = _check(ctx, res, lens, TWO, w0, w1, views, None, 1)
    bins, alive = rec[0], rec[1]
    assert alive.mean() > 0.99 and (bins[alive] == the_bin).all()
    assert int(first[the_bin]) == 0 and int(first[the_bin + 1]) == int(alive.sum()) == len(tab[0])
    # whole tiles of one bin: every wave hands its place to the next, tile after tile
    full = alive[:n - n % sc.BLOCK].reshape(-1, sc.BLOCK).all(axis=1)
    assert full.sum() > 200 and full[:256].reshape(-1, 2).all(axis=1).any()   # both tiles of a block
    src, _ = sc.sources(tab, first, rec)
    np.testing.assert_array_equal(src, np.flatnonzero(alive))   # the identity over the survivors
    assert len(np.unique(np.stack([x.astype(np.int64) for x in tab], axis=1), axis=0)) >= len(reads)


# ---- 2. operand_of beyond the benchmark's shape -------------------------------------------------

@functools.lru_cache(maxsize=None)
def demux_reads():
    rng = np.random.default_rng([SEED, 1])
    sp5, sp27 = vc.bench_panels()
    return vc.demux_reads(rng, N, sp5, sp27, lo=200, hi=420), sp5, sp27


@functools.lru_cache(maxsize=None)
def crossed_reads():
    """N reads for round 0 = SP27 as BACK, round 1 = SP5 as FRONT: half carry SP5 + body + SP27,
    half body + revcomp(SP5) + SP27, whose SP5 copy round 1 finds on the other strand of what
    round 0 left; a third of either kind is stored reverse-complemented."""
    rng = np.random.default_rng([SEED, 2])
    sp5, sp27 = vc.bench_panels()
    out = []
    for k in range(N):
        f = vc.sw.mutate(rng, sp5[int(rng.integers(len(sp5)))], 0.05)
        b = vc.sw.mutate(rng, sp27[int(rng.integers(len(sp27)))], 0.05)
        body = oc.rand_seq(rng, rng.integers(90, 260))
        lf, rf = oc.rand_seq(rng, rng.integers(0, 25)), oc.rand_seq(rng, rng.integers(0, 25))
        s = lf + (f + body if k % 2 else body + oc.revcomp(f)) + b + rf
        out.append(oc.revcomp(s) if rng.random() < 0.33 else s)
    return out, sp5, sp27


def _random_views(rng, reads, n):
    rd = rng.integers(0, len(reads), size=n)
    L = np.array([len(reads[int(r)]) for r in rd])
    return (rd.astype(np.uint32), rng.integers(0, 15, size=n).astype(np.int32),
            (L - rng.integers(0, 15, size=n)).astype(np.int32),
            rng.integers(0, 2, size=n).astype(np.uint8))


@pytest.mark.parametrize("where", [F, B])
def test_single_mode(ctx, where):
    reads, sp5, sp27 = demux_reads()
    pan = sp5 if where == F else sp27
    w0, _ = _panels(ctx, SINGLE, (pan, where))
    res, lens = _exec(ctx, reads, None)
    assert ctx.n_counts() - 2 == len(pan) + 1
    tab, first, rec = _check(ctx, res, lens, SINGLE, w0, None, None, None, 1)
    matched = int((res["bin1"] >= 0).sum())
    assert len(tab[0]) == matched and N // 2 < matched < N and set(tab[3].tolist()) == {0, 1}
    # every bin kept: the unknown bin's untrimmed, oriented records come too
    tab, first, rec = _check(ctx, res, lens, SINGLE, w0, None, None, np.ones(len(pan) + 1), 1)
    assert len(tab[0]) == N and rec[1].all() and ((tab[2] - tab[1]) > 0).all()
    unknown = slice(0, int(first[1]))
    assert int(first[1]) == N - matched
    np.testing.assert_array_equal(tab[1][unknown], 0)
    np.testing.assert_array_equal(tab[2][unknown], np.array(lens)[tab[0][unknown]])
    # a 5' adapter trims the record's start, a 3' adapter its end (on the strand it was found)
    ln = np.array(lens)[tab[0]]
    rest = slice(int(first[1]), N)
    fwd = tab[3][rest] == 0
    edge = np.where(fwd == (where == F), tab[2][rest] == ln[rest], tab[1][rest] == 0)
    assert edge.all() and fwd.any() and (~fwd).any()


@pytest.mark.parametrize("with_views", [False, True])
def test_two_rounds_back_then_front(ctx, with_views):
    reads, sp5, sp27 = crossed_reads()
    views = _random_views(np.random.default_rng([SEED, 3]), reads, N) if with_views else None
    w0, w1 = _panels(ctx, TWO, (sp27, B), (sp5, F))
    res, lens = _exec(ctx, reads, views)
    both = (res["bin1"] >= 0) & (res["bin2"] >= 0)
    assert {(int(a), int(b)) for a, b in zip(res["rc1"][both], res["rc2"][both])} == \
        {(0, 0), (0, 1), (1, 0), (1, 1)}
    if with_views:
        assert set(views[3][both].tolist()) == {0, 1}
    tab, first, _ = _check(ctx, res, lens, TWO, w0, w1, views, None, 1)
    assert len(tab[0]) == int(both.sum()) > N // 2 and set(tab[3].tolist()) == {0, 1}
    _check(ctx, res, lens, TWO, w0, w1, views, np.ones(len(first) - 1), 1)
    _check(ctx, res, lens, TWO, w0, w1, views, None, 50)


def test_benchmark_order_every_bin_kept(ctx):
    reads, sp5, sp27 = demux_reads()
    w0, w1 = _panels(ctx, TWO, (sp5, F), (sp27, B))
    res, lens = _exec(ctx, reads, None)
    a1 = len(sp27) + 1
    half = (res["bin1"] >= 0) & (res["bin2"] < 0)
    none = res["bin1"] < 0
    assert half.sum() > 20 and none.sum() > 20 and res["rc1"][half].any()
    tab, first, rec = _check(ctx, res, lens, TWO, w0, w1, None, np.ones(len(sp5) * a1 + a1), 1)
    assert len(tab[0]) == N
    # their rows, bin by bin, are the host twin's (_check) and name these very items
    src, _ = sc.sources(tab, first, rec)
    bins = rec[0]
    for b in np.unique(bins[half | none]):
        lo, hi = int(first[b]), int(first[b + 1])
        np.testing.assert_array_equal(src[lo:hi], np.flatnonzero(bins == b))
    assert set(np.unique(bins[none]).tolist()) == {0}
    assert (np.unique(bins[half]) % a1 == 0).all() and len(np.unique(bins[half])) > 1
    # an unmatched round leaves its view whole: the read itself, or round 0's trim to the end
    rows = np.empty(N, np.int64)
    rows[src] = np.arange(N)
    ln = np.array(lens)
    assert (tab[1][rows[none]] == 0).all() and (tab[2][rows[none]] == ln[none]).all()
    k = rows[half]
    fwd = tab[3][k] == 0
    assert (np.where(fwd, tab[2][k] == ln[half], tab[1][k] == 0)).all() and fwd.any() and (~fwd).any()
    np.testing.assert_array_equal(tab[3][k], res["rc1"][half] ^ res["rc2"][half])


def test_min_len_boundary_on_the_device(ctx):
    reads, sp5, sp27 = demux_reads()
    w0, w1 = _panels(ctx, TWO, (sp5, F), (sp27, B))
    res, lens = _exec(ctx, reads, None)
    tab, _, _ = _check(ctx, res, lens, TWO, w0, w1, None, None, 1)
    final = (tab[2] - tab[1]).astype(np.int64)
    m = int(np.sort(final)[len(final) // 3])
    assert (final == m).any() and (final < m).any()
    tab, _, _ = _check(ctx, res, lens, TWO, w0, w1, None, None, m)
    assert len(tab[0]) == int((final >= m).sum()) and (tab[2] - tab[1]).min() == m   # m is kept
    tab, _, _ = _check(ctx, res, lens, TWO, w0, w1, None, None, m + 1)
    assert len(tab[0]) == int((final > m).sum()) and (tab[2] - tab[1]).min() > m     # m is dropped


def test_empty_view_run(ctx):
    reads, sp5, sp27 = demux_reads()
    w0, w1 = _panels(ctx, TWO, (sp5, F), (sp27, B))
    # a table from before: the empty run must not serve it
    res, lens = _exec(ctx, reads, None)
    _check(ctx, res, lens, TWO, w0, w1, None, None, 1)
    empty = vc.view_arrays([])
    res, lens = _exec(ctx, reads, empty)
    assert len(res) == 0
    n_bins = (len(sp5) + 1) * (len(sp27) + 1)
    for keep in (None, np.ones(n_bins, np.uint8)):
        tab, first, _ = _check(ctx, res, lens, TWO, w0, w1, empty, keep, 1)
        assert len(first) == n_bins + 1 and not first.any() and len(tab[0]) == 0
        with pytest.raises(lib.DmxError, match=r"\(-1\)"):   # operand 0 of an empty table
            ctx.pairdist([0], [0])


def test_rebuilding_on_one_context(ctx):
    reads, sp5, sp27 = demux_reads()
    n_bins = (len(sp5) + 1) * (len(sp27) + 1)
    w0, w1 = _panels(ctx, TWO, (sp5, F), (sp27, B))
    res, lens = _exec(ctx, reads, None)
    big, _, _ = _check(ctx, res, lens, TWO, w0, w1, None, np.ones(n_bins, np.uint8), 1)
    assert len(big[0]) == N                                          # four blocks, every bin
    # a smaller run with fewer blocks and one kept bin: nothing of the larger table shows
    views = _random_views(np.random.default_rng([SEED, 4]), reads, 150)
    res2, _ = _exec(ctx, reads, views)
    counts = np.bincount(sc.item_records(res2, lens, views, TWO, w0, w1, None, 1)[0],
                         minlength=n_bins)
    keep = np.zeros(n_bins, np.uint8)
    keep[int(np.argmax(counts))] = 1
    small, first, _ = _check(ctx, res2, lens, TWO, w0, w1, views, keep, 1)
    assert 0 < len(small[0]) == counts.max() < 150 and len(ctx.operands()[0]) == len(small[0])
    # keep=None after a keep build: the flags of the build before are not read
    tab, first, _ = _check(ctx, res2, lens, TWO, w0, w1, views, None, 1)
    assert len(tab[0]) > len(small[0]) and (np.diff(first.astype(np.int64)) > 0).sum() > 4
    none_kept = np.zeros(n_bins, np.uint8)
    tab, first, _ = _check(ctx, res2, lens, TWO, w0, w1, views, none_kept, 1)
    assert len(tab[0]) == 0 and not first.any()
    # other bins: single mode after two rounds on the same context
    w0s, _ = _panels(ctx, SINGLE, (sp27, B))
    res3, _ = _exec(ctx, reads, None)
    tab, first, _ = _check(ctx, res3, lens, SINGLE, w0s, None, None, None, 60)
    assert len(first) == len(sp27) + 2 and 0 < len(tab[0]) < N
