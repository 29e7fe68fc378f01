"""Cases of the operand builder past one tile per block (csrc/dmx_operands.hip
dmx_result_operands), shared by tests/test_operands_scale_host.py (no GPU) and
tests/test_operands_scale.py: the launch arithmetic restated, view lists of tens of thousands of
distinct views over a few hundred reads, a numpy statement of the record of every item, and the
source item of every table row."""
from __future__ import annotations

import functools

import numpy as np

import operands_cases as oc
import views_cases as vc
from dmx import lib

SEED = 31805
BLOCK = 256   # kOpBlock: items per tile, threads per block
GRID = 256    # kOpGrid: blocks at most
EDGE = 20     # a view starts 0 .. EDGE - 1 nt inside its read and ends as far before its end

SHAPES = {
    "two_tiles": GRID * BLOCK + BLOCK + 1,      # 258 tiles: a second tile per block, empty blocks
    "three_tiles": 2 * GRID * BLOCK + 300,      # 514 tiles: a bin's place carried twice in a block
    "one_tile": GRID * BLOCK,                   # the largest count with one tile in every block
}


def launch_shape(n: int):
    """(tiles, n_blocks, span) as dmx_result_operands sizes its three launches for n items."""
    tiles = (n + BLOCK - 1) // BLOCK
    n_blocks = max(1, min(tiles, GRID))
    span = max(1, (tiles + n_blocks - 1) // n_blocks) * BLOCK
    return tiles, n_blocks, span


def empty_blocks(n: int) -> int:
    """Blocks whose first item lies past the last one (lo >= n_items): they load their places
    and walk no tile."""
    _, n_blocks, span = launch_shape(n)
    return sum(1 for b in range(n_blocks) if b * span >= n)


# ---- reads and views ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bench_reads(n=480):
    """tests/test_operands.py demux_case's kind of reads: 200-420 nt with the benchmark's panels.
    Only the last `rare` reads carry the last SP5 adapter, so that its bins get an item every few
    hundred: some blocks feed them from one of their tiles alone."""
    rng = np.random.default_rng([SEED, 1])
    sp5, sp27 = vc.bench_panels()
    rare = 6
    reads = vc.demux_reads(rng, n - rare, sp5[:-1], sp27, lo=200, hi=420)
    for k in range(rare):
        s = (oc.rand_seq(rng, EDGE + 3 + k) + sp5[-1] + oc.rand_seq(rng, 150 + 20 * k) +
             sp27[k % len(sp27)] + oc.rand_seq(rng, EDGE + 9 - k))
        reads.append(oc.revcomp(s) if k % 3 == 2 else s)
    return reads, sp5, sp27


@functools.lru_cache(maxsize=None)
def one_pair_reads(n=480):
    """Every read carries unedited SP5[1] and SP27[2] behind flanks longer than any view cuts, a
    third stored reverse-complemented: every view of them lands in one bin."""
    rng = np.random.default_rng([SEED, 2])
    sp5, sp27 = vc.bench_panels()
    out = []
    for _ in range(n):
        s = (oc.rand_seq(rng, rng.integers(EDGE + 4, EDGE + 20)) + sp5[1] +
             oc.rand_seq(rng, rng.integers(150, 330)) + sp27[2] +
             oc.rand_seq(rng, rng.integers(EDGE + 4, EDGE + 20)))
        out.append(oc.revcomp(s) if rng.random() < 0.33 else s)
    return out, sp5, sp27


def distinct_views(rng, reads, n, edge=EDGE):
    """n views in random order, no two alike: (read, start, stop, strand) drawn without
    replacement from every read x start 0 .. edge - 1 x stop len - edge + 1 .. len x strand."""
    total = len(reads) * edge * edge * 2
    assert n <= total
    code = rng.choice(total, size=n, replace=False)
    strand = code % 2
    cut = (code // 2) % edge
    a = (code // (2 * edge)) % edge
    rd = code // (2 * edge * edge)
    L = np.array([len(s) for s in reads], np.int64)[rd]
    assert (L > 2 * edge).all()
    return (rd.astype(np.uint32), a.astype(np.int32), (L - cut).astype(np.int32),
            strand.astype(np.uint8))


def all_distinct(views) -> bool:
    rows = np.stack([np.asarray(x, np.int64) for x in views], axis=1)
    return len(np.unique(rows, axis=0)) == len(rows)


@functools.lru_cache(maxsize=None)
def views_of(shape: str, one_pair: bool = False):
    n = SHAPES[shape]
    reads = (one_pair_reads if one_pair else bench_reads)()[0]
    rng = np.random.default_rng([SEED, 3, sorted(SHAPES).index(shape), int(one_pair)])
    return distinct_views(rng, reads, n)


# ---- the record of every item, in numpy ---------------------------------------------------------

def item_records(res, lens, views, mode, w0, w1, keep, min_len):
    """Per item of round 0: (bin, alive, read, start, stop, strand), the trims composed as
    intervals of the item in the orientation each round took it (include/dmx.h
    dmx_result_operands).  views: None for whole reads."""
    two = mode == lib.MODE_TWO_ROUND
    n = len(res)
    lens = np.asarray(lens, np.int64)
    if views is None:
        rd = np.arange(n, dtype=np.int64)
        vs, ve, vst = np.zeros(n, np.int64), lens[:n].copy(), np.zeros(n, np.int64)
    else:
        rd, vs, ve, vst = (np.asarray(x, np.int64) for x in views)
    b1 = res["bin1"].astype(np.int64)
    b2 = res["bin2"].astype(np.int64) if two else np.full(n, -1, np.int64)
    a1 = len(w1) if two else 0
    bins = (b1 + 1) * (a1 + 1) + (b2 + 1)
    if keep is not None:
        kept = np.asarray(keep)[bins] != 0
    else:
        kept = (b1 >= 0) & ((b2 >= 0) if two else True)
    nn = ve - vs
    front0 = np.asarray(w0, np.int64)[np.maximum(b1, 0)] == oc.F
    m1 = b1 >= 0
    x = np.where(m1 & front0, res["m1_rstop"].astype(np.int64), 0)
    y = np.where(m1 & ~front0, res["m1_rstart"].astype(np.int64), nn)
    o = res["rc1"].astype(np.int64) & 1
    if two:
        front1 = np.asarray(w1, np.int64)[np.maximum(b2, 0)] == oc.F
        m2 = b2 >= 0
        n1 = y - x
        x2 = np.where(m2 & front1, res["m2_rstop"].astype(np.int64), 0)
        y2 = np.where(m2 & ~front1, res["m2_rstart"].astype(np.int64), n1)
        rc2 = res["rc2"].astype(np.int64) & 1
        base = np.where(rc2 == 1, nn - y, x)   # round 1's view on the strand it was taken
        o = np.where(m1, o ^ rc2, o)
        x, y = np.where(m1, base + x2, x), np.where(m1, base + y2, y)
    assert ((0 <= x) & (x <= y) & (y <= nn))[kept].all()
    alive = kept & (y - x >= min_len)
    t = vst ^ o
    start = np.where(t == 1, ve - y, vs + x)
    stop = np.where(t == 1, ve - x, vs + y)
    return bins, alive, rd, start, stop, t


def expected_table(rec):
    """(table, bin_first) of item_records' answer: the alive items, bin after bin in item order."""
    bins, alive, rd, start, stop, t = rec
    idx = np.flatnonzero(alive)
    idx = idx[np.argsort(bins[idx], kind="stable")]
    return (rd[idx].astype(np.uint32), start[idx].astype(np.int32), stop[idx].astype(np.int32),
            t[idx].astype(np.uint8)), idx


def sources(table, first, rec):
    """The source item of every table row, and the share of rows whose record no other item of
    their bin gives.  Items of one bin that give the same record (views of one read that hold
    both adapters trim to one record) cannot be told apart by their rows: the k-th row with a
    record is taken to be the k-th item that gives it.  Asserts that the rows of every bin are
    the records of its alive items, each as often."""
    bins, alive, rd, start, stop, t = rec
    idx = np.flatnonzero(alive)
    n = len(table[0])
    assert n == len(idx) == int(first[-1])
    row_bin = np.searchsorted(np.asarray(first, np.int64), np.arange(n), side="right") - 1
    items = np.stack([bins[idx], rd[idx], start[idx], stop[idx], t[idx]], axis=1)
    rows = np.stack([row_bin] + [np.asarray(x, np.int64) for x in table], axis=1)
    _, inv, cnt = np.unique(np.concatenate([items, rows]), axis=0, return_inverse=True,
                            return_counts=True)
    inv = inv.reshape(-1)
    ki, kr = inv[:n], inv[n:]
    oi, orr = np.argsort(ki, kind="stable"), np.argsort(kr, kind="stable")
    np.testing.assert_array_equal(ki[oi], kr[orr], err_msg="rows are not the items' records")
    src = np.empty(n, np.int64)
    src[orr] = idx[oi]
    return src, float((cnt[kr] == 2).mean())


def strictly_increasing_inside_bins(src, first) -> bool:
    d = np.diff(src) > 0
    edges = np.asarray(first, np.int64)[1:-1] - 1   # the step from a bin's last row to the next bin's
    d[edges[(edges >= 0) & (edges < len(d))]] = True
    return bool(d.all())


def tile_facts(rec, n):
    """What the alive items make of the launch: (a (block, bin) fed from two tiles of the block,
    a (block, bin) fed by the block's second tile and not by its first)."""
    bins, alive, *_ = rec
    _, _, span = launch_shape(n)
    k = np.flatnonzero(alive)
    tile = (k % span) // BLOCK
    key = (k // span) * (int(bins.max()) + 1) + bins[k]
    pairs = np.unique(np.stack([key, tile], axis=1), axis=0)
    keys, n_tiles = np.unique(pairs[:, 0], return_counts=True)
    with0 = set(pairs[pairs[:, 1] == 0, 0].tolist())
    second_only = any(x not in with0 for x in pairs[pairs[:, 1] == 1, 0].tolist())
    return bool((n_tiles >= 2).any()), second_only


def fast_results(rng, lens, a0, a1, floor=24):
    """operands_cases.synthetic_results for the benchmark's shape (round 0 FRONT, round 1 BACK)
    without the Python loop: random bins (-1 included; the last SP5 adapter in one item of
    fifty), orientations and trims that leave at least `floor` nt."""
    n = len(lens)
    L = np.asarray(lens, np.int64)
    res = np.zeros(n, dtype=lib.RESULT_DTYPE)
    b1 = np.where(rng.random(n) < 0.02, a0 - 1, rng.integers(-1, a0 - 1, size=n))
    b2 = np.where(b1 >= 0, rng.integers(-1, a1, size=n), -1)
    res["bin1"], res["bin2"] = b1, b2
    res["rc1"] = rng.integers(0, 2, size=n)
    res["rc2"] = np.where(b1 >= 0, rng.integers(0, 2, size=n), 0)
    cut1 = np.where(b1 >= 0, rng.integers(0, np.maximum(1, (L - floor) // 2)), 0)
    res["m1_rstop"] = cut1
    res["m1_rstart"] = np.maximum(0, cut1 - 20)
    n1 = L - cut1
    cut2 = np.where(b2 >= 0, rng.integers(0, np.maximum(1, n1 - floor)), 0)
    res["m2_rstart"] = np.where(b2 >= 0, n1 - cut2, 0)
    res["m2_rstop"] = np.where(b2 >= 0, np.minimum(n1, n1 - cut2 + 20), 0)
    return res


def loop_keep(a0, a1):
    """The loop's keep: no unknown bin in either round."""
    keep = np.ones((a0 + 1, a1 + 1), np.uint8)
    keep[0, :] = 0
    keep[:, 0] = 0
    return keep.reshape(-1)
