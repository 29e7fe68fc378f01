"""What tests/operands_scale_cases.py claims, as far as it needs no GPU (csrc/dmx_operands.hip
dmx_result_operands): the launch arithmetic of the three shapes, the
distinctness of their views, the numpy statement of the records against the host twin, and the
host twin's strict item order inside every bin at those item counts."""
import numpy as np
import pytest

import operands_cases as oc
import operands_scale_cases as sc
from dmx import lib

F, B = oc.F, oc.B


def test_launch_arithmetic_of_the_shapes():
    assert sc.launch_shape(3 * 256 + 1) == (4, 4, 256)            # tests/test_operands.py's cases
    assert sc.launch_shape(1_000_000) == (3907, 256, 16 * 256)    # the 1 M-read workload
    assert sc.launch_shape(0) == (0, 1, 256)
    tiles, n_blocks, span = sc.launch_shape(sc.SHAPES["two_tiles"])
    assert (tiles, n_blocks, span // 256) == (258, 256, 2)
    n = sc.SHAPES["two_tiles"]
    assert sc.empty_blocks(n) == 127 and (n - 128 * span) == 257   # block 128: a tile and 1 item
    tiles, n_blocks, span = sc.launch_shape(sc.SHAPES["three_tiles"])
    assert (tiles, n_blocks, span // 256) == (514, 256, 3) and sc.empty_blocks(sc.SHAPES["three_tiles"]) > 0
    tiles, n_blocks, span = sc.launch_shape(sc.SHAPES["one_tile"])
    assert (tiles, n_blocks, span // 256) == (256, 256, 1) and sc.empty_blocks(sc.SHAPES["one_tile"]) == 0
    assert sc.launch_shape(sc.SHAPES["one_tile"] + 1)[2] == 2 * 256   # the first count past it


@pytest.mark.parametrize("shape", list(sc.SHAPES))
@pytest.mark.parametrize("one_pair", [False, True])
def test_views_are_distinct_sub_ranges(shape, one_pair):
    if one_pair and shape != "two_tiles":
        return
    reads = (sc.one_pair_reads if one_pair else sc.bench_reads)()[0]
    v = sc.views_of(shape, one_pair)
    assert len(v[0]) == sc.SHAPES[shape] and sc.all_distinct(v)
    L = np.array([len(s) for s in reads])[v[0]]
    assert 200 < len(reads) < 1000 and (v[1] >= 0).all() and (v[1] < v[2]).all() and (v[2] <= L).all()
    assert set(v[3].tolist()) == {0, 1} and (v[1] == 0).any() and (v[2] == L).any()
    assert len(np.unique(v[0])) == len(reads)
    lib.operands_check_host([len(s) for s in reads], *v)   # what dmx_set_views asks of a list too


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_host_twin_keeps_item_order_inside_every_bin(shape):
    reads, sp5, sp27 = sc.bench_reads()
    views = sc.views_of(shape)
    n = len(views[0])
    rng = np.random.default_rng([sc.SEED, 9, n])
    res = sc.fast_results(rng, views[2] - views[1], len(sp5), len(sp27))
    lens = [len(s) for s in reads]
    w0, w1 = [F] * len(sp5), [B] * len(sp27)
    n_bins = (len(sp5) + 1) * (len(sp27) + 1)
    for keep, min_len in ((None, 1), (sc.loop_keep(len(sp5), len(sp27)), 1),
                          (np.ones(n_bins, np.uint8), 60)):
        tab, first = lib.result_operands_host(res, lens, lib.MODE_TWO_ROUND, w0, w1, views=views,
                                              keep=keep, min_len=min_len)
        rec = sc.item_records(res, lens, views, lib.MODE_TWO_ROUND, w0, w1, keep, min_len)
        exp, _ = sc.expected_table(rec)
        for g, e, name in zip(tab, exp, ("read", "start", "stop", "strand")):
            np.testing.assert_array_equal(g, e, err_msg=name)
        np.testing.assert_array_equal(np.diff(first.astype(np.int64)),
                                      np.bincount(rec[0][rec[1]], minlength=n_bins))
        src, unique = sc.sources(tab, first, rec)
        assert sc.strictly_increasing_inside_bins(src, first)
        # random trims: nearly every record is its item's alone, so the order check is sharp
        assert unique > 0.95 and len(src) > n // 2
        two, second_only = sc.tile_facts(rec, n)
        assert two == second_only == (shape != "one_tile")


def test_sources_notices_a_swap():
    """The order check of the GPU tests fails on a table with two rows of a bin exchanged, and on
    one whose second tile took the first tile's places."""
    reads, sp5, sp27 = sc.bench_reads()
    views = tuple(x[:3000] for x in sc.views_of("one_tile"))
    rng = np.random.default_rng([sc.SEED, 10])
    res = sc.fast_results(rng, views[2] - views[1], len(sp5), len(sp27))
    lens = [len(s) for s in reads]
    w0, w1 = [F] * len(sp5), [B] * len(sp27)
    tab, first = lib.result_operands_host(res, lens, lib.MODE_TWO_ROUND, w0, w1, views=views)
    rec = sc.item_records(res, lens, views, lib.MODE_TWO_ROUND, w0, w1, None, 1)
    b = int(np.argmax(np.diff(first.astype(np.int64))))
    i, j = int(first[b]), int(first[b + 1]) - 1
    assert j > i
    bad = [x.copy() for x in tab]
    for x in bad:
        x[i], x[j] = x[j], x[i]
    src, _ = sc.sources(bad, first, rec)
    assert not sc.strictly_increasing_inside_bins(src, first)
    with pytest.raises(AssertionError):
        dup = [x.copy() for x in tab]
        for x in dup:
            x[j] = x[i]
        sc.sources(dup, first, rec)
