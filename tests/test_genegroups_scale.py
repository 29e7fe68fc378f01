"""dmx_pairhits, dmx_pairhits_fetch and dmx_hitgroups on pair lists of many blocks and tiles
(csrc/dmx_groups.hip).  A block of the compaction takes 256 pairs and
lg_scan_kernel scans the block counts 256 at a time, four waves of 64: its cross-wave offset
runs from 65 blocks (16,385 pairs) on, its tile loop and carry from 257 blocks (65,537 pairs) on.
The lists, and what is expected of them from numpy alone, are genegroups_cases.scale_case; the
host twins, pinned to that oracle by test_genegroups_host.py, are compared as well."""
import ctypes

import numpy as np
import pytest

import genegroups_cases as gc
from dmx import lib

pytestmark = pytest.mark.gpu


def run_and_check(ctx, c):
    """pairhits + fetch of c's list on the loaded batch against the oracle and the host twin."""
    best, n_hits = ctx.pairhits(*c.args())
    assert n_hits == c.n_hits
    check_fetch(ctx, c)
    gc.assert_same(best, c.best, "best")
    gc.assert_same(best, c.host.best, "best (host twin)")


def check_fetch(ctx, c):
    pair, d, rev = ctx.pairhits_fetch()
    hp, hd, hr = c.host.fetch()
    for got, exp, twin, what in ((pair, c.pair, hp, "pair"), (d, c.d, hd, "d"),
                                 (rev, c.rev, hr, "rev")):
        gc.assert_same(got, exp, what)
        gc.assert_same(got, twin, what + " (host twin)")


def check_labels(ctx, c):
    for name, tie in c.ties().items():
        labels = ctx.hitgroups(tie)
        gc.assert_same(labels, c.labels(tie), f"labels, tie = {name}")
        gc.assert_same(labels, lib.hitgroups_host(c.host, tie), f"labels, tie = {name} (host twin)")


@pytest.mark.parametrize("layout,n", gc.scale_cases())
def test_pairhits_at_scale(ctx, layout, n):
    c = gc.scale_case(layout, n)
    ctx.load(c.packed)
    run_and_check(ctx, c)


@pytest.mark.parametrize("layout", ["mixed", "one_target", "block_stripes"])
def test_hitgroups_at_scale(ctx, layout):
    c = gc.scale_case(layout, gc.SCALE_TOP)
    ctx.load(c.packed)
    run_and_check(ctx, c)
    check_labels(ctx, c)
    assert ctx.hitgroups_stats()["compact"] > 0
    check_fetch(ctx, c)            # the edge compaction has not disturbed the hits


def test_chunked_launches(ctx, monkeypatch):
    """Launches of 50,000 pairs, a multiple of neither 256 nor 64: the retry bitmap counts from
    the launch's first pair, and blocks and launches end at different pairs."""
    c = gc.scale_case("mixed", gc.SCALE_TOP)
    assert c.n > 2 * 50000 and 50000 % 64 and 50000 % 256
    ctx.load(c.packed)
    monkeypatch.setenv("DMX_PD_CHUNK", "50000")
    run_and_check(ctx, c)
    check_labels(ctx, c)
    monkeypatch.delenv("DMX_PD_CHUNK")


def test_fetch_without_room_is_refused(ctx):
    c = gc.scale_case("mixed", gc.SCALE_TOP)
    ctx.load(c.packed)
    _, n_hits = ctx.pairhits(*c.args())
    assert n_hits == c.n_hits > 1
    L = lib.load()
    pair, d = np.zeros(n_hits, dtype=np.uint32), np.zeros(n_hits, dtype=np.uint32)
    rev = np.zeros(n_hits, dtype=np.uint8)
    n = ctypes.c_size_t(0)
    rc = L.dmx_pairhits_fetch(ctx._h, pair.ctypes.data, d.ctypes.data, rev.ctypes.data,
                              n_hits - 1, ctypes.byref(n))
    assert rc == -1 and n.value == n_hits      # refused, and the room needed is reported
    assert not pair.any() and not d.any() and not rev.any()
    rc = L.dmx_pairhits_fetch(ctx._h, pair.ctypes.data, d.ctypes.data, rev.ctypes.data,
                              n_hits, ctypes.byref(n))
    assert rc == 0 and n.value == n_hits
    gc.assert_same(pair, c.pair, "pair")
    gc.assert_same(d, c.d, "d")
    gc.assert_same(rev, c.rev, "rev")


def test_a_second_list_owes_nothing_to_the_first(ctx):
    """The first list has more pairs and more hits than the second, so stale block offsets or
    selected hits would show; then a list of as many pairs and no hit at all."""
    first = gc.scale_case("all_forward", gc.SCALE_TOP)
    ctx.load(first.packed)
    run_and_check(ctx, first)
    check_labels(ctx, first)
    for layout, n in (("mixed", 16385), ("none", gc.SCALE_TOP), ("every_257th", gc.SCALE_TOP)):
        second = gc.scale_case(layout, n)
        assert second.n_hits < first.n_hits
        run_and_check(ctx, second)
        check_labels(ctx, second)
