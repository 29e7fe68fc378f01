"""Operand tables on the GPU (include/dmx.h dmx_set_operands, dmx_result_operands; DESIGN.md
§3.18).  The oracle in every case is the existing host twin on the operands' sequences repacked
with dmx_pack: "the results are those the same call returns on a batch whose reads are the
operands' sequences"."""
import functools

import numpy as np
import pytest

import operands_cases as oc
import rowassign_cases as rac
import views_cases as vc
from dmx import lib

pytestmark = pytest.mark.gpu
SEED = 31802
NONE = lib.LG_NONE


@pytest.fixture(scope="module")
def ctx():
    with lib.Context(0) as c:
        yield c


def _load(ctx, reads, table):
    ctx.load(oc.pack(reads))
    ctx.set_operands(*table)
    return oc.pack(oc.extract(reads, table))   # the repacked batch of the oracle


# ---- geometry: dmx_pairdist ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", [lib.PD_NW, lib.PD_HW])
@pytest.mark.parametrize("capped", [False, True])
def test_pairdist_on_operands(ctx, mode, capped):
    reads, tab, pairs = oc.geometry()
    rep = _load(ctx, reads, tab)
    rng = np.random.default_rng([SEED, 2, mode, capped])
    q = np.concatenate([pairs[:, 0], pairs[:, 1]])
    t = np.concatenate([pairs[:, 1], pairs[:, 0]])
    flags = rng.integers(0, 2, size=len(q)).astype(np.uint8)
    caps = rng.integers(0, 40, size=len(q)).astype(np.uint32) if capped else None
    exp = lib.pairdist_host(rep, q, t, mode, flags, caps, n_threads=8)
    got = ctx.pairdist(q, t, mode, flags, caps)
    np.testing.assert_array_equal(got, exp)
    # the trap is armed: whole reads (operands and their flanks) give other distances
    if not capped:
        ctx.clear_operands()
        whole = ctx.pairdist(tab[0][q], tab[0][t], mode, flags)
        assert (whole != exp).mean() > 0.25
        ctx.set_operands(*tab)


# ---- dmx_pairhits and what reads its outcomes ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def hit_bin():
    """40 operands over 12 reads: three families of near copies on mixed strands.  Family 2's
    members are stored so that a pair's oriented sequences are each other's reverse complement:
    their only hit is the reverse retry."""
    rng = np.random.default_rng([SEED, 3])
    fam = [oc.rand_seq(rng, L) for L in (150, 180, 210)]
    reads = [""] * 12
    ops, famof = [], []
    for k in range(40):
        f = k % 3
        s = list(fam[f])
        for i in range(len(s)):
            if rng.random() < 0.04:
                s[i] = "ACGT"[int(rng.integers(4))]
        s = "".join(s)
        strand = int(rng.integers(2))
        if f == 2 and k % 2:   # the oriented sequence is the family's reverse complement
            s = oc.revcomp(s)
        mem = oc.revcomp(s) if strand else s
        r = k % 12
        a = len(reads[r]) + 3
        reads[r] += "ACG" + mem
        ops.append((r, a, a + len(mem), strand))
        famof.append(f)
    pairs = [(i, j) for i in range(40) for j in range(i + 1, 40)]
    return reads, oc.table_arrays(ops), np.array(pairs, np.uint32), np.array(famof)


def _hit_caps(ln, t):
    from dmx import sorter
    ch = np.array([sorter.identity_cap(int(ln[x]), 0.85) for x in t], np.int32)
    cf = np.array([sorter.identity_cap(int(ln[x]), 0.5) for x in t], np.int32)
    return ch, cf


def test_pairhits_family_on_operands(ctx):
    reads, tab, pairs, fam = hit_bin()
    rep = _load(ctx, reads, tab)
    n = len(tab[0])
    assert n == 40 and len(reads) == 12
    ln = (tab[2] - tab[1]).astype(int)
    q, t = pairs[:, 0].copy(), pairs[:, 1].copy()
    ch, cf = _hit_caps(ln, t)
    hh = lib.pairhits_host(rep, q, t, ch, cf, n_threads=8)
    best, nh = ctx.pairhits(q, t, ch, cf)
    assert best.shape == (40,) and nh == int((hh.outcome != NONE).sum()) > 40
    np.testing.assert_array_equal(best, hh.best)
    got, exp = ctx.pairhits_fetch(), hh.fetch()
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    # mixed strands whose only hit is the reverse retry
    rev_pairs = exp[0][exp[2] == 1]
    assert len(rev_pairs) and (tab[3][q[rev_pairs]] != tab[3][t[rev_pairs]]).any() \
        and (tab[3][q[rev_pairs]] == tab[3][t[rev_pairs]]).any()
    tie = np.where(hh.best == NONE, 0, hh.best + 2).astype(np.uint32)
    np.testing.assert_array_equal(ctx.hitgroups(tie), lib.hitgroups_host(hh, tie))
    # dmx_hithist: a row of classes per operand
    width = int(ch.max()) + 1
    bin_off = (np.arange(n) * width).astype(np.uint32)
    bins = (np.arange(n * width) % 7).astype(np.uint16)
    np.testing.assert_array_equal(ctx.hithist(bin_off, bins, 7), lib.hithist_host(hh, bin_off, bins, 7))
    label = np.where(np.arange(n) % 5 == 0, NONE, fam).astype(np.uint32)
    cap2 = np.full(n, 12, np.int32)
    for g, e in zip(ctx.pairhits_cross(label, cap2), lib.pairhits_cross_host(hh, label, cap2)):
        np.testing.assert_array_equal(g, e)
    tie2 = np.full(n, 10, np.uint32)
    xa, xb = [40, 41], [0, 40]
    np.testing.assert_array_equal(ctx.hitgroups_within(tie2, label, xa, xb, n_nodes=42),
                                  lib.hitgroups_within_host(hh, tie2, label, xa, xb, n_nodes=42))


# ---- dmx_groupalign(_strands) -------------------------------------------------------------------

def test_groupalign_on_operands(ctx):
    reads, tab, _, fam = hit_bin()
    rep = _load(ctx, reads, tab)
    strings = oc.extract(reads, tab)
    groups = [[int(x) for x in np.flatnonzero(fam == f)[:4]] for f in range(3)]
    seeds = [strings[g[0]] for g in groups]
    strands = [[0, 1, 0, 1], [1, 1, 0, 0], [0, 0, 1, 0]]
    assert len({int(tab[3][m]) for g in groups for m in g}) == 2
    exp = lib.groupalign_host(rep, seeds, groups, paths=True, strands=strands)
    got = ctx.groupalign(seeds, groups, paths=True, strands=strands)
    for k in ("col_off", "mask", "count", "first", "dist", "op_off", "ops"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
    # dmx_groupalign itself: strand-1 members go through the strands launch ...
    exp = lib.groupalign_host(rep, seeds, groups)
    got = ctx.groupalign(seeds, groups)
    for k in ("col_off", "mask", "count", "first", "dist"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
    # ... and a group whose members are all on strand 0 is served by the plain one
    g0 = [int(x) for x in np.flatnonzero((fam == 0) & (tab[3] == 0))[:4]]
    assert len(g0) >= 2
    exp = lib.groupalign_host(rep, [strings[g0[0]]], [g0])
    got = ctx.groupalign([strings[g0[0]]], [g0])
    for k in ("col_off", "mask", "count", "first", "dist"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)


# ---- dmx_rowdist, dmx_rowassign -----------------------------------------------------------------

def _rows(strings, fam, rng):
    """Per family a consensus-like row with IUPAC and gap columns, and its reverse complement."""
    rows = []
    for f in range(3):
        s = list(strings[int(np.flatnonzero(fam == f)[0])])
        for i in range(5, len(s), 23):
            s[i] = "RYMKSW"[int(rng.integers(6))]
        for i in range(11, len(s), 41):
            s.insert(i, "-")
        m = lib.mask_row("".join(s))
        rows.extend([m, lib.mask_rc(m)])
    return rows


def test_rowdist_on_operands(ctx):
    reads, tab, _, fam = hit_bin()
    rep = _load(ctx, reads, tab)
    rows = _rows(oc.extract(reads, tab), fam, np.random.default_rng([SEED, 5]))
    q = np.repeat(np.arange(40, dtype=np.uint32), len(rows))
    r = np.tile(np.arange(len(rows), dtype=np.uint32), 40)
    assert (tab[3][q] == 1).any() and (tab[3][q] == 0).any()
    for caps in (None, np.full(len(q), 25, np.uint32)):
        np.testing.assert_array_equal(ctx.rowdist(rows, q, r, caps),
                                      lib.rowdist_host(rep, rows, q, r, caps, n_threads=8))


def test_rowassign_on_operands(ctx):
    reads, tab, _, fam = hit_bin()
    rep = _load(ctx, reads, tab)
    strings = oc.extract(reads, tab)
    rows = _rows(strings, fam, np.random.default_rng([SEED, 6]))[::2]   # forward rows only
    ln = [len(s) for s in strings] + [len(x) for x in rows]
    cap_hit, cap_half, bin_off, bins = rac.tables(ln)
    sel = np.arange(40, dtype=np.uint32)[::-1].copy()
    exp = lib.rowassign_host(rep, rows, sel, cap_hit, cap_half, bin_off, bins, n_threads=8)
    got = ctx.rowassign(rows, sel, cap_hit, cap_half, bin_off, bins)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    rev = (exp[1] != NONE) & ((exp[1] & lib.LG_REV) != 0)
    assert rev.any() and (tab[3][sel][rev] == 1).any() and (tab[3][sel][rev] == 0).any()
    assert ((exp[1] != NONE) & ~rev & (tab[3][sel] == 1)).any()


# ---- the same calls on the trapped geometry -----------------------------------------------------
# Edge lengths (1, 63 .. 129, 4200), every start % 32, strand-1 operands of len % 64 in {0, 1, 63},
# N bases and batch edges: where the host folds a strand into pair flags (pairhits), into the
# strands launch (groupalign) or into which copy of a row is read (rowdist, rowassign).

def _both_ways(pairs):
    return (np.concatenate([pairs[:, 0], pairs[:, 1]]).astype(np.uint32),
            np.concatenate([pairs[:, 1], pairs[:, 0]]).astype(np.uint32))


def geo_hit_case():
    """The geometry's pairs both ways round with _hit_caps' caps."""
    reads, tab, pairs = oc.geometry()
    q, t = _both_ways(pairs)
    ln = (tab[2] - tab[1]).astype(int)
    ch, cf = _hit_caps(ln, t)
    return q, t, ch, cf


def test_pairhits_on_the_geometry(ctx):
    reads, tab, pairs = oc.geometry()
    rep = _load(ctx, reads, tab)
    n = len(tab[0])
    ln, st = (tab[2] - tab[1]).astype(int), tab[3]
    q, t, ch, cf = geo_hit_case()
    hh = lib.pairhits_host(rep, q, t, ch, cf, n_threads=8)
    best, nh = ctx.pairhits(q, t, ch, cf)
    assert best.shape == (n,) and nh == int((hh.outcome != NONE).sum()) > len(pairs)
    np.testing.assert_array_equal(best, hh.best)
    got, exp = ctx.pairhits_fetch(), hh.fetch()
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    hit = exp[0]
    for L in (1, 63, 64, 65, 4200):   # hits between operands of every edge length
        assert ((ln[q[hit]] == L) & (ln[t[hit]] == L)).any(), L
    assert {(int(a), int(b)) for a, b in zip(st[q[hit]], st[t[hit]])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the reverse retry ran for pairs of equal and of mixed strands: no forward hit, df > cap_half
    df = lib.pairdist_host(rep, q, t, lib.PD_NW, n_threads=8).astype(np.int64)
    retried = (df > ch) & (df > cf) & (ch >= 0)
    assert (retried & (st[q] != st[t])).any() and (retried & (st[q] == st[t])).any()
    tie = np.where(hh.best == NONE, 0, hh.best + 2).astype(np.uint32)
    np.testing.assert_array_equal(ctx.hitgroups(tie), lib.hitgroups_host(hh, tie))
    # the trap is armed: on whole reads the flanks' copies change the outcomes
    ctx.clear_operands()
    ctx.pairhits(tab[0][q], tab[0][t], ch, cf)
    whole = ctx.pairhits_fetch()
    assert len(whole[0]) != len(hit) or (whole[1] != exp[1]).mean() > 0.25
    ctx.set_operands(*tab)


def geo_groups():
    """One group per geometry pair (seed: the first operand's sequence), then groups of three
    operands whose lengths straddle 64 and 128, and per member a requested strand such that every
    (member's strand, requested strand) occurs."""
    reads, tab, pairs = oc.geometry()
    strings = oc.extract(reads, tab)
    ln, st = (tab[2] - tab[1]).astype(int), tab[3]
    groups = [[int(a), int(b)] for a, b in pairs]
    for lens3 in ((63, 64, 65), (127, 128, 129), (65, 63, 64), (129, 127, 128)):
        for s in (0, 1):
            groups.append([int(np.flatnonzero((ln == L) & (st == (s ^ (i & 1))))[i])
                           for i, L in enumerate(lens3)])
    seeds = [strings[g[0]] for g in groups]
    strands = [[(k + i) % 2 for i in range(len(g))] for k, g in enumerate(groups)]
    return groups, seeds, strands


def test_groupalign_on_the_geometry(ctx):
    reads, tab, pairs = oc.geometry()
    rep = _load(ctx, reads, tab)
    groups, seeds, strands = geo_groups()
    st = tab[3]
    combos = {(int(st[m]), s) for g, ss in zip(groups, strands) for m, s in zip(g, ss)}
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    ln = (tab[2] - tab[1]).astype(int)
    assert {1, 4200} <= {int(ln[m]) for g in groups for m in g}
    exp = lib.groupalign_host(rep, seeds, groups, paths=True, strands=strands, n_threads=8)
    got = ctx.groupalign(seeds, groups, paths=True, strands=strands)
    for k in ("col_off", "mask", "count", "first", "dist", "op_off", "ops"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
    # dmx_groupalign itself: the table's strands alone decide which launch serves a member
    exp = lib.groupalign_host(rep, seeds, groups, n_threads=8)
    got = ctx.groupalign(seeds, groups)
    for k in ("col_off", "mask", "count", "first", "dist"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
    # near copies on their own strands: most members lie close to their seed
    sizes = np.array([len(g) for g in groups])
    seedlen = np.repeat([len(s) for s in seeds], sizes)
    assert (exp["dist"] <= 0.25 * seedlen + 2).mean() > 0.5
    ctx.clear_operands()
    whole = ctx.groupalign(seeds, [[int(tab[0][m]) for m in g] for g in groups])
    assert (whole["dist"] != exp["dist"]).mean() > 0.25
    ctx.set_operands(*tab)


def geo_rows(rng, flip=False):
    """Per geometry operand a consensus-like row of its sequence (IUPAC and gap columns from 63 nt
    up, as _rows writes them).  flip: every second row is written reverse-complemented."""
    reads, tab, _ = oc.geometry()
    rows = []
    for k, s in enumerate(oc.extract(reads, tab)):
        s = list(s)
        if len(s) >= 63:
            for i in range(5, len(s), 23):
                s[i] = "RYMKSW"[int(rng.integers(6))]
            for i in range(11, len(s), 41):
                s.insert(i, "-")
        m = lib.mask_row("".join(s))
        rows.append(lib.mask_rc(m) if flip and k % 2 else m)
    return rows


def test_rowdist_on_the_geometry(ctx):
    reads, tab, pairs = oc.geometry()
    rep = _load(ctx, reads, tab)
    n = len(tab[0])
    fwd = geo_rows(np.random.default_rng([SEED, 9]))
    rows = [x for m in fwd for x in (m, lib.mask_rc(m))]   # row 2 k and its reverse complement
    a, b = _both_ways(pairs)
    q = np.concatenate([a, a, a]).astype(np.uint32)
    r = np.concatenate([2 * b, 2 * b + 1, 2 * a]).astype(np.uint32)
    assert set(q.tolist()) == set(range(n))               # every operand is a query
    for caps in (None, np.full(len(q), 7, np.uint32)):
        exp = lib.rowdist_host(rep, rows, q, r, caps, n_threads=8)
        np.testing.assert_array_equal(ctx.rowdist(rows, q, r, caps), exp)
    exp = lib.rowdist_host(rep, rows, q, r, None, n_threads=8)
    own = exp[2 * len(a):]
    ln = (tab[2] - tab[1]).astype(int)
    # an operand against its own row: the gap columns and the IUPAC columns that lost its base
    assert (own <= ln[a] // 41 + ln[a] // 23 + 2).all() and (own[ln[a] >= 63] > 0).all()
    # the trap is armed: a table that is ignored reads whole reads, flanks and all
    ctx.clear_operands()
    whole = ctx.rowdist(rows, tab[0][q], r)
    assert (whole != exp).mean() > 0.25
    ctx.set_operands(*tab)


def test_rowassign_on_the_geometry(ctx):
    reads, tab, pairs = oc.geometry()
    rep = _load(ctx, reads, tab)
    n = len(tab[0])
    strings = oc.extract(reads, tab)
    every = geo_rows(np.random.default_rng([SEED, 10]), flip=True)
    rows = [every[int(a)] for a in pairs[:, 0]]            # forward rows only: the call turns them
    ln = [len(s) for s in strings] + [len(x) for x in rows]
    cap_hit, cap_half, bin_off, bins = rac.tables(ln)
    sel = np.arange(n, dtype=np.uint32)[::-1].copy()
    exp = lib.rowassign_host(rep, rows, sel, cap_hit, cap_half, bin_off, bins, n_threads=8)
    got = ctx.rowassign(rows, sel, cap_hit, cap_half, bin_off, bins)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    st = tab[3][sel]
    has = exp[0] != NONE
    rev = has & ((exp[1] & lib.LG_REV) != 0)
    assert rev.any() and (st[rev] == 1).any() and (st[rev] == 0).any()
    assert (has & ~rev & (st == 1)).any() and (has & ~rev & (st == 0)).any()
    sl = np.array([len(s) for s in strings])[sel]
    for L in (1, 63, 64, 65, 4200):
        assert (has & (sl == L)).any(), L
    ctx.clear_operands()
    whole = ctx.rowassign(rows, tab[0][sel], *rac.tables(
        [len(x) for x in reads] + [len(x) for x in rows]))
    assert (whole[0] != exp[0]).mean() > 0.25
    ctx.set_operands(*tab)


# ---- dmx_result_operands ------------------------------------------------------------------------

BLOCK = 256  # the builder's tile (csrc/dmx_operands.hip kOpBlock)


@functools.lru_cache(maxsize=None)
def demux_case():
    """3 x BLOCK + 1 reads for the benchmark's two-round panels; the last read alone carries the
    last SP5 adapter, so only the last block feeds its bins."""
    rng = np.random.default_rng([SEED, 7])
    sp5, sp27 = vc.bench_panels()
    reads = vc.demux_reads(rng, 3 * BLOCK, sp5[:-1], sp27, lo=200, hi=420)
    tail = oc.rand_seq(rng, 20) + sp5[-1] + oc.rand_seq(rng, 180) + sp27[0] + oc.rand_seq(rng, 9)
    return reads + [tail], sp5, sp27


def _set_bench(ctx, sp5, sp27):
    ctx.set_panel(0, sp5, lib.DMX_FRONT | lib.DMX_RC, 0.1, 3)
    ctx.set_panel(1, sp27, lib.DMX_BACK | lib.DMX_RC, 0.1, 3)
    ctx.set_mode(lib.MODE_TWO_ROUND)


def _builder_check(ctx, reads, sp5, sp27, views, keep, min_len):
    res = ctx.fetch()
    lens = [len(r) for r in reads]
    exp, efirst = lib.result_operands_host(res, lens, lib.MODE_TWO_ROUND, [oc.F] * len(sp5),
                                           [oc.B] * len(sp27), views=views, keep=keep,
                                           min_len=min_len)
    first = ctx.result_operands(keep, min_len)
    np.testing.assert_array_equal(first, efirst)
    got = ctx.operands()
    for g, e, name in zip(got, exp, ("read", "start", "stop", "strand")):
        np.testing.assert_array_equal(g, e, err_msg=name)
    return res, got, first


def test_result_operands_whole_reads(ctx):
    reads, sp5, sp27 = demux_case()
    _set_bench(ctx, sp5, sp27)
    ctx.load(oc.pack(reads))
    ctx.exec_checked()
    res, tab, first = _builder_check(ctx, reads, sp5, sp27, None, None, 50)
    counts = np.diff(first.astype(np.int64))
    a1 = len(sp27) + 1
    assert (counts == 0).any() and counts.sum() > BLOCK
    # a bin that only the last block feeds: (last SP5, SP27 0), the last read's
    lastbin = len(sp5) * a1 + 1
    bins = (res["bin1"].astype(int) + 1) * a1 + res["bin2"].astype(int) + 1
    assert bins[-1] == lastbin and not (bins[:-1] == lastbin).any()
    assert counts[lastbin] == 1 and tab[0][int(first[lastbin])] == 3 * BLOCK
    # the script's post-filter as keep: no unknown, not the last SP27 adapter
    keep = np.ones(len(counts), np.uint8).reshape(len(sp5) + 1, a1)
    keep[0, :] = 0
    keep[:, 0] = 0
    keep[:, -1:] = 0
    _builder_check(ctx, reads, sp5, sp27, None, keep.reshape(-1), 50)
    # one bin's operands through dmx_pairdist against the host twin on its rendered records
    _, tab, first = _builder_check(ctx, reads, sp5, sp27, None, None, 50)
    b = int(np.argmax(counts))
    lo, hi = int(first[b]), int(first[b + 1])
    assert hi - lo >= 3
    rep = oc.pack(oc.extract(reads, tuple(x[lo:hi] for x in tab)))
    idx = np.arange(hi - lo, dtype=np.uint32)
    q, t = np.repeat(idx, len(idx)), np.tile(idx, len(idx))
    np.testing.assert_array_equal(ctx.pairdist(q + lo, t + lo, lib.PD_NW),
                                  lib.pairdist_host(rep, q, t, lib.PD_NW, n_threads=8))


def test_result_operands_of_a_view_run(ctx):
    reads, sp5, sp27 = demux_case()
    rng = np.random.default_rng([SEED, 8])
    _set_bench(ctx, sp5, sp27)
    ctx.load(oc.pack(reads))
    n = 3 * BLOCK + 1
    rd = rng.integers(0, len(reads), size=n)
    rd[:40] = rd[40:80]   # repeated views
    L = np.array([len(reads[int(r)]) for r in rd])
    a = rng.integers(0, 15, size=n)
    b = L - rng.integers(0, 15, size=n)
    views = (rd.astype(np.uint32), a.astype(np.int32), b.astype(np.int32),
             rng.integers(0, 2, size=n).astype(np.uint8))
    ctx.set_views(*views)
    ctx.exec_checked()
    _, tab, first = _builder_check(ctx, reads, sp5, sp27, views, None, 50)
    assert len(tab[0]) > BLOCK and set(tab[3].tolist()) == {0, 1}
    # a list changed since the exec is refused, and the table is independent of it otherwise
    ctx.clear_views()
    with pytest.raises(lib.DmxError, match=r"\(-5\)"):
        ctx.result_operands()


# ---- state --------------------------------------------------------------------------------------

def test_state(ctx):
    reads, tab, pairs, _ = hit_bin()
    _load(ctx, reads, tab)
    ln = (tab[2] - tab[1]).astype(int)
    q, t = pairs[:50, 0].copy(), pairs[:50, 1].copy()
    ch, cf = _hit_caps(ln, t)
    ctx.pairhits(q, t, ch, cf)
    ctx.clear_operands()
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):   # the outcomes died with the table
        ctx.hitgroups(np.zeros(len(reads), np.uint32))
    ctx.set_operands(*tab)
    with pytest.raises(lib.DmxError, match=r"\(-4\)"):
        ctx.pairalign([0], [1])
    # a refused set leaves the old table fetchable and unchanged
    bad = [x.copy() for x in tab]
    bad[2][7] = 10 ** 6
    with pytest.raises(lib.DmxError, match="operand 7"):
        ctx.set_operands(*bad)
    for g, e in zip(ctx.operands(), tab):
        np.testing.assert_array_equal(g, e)
    np.testing.assert_array_equal(ctx.pairdist([0], [3]),
                                  lib.pairdist_host(oc.pack(oc.extract(reads, tab)), [0], [3]))
    # dmx_load drops the table: indices name reads again
    ctx.load(oc.pack(reads))
    assert all(len(x) == 0 for x in ctx.operands())
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.pairdist([20], [0])   # 12 reads
    np.testing.assert_array_equal(ctx.pairdist([0], [3]), lib.pairdist_host(oc.pack(reads), [0], [3]))
