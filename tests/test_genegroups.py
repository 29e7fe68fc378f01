"""Gene groups on the GPU (csrc/dmx_groups.hip, dmx_pairhits in csrc/dmx_pairdist.hip; DESIGN.md
§8i) against the host twins, themselves pinned by test_genegroups_host.py to a literal restatement
of amplicon_sorter.py update_list (:983-1034) and merge_groups (:1058-1087)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import genegroups_cases as gc
import pairdist_cases as pc
from dmx import lib, sorter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")


@pytest.mark.parametrize("name", sorted(gc.small_graphs()))
def test_edgegroups_small_graphs(ctx, name):
    a, b, n = gc.small_graphs()[name]
    np.testing.assert_array_equal(ctx.edgegroups(a, b, n), lib.edgegroups_host(a, b, n))


@pytest.mark.parametrize("name", sorted(gc.big_graphs()))
def test_edgegroups_big_graphs(ctx, name):
    a, b, n = gc.big_graphs()[name]
    got = ctx.edgegroups(a, b, n)
    np.testing.assert_array_equal(got, lib.edgegroups_host(a, b, n))
    st = ctx.hitgroups_stats()
    assert st["rounds"] >= 2 and st["components"] > 0
    if name.startswith("path"):
        assert (got == 0).all()


@pytest.fixture(scope="module")
def bin_host():
    reads, _ = gc.gene_bin()
    plan = gc.bin_plan(reads)
    p, ln, q, t, cap_hit, cap_half = plan
    st = lib.pairhits_host(p, q, t, cap_hit, cap_half, n_threads=16)
    return reads, plan, st


def check_hits(ctx, q, t, cap_hit, cap_half, host, n_reads):
    best, n_hits = ctx.pairhits(q, t, cap_hit, cap_half)
    pair, d, rev = ctx.pairhits_fetch()
    hp, hd, hr = host.fetch()
    assert n_hits == len(hp)
    np.testing.assert_array_equal(pair, hp)
    np.testing.assert_array_equal(d, hd)
    np.testing.assert_array_equal(rev, hr)
    exp = np.full(n_reads, lib.LG_NONE, dtype=np.uint32)
    np.minimum.at(exp, np.asarray(t)[pair], d)
    np.testing.assert_array_equal(best, exp)
    np.testing.assert_array_equal(best, host.best)
    return pair, d, rev


def test_pairhits_on_the_bin(ctx, bin_host, monkeypatch):
    reads, (p, ln, q, t, cap_hit, cap_half), host = bin_host
    ctx.load(p)
    pair, d, rev = check_hits(ctx, q, t, cap_hit, cap_half, host, len(reads))
    assert rev.any() and not rev.all() and 0 < len(pair) < len(q)
    assert ctx.hitgroups_stats()["forward"] > 0
    # the same list in at least four launches (and the retries in launches of their own)
    assert len(q) >= 4 * 150
    monkeypatch.setenv("DMX_PD_CHUNK", "150")
    check_hits(ctx, q, t, cap_hit, cap_half, host, len(reads))
    monkeypatch.delenv("DMX_PD_CHUNK")


def test_pairhits_boundary_lengths(ctx):
    """One word, 64 G +- 1 for a few group sizes G, and a pair of more than 4,096 rows (two
    stripes); every third target reverse-complemented, so forward hits, reverse hits and
    misses all occur."""
    rng = np.random.default_rng(22)
    reads = []
    for k, m in enumerate([20, 63, 64, 65, 127, 128, 129, 319, 320, 321, 1023, 1024, 1025, 4200]):
        a = pc.rand_seq(rng, m)
        b = pc.mutate(rng, a, 0.08 if k % 2 else 0.3)
        reads += [a, pc.revcomp(b) if k % 3 == 1 else b]
    p = pc.pack_reads(reads)
    q = np.arange(0, len(reads), 2, dtype=np.uint32)
    t = q + 1
    lt = p.lengths[t]
    cap_hit = np.array([sorter.identity_cap(int(L), 0.8) for L in lt], dtype=np.int32)
    cap_half = np.array([sorter.identity_cap(int(L), 0.5) for L in lt], dtype=np.int32)
    host = lib.pairhits_host(p, q, t, cap_hit, cap_half, n_threads=16)
    ctx.load(p)
    pair, d, rev = check_hits(ctx, q, t, cap_hit, cap_half, host, len(reads))
    assert rev.any() and not rev.all() and len(pair) < len(q)
    # the other way round: the mutated copy is the query
    host = lib.pairhits_host(p, t, q, cap_hit, cap_half, n_threads=16)
    check_hits(ctx, t, q, cap_hit, cap_half, host, len(reads))


def test_hitgroups_and_gene_groups(ctx, bin_host):
    reads, (p, ln, q, t, cap_hit, cap_half), host = bin_host
    _, _, _, groups = gc.gene_bin_oracle()
    ctx.load(p)
    best, _ = ctx.pairhits(q, t, cap_hit, cap_half)
    tie = np.array([sorter.identity_tie(int(b), int(L)) if b != lib.LG_NONE else lib.LG_NONE
                    for b, L in zip(best, ln)], dtype=np.uint32)
    assert (tie[best != lib.LG_NONE] > best[best != lib.LG_NONE]).any()   # a rounding tie
    labels = ctx.hitgroups(tie)
    np.testing.assert_array_equal(labels, lib.hitgroups_host(host, tie))
    assert gc.groups_of(labels) == sorted(groups)
    assert ctx.hitgroups_stats()["compact"] > 0
    # tie = best: the rounding ties are dropped, so some link goes
    np.testing.assert_array_equal(ctx.hitgroups(best), lib.hitgroups_host(host, best))
    # the whole path, twice on one context: the state of the first call does not leak
    for _ in range(2):
        got = sorter.gene_groups(ctx, reads, minlength=0)
        assert [g.tolist() for g in got] == groups
    assert [g.tolist() for g in sorter.gene_groups(None, reads, minlength=0)] == groups
    assert sorter.gene_groups(ctx, gc.quiet_bin(), minlength=0) == []


def test_refusals(ctx):
    reads = [b"ACGT" * 20, b"ACGT" * 19 + b"AAAA", b"", b"ACGT" * 10]
    ctx.load(pc.pack_reads(reads))
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.hitgroups(np.zeros(4, dtype=np.uint32))       # no pairhits since the load
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.pairhits_fetch()
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.edgegroups([0, 5], [1, 2], 5)                 # an endpoint out of range
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.pairhits([0], [4], [5], [5])                  # a read outside the batch
    with pytest.raises(lib.DmxError, match=r"\(-4\)"):
        ctx.pairhits([0], [2], [5], [5])                  # a zero-length read
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.pairhits([0], [1], [-2], [5])
    # caps of -1: nothing hits, nothing is retried; the state is valid and empty
    best, n = ctx.pairhits([0, 0], [1, 3], [-1, -1], [-1, 30])
    assert n == 0 and (best == lib.LG_NONE).all()
    assert (ctx.hitgroups(best) == lib.LG_NONE).all() and len(ctx.pairhits_fetch()[0]) == 0
    best, n = ctx.pairhits([0], [1], [16], [40])
    assert n == 1 and best.tolist() == [lib.LG_NONE, 3, lib.LG_NONE, lib.LG_NONE]
    assert ctx.hitgroups(best).tolist() == [0, 0, lib.LG_NONE, lib.LG_NONE]
    ctx.load(pc.pack_reads(reads))                        # a new batch: the outcomes are stale
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.hitgroups(best)


def test_cli_writes_the_groups(bin_host, tmp_path):
    reads, _, _ = bin_host
    _, _, _, groups = gc.gene_bin_oracle()
    src = tmp_path / "bin.fastq"
    src.write_text("".join(f"@read{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    out = tmp_path / "groups.txt"
    r = subprocess.run([sys.executable, os.path.join(PKG, "bin", "dmx-similarity"), "-i", str(src),
                        "--groups", str(out), "-min", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_text() == "".join(" ".join(map(str, g)) + "\n" for g in groups)
