"""dmx_hithist, dmx_pairhits_cross and dmx_hitgroups_within on the GPU (csrc/dmx_groups.hip;
DESIGN.md §8k) against the host twins and numpy: on the species bin, and on the pair lists of
genegroups_cases.scale_case at the sizes where the compaction's waves, blocks and tiles change
(one block of 256 pairs and its neighbours; 65 blocks; 257 blocks; 514 blocks)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import genegroups_cases as gc
import species_cases as sc
from dmx import lib, sorter
from dmx.lib import DmxError

pytestmark = pytest.mark.gpu

NONE = lib.LG_NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")
SIZES = (255, 256, 257, 16385, 65537, 131329)
LAYOUTS = ("all_forward", "none", "every_257th", "last_only")


def bin_state(ctx):
    """The bin loaded and its pairhits run; the plan and the host twin's state."""
    p, ln, q, t, cap_sg, cap_half, hits = sc.species_plan()
    ctx.load(p)
    best, n_hits = ctx.pairhits(q, t, cap_sg, cap_half)
    gc.assert_same(best, hits.best, "best")
    return ln, q, t, cap_sg, hits


def test_the_bin_against_the_twins(ctx):
    reads, role, groups = sc.species_bin()
    ln, q, t, cap_sg, hits = bin_state(ctx)
    bin_off, bins = sorter._identity_table(ln, t, cap_sg)
    gc.assert_same(ctx.hithist(bin_off, bins, sorter.N_CLASSES),
                   lib.hithist_host(hits, bin_off, bins, sorter.N_CLASSES), "hist")
    assert ctx.hitgroups_stats()["hist"] > 0
    label = np.full(len(ln), NONE, dtype=np.uint32)
    for k, g in enumerate(groups):
        label[g] = k
    cap2 = np.array([sorter.identity_cap(int(L), sc.SSG / 100) for L in ln], dtype=np.int32)
    for got, exp, what in zip(ctx.pairhits_cross(label, cap2),
                              lib.pairhits_cross_host(hits, label, cap2), ("pair", "d", "rev")):
        gc.assert_same(got, exp, what)
        assert len(exp) > 0
    tie2 = np.where(hits.best.astype(np.int64) <= cap2, hits.best, NONE).astype(np.uint32)
    n = len(ln)
    for xa, xb, nn in (([], [], n), ([0, 3, n + 1], [n, n, 5], n + 2)):
        gc.assert_same(ctx.hitgroups_within(tie2, label, xa, xb, nn),
                       lib.hitgroups_within_host(hits, tie2, label, xa, xb, nn), "labels")
    st = ctx.hitgroups_stats()
    assert st["compact"] > 0 and st["components"] > 0


def test_the_sorter_on_the_bin(ctx):
    reads, role, groups = sc.species_bin()
    exp = sc.species_oracle()[2]
    assert sorter.estimate_ssg(ctx, reads, minlength=0) == sorter.estimate_ssg(None, reads, minlength=0)
    gc.assert_same(sorter.identity_histogram(ctx, reads, minlength=0),
                   sorter.identity_histogram(None, reads, minlength=0), "hist")
    got = sorter.species_groups(ctx, reads, groups, sc.SSG, minlength=0)
    host = sorter.species_groups(None, reads, groups, sc.SSG, minlength=0)
    assert [[m.tolist() for m in sp] for sp in got] == [[m.tolist() for m in sp] for sp in host]
    assert [{frozenset(m.tolist()) for m in sp} for sp in got] == exp


def test_several_launches(ctx, monkeypatch):
    """DMX_PD_CHUNK=150: the bin's pairs run as several launches; same histogram, same groups."""
    reads, role, groups = sc.species_bin()
    assert len(sc.species_plan()[2]) > 3 * 150
    monkeypatch.setenv("DMX_PD_CHUNK", "150")
    hist = sorter.identity_histogram(ctx, reads, minlength=0)
    got = sorter.species_groups(ctx, reads, groups, sc.SSG, minlength=0)
    monkeypatch.delenv("DMX_PD_CHUNK")
    gc.assert_same(hist, sorter.identity_histogram(None, reads, minlength=0), "hist")
    assert [{frozenset(m.tolist()) for m in sp} for sp in got] == sc.species_oracle()[2]


def state_of(c):
    """The host twin's state of a scale case, from its numpy oracle (no DP)."""
    return lib.HostHits(np.ascontiguousarray(c.q, dtype=np.uint32),
                        np.ascontiguousarray(c.t, dtype=np.uint32), c.outcome, c.best, c.n_reads)


def check_hithist(ctx, c, hits):
    rng = np.random.default_rng(c.n)
    top_d = int(c.d.max()) if c.n_hits else 0
    for n_classes, spread in ((sorter.N_CLASSES, 1), (1024, 1024)):
        bin_off, bins = sc.flat_table(c.n_reads, top_d, n_classes, spread, rng)
        exp = (sc.np_hithist(c.t, c.pair, c.d, bin_off, bins, n_classes) if c.n_hits
               else np.zeros(n_classes, dtype=np.uint64))
        got = ctx.hithist(bin_off, bins, n_classes)
        gc.assert_same(got, exp, f"hist, {spread} classes")
        gc.assert_same(got, lib.hithist_host(hits, bin_off, bins, n_classes), "hist (host twin)")
        assert int(got.sum()) == c.n_hits
        if spread == 1:
            assert int(got[n_classes - 1]) == c.n_hits
    if not c.n_hits:
        return
    # the largest table index exactly at n_bins - 1 is read; at n_bins the call refuses
    last = int((bin_off[c.t[c.pair]].astype(np.int64) + c.d).max())
    gc.assert_same(ctx.hithist(bin_off, bins[:last + 1], 1024), exp, "hist, index at n_bins - 1")
    with pytest.raises(DmxError, match="table index"):
        ctx.hithist(bin_off, bins[:last], 1024)
    with pytest.raises(DmxError, match="class"):
        ctx.hithist(bin_off, bins, int(bins[bin_off[c.t[c.pair]] + c.d].max()))
    gc.assert_same(ctx.hithist(bin_off, bins, 1024), exp, "hist after a refused call")


def check_cross(ctx, c, hits):
    r = np.arange(c.n_reads)
    cap2 = np.where(c.best != NONE, c.best.astype(np.int64) + 2, -1).astype(np.int32)
    for name, label in (("alternating", (r % 2).astype(np.uint32)),
                        ("equal", np.zeros(c.n_reads, dtype=np.uint32)),
                        ("none", np.full(c.n_reads, NONE, dtype=np.uint32)),
                        ("some none", np.where(r % 3 == 0, NONE, r % 2).astype(np.uint32))):
        keep = sc.np_cross(c.q, c.t, c.pair, c.d, label, cap2)
        got = ctx.pairhits_cross(label, cap2)
        twin = lib.pairhits_cross_host(hits, label, cap2)
        for g, e, tw, what in zip(got, (c.pair[keep], c.d[keep], c.rev[keep]), twin,
                                  ("pair", "d", "rev")):
            gc.assert_same(g, e, f"{what}, labels {name}")
            gc.assert_same(g, tw, f"{what}, labels {name} (host twin)")
        if name in ("equal", "none"):
            assert not len(got[0])


def check_within(ctx, c, hits):
    n = c.n_reads
    same = np.zeros(n, dtype=np.uint32)
    for name, tie in c.ties().items():
        got = ctx.hitgroups_within(tie, same)
        gc.assert_same(got, ctx.hitgroups(tie), f"within == hitgroups, tie = {name}")
        gc.assert_same(got, c.labels(tie), f"labels, tie = {name}")
    tie = c.ties()["best+1"]
    label = np.where(np.arange(n) % 5 == 0, NONE, np.arange(n) % 2).astype(np.uint32)
    xa, xb, nn = [0, 1, 2, n], [n, n + 1, n + 1, n + 2], n + 4      # clones n .. n + 2; n + 3 idle
    got = ctx.hitgroups_within(tie, label, xa, xb, nn)
    gc.assert_same(got, sc.np_within(c.q, c.t, c.pair, c.d, tie, label, xa, xb, nn), "clones")
    gc.assert_same(got, lib.hitgroups_within_host(hits, tie, label, xa, xb, nn), "clones (host twin)")
    assert got[n + 3] == NONE and got[n] == 0
    gc.assert_same(ctx.hitgroups_within(np.full(n, NONE, dtype=np.uint32), same),
                   np.full(n, NONE, dtype=np.uint32), "tie NONE is no edge")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_at_scale(ctx, layout, n):
    c = gc.scale_case(layout, n)
    hits = state_of(c)
    ctx.load(c.packed)
    best, n_hits = ctx.pairhits(*c.args())
    assert n_hits == c.n_hits
    gc.assert_same(best, c.best, "best")
    check_hithist(ctx, c, hits)
    check_cross(ctx, c, hits)
    check_within(ctx, c, hits)
    # the outcomes, the hits and the gene groups are what they were
    for got, exp, what in zip(ctx.pairhits_fetch(), (c.pair, c.d, c.rev), ("pair", "d", "rev")):
        gc.assert_same(got, exp, what + " afterwards")
    gc.assert_same(ctx.hitgroups(c.best), c.labels(c.best), "hitgroups afterwards")


def test_refusals(ctx):
    c = gc.scale_case("all_forward", 257)
    ctx.load(c.packed)
    n = c.n_reads
    zeros = np.zeros(n, dtype=np.uint32)
    with pytest.raises(DmxError, match="no dmx_pairhits"):
        ctx.hithist(zeros, np.zeros(4, dtype=np.uint16), 4)
    with pytest.raises(DmxError, match="no dmx_pairhits"):
        ctx.pairhits_cross(zeros, np.zeros(n, dtype=np.int32))
    with pytest.raises(DmxError, match="no dmx_pairhits"):
        ctx.hitgroups_within(zeros, zeros)
    ctx.pairhits(*c.args())
    with pytest.raises(DmxError, match="outside"):
        ctx.hitgroups_within(c.best, zeros, [0], [n + 1], n + 1)
    with pytest.raises(DmxError, match="nodes for"):
        ctx.hitgroups_within(c.best, zeros, [], [], n - 1)
    with pytest.raises(DmxError, match="n_classes"):
        ctx.hithist(zeros, np.zeros(4, dtype=np.uint16), 1025)
    gc.assert_same(ctx.hitgroups(c.best), c.labels(c.best), "the context is usable")


def test_cli_writes_the_species_groups(tmp_path):
    reads, _, _ = sc.species_bin()
    src = tmp_path / "bin.fastq"
    src.write_text("".join(f"@read{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    groups = sorter.gene_groups(None, reads, minlength=0)

    def expected(ssg, how):
        sp = sorter.species_groups(None, reads, groups, ssg, minlength=0)
        return f"# ssg {ssg:g} {how}\n" + "".join(
            f"{k}: " + " ".join(map(str, m.tolist())) + "\n" for k, s in enumerate(sp) for m in s)

    for extra, ssg, how in (([], sorter.estimate_ssg(None, reads, minlength=0), "estimated"),
                            (["-ssg", "95"], 95.0, "given")):
        grp, out = tmp_path / "groups.txt", tmp_path / "species.txt"
        r = subprocess.run([sys.executable, os.path.join(PKG, "bin", "dmx-similarity"), "-i",
                            str(src), "--groups", str(grp), "--species-groups", str(out), "-min",
                            "0"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("estimated ssg = " in r.stderr) == (how == "estimated")
        assert out.read_text() == expected(ssg, how)
        assert len(out.read_text().splitlines()) > 2


CHILD = """
import json, sys
sys.path[:0] = [{tests!r}, {pkg!r}]
import numpy as np
import species_cases as sc
from dmx import lib, sorter
reads, role, groups = sc.species_bin()
with lib.Context(0) as c:
    hist = sorter.identity_histogram(c, reads, minlength=0)
    sp = sorter.species_groups(c, reads, groups, sc.SSG, minlength=0)
print(json.dumps({{'lib': lib.LIB_PATH, 'hist': hist.tolist(),
                  'species': [[m.tolist() for m in s] for s in sp]}}))
"""


def test_bounds_build(tmp_path):
    """The bin through the bounds-checked library (the histogram's table access is checked under
    its own buffer kind): no violation, the host's results."""
    reads, role, groups = sc.species_bin()
    script = tmp_path / "run.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=PKG))
    env = dict(os.environ)
    env.pop("DMX_LIBDMX", None)
    env.pop("DMX_PD_CHUNK", None)
    env["DMX_DEBUG_BOUNDS"] = "1"
    res = subprocess.run([sys.executable, str(script)], capture_output=True, text=True,
                         timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["lib"].endswith("libdmx_bounds.so")
    assert out["hist"] == sorter.identity_histogram(None, reads, minlength=0).tolist()
    host = sorter.species_groups(None, reads, groups, sc.SSG, minlength=0)
    assert out["species"] == [[m.tolist() for m in s] for s in host]
