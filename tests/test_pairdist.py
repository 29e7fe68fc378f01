"""dmx_pairdist (csrc/dmx_pairdist.hip) on the GPU against dmx_pairdist_host, itself pinned to a
numpy DP by test_pairdist_host.py; dmx.sorter.similarity and bin/dmx-similarity against a plain
restatement of amplicon_sorter.py:777-808 on the numpy DP and built-in round."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pairdist_cases as pc
from dmx import lib, sorter, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")


def boundary_reads():
    """Pairs (2i, 2i + 1) whose query lengths straddle every boundary of the design: one word,
    the group sizes the library instantiates (64 G - 1, 64 G, 64 G + 1 for each), more than
    one stripe (above 4096 rows), three stripes, ~4200 x 4200, and a 1-nt query on a long
    target.  Targets are mutated copies (or cut / unrelated where the sizes differ on purpose)."""
    rng = np.random.default_rng(21)
    sizes = lib.pairdist_group_sizes()
    assert sizes[-1] == 64
    qlens = {1, 63, 64, 65, 127, 128, 129}
    for g in sizes:
        qlens |= {64 * g - 1, 64 * g, 64 * g + 1}
    reads = []
    for m in sorted(qlens):
        a = pc.rand_seq(rng, m)
        reads += [a, pc.mutate(rng, a, 0.08)]
    a = pc.rand_seq(rng, 4200)
    reads += [a, pc.mutate(rng, a, 0.1)]                 # near 4,200 x 4,200: two stripes
    a = pc.rand_seq(rng, 2 * 4096 + 70)
    reads += [a, pc.mutate(rng, a[3000:3400], 0.05)]     # three stripes, a short target
    a = pc.rand_seq(rng, lib.PD_MAX_LEN)
    reads += [a, pc.mutate(rng, a[:300], 0.05)]          # the longest query: four stripes
    reads += [b"G", pc.rand_seq(rng, 5000)]              # a long target with a 1-nt query
    reads += [pc.rand_seq(rng, 70), pc.rand_seq(rng, 3000)]
    return reads


@pytest.fixture(scope="module")
def boundary():
    reads = boundary_reads()
    p = pc.pack_reads(reads)
    q = np.arange(0, len(reads), 2, dtype=np.uint32)
    t = q + 1
    flags = (np.arange(len(q)) % 3 == 1).astype(np.uint8)
    exp = {m: lib.pairdist_host(p, q, t, m, flags, n_threads=16) for m in (lib.PD_NW, lib.PD_HW)}
    return p, q, t, flags, exp


@pytest.fixture(scope="module")
def random_batch():
    reads, q, t, flags, exp = pc.random_set()
    return pc.pack_reads(reads), q, t, flags, exp


@pytest.mark.parametrize("mode", [lib.PD_NW, lib.PD_HW])
def test_random_pairs_match_the_host_dp(ctx, random_batch, mode):
    p, q, t, flags, exp = random_batch
    host = lib.pairdist_host(p, q, t, mode, flags, n_threads=16)
    np.testing.assert_array_equal(host, exp[mode])
    ctx.load(p)
    got = ctx.pairdist(q, t, mode, flags)
    np.testing.assert_array_equal(got, host)
    assert ctx.pairdist_ms() > 0
    caps, capped = pc.cap_cycle(host)
    np.testing.assert_array_equal(ctx.pairdist(q, t, mode, flags, caps), capped)
    # no flags: every pair forward
    np.testing.assert_array_equal(ctx.pairdist(q, t, mode),
                                  lib.pairdist_host(p, q, t, mode, n_threads=16))


@pytest.mark.parametrize("mode", [lib.PD_NW, lib.PD_HW])
def test_boundary_lengths(ctx, boundary, mode):
    p, q, t, flags, exp = boundary
    ctx.load(p)
    got = ctx.pairdist(q, t, mode, flags)
    bad = np.flatnonzero(got != exp[mode])
    assert len(bad) == 0, [(int(p.lengths[q[i]]), int(p.lengths[t[i]]), int(flags[i]),
                            int(got[i]), int(exp[mode][i])) for i in bad[:10]]
    # the other way round: the long read is the target
    got = ctx.pairdist(t, q, mode, flags)
    np.testing.assert_array_equal(got, lib.pairdist_host(p, t, q, mode, flags, n_threads=16))


def test_mixed_sizes_counts_duplicates_and_chunks(ctx, boundary, monkeypatch):
    """Short and long pairs in one call (groups of different sizes share the launch and, at the
    class borders, waves), n_pairs of 0, 1 and a count that fills no wave evenly, duplicate and
    unordered pairs, and a list cut into chunks by DMX_PD_CHUNK: all equal the one-shot result."""
    p, q, t, flags, exp = boundary
    ctx.load(p)
    assert len(ctx.pairdist([], [], lib.PD_NW)) == 0
    one = ctx.pairdist(q[5:6], t[5:6], lib.PD_NW, flags[5:6])
    assert one.tolist() == [int(exp[lib.PD_NW][5])]
    rng = np.random.default_rng(4)
    short = np.flatnonzero(p.lengths[q] <= 600)
    pick = np.concatenate([rng.choice(short, 197), np.arange(len(q)), np.arange(len(q))[::-1],
                           [3, 3, 3]])
    rng.shuffle(pick)
    assert len(pick) % 64 and len(pick) % 21 and len(pick) % 3
    qq, tt, ff = q[pick], t[pick], flags[pick]
    for mode in (lib.PD_NW, lib.PD_HW):
        got = ctx.pairdist(qq, tt, mode, ff)
        np.testing.assert_array_equal(got, exp[mode][pick])
        monkeypatch.setenv("DMX_PD_CHUNK", "37")
        chunked = ctx.pairdist(qq, tt, mode, ff)
        monkeypatch.delenv("DMX_PD_CHUNK")
        np.testing.assert_array_equal(chunked, got)


def test_refusals_launch_nothing(ctx):
    reads = [b"ACGT" * 20, b"", b"A" * (lib.PD_MAX_LEN + 1), b"ACGT" * 10]
    ctx.load(pc.pack_reads(reads))
    assert ctx.pairdist([0], [3], lib.PD_NW).tolist() == [40]
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.pairdist([0, 0], [3, 4], lib.PD_NW)          # an index >= n_reads
    with pytest.raises(lib.DmxError, match=r"\(-4\)"):
        ctx.pairdist([0, 1], [3, 3], lib.PD_NW)          # a zero-length read
    with pytest.raises(lib.DmxError, match=r"\(-4\)"):
        ctx.pairdist([0], [2], lib.PD_HW)                # a read above the maximum
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.pairdist([0], [3], lib.PD_NW, flags=[2])     # an unknown flag
    assert ctx.pairdist_ms() == 0.0                      # nothing ran in the refused calls


# ---- the similarity pass ------------------------------------------------------------------------

def make_bin():
    """~120 reads: three amplicon families of 300-420 nt, copies mutated 3-12 %, a quarter
    reverse-complemented, a few reads with N; some copies fall under the 300-nt filter."""
    reads = []
    for k, L in enumerate((308, 362, 420)):
        reads += synth.amplicon_bin(40, families=1, length=(L, L), mutate=(0.03, 0.12),
                                    rc_frac=0.25, n_reads_with_n=2, seed=50 + k)
    rng = np.random.default_rng(2)
    rng.shuffle(reads)
    return reads


def restated_similarity(reads, sg=80.0, minlength=300):
    """amplicon_sorter.py:550-571, 669-683, 777-808 in plain Python on the numpy DP: one group
    (fewer than 1000 reads), a stable sort by length, the 5 % rule, then per pair the forward
    identity and, below 0.5, the identity against the longer read's reverse complement."""
    comp = [r.upper().encode() for r in reads if len(r) >= minlength]
    d = sorted(range(len(comp)), key=lambda i: len(comp[i]))
    todo = []
    for p in range(len(d) - 1):
        for p2 in range(p + 1, len(d)):
            if len(comp[d[p]]) * 1.05 < len(comp[d[p2]]):
                continue
            todo.append((d[p], d[p2]))
    fwd = pc.np_dist([comp[a] for a, _ in todo], [comp[b] for _, b in todo], lib.PD_NW)
    lines = []
    for (a, b), df in zip(todo, fwd):
        iden = round(1 - int(df) / len(comp[b]), 3)
        if iden >= sg / 100:
            lines.append(str(a) + ":" + str(b) + ":" + str(iden))
        elif iden < 0.5:
            lines.append((a, b))   # the reverse complement is tried: filled in below
    again = [x for x in lines if isinstance(x, tuple)]
    rev = pc.np_dist([comp[a] for a, _ in again], [pc.revcomp(comp[b]) for _, b in again],
                     lib.PD_NW)
    found = {}
    for (a, b), dr in zip(again, rev):
        iden = round(1 - int(dr) / len(comp[b]), 3)
        found[(a, b)] = str(a) + ":" + str(b) + ":" + str(iden) + ":reverse" \
            if iden >= sg / 100 else None
    lines = [found[x] if isinstance(x, tuple) else x for x in lines]
    lines = [x for x in lines if x is not None]
    n_all = len(comp) * (len(comp) - 1) // 2
    return lines, len(todo), n_all


@pytest.fixture(scope="module")
def sim_bin():
    reads = make_bin()
    lines, n_pairs, n_all = restated_similarity(reads)
    return reads, lines, n_pairs, n_all


def test_similarity_lines_equal_the_restatement(ctx, sim_bin, tmp_path):
    reads, exp, n_pairs, n_all = sim_bin
    assert 100 <= len(reads) <= 130 and any("N" in r for r in reads)
    assert any(len(r) < 300 for r in reads)            # the filter renumbers the reads
    assert n_pairs < n_all                              # the 5 % rule dropped pairs
    assert any(x.endswith(":reverse") for x in exp) and any(x.count(":") == 2 for x in exp)
    out = tmp_path / "sim.txt"
    got = sorter.similarity(ctx, reads, out=str(out))
    assert got == exp
    assert out.read_text() == "".join(x + "\n" for x in exp)
    # lower case in, the same lines out
    assert sorter.similarity(ctx, [r.lower() for r in reads]) == exp


def test_cli_writes_the_same_file(sim_bin, tmp_path):
    reads, exp, _, _ = sim_bin
    src = tmp_path / "bin.fastq.gz"
    with gzip.open(src, "wt") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{r}\n+\n{'I' * len(r)}\n")
    out = tmp_path / "similarities.txt"
    r = subprocess.run([sys.executable, os.path.join(PKG, "bin", "dmx-similarity"), "-i", str(src),
                        "-o", str(out), "-sg", "80"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_text() == "".join(x + "\n" for x in exp)


def test_bounds_build_runs_a_mixed_call_clean(boundary, tmp_path):
    """The bounds-checked library (every gather of the packed batch checked) in a child
    process: one mixed call, no violation, the release results."""
    _, q, t, flags, exp = boundary
    reads = boundary_reads()
    keep = [i for i in range(len(q)) if len(reads[2 * i]) <= 1400 or len(reads[2 * i]) > 8000]
    np.save(tmp_path / "exp.npy", exp[lib.PD_HW][keep])
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, json, numpy as np\n"
        f"sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {PKG!r}]\n"
        "import pairdist_cases as pc\nimport test_pairdist as tp\nfrom dmx import lib\n"
        "reads = tp.boundary_reads()\n"
        f"keep = np.array({keep!r})\n"
        "q = (2 * keep).astype(np.uint32); t = q + 1\n"
        "flags = (keep % 3 == 1).astype(np.uint8)\n"
        "with lib.Context(0) as c:\n"
        "    c.load(pc.pack_reads(reads))\n"
        "    got = c.pairdist(q, t, lib.PD_HW, flags)\n"
        "print(json.dumps({'lib': lib.LIB_PATH, 'got': got.tolist()}))\n")
    env = dict(os.environ, DMX_DEBUG_BOUNDS="1")
    env.pop("DMX_LIBDMX", None)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["lib"].endswith("libdmx_bounds.so")
    assert res["got"] == np.load(tmp_path / "exp.npy").tolist()
