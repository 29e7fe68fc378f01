"""dmx_pairalign (csrc/dmx_pairdist.hip pairalign_kernel + pairalign_traceback_kernel; DESIGN.md
§8f) on the GPU against dmx_pairalign_host, itself pinned to a numpy DP and hand cases by
test_pairalign_host.py: distances, path offsets and ops must be equal byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pairdist_cases as pc
from dmx import lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")


def boundary_reads():
    """Pairs (2i, 2i + 1): query lengths around one and two words and around every group size
    (64 G - 1, 64 G, 64 G + 1) against mutated copies; 4,200 against a 300-nt cut of itself (two
    stripes); 2 x 4,096 + 70 against a 400-nt target (three stripes); the longest read against
    300 nt; one 4,200 x 4,200 pair; a 1-nt query against 5,000 nt.  Where a word, group, stripe
    or trace index can go wrong, not the workload's shapes."""
    rng = np.random.default_rng(33)
    qlens = {1, 63, 64, 65, 128, 129}
    for g in lib.pairdist_group_sizes():
        qlens |= {64 * g - 1, 64 * g, 64 * g + 1}
    reads = []
    for m in sorted(qlens):
        a = pc.rand_seq(rng, m)
        reads += [a, pc.mutate(rng, a, 0.08)]
    a = pc.rand_seq(rng, 4200)
    reads += [a, pc.mutate(rng, a[2000:2300], 0.05)]
    a = pc.rand_seq(rng, 2 * 4096 + 70)
    reads += [a, pc.mutate(rng, a[3000:3400], 0.05)]
    a = pc.rand_seq(rng, lib.PD_MAX_LEN)
    reads += [a, pc.mutate(rng, a[9000:9300], 0.05)]
    a = pc.rand_seq(rng, 4200)
    reads += [a, pc.mutate(rng, a, 0.1)]
    reads += [b"G", pc.rand_seq(rng, 5000)]
    return reads


def boundary_pairs(n_reads):
    """Every pair and the same pair the other way round; RC on a third of them."""
    a = np.arange(0, n_reads, 2, dtype=np.uint32)
    q = np.concatenate([a, a + 1])
    t = np.concatenate([a + 1, a])
    flags = (np.arange(len(q)) % 3 == 1).astype(np.uint8)
    return q, t, flags


def same(got, exp):
    for g, e, name in zip(got, exp, ("dist", "op_off", "ops")):
        assert g.dtype == e.dtype and g.shape == e.shape, name
        bad = np.flatnonzero(g != e)
        assert len(bad) == 0, (name, bad[:10].tolist())


@pytest.fixture(scope="module")
def boundary():
    reads = boundary_reads()
    p = pc.pack_reads(reads)
    q, t, flags = boundary_pairs(len(reads))
    return p, q, t, flags, lib.pairalign_host(p, q, t, flags, n_threads=16)


@pytest.fixture(scope="module")
def random_batch():
    reads, q, t, flags, exp = pc.random_set()
    p = pc.pack_reads(reads)
    host = lib.pairalign_host(p, q, t, flags, n_threads=16)
    np.testing.assert_array_equal(host[0], exp[lib.PD_NW])
    return p, q, t, flags, host


def test_random_pairs_equal_the_host_paths(ctx, random_batch):
    p, q, t, flags, host = random_batch
    ctx.load(p)
    same(ctx.pairalign(q, t, flags), host)
    assert ctx.pairalign_ms() > 0
    st = ctx.pairalign_stats()
    assert st["launches"] == 1 and st["forward"] > 0 and st["traceback"] > 0
    # no flags: every pair forward
    same(ctx.pairalign(q[:100], t[:100]), lib.pairalign_host(p, q[:100], t[:100], n_threads=16))


def test_boundary_lengths_both_ways_round(ctx, boundary):
    p, q, t, flags, host = boundary
    ctx.load(p)
    got = ctx.pairalign(q, t, flags)
    bad = np.flatnonzero(got[0] != host[0])
    assert len(bad) == 0, [(int(p.lengths[q[i]]), int(p.lengths[t[i]]), int(flags[i]),
                            int(got[0][i]), int(host[0][i])) for i in bad[:10]]
    plen, hlen = np.diff(got[1].astype(np.int64)), np.diff(host[1].astype(np.int64))
    bad = np.flatnonzero(plen != hlen)
    assert len(bad) == 0, [(int(p.lengths[q[i]]), int(p.lengths[t[i]]), int(plen[i]),
                            int(hlen[i])) for i in bad[:10]]
    for i in range(len(q)):   # name the first pair whose path differs
        a, b = got[2][got[1][i]:got[1][i + 1]], host[2][host[1][i]:host[1][i + 1]]
        d = np.flatnonzero(a != b)
        assert len(d) == 0, (int(p.lengths[q[i]]), int(p.lengths[t[i]]), int(flags[i]),
                             "first differing op", int(d[0]), "of", len(a))
    same(got, host)
    # the distance form of the one forward pass agrees with the trace form at every group size,
    # at the stripe boundaries and under RC
    np.testing.assert_array_equal(ctx.pairdist(q, t, lib.PD_NW, flags), got[0])
    # counts of 0 and 1, repeated and unordered pairs
    d, off, ops = ctx.pairalign([], [])
    assert len(d) == 0 and off.tolist() == [0] and len(ops) == 0
    pick = np.array([7, 3, 7, 0, len(q) - 1, 7])
    same(ctx.pairalign(q[pick], t[pick], flags[pick]),
         lib.pairalign_host(p, q[pick], t[pick], flags[pick], n_threads=8))


def test_chunked_by_trace_budget_in_a_child_process(random_batch, tmp_path):
    """DMX_PA_TRACE_MB=1 cuts the random set's trace (about 18 bytes per word and column) into
    several launches: identical output."""
    _, q, t, flags, host = random_batch
    np.savez(tmp_path / "exp.npz", dist=host[0], off=host[1], ops=host[2])
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, json, numpy as np\n"
        f"sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {PKG!r}]\n"
        "import pairdist_cases as pc\nfrom dmx import lib\n"
        "reads, q, t, flags, _ = pc.random_set()\n"
        f"e = np.load({str(tmp_path / 'exp.npz')!r})\n"
        "with lib.Context(0) as c:\n"
        "    c.load(pc.pack_reads(reads))\n"
        "    d, off, ops = c.pairalign(q, t, flags)\n"
        "    n = c.pairalign_stats()['launches']\n"
        "ok = d.tolist() == e['dist'].tolist() and off.tolist() == e['off'].tolist() \\\n"
        "    and ops.tobytes() == e['ops'].tobytes()\n"
        "print(json.dumps({'launches': n, 'same': bool(ok)}))\n")
    env = dict(os.environ, DMX_PA_TRACE_MB="1")
    env.pop("DMX_DEBUG_BOUNDS", None)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["launches"] > 3 and res["same"], res


def test_refusals_launch_nothing(ctx):
    reads = [b"ACGT" * 20, b"", b"A" * (lib.PD_MAX_LEN + 1), b"ACGT" * 10]
    p = pc.pack_reads(reads)
    ctx.load(p)
    d, off, ops = ctx.pairalign([0], [3])
    assert d.tolist() == [40] and len(ops) == 80 == off[-1]      # 40 matches, 40 inserts
    assert ctx.pairalign_ms() > 0
    L, n = lib.load(), 2
    qa, ta = np.array([0, 0], dtype=np.uint32), np.array([3, 3], dtype=np.uint32)
    dist, offs = np.zeros(n, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint64)
    buf = np.zeros(239, dtype=np.uint8)                # 2 x (80 + 40) = 240 needed
    rc = L.dmx_pairalign(ctx._h, qa.ctypes.data, ta.ctypes.data, None, n, dist.ctypes.data,
                         offs.ctypes.data, buf.ctypes.data, len(buf))
    assert rc == -1 and b"ops_cap" in L.dmx_last_error(ctx._h)
    assert ctx.pairalign_ms() == 0.0
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.pairalign([0, 0], [3, 4])                  # an index >= n_reads
    with pytest.raises(lib.DmxError, match=r"\(-4\)"):
        ctx.pairalign([0, 1], [3, 3])                  # a zero-length read
    with pytest.raises(lib.DmxError, match=r"\(-4\)"):
        ctx.pairalign([0], [2])                        # a read above the maximum
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        ctx.pairalign([0], [3], flags=[2])             # an unknown flag
    assert ctx.pairalign_ms() == 0.0                   # nothing ran in the refused calls
    assert ctx.pairalign_stats()["launches"] == 0


def test_bounds_build_runs_the_boundary_set_clean(boundary, tmp_path):
    """The bounds-checked library (every gather of the packed batch, every trace and op-region
    access checked) in a child process: one call over the boundary set, no violation, the
    host's paths."""
    _, _, _, _, host = boundary
    np.savez(tmp_path / "exp.npz", dist=host[0], off=host[1], ops=host[2])
    script = tmp_path / "run.py"
    script.write_text(
        "import sys, json, numpy as np\n"
        f"sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {PKG!r}]\n"
        "import pairdist_cases as pc\nimport test_pairalign as tp\nfrom dmx import lib\n"
        "reads = tp.boundary_reads()\n"
        "q, t, flags = tp.boundary_pairs(len(reads))\n"
        f"e = np.load({str(tmp_path / 'exp.npz')!r})\n"
        "with lib.Context(0) as c:\n"
        "    c.load(pc.pack_reads(reads))\n"
        "    d, off, ops = c.pairalign(q, t, flags)\n"
        "ok = d.tolist() == e['dist'].tolist() and off.tolist() == e['off'].tolist() \\\n"
        "    and ops.tobytes() == e['ops'].tobytes()\n"
        "print(json.dumps({'lib': lib.LIB_PATH, 'same': bool(ok)}))\n")
    env = dict(os.environ, DMX_DEBUG_BOUNDS="1")
    env.pop("DMX_LIBDMX", None)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["lib"].endswith("libdmx_bounds.so") and res["same"], res
