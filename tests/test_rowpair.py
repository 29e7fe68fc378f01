"""dmx_rowpairdist / dmx_rowhits (csrc/dmx_pairdist.hip rowpair_kernel) on the GPU
against their host twins, themselves pinned to an in-test numpy DP by test_rowpair_host.py: the
distances and the hits must be equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pairdist_cases as pc
import rowdist_cases as rc
import rowpair_cases as rp
from dmx import lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")
MODES = (lib.PD_NW, lib.PD_HW)


@pytest.fixture(scope="module")
def boundary():
    """The boundary set with the host's distances per mode (computed once)."""
    rows, q, t, f = rp.boundary_case()
    exp = {m: lib.rowpairdist_host(rows, q, t, m, flags=f, n_threads=16) for m in MODES}
    return rows, q, t, f, exp


def explain(rows, q, t, f, got, exp):
    bad = np.flatnonzero(got != exp)
    return [(len(rows[q[i]]), len(rows[t[i]]), int(f[i]), int(got[i]), int(exp[i]))
            for i in bad[:10]]


def test_boundary_lengths(ctx, boundary):
    rows, q, t, f, exp = boundary
    ql = {len(rows[i]) for i in q}
    need = {1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4200}
    for g in lib.pairdist_group_sizes():
        need |= {64 * g - 1, 64 * g, 64 * g + 1}
    assert need <= ql
    assert {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1200} <= {len(rows[j]) for j in t}
    assert f.any() and not f.all()
    for mode in MODES:
        got = ctx.rowpairdist(rows, q, t, mode, flags=f)
        assert not explain(rows, q, t, f, got, exp[mode])
        assert ctx.rowhits_ms() > 0
        caps, capped = pc.cap_cycle(exp[mode])
        np.testing.assert_array_equal(ctx.rowpairdist(rows, q, t, mode, flags=f, caps=caps), capped)
    # no flags at all: no reversed copies are made
    fwd = np.flatnonzero(f == 0)
    np.testing.assert_array_equal(ctx.rowpairdist(rows, q[fwd], t[fwd], lib.PD_HW),
                                  exp[lib.PD_HW][fwd])


def test_mixed_sizes_duplicates_and_chunks(ctx, boundary, monkeypatch):
    """Short and long pairs in one call, duplicates, no order, a count that fills no wave
    evenly; n_pairs of 0 and 1; the list cut into chunks by DMX_PD_CHUNK: the same result."""
    rows, q, t, f, exp = boundary
    assert len(ctx.rowpairdist(rows, [], [], lib.PD_HW)) == 0
    assert ctx.rowpairdist(rows, q[5:6], t[5:6], lib.PD_NW, flags=f[5:6]).tolist() == \
        [int(exp[lib.PD_NW][5])]
    pick = rp.mixed_pick(rows, q)
    for mode in MODES:
        got = ctx.rowpairdist(rows, q[pick], t[pick], mode, flags=f[pick])
        assert not explain(rows, q[pick], t[pick], f[pick], got, exp[mode][pick])
        caps, capped = pc.cap_cycle(exp[mode][pick])
        monkeypatch.setenv("DMX_PD_CHUNK", "37")
        chunked = ctx.rowpairdist(rows, q[pick], t[pick], mode, flags=f[pick])
        chunked_caps = ctx.rowpairdist(rows, q[pick], t[pick], mode, flags=f[pick], caps=caps)
        monkeypatch.delenv("DMX_PD_CHUNK")
        np.testing.assert_array_equal(chunked, got)
        np.testing.assert_array_equal(chunked_caps, capped)


def test_rows_of_resident_reads_equal_pairdist(ctx):
    """Rows that are mask_row of resident reads: pairdist on those reads, NW and HW, forward and
    PD_RC."""
    reads, q, t, _, _ = pc.random_set()
    ctx.load(pc.pack_reads(reads))
    q, t = q[:120], t[:120]
    rows = [lib.mask_row(r) for r in reads[:240]]
    rcf = np.full(len(q), lib.PD_RC, dtype=np.uint8)
    for mode in MODES:
        np.testing.assert_array_equal(ctx.rowpairdist(rows, q, t, mode),
                                      ctx.pairdist(q, t, mode))
        np.testing.assert_array_equal(ctx.rowpairdist(rows, q, t, mode, flags=rcf),
                                      ctx.pairdist(q, t, mode, flags=rcf))


def hits_equal(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_rowhits_equals_the_host(ctx, boundary, monkeypatch):
    rows, q, t, _, _ = boundary
    keep = np.flatnonzero(np.array([len(rows[i]) for i in q]) <= 1300)
    q, t = q[keep], t[keep]
    n = len(q)
    for mode in MODES:
        df = lib.rowpairdist_host(rows, q, t, mode, n_threads=16).astype(np.int64)
        dr = lib.rowpairdist_host(rows, q, t, mode, flags=np.full(n, lib.PD_RC, dtype=np.uint8),
                                  n_threads=16).astype(np.int64)
        d = np.minimum(df, dr)
        k = np.arange(n) % 5
        cap = np.where(k == 0, -1, np.where(k == 1, 0, np.where(k == 2, d - 1,
                                                                np.where(k == 3, d, d + 1))))
        exp = lib.rowhits_host(rows, q, t, cap, mode, n_threads=16)
        assert 0 < len(exp[0]) < n and exp[2].any() and not exp[2].all()
        hits_equal(ctx.rowhits(rows, q, t, cap, mode), exp)
        assert ctx.rowhits_ms() > 0
        monkeypatch.setenv("DMX_PD_CHUNK", "37")
        hits_equal(ctx.rowhits(rows, q, t, cap, mode), exp)
        monkeypatch.delenv("DMX_PD_CHUNK")
        # no hit at all, and every pair a hit
        assert [len(x) for x in ctx.rowhits(rows, q, t, np.full(n, -1), mode)] == [0, 0, 0]
        pair, dd, rev = ctx.rowhits(rows, q, t, np.full(n, 20000), mode)
        np.testing.assert_array_equal(pair, np.arange(n))
        np.testing.assert_array_equal(dd, d)
        np.testing.assert_array_equal(rev, dr < df)
    assert [len(x) for x in ctx.rowhits(rows, [], [], [])] == [0, 0, 0]


def short_pairs(n=3000, seed=94):
    """A few thousand short pairs over 80 rows of 20..90 columns, half of them related."""
    rng = np.random.default_rng(seed)
    base = [rp.rand_row(rng, int(m), 0.05) for m in rng.integers(20, 91, 40)]
    rows = base + [rc.planted_row(rng, b.replace("-", "A").encode().translate(
        bytes.maketrans(b"RYMKSW", b"AGCTCA")), 0.08) for b in base]
    rows = [rc.revcomp_row(r) if k % 3 == 0 else r for k, r in enumerate(rows)]
    q = rng.integers(0, len(rows), n).astype(np.uint32)
    t = np.where(rng.random(n) < 0.5, (q + 40) % 80, rng.integers(0, len(rows), n)).astype(np.uint32)
    cap = np.array([max(len(rows[a]), len(rows[b])) * 2 // 5 for a, b in zip(q, t)])
    cap[rng.random(n) < 0.1] = -1
    return rows, q, t, cap


def test_rowhits_compaction_crosses_many_blocks(ctx):
    rows, q, t, cap = short_pairs()
    exp = lib.rowhits_host(rows, q, t, cap, lib.PD_HW, n_threads=16)
    assert 256 * 3 < len(exp[0]) < len(q) - 256     # several compaction blocks, hits and misses
    hits_equal(ctx.rowhits(rows, q, t, cap, lib.PD_HW), exp)


def test_resident_batch_is_undisturbed(ctx, boundary):
    reads, q, t, _, _ = pc.random_set()
    ctx.load(pc.pack_reads(reads))
    q, t = q[:200], t[:200]
    cap = np.full(len(q), 60, dtype=np.int32)
    best, n_hits = ctx.pairhits(q, t, cap, cap)
    before = ctx.pairhits_fetch()
    dist = ctx.pairdist(q, t, lib.PD_HW)
    rows, rq, rt, rcap = short_pairs(600)
    exp = lib.rowhits_host(rows, rq, rt, rcap, lib.PD_HW, n_threads=16)
    hits_equal(ctx.rowhits(rows, rq, rt, rcap, lib.PD_HW), exp)
    assert n_hits > 0 and n_hits == len(before[0])
    hits_equal(ctx.pairhits_fetch(), before)
    np.testing.assert_array_equal(ctx.pairdist(q, t, lib.PD_HW), dist)


def test_refusals_launch_nothing(ctx):
    rows = ["ACGTACGT", "ACGTTCGT"]
    assert ctx.rowpairdist(rows, [0], [1], lib.PD_NW).tolist() == [1]
    assert ctx.rowhits_ms() > 0
    big = "A" * (lib.PD_MAX_LEN + 1)
    for code, match, rws, q, t, kw in (
            (-1, "mode must be", rows, [0], [0], {"mode": 2}),
            (-1, "pair 1 names a row outside the 2 given", rows, [0, 0], [1, 2], {}),
            (-1, "pair 1 has an unknown flag", rows, [0, 0], [0, 0], {"flags": [1, 2]}),
            (-1, "row 1: column 2 has a mask bit",
             ["ACGT", np.array([1, 2, 32], dtype=np.uint8)], [0], [0], {}),
            (-4, "pair 1: row 1 has 0 columns", ["ACGT", ""], [0, 0], [0, 1], {}),
            (-4, "pair 0: row 0 has", [big], [0], [0], {})):
        mode = kw.pop("mode", lib.PD_NW)
        with pytest.raises(lib.DmxError, match=rf"\({code}\).*dmx_rowpairdist: {match}"):
            ctx.rowpairdist(rws, q, t, mode, **kw)
        assert ctx.rowhits_ms() == 0.0
    assert ctx.rowhits(rows, [0], [1], [1])[1].tolist() == [1]
    assert ctx.rowhits_ms() > 0
    with pytest.raises(lib.DmxError, match=r"\(-1\).*dmx_rowhits: pair 1: a cap is"):
        ctx.rowhits(rows, [0, 0], [0, 1], [0, -2])
    assert ctx.rowhits_ms() == 0.0
    with pytest.raises(lib.DmxError, match=r"\(-1\).*dmx_rowhits: pair 0 names a row outside"):
        ctx.rowhits(rows, [2], [1], [0])
    assert ctx.rowhits_ms() == 0.0
    L = lib.load()
    one = np.zeros(1, dtype=np.uint32)
    assert L.dmx_rowpairdist(ctx._h, 0, 1, None, None, one.ctypes.data, one.ctypes.data, None,
                             None, 1, one.ctypes.data) == -1
    assert b"null" in L.dmx_last_error(ctx._h)
    assert ctx.rowhits_ms() == 0.0
    # the context works afterwards
    assert ctx.rowpairdist(rows, [0, 1], [1, 1], lib.PD_HW).tolist() == [1, 0]


FRESH = """import sys, json, numpy as np
sys.path[:0] = [{tests!r}, {pkg!r}]
import rowpair_cases as rp
from dmx import lib
rows, q, t, f = rp.boundary_case()
keep = np.flatnonzero(np.array([len(rows[i]) for i in q]) <= 1300)
pick = rp.mixed_pick(rows, q)
cap = np.array([len(rows[j]) // 3 for j in t[keep]])
with lib.Context(0) as c:      # nothing is ever loaded into this context
    hits = c.rowhits(rows, q[keep], t[keep], cap, lib.PD_HW)
    got = [c.rowpairdist(rows, q, t, m, flags=f).tolist() for m in (lib.PD_NW, lib.PD_HW)]
    mixed = c.rowpairdist(rows, q[pick], t[pick], lib.PD_HW, flags=f[pick]).tolist()
print(json.dumps({{'lib': lib.LIB_PATH, 'hits': [x.tolist() for x in hits], 'got': got,
                  'mixed': mixed}}))
"""


def run_child(tmp_path, bounds):
    script = tmp_path / "run.py"
    script.write_text(FRESH.format(tests=os.path.join(ROOT, "tests"), pkg=PKG))
    env = dict(os.environ)
    env.pop("DMX_LIBDMX", None)
    env.pop("DMX_PD_CHUNK", None)
    env.pop("DMX_DEBUG_BOUNDS", None)
    if bounds:
        env["DMX_DEBUG_BOUNDS"] = "1"
    res = subprocess.run([sys.executable, str(script)], capture_output=True, text=True,
                         timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("bounds", [False, True], ids=["fresh-context", "bounds-build"])
def test_fresh_context_and_bounds_build(boundary, tmp_path, bounds):
    """A context that never saw a load, in a child process; and the same through the
    bounds-checked library (every row, scratch and output access checked): no violation, the
    host's results."""
    rows, q, t, f, exp = boundary
    out = run_child(tmp_path, bounds)
    assert out["lib"].endswith("libdmx_bounds.so" if bounds else "libdmx.so")
    assert out["got"] == [exp[m].tolist() for m in MODES]
    assert out["mixed"] == exp[lib.PD_HW][rp.mixed_pick(rows, q)].tolist()
    keep = np.flatnonzero(np.array([len(rows[i]) for i in q]) <= 1300)
    cap = np.array([len(rows[j]) // 3 for j in t[keep]])
    hits = lib.rowhits_host(rows, q[keep], t[keep], cap, lib.PD_HW, n_threads=16)
    assert out["hits"] == [x.tolist() for x in hits] and len(hits[0]) > 0
