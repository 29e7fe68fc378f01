"""dmx_rowdist (csrc/dmx_pairdist.hip rowdist_kernel) on the GPU against
dmx_rowdist_host, itself pinned to an in-test numpy DP by test_rowdist_host.py: the distances
must be equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pairdist_cases as pc
import rowdist_cases as rc
from dmx import lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")


@pytest.fixture(scope="module")
def boundary():
    """The boundary set, packed, with the host's distances (computed once)."""
    reads, rows, q, r = rc.boundary_case()
    p = pc.pack_reads(reads)
    return p, rows, q, r, lib.rowdist_host(p, rows, q, r, n_threads=16)


def explain(p, rows, q, r, got, exp):
    bad = np.flatnonzero(got != exp)
    return [(int(p.lengths[q[i]]), len(rows[r[i]]), int(got[i]), int(exp[i])) for i in bad[:10]]


def test_boundary_lengths(ctx, boundary):
    p, rows, q, r, exp = boundary
    lens = set(p.lengths[q].tolist())
    assert {1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4200} <= lens
    assert {1, 15, 16, 17, 31, 32, 33, 1200} <= {len(rows[j]) for j in r}
    assert any("-" in x for x in rows) and any(set(x) & set("RYMKSW") for x in rows)
    assert any("N" in x for x in rows)
    ctx.load(p)
    got = ctx.rowdist(rows, q, r)
    assert not explain(p, rows, q, r, got, exp)
    assert ctx.rowdist_ms() > 0
    # a second identical call
    np.testing.assert_array_equal(ctx.rowdist(rows, q, r), got)
    caps, capped = pc.cap_cycle(exp)
    np.testing.assert_array_equal(ctx.rowdist(rows, q, r, caps), capped)


def test_mixed_sizes_duplicates_and_chunks(ctx, boundary, monkeypatch):
    """Short and long pairs in one call, duplicates, no order, a count that fills no wave
    evenly; n_pairs of 0 and 1; the list cut into chunks by DMX_PD_CHUNK: the same result."""
    p, rows, q, r, exp = boundary
    ctx.load(p)
    assert len(ctx.rowdist(rows, [], [])) == 0
    assert ctx.rowdist(rows, q[5:6], r[5:6]).tolist() == [int(exp[5])]
    pick = rc.mixed_pick(q, p.lengths)
    got = ctx.rowdist(rows, q[pick], r[pick])
    assert not explain(p, rows, q[pick], r[pick], got, exp[pick])
    caps, capped = pc.cap_cycle(exp[pick])
    monkeypatch.setenv("DMX_PD_CHUNK", "37")
    chunked = ctx.rowdist(rows, q[pick], r[pick])
    chunked_caps = ctx.rowdist(rows, q[pick], r[pick], caps)
    monkeypatch.delenv("DMX_PD_CHUNK")
    np.testing.assert_array_equal(chunked, got)
    np.testing.assert_array_equal(chunked_caps, capped)


def test_rows_of_resident_reads_equal_pairdist(ctx):
    """A row that is mask_row of resident read t: pairdist(q, t, NW); its mask_rc: PD_RC."""
    reads, q, t, _, _ = pc.random_set()
    ctx.load(pc.pack_reads(reads))
    q, t = q[:120], t[:120]
    rows = [lib.mask_row(reads[j]) for j in t]
    idx = np.arange(len(q), dtype=np.uint32)
    np.testing.assert_array_equal(ctx.rowdist(rows, q, idx), ctx.pairdist(q, t, lib.PD_NW))
    np.testing.assert_array_equal(
        ctx.rowdist([lib.mask_rc(x) for x in rows], q, idx),
        ctx.pairdist(q, t, lib.PD_NW, flags=np.full(len(q), lib.PD_RC, dtype=np.uint8)))


def test_refusals_launch_nothing(ctx, boundary):
    reads = [b"ACGT" * 5, b"", b"A" * (lib.PD_MAX_LEN + 1)]
    ctx.load(pc.pack_reads(reads))
    assert ctx.rowdist(["ACGT"], [0], [0]).tolist() == [16]
    assert ctx.rowdist_ms() > 0
    for code, match, rows, q, r in (
            (-1, "pair 1 names a read outside the batch", ["ACGT"], [0, 3], [0, 0]),
            (-1, "pair 2 names a row outside", ["ACGT", "AC"], [0, 0, 0], [0, 1, 2]),
            (-4, r"pair 1: reads of 1\.\.", ["ACGT"], [0, 1], [0, 0]),
            (-4, r"pair 0: reads of 1\.\.", ["ACGT"], [2], [0]),
            (-4, "pair 1: row 1 has 0 columns", ["ACGT", ""], [0, 0], [0, 1]),
            (-4, "pair 0: row 0 has", ["A" * (lib.PD_MAX_LEN + 1)], [0], [0]),
            (-1, "row 1: column 2 has a mask bit",
             ["ACGT", np.array([1, 2, 32], dtype=np.uint8)], [0], [0])):
        with pytest.raises(lib.DmxError, match=rf"\({code}\).*{match}"):
            ctx.rowdist(rows, q, r)
        assert ctx.rowdist_ms() == 0.0
    L = lib.load()
    one = np.zeros(1, dtype=np.uint32)
    assert L.dmx_rowdist(ctx._h, 1, None, None, one.ctypes.data, one.ctypes.data, None, 1,
                         one.ctypes.data) == -1
    assert b"null" in L.dmx_last_error(ctx._h)
    assert ctx.rowdist_ms() == 0.0
    # the context works afterwards
    assert ctx.rowdist(["ACGT"], [0], [0]).tolist() == [16]
    p, rows, q, r, exp = boundary
    ctx.load(p)
    np.testing.assert_array_equal(ctx.rowdist(rows, q[:20], r[:20]), exp[:20])


CHILD = """import sys, json, numpy as np
sys.path[:0] = [{tests!r}, {pkg!r}]
import pairdist_cases as pc
import rowdist_cases as rc
from dmx import lib
reads, rows, q, r = rc.boundary_case()
pick = rc.mixed_pick(q, np.array([len(x) for x in reads]))
with lib.Context(0) as c:
    c.load(pc.pack_reads(reads))
    got = c.rowdist(rows, q, r)
    mixed = c.rowdist(rows, q[pick], r[pick])
print(json.dumps({{'lib': lib.LIB_PATH, 'got': got.tolist(), 'mixed': mixed.tolist()}}))
"""


def test_bounds_build_runs_the_boundary_set_clean(boundary, tmp_path):
    """The bounds-checked library (every gather of the packed batch, every row and scratch
    access checked) in a child process: no violation, the host's result."""
    p, rows, q, r, exp = boundary
    script = tmp_path / "run.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=PKG))
    env = dict(os.environ, DMX_DEBUG_BOUNDS="1")
    env.pop("DMX_LIBDMX", None)
    env.pop("DMX_PD_CHUNK", None)
    res = subprocess.run([sys.executable, str(script)], capture_output=True, text=True,
                         timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["lib"].endswith("libdmx_bounds.so")
    assert out["got"] == exp.tolist()
    assert out["mixed"] == exp[rc.mixed_pick(q, p.lengths)].tolist()
