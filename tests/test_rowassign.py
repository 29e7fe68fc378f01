"""dmx_rowassign (csrc/dmx_pairdist.hip rowassign_kernel, rowassign_decide_kernel,
rowassign_finish_kernel) on the GPU against dmx_rowassign_host, itself pinned to
the in-test oracle by test_rowassign_host.py: all five outputs must be equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pairdist_cases as pc
import rowassign_cases as ra
from dmx import lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")


def as_exp(got):
    row, d, cls, n_pairs, n_lines = got
    return dict(best_row=row, best_d=d, best_class=cls, n_pairs=n_pairs, n_lines=n_lines)


@pytest.fixture(scope="module")
def host_case():
    reads, rows, sel, tb, exp, _ = ra.host_set()
    p = pc.pack_reads(reads)
    got = lib.rowassign_host(p, rows, sel, *tb, n_threads=16)
    ra.same(got, exp)
    return p, rows, sel, tb, as_exp(got)


@pytest.fixture(scope="module")
def boundary():
    """The boundary set, packed, with the host twin's answer (computed once)."""
    reads, rows, sel, tb = ra.boundary_set()
    p = pc.pack_reads(reads)
    return p, rows, sel, tb, as_exp(lib.rowassign_host(p, rows, sel, *tb, n_threads=16))


def test_cpu_case_set(ctx, host_case):
    p, rows, sel, tb, exp = host_case
    ctx.load(p)
    ra.same(ctx.rowassign(rows, sel, *tb), exp)
    assert ctx.rowassign_ms() > 0
    # the stop rule, and nothing to compare
    stop = as_exp(lib.rowassign_host(p, rows, sel, *tb, chunk=50, max_chunks=2, n_threads=16))
    assert stop["n_pairs"] < exp["n_pairs"]
    ra.same(ctx.rowassign(rows, sel, *tb, chunk=50, max_chunks=2), stop)
    row, d, cls, n_pairs, n_lines = ctx.rowassign(rows, [], *tb)
    assert len(row) == 0 and (n_pairs, n_lines) == (0, 0)
    row, d, cls, n_pairs, n_lines = ctx.rowassign([], sel[:4], *tb)
    assert (row == ra.NONE).all() and (d == ra.NONE).all() and (cls == 0).all() and n_pairs == 0


def test_boundary_lengths(ctx, boundary):
    p, rows, sel, tb, exp = boundary
    assert {1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4200} == set(p.lengths.tolist())
    assert {63, 64, 65, 127, 128, 129} <= {len(x) for x in rows}
    assert exp["n_pairs"] >= 3 * len(sel) and (exp["best_row"] != ra.NONE).all()
    assert exp["n_lines"] >= 2 * len(sel)       # the planted copy and the reversed one
    ctx.load(p)
    got = ctx.rowassign(rows, sel, *tb)
    ra.same(got, exp)
    # a second identical call
    ra.same(ctx.rowassign(rows, sel, *tb), exp)
    assert ctx.rowassign_ms() > 0


def test_chunks_of_37_pairs_give_the_same(ctx, host_case, boundary, monkeypatch):
    """A place's rows span several launches, and some retries run in a later launch than their
    forward pass."""
    for p, rows, sel, tb, exp in (host_case, boundary):
        ctx.load(p)
        if exp is host_case[4]:
            assert exp["n_pairs"] > 4 * 37
        monkeypatch.setenv("DMX_PD_CHUNK", "37")
        got = ctx.rowassign(rows, sel, *tb)
        monkeypatch.delenv("DMX_PD_CHUNK")
        ra.same(got, exp, "DMX_PD_CHUNK=37")


def test_rows_of_resident_reads_agree_with_pairdist(ctx):
    """Rows that are mask_row of resident reads: best_d is pairdist's distance (NW; PD_RC for a
    reverse line)."""
    reads, q, t, _, _ = pc.random_set()
    p = pc.pack_reads(reads)
    ctx.load(p)
    targets = np.unique(t[:40])
    rows = [lib.mask_row(reads[j]) for j in targets]
    sel = np.unique(q[:40]).astype(np.uint32)
    lengths = {len(x) for x in reads}
    tb = ra.tables(sorted(lengths), threshold=0.6)
    row, d, cls, n_pairs, n_lines = ctx.rowassign(rows, sel, *tb)
    has = np.flatnonzero(row != ra.NONE)
    assert len(has) >= 5 and n_lines >= len(has)
    rev = (d[has] & ra.REV) != 0
    dist = ctx.pairdist(sel[has], targets[row[has]], lib.PD_NW,
                        flags=np.where(rev, lib.PD_RC, 0).astype(np.uint8))
    np.testing.assert_array_equal(d[has] & (ra.REV - 1), dist)


def test_pairhits_outcomes_survive(ctx, host_case):
    p, rows, sel, tb, exp = host_case
    ctx.load(p)
    n = p.n_reads
    q = np.arange(6, 28, dtype=np.uint32)
    t = q + 2                                   # copies of one founder
    cap = np.full(len(q), 60, dtype=np.int32)
    best, n_hits = ctx.pairhits(q, t, cap, cap + 40)
    before = ctx.pairhits_fetch()
    assert n_hits > 0 and n == len(best)
    ra.same(ctx.rowassign(rows, sel, *tb), exp)
    after = ctx.pairhits_fetch()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


def test_refusals_launch_nothing(ctx, host_case):
    p, rows, sel, tb, exp = host_case
    ctx.load(p)
    ra.same(ctx.rowassign(rows, sel, *tb), exp)
    assert ctx.rowassign_ms() > 0
    cap_hit, cap_half, bin_off, bins = tb
    bad_cap = cap_hit.copy()
    bad_cap[200] = -3
    for code, match, args, kw in (
            (-1, "place 2 names a read outside the batch", (rows, [0, 1, 999], *tb), {}),
            (-1, "chunk must be at least 1", (rows, sel, *tb), dict(chunk=0)),
            (-1, "length 200: a cap is a distance", (rows, sel, bad_cap, cap_half, bin_off, bins), {}),
            (-1, "is outside the 100 entries of the tables",
             (rows, sel, cap_hit[:100], cap_half[:100], bin_off[:100], bins), {}),
            (-1, "its classes end outside", (rows, sel, cap_hit, cap_half, bin_off, bins[:5]), {}),
            (-1, "row 0: column 1 has a mask bit",
             ([np.array([1, 64], dtype=np.uint8)], sel, *tb), {})):
        with pytest.raises(lib.DmxError, match=rf"\({code}\).*{match}") as e:
            ctx.rowassign(*args, **kw)
        assert ctx.rowassign_ms() == 0.0
        assert all((x == (0xBEEF if x.dtype == np.uint16 else 0xDEADBEEF)).all()
                   for x in e.value.outputs)
    # the context works afterwards
    ra.same(ctx.rowassign(rows, sel, *tb), exp)


CHILD = """import sys, json, numpy as np
sys.path[:0] = [{tests!r}, {pkg!r}]
import pairdist_cases as pc
import rowassign_cases as ra
from dmx import lib
reads, rows, sel, tb, exp, _ = ra.host_set()
with lib.Context(0) as c:
    c.load(pc.pack_reads(reads))
    row, d, cls, n_pairs, n_lines = c.rowassign(rows, sel, *tb)
print(json.dumps({{'lib': lib.LIB_PATH, 'row': row.tolist(), 'd': d.tolist(), 'cls': cls.tolist(),
                  'n': [n_pairs, n_lines]}}))
"""


def test_bounds_build_runs_the_case_set_clean(host_case, tmp_path):
    """The bounds-checked library (the rows, the tables and the places checked in the new
    kernels as every other access is) in a child process: no violation, the host's result."""
    p, rows, sel, tb, exp = host_case
    script = tmp_path / "run.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=PKG))
    env = dict(os.environ, DMX_DEBUG_BOUNDS="1", DMX_PD_CHUNK="53")
    env.pop("DMX_LIBDMX", None)
    res = subprocess.run([sys.executable, str(script)], capture_output=True, text=True,
                         timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["lib"].endswith("libdmx_bounds.so")
    assert out["row"] == exp["best_row"].tolist() and out["d"] == exp["best_d"].tolist()
    assert out["cls"] == exp["best_class"].tolist()
    assert out["n"] == [exp["n_pairs"], exp["n_lines"]]
