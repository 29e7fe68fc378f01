"""GPU parity of view runs (dmx_set_views): the demultiplexer on oriented
sub-ranges of the resident reads.  Per stratum of views_cases.py, and per screen switch that
changes its path, all 40 result bytes of every view and dmx_counts must equal (a) the CPU oracle
on the extracted view strings and (b) the merged path, the same strings packed and run as reads
of their own; a disagreement between (a) and (b) is reported as such."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import views_cases as vc
from dmx import lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")
# the screen switches, set the way tests/test_sweep.py sets them
VARIANTS = {"default": {}, "no_flat": {"DMX_NO_FLAT": "1"}, "no_screen": {"DMX_NO_SCREEN": "1"},
            "no_filter": {"DMX_NO_FILTER": "1"}}


@pytest.fixture(autouse=True)
def _whole_reads_afterwards(ctx):
    """The session's shared context goes back to whole-read runs after every test here."""
    yield
    ctx.clear_views()


def _check(c, got, counts, flags, merged, what):
    exp = c.expected()
    assert len(got) == len(exp) == len(c.views[0]), what
    ab = vc.differing(merged, exp)
    assert len(ab) == 0, f"{what}: references (a) and (b) disagree on {len(ab)} views, first {ab[:10]}"
    bad = vc.differing(got, exp)
    assert len(bad) == 0, f"{what}: {len(bad)} views differ from the oracle, first {bad[:10]}"
    assert len(vc.differing(got, merged)) == 0, what
    a0, a1 = c.n_adapters()
    assert counts.tolist() == vc.counts_of(exp, a0, a1, c.two_round).tolist(), what
    assert flags == 0, f"{what}: pipeline flags {flags}"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", vc.STRATA)
def test_view_run_equals_oracle_and_merged_path(name, variant, ctx, monkeypatch):
    c = vc.case(name)
    if variant == "default":
        got, counts, flags = vc.run_views(ctx, c)
        merged = vc.run_merged(ctx, c)
    else:   # the switches are read in dmx_open, dmx_set_panel and at the run
        for k, v in VARIANTS[variant].items():
            monkeypatch.setenv(k, v)
        with lib.Context(0) as cx:
            got, counts, flags = vc.run_views(cx, c)
            merged = vc.run_merged(cx, c)
    _check(c, got, counts, flags, merged, f"{name} [{variant}]")


def test_single_mode_views(ctx):
    """DMX_MODE_SINGLE on views: round 0 alone (strata M and S with the round-0 panel only)."""
    for name in ("M", "S"):
        full = vc.case(name)
        c = vc.Case(name + "1", full.reads, full.views, full.r0)
        got, counts, flags = vc.run_views(ctx, c)
        _check(c, got, counts, flags, vc.run_merged(ctx, c), name + " single")


def test_identity_views_equal_the_whole_read_run(ctx):
    c = vc.case("I")
    got, counts, _ = vc.run_views(ctx, c)
    ctx.clear_views()
    ctx.exec()
    whole, wcounts = ctx.fetch(), ctx.counts()
    assert len(vc.differing(got, whole)) == 0
    assert counts.tolist() == wcounts.tolist()
    assert len(vc.differing(whole, ctx.run(c.packed()))) == 0


def test_views_fetch_returns_the_list(ctx):
    c = vc.case("S")
    vc.run_views(ctx, c)
    for a, b in zip(ctx.views(), c.views):
        assert a.tolist() == b.tolist()
    ctx.clear_views()
    assert ctx._L.dmx_views_fetch(ctx._h, None, None, None, None, 0) == 0


def _whole_ok(ctx, c):
    exp = vc.Case("whole", c.reads, vc.view_arrays((i, 0, len(s), 0)
                                                   for i, s in enumerate(c.reads)), c.r0, c.r1)
    got = ctx.run(c.packed())
    assert len(vc.differing(got, exp.expected())) == 0


def test_refusals_leave_the_context_usable():
    c = vc.case("I")
    n = len(c.reads)
    L0 = len(c.reads[0])
    one = lambda r, a, b, s: ([r], [a], [b], [s])   # noqa: E731
    with lib.Context(0) as cx:
        c.set_panels(cx)
        with pytest.raises(lib.DmxError, match=r"\(-5\)"):       # no resident batch
            cx.set_views(*one(0, 0, 1, 0))
        _whole_ok(cx, c)
        cx.load(c.packed())
        for bad, why in ((one(n, 0, 1, 0), "outside the batch"), (one(0, 5, 4, 0), "start > stop"),
                         (one(0, 0, L0 + 1, 0), "past its read"), (one(0, 0, 1, 2), "strand"),
                         (one(0, -1, 1, 0), "start < 0")):
            with pytest.raises(lib.DmxError, match=r"\(-1\).*view 0.*" + why):
                cx.set_views(*bad)
            # a refused call sets no list: the next exec is the whole-read run it was before
            cx.exec()
            assert len(vc.differing(cx.fetch(), c.expected())) == 0   # I's views: its reads
        with pytest.raises(lib.DmxError, match=r"\(-1\).*view 2"):   # names the offending view
            cx.set_views([0, 1, n + 3], [0, 0, 0], [1, 1, 1], [0, 0, 0])
        # more than 2^31 views: refused from the count alone, before any array is read
        rc = cx._L.dmx_set_views(cx._h, c.views[0].ctypes.data, c.views[1].ctypes.data,
                                 c.views[2].ctypes.data, c.views[3].ctypes.data, (1 << 31) + 1)
        assert rc == -4
        with pytest.raises(lib.DmxError, match=r"\(-5\)"):       # no dmx_chop_exec on this batch
            cx.chop_views(None, 50)
        _whole_ok(cx, c)
        # linked mode with views set is refused at dmx_exec; the list survives a mode change
        cx.load(c.packed())
        cx.set_views(*c.views)
        cx.set_mode(lib.MODE_LINKED)
        with pytest.raises(lib.DmxError, match=r"\(-4\)"):
            cx.exec()
        c.set_panels(cx)
        cx.exec()
        assert len(vc.differing(cx.fetch(), c.expected())) == 0
        _whole_ok(cx, c)


def test_load_after_set_views_restores_whole_read_results(ctx):
    m, i = vc.case("M"), vc.case("I")
    got, _, _ = vc.run_views(ctx, m)
    assert len(got) == 3 * len(m.reads)
    ctx.load(i.packed())          # dmx_load drops the list
    ctx.exec()
    whole = ctx.fetch()
    assert len(whole) == len(i.reads)
    assert len(vc.differing(whole, i.expected())) == 0      # I's views are its whole reads
    # a smaller two-round batch after the 3-views-per-read run, then views again: the buffers
    # sized by the view count are reused, not outgrown
    got2, counts2, flags2 = vc.run_views(ctx, m)
    assert len(vc.differing(got2, got)) == 0 and flags2 == 0


def test_fetch_is_sized_by_the_exec_not_by_the_list_set_since(ctx):
    """dmx_fetch copies what the last exec computed.  A list cleared or set after the exec
    changes neither the number of results nor the results."""
    m = vc.case("M")
    n = len(m.reads)
    got, _, _ = vc.run_views(ctx, m)              # load; set_views(3n); exec
    ctx.clear_views()
    late = ctx.fetch()                            # ... clear_views; fetch: still 3n results
    assert len(late) == 3 * n and len(vc.differing(late, got)) == 0
    ctx.exec()                                    # load; exec (whole reads) ...
    whole = ctx.fetch()
    assert len(whole) == n
    k = n // 2
    ctx.set_views(*[a[:k] for a in m.views])      # ... set_views(k < n); fetch: still n results
    late = ctx.fetch()
    assert len(late) == n and len(vc.differing(late, whole)) == 0
    ctx.exec()
    assert len(vc.differing(ctx.fetch(), m.expected()[:k])) == 0
    ctx.chop_set(["ACGTACGTACGTACGTACGT"], [], 0.1)
    ctx.chop_exec()
    assert ctx.chop_views(None, 0) == 0           # no rules, no segments: an empty list
    assert len(ctx.fetch()) == k                  # the exec before it ran on k views


def test_bounds_build_reports_no_violation():
    """Strata M, B and E on dmx/libdmx_bounds.so (tests/test_bounds.py's mechanism): every item,
    slot, result and view access of a view run is checked; none may be reported."""
    path = os.path.join(PKG, "dmx", "libdmx_bounds.so")
    assert os.path.exists(path)
    env = dict(os.environ, DMX_DEBUG_BOUNDS="1")
    env.pop("DMX_LIBDMX", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "views_cases.py")],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["lib"] == "libdmx_bounds.so"
    assert set(out["cases"]) == {"M", "B", "E"}
    for name, (bad, n, flags, err) in out["cases"].items():
        assert err == "" and bad == 0 and flags == 0 and n > 0, (name, bad, n, flags, err)
