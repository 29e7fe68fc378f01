"""dmx_groupalign_strands (a strand per member: groupalign_strands_kernel's reversed query masks,
groupalign_merge_kernel's reversed symbols) on the GPU against the host path, which
test_groupalign_strands_host.py pins to the unflagged code on physically turned reads; and
sorter.make_consensus on the GPU against its host route."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import groupalign_cases as gc
import groupalign_strand_cases as sc
import pairdist_cases as pc
import test_groupalign_strands_host as th
from dmx import lib, sorter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nanopore-barcoding-orc_amd")


@pytest.mark.parametrize("name,kind", sc.RUNS)
def test_kernels_equal_the_host(ctx, name, kind):
    case, exp = sc.expected(name)
    _, seeds, groups, strands = case
    ctx.load(sc.packed(case, kind))
    got = ctx.groupalign(seeds, groups, paths=True, strands=strands)
    gc.same_result(got, exp)
    st = ctx.groupalign_stats()
    assert st["rounds"] == max(len(g) for g in groups) and st["launches"] == st["rounds"]
    # a second run is identical; without paths the columns are the same
    gc.same_result(ctx.groupalign(seeds, groups, paths=True, strands=strands), got)
    plain = ctx.groupalign(seeds, groups, strands=strands)
    assert "ops" not in plain
    for key in ("col_off", "mask", "count", "first", "dist"):
        np.testing.assert_array_equal(plain[key], exp[key])


def test_a_bad_flag_is_refused_and_the_context_stays_usable(ctx):
    case, exp = sc.expected("uneven")
    _, seeds, groups, strands = case
    ctx.load(sc.packed(case, "normal"))
    bad = [list(s) for s in strands]
    bad[2][1] = 2
    with pytest.raises(lib.DmxError, match=r"\(-1\).*group 2.*member 1.*flag"):
        ctx.groupalign(seeds, groups, paths=True, strands=bad)
    st = ctx.groupalign_stats()
    assert st["rounds"] == 0 and st["forward"] == 0.0      # nothing was launched
    gc.same_result(ctx.groupalign(seeds, groups, paths=True, strands=strands), exp)


CHILD = """import sys, json, numpy as np
sys.path[:0] = [{tests!r}, {pkg!r}]
import groupalign_strand_cases as sc
from dmx import lib
same, launches, rounds = True, 0, 0
with lib.Context(0) as c:
    for name, kind in {runs!r}:
        case, exp = sc.expected(name)
        c.load(sc.packed(case, kind))
        got = c.groupalign(case[1], case[2], paths=True, strands=case[3])
        st = c.groupalign_stats()
        launches += st['launches']
        rounds += st['rounds']
        for key in ('col_off', 'mask', 'count', 'first', 'dist', 'op_off', 'ops'):
            same = same and got[key].tobytes() == exp[key].tobytes()
print(json.dumps({{'lib': lib.LIB_PATH, 'same': bool(same), 'launches': launches,
                  'rounds': rounds}}))
"""


def run_child(runs, tmp_path, env):
    script = tmp_path / "run.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=PKG, runs=list(runs)))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_chunked_by_trace_budget_in_a_child_process(tmp_path):
    """DMX_PA_TRACE_MB=1 cuts both rounds of the budget case (over 2 MiB of trace each) into
    several launches; the stripe and length cases ride along: identical output."""
    env = dict(os.environ, DMX_PA_TRACE_MB="1")
    env.pop("DMX_DEBUG_BOUNDS", None)
    res = run_child([("budget", "normal"), ("stripes", "normal"), ("lengths", "tight")], tmp_path,
                    env)
    assert res["same"] and res["launches"] >= res["rounds"] + 2, res


def test_bounds_build_runs_every_case_clean(tmp_path):
    """The bounds-checked library in a child process, the tight-pack cases included (a reversed
    last word of read 0 at offset 16): no violation, the host's result."""
    env = dict(os.environ, DMX_DEBUG_BOUNDS="1")
    env.pop("DMX_LIBDMX", None)
    res = run_child(sc.RUNS, tmp_path, env)
    assert res["lib"].endswith("libdmx_bounds.so") and res["same"], res


def test_make_consensus_on_the_gpu_equals_the_host(ctx):
    reads, groups, _, _ = th.mixed_bin()
    exp = sorter.make_consensus(None, reads, groups)
    assert sorter.make_consensus(ctx, reads, groups) == exp
    st = ctx.groupalign_stats()
    assert st["merge"] > 0 and st["rounds"] > 0


def edit_distance(a: str, b: str) -> int:
    return int(pc.np_dist([a.encode()], [b.encode()], lib.PD_NW)[0])


@functools.lru_cache(maxsize=None)
def two_family_bin():
    """Two unrelated families of 300 and 320 nt, 20 reads each at 2..6 % errors, interleaved, a
    seeded half reverse-complemented."""
    rng = np.random.default_rng(191)
    fam = [pc.rand_seq(rng, 300, p_n=0.0), pc.rand_seq(rng, 320, p_n=0.0)]
    reads = []
    for k in range(40):
        r = pc.mutate(rng, fam[k % 2], float(rng.uniform(0.02, 0.06)))
        r = r.replace(b"N", b"A")
        reads.append(pc.revcomp(r) if rng.random() < 0.5 else r)
    return fam, reads


def test_similarity_to_gene_groups_to_consensus_on_one_batch(ctx):
    """End to end: gene groups of a mixed-strand bin, then make_consensus of those groups.

    Measured on the host route (ctx=None) on this bin: two groups of 20 reads, one per family;
    the 320-nt family's consensus (320 nt) is at edit distance 0 from the family's reverse
    complement (167 from the family itself: its anchor is a turned read), the 300-nt family's
    (300 nt) at distance 0 from the family (161 from its reverse complement).  No threshold is
    invented: the host route's distances are computed here first, and the GPU must give the
    host route's strings exactly."""
    fam, reads = two_family_bin()
    hgroups = sorter.gene_groups(None, reads, minlength=0)
    hcons = sorter.make_consensus(None, reads, hgroups)
    dist = []
    for c in hcons:
        dist.append(min(min(edit_distance(c, f.decode()), edit_distance(c, pc.revcomp(f).decode()))
                        for f in fam))
    print("host route: groups", [len(g) for g in hgroups], "consensus lengths",
          [len(c) for c in hcons], "edit distance to the nearer family strand", dist)
    groups = sorter.gene_groups(ctx, reads, minlength=0)
    assert [g.tolist() for g in groups] == [g.tolist() for g in hgroups]
    cons = sorter.make_consensus(ctx, reads, groups)
    assert cons == hcons
    assert len(cons) == 2 and sorted(len(g) for g in groups) == [20, 20]
    # each consensus is as near its family (either strand) as the host route's is
    assert [min(min(edit_distance(c, f.decode()), edit_distance(c, pc.revcomp(f).decode()))
                for f in fam) for c in cons] == dist
