"""The end-window stage's structure slice on the GPU: the kernels against
dmx_ends_host on the cases of ends_struct_cases.py, which test_ends_struct_host.py pins to the
oracle and to the structure each case claims (queue drains, round-1 views, wide panels, long
reads)."""
import json
import os
import subprocess
import sys

import pytest

import ends_cases as ec
import ends_struct_cases as sc
from dmx import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
Q_IDS = [f"{sc.NAMES[w]}-e{e}" for w, e in sc.Q_SPECS]


@pytest.mark.parametrize("spec", sc.Q_SPECS, ids=Q_IDS)
def test_q_mid_loop_drains(ctx, spec):
    """12 loop steps in each of the 2048 blocks, three or more mid-loop drains in most of them
    (test_q_plan_drains_the_queue_in_every_block): the records of the 600 distinct reads, tiled.
    -e 0.3 is a ring round, so ends_kernel<1> drains its queue the same way: costs above 7 are
    accepted and the band key's overflow flag (2) stays clear."""
    where, e = spec
    reps = sc.q_reps()
    got, exp = sc.run_q(ctx, where, e, reps)
    n = reps * sc.Q_BASE
    assert len(got) == n >= 8 * sc.ENDS_GRID * sc.ENDS_BLOCK // 48
    assert len(ec.same_records(got, exp)) == 0
    st = ctx.stats()
    assert st["flags"] == 0
    planned = int(sc.q_accepted(where, e).sum()) * reps
    assert st["ends_seen"][0] == n * 48
    assert planned <= st["ends_dp"][0] < st["ends_seen"][0]
    assert ((got["m1_errors"] > 7).sum() > 0) == (e > 0.25)
    cnt = lib.bin_totals(ctx.counts(), 24, 0)[:, 0]
    assert cnt.tolist() == [int((got["bin1"] == b).sum()) for b in range(-1, 24)]


@pytest.mark.parametrize("r", sc.Q_TAILS)
@pytest.mark.parametrize("where", ec.RESTRICTED, ids=[sc.NAMES[w] for w in ec.RESTRICTED])
def test_q_last_block_step(ctx, where, r):
    """The last block-step holds 1, 127, 128 or 129 (128 + 1) triples; the grid is below
    kEndsGrid, so every block makes one step and drains after the loop."""
    seqs, rc, n = sc.q_tail_case(where, r)
    reads = sc.q_tail_reads(where, n)
    blob, offs, lens = ec.oracle.pack_ascii(reads)
    p = lib.pack(blob, offs, lens)
    wheres = [where] * len(seqs)
    ctx.set_panel_ex(0, seqs, wheres, rc, 0.2, 3)
    ctx.set_mode(lib.MODE_SINGLE)
    got = ctx.run(p)
    assert len(ec.same_records(got, lib.ends_host(seqs, wheres, p, rc, 0.2, 3))) == 0
    st = ctx.stats()
    assert st["flags"] == 0 and st["ends_seen"][0] == n * len(seqs) * (2 if rc else 1)
    assert 0 < st["ends_dp"][0] < st["ends_seen"][0]


@pytest.mark.parametrize("name", sc.R_NAMES)
def test_r_round_one_over_item_views(ctx, name):
    """DMX_MODE_TWO_ROUND against two single rounds of the host twin on reads trimmed in Python,
    then a second dmx_exec on the resident batch."""
    c = sc.r_case(name)
    bad, n, flags = sc.run_case(ctx, c)
    assert (bad, flags) == (0, 0), f"{bad} of 2 x {n} records differ, pipeline flags {flags}"
    exp = c.host()
    assert (exp["bin2"] >= 0).sum() > 20 and exp["rc1"].sum() > 50


@pytest.mark.parametrize("name", sc.W_NAMES)
def test_w_wide_panels(ctx, name):
    c = sc.w_case(name)
    bad, n, flags = sc.run_case(ctx, c)
    assert (bad, flags) == (0, 0), f"{bad} of {n} records differ, pipeline flags {flags}"
    st = ctx.stats()
    n_restricted = sum(w in ec.RESTRICTED for w in c.r0[1])
    assert st["ends_seen"][0] == n * n_restricted * 2
    cnt = lib.bin_totals(ctx.counts(), len(c.r0[0]), 0)[:, 0]
    assert cnt.tolist() == [int((c.host()["bin1"] == b).sum()) for b in range(-1, len(c.r0[0]))]


@pytest.mark.parametrize("e", sc.L_E)
def test_l_long_reads(ctx, e):
    c = sc.l_case(e)
    bad, n, flags = sc.run_case(ctx, c)
    assert (bad, flags) == (0, 0), f"{bad} of {n} records differ, pipeline flags {flags}"
    st = ctx.stats()     # (a 26-nt read has no room for the 36-nt A$)
    assert 0 < st["ends_dp"][0] < st["ends_seen"][0] <= n * 8


def test_bounds_checked_library():
    """Strata R, W and L, and Q at two loop steps per block, under DMX_DEBUG_BOUNDS=1
    (dmx/libdmx_bounds.so) in a child process: no violation, the host twin's records."""
    env = dict(os.environ, DMX_DEBUG_BOUNDS="1")
    env.pop("DMX_LIBDMX", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ends_struct_cases.py")],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["lib"] == "libdmx_bounds.so"
    assert (out["err"], out["bad"], out["flags"]) == ("", 0, 0), out
    assert out["n"] > 8 * sc.q_reps(2) * sc.Q_BASE
