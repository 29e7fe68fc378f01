"""The end-window stage's structure slice on the host (no GPU): dmx_ends_host
against the Python demux oracle on the distinct reads of every stratum of ends_struct_cases.py,
and the conditions that make each stratum the case it claims to be: the queue plan of Q, the
coverage of R, every winner of W, the window starts of L."""
import os
import re

import numpy as np
import pytest

import ends_cases as ec
import ends_struct_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_IDS = [f"{sc.NAMES[w]}-e{e}" for w, e in sc.Q_SPECS]


def _same(got, exp, what, reads):
    bad = ec.same_records(got, exp)
    assert len(bad) == 0, (what, len(bad), reads[bad[0]][:120], got[bad[0]], exp[bad[0]])


def test_mirrored_constants_are_the_kernels():
    """ENDS_BLOCK and ENDS_GRID are what csrc/dmx_ends.hip says: a retuned kernel moves the
    block-steps the plan below counts, and has to fail here first."""
    src = open(os.path.join(ROOT, "nanopore-barcoding-orc_amd", "csrc", "dmx_ends.hip")).read()
    vals = {}
    for name in ("kEndsBlock", "kEndsGrid"):
        rhs = re.findall(rf"^constexpr int {name} = ([0-9 *]+);", src, flags=re.M)
        assert len(rhs) == 1, name
        vals[name] = int(np.prod([int(x) for x in rhs[0].split("*")]))
    assert vals == {"kEndsBlock": sc.ENDS_BLOCK, "kEndsGrid": sc.ENDS_GRID}
    assert re.search(r"s_qi\[2 \* kEndsBlock\], s_qs\[2 \* kEndsBlock\]", src)
    assert sc.QUEUE_CAP == 2 * sc.ENDS_BLOCK


def test_shared_panel_shape():
    seqs = sc.shared_panel()
    assert len(set(seqs)) == 24 and {len(s) for s in seqs} == {30}
    assert len({s[:25] for s in seqs}) == 1 and len({s[25:29] for s in seqs}) == 24
    assert (sc.panel_kk(0.2, 30), sc.panel_kk(0.3, 30)) == (6, 9)


@pytest.mark.parametrize("spec", sc.Q_SPECS, ids=Q_IDS)
def test_q_host_twin_equals_the_oracle(spec):
    where, e = spec
    base = list(sc.q_base(where, e))
    assert len(set(base)) == sc.Q_BASE and 45 <= min(map(len, base)) and max(map(len, base)) <= 90
    host = sc.q_host(where, e)
    _same(host, ec.demux(list(sc.shared_panel()), [where] * 24, base, True, e, 3), spec, base)
    assert 0.65 < (host["bin1"] >= 0).mean() and 0.25 < host["rc1"].mean() < 0.6
    assert set(host["bin1"].tolist()) >= set(range(24))
    # the ring round shows on the GPU as costs above kBandMaxCost = 7 without the band flag
    assert (host["m1_errors"] > 7).sum() >= (5 if e > 0.25 else 0)
    assert (host["m1_errors"] > 7).sum() == 0 or e > 0.25


@pytest.mark.parametrize("spec", sc.Q_SPECS, ids=Q_IDS)
def test_q_plan_drains_the_queue_in_every_block(spec):
    """A condition on the input, from the exact DP's accepted triples alone (each of them
    passes the prefilter, so the kernel's queues hold at least these): every block makes
    Q_STEPS loop steps and at least two mid-loop drains, half of the blocks drain above a
    residual, and some queue fills beyond three quarters."""
    acc = sc.q_accepted(*spec)
    # a carrier's copy is within k edits of all 24 adapters (the tails differ in <= 5 places):
    # the whole panel runs the DP in the carrying orientation (not the ten 8-error carriers)
    assert acc.all(axis=2).any(axis=1).mean() >= 0.68
    p = sc.q_plan(acc, sc.q_reps())
    assert p["grid"] == sc.ENDS_GRID and p["steps"] >= sc.Q_STEPS >= 8
    assert p["total"] >= 8 * sc.ENDS_GRID * sc.ENDS_BLOCK
    assert p["per_block"].min() >= 3 * sc.ENDS_BLOCK
    assert p["drains"].min() >= 2
    assert p["partial"].mean() >= 0.5
    assert 192 < p["peak"].max() <= sc.QUEUE_CAP
    small = sc.q_plan(acc, sc.q_reps(2))     # the bounds-checked run: two steps, drains too
    assert small["steps"] >= 2 and small["drains"].sum() > 0


@pytest.mark.parametrize("r", sc.Q_TAILS)
@pytest.mark.parametrize("where", ec.RESTRICTED, ids=[sc.NAMES[w] for w in ec.RESTRICTED])
def test_q_tail_edge_cases(where, r):
    seqs, rc, n = sc.q_tail_case(where, r)
    total = n * len(seqs) * (2 if rc else 1)
    assert total % sc.ENDS_BLOCK == r % sc.ENDS_BLOCK and total > sc.ENDS_BLOCK + r
    assert -(-total // sc.ENDS_BLOCK) < sc.ENDS_GRID
    reads = sc.q_tail_reads(where, n)
    host = ec.host_round(seqs, [where] * len(seqs), reads, rc, 0.2, 3)
    _same(host, ec.demux(seqs, [where] * len(seqs), reads, rc, 0.2, 3), (where, r), reads)
    assert (host["bin1"][-3:] >= 0).any() or (host["bin1"] >= 0).mean() > 0.3


@pytest.mark.parametrize("name", sc.R_NAMES)
def test_r_host_twin_equals_the_oracle(name):
    c = sc.r_case(name)
    assert 240 <= len(c.reads) <= 400
    _same(c.host(), c.oracle(), name, c.reads)
    exp = c.host()
    assert (exp["bin1"] >= 0).mean() > 0.7 and 0.3 < exp["rc1"].mean() < 0.7


def test_r_covers_every_stratum():
    missing = sc.r_required() - sc.r_coverage()
    assert not missing, sorted(map(str, missing))


def test_r_rounds_are_what_the_cases_say():
    """Band and ring rounds, the remap and the per-orientation slots, from the panels."""
    for name in sc.R_NAMES:
        c = sc.r_case(name)
        kk0 = max(sc.panel_kk(c.r0[3], len(s)) for s in c.r0[0])
        kk1 = max(sc.panel_kk(c.r1[3], len(s)) for s in c.r1[0])
        assert kk0 <= 7 and (kk1 > 7) == (name == "ring"), name
    m = sc.r_case("mixed").r1
    assert m[1] == [ec.B, ec.SUFFIX, ec.B, ec.BACKX] and m[0][1] == m[0][2]
    exp = sc.r_case("oslot").host()
    assert (exp["m2_score"][exp["bin2"] >= 0] <= 0).any()     # the panel accepts score <= 0
    exp = sc.r_case("tiny_e1").host()
    assert (exp["m2_score"][exp["bin2"] >= 0] < 0).any()


@pytest.mark.parametrize("name", sc.W_NAMES)
def test_w_host_twin_equals_the_oracle_and_every_adapter_wins(name):
    c = sc.w_case(name)
    seqs, wheres, rc, e, o = c.r0
    assert 450 <= len(c.reads) <= 550 and rc
    _same(c.host(), c.oracle(), name, c.reads)
    exp = c.host()
    wins = np.bincount(exp["bin1"][exp["bin1"] >= 0], minlength=len(seqs))
    assert (wins > 0).all(), np.nonzero(wins == 0)[0]
    assert exp["rc1"].sum() > 100 and (exp["bin1"] < 0).sum() >= 1
    n_restricted = sum(w in ec.RESTRICTED for w in wheres)
    if name.startswith("shared"):
        assert len(seqs) == 48 and set(seqs) == set(sc.shared_panel())
    else:
        assert len(seqs) == 64 and n_restricted == (64 if name == "wide64" else 32)
    if name == "wide64":
        assert [wheres.count(w) for w in ec.RESTRICTED] == [16] * 4
        assert seqs[0] == seqs[63] and (wheres[0], wheres[63]) == (ec.PREFIX, ec.FRONTX)
        tie = [i for i, lab in enumerate(c.labels) if lab == "tie_0_63"]
        assert len(tie) >= 4 and (exp["bin1"][tie] == 0).all()
        for i in tie:   # a tie indeed: index 63 alone gives the same score and errors
            alone = ec.host_round([seqs[63]], [wheres[63]], [c.reads[i]], True, e, o)[0]
            assert (alone["m1_score"], alone["m1_errors"]) == \
                (exp["m1_score"][i], exp["m1_errors"][i])
    if name == "mixed64":    # the remap moves every regular index
        assert all(w == ec.F for w in wheres[1::2]) and all(w in ec.RESTRICTED for w in wheres[::2])


@pytest.mark.parametrize("e", sc.L_E)
def test_l_host_twin_equals_the_oracle(e):
    c = sc.l_case(e)
    seqs, wheres, rc, _, o = c.r0
    assert 120 <= len(c.reads) <= 180
    assert sorted({len(r) for r in c.reads if len(r) > 100}) == list(sc.L_LENS)
    _same(c.host(), c.oracle(), c.name, c.reads)
    exp = c.host()
    assert (sc.panel_kk(e, 40) > 7) == (e == 0.25)
    # the layout: lib.pack's first offset, then every residue the gather distinguishes
    assert c.offsets[0] == sc.lib.PACK_PAD
    assert {x % 16 for x in c.offsets[1:]} == {0, 1, 15}
    assert all(b - (a + len(r)) >= 16 for a, b, r in zip(c.offsets, c.offsets[1:], c.reads))
    for n in sc.L_LENS:
        idx = [i for i, lab in enumerate(c.labels) if lab == f"len_{n}"]
        won = {(wheres[exp["bin1"][i]], int(exp["rc1"][i])) for i in idx if exp["bin1"][i] >= 0}
        assert won == {(w, s) for w in ec.RESTRICTED for s in (0, 1)}, n
        for i in idx:   # a 3' match ends on the read's last column
            if exp["bin1"][i] >= 0 and wheres[exp["bin1"][i]] & ec.B:
                assert exp["m1_rstop"][i] == n
    # window starts j0 = len - (m + k) of 0, 1 and 16 for this setting's k, both 3' types
    for a in (2, 3):
        k = sc.panel_kk(e, len(seqs[a]))
        for extra in (0, 1, 16):
            idx = [i for i, lab in enumerate(c.labels) if lab == f"j0_{k}_{extra}" and
                   len(c.reads[i]) == len(seqs[a]) + k + extra]
            assert len(idx) == 2 and all(exp["bin1"][i] == a for i in idx), (a, extra)
            assert {int(exp["rc1"][i]) for i in idx} == {0, 1}


def test_pack_at_equals_lib_pack():
    """ec._pack_at at lib.pack's own offsets gives lib.pack's words (N included)."""
    rng = np.random.default_rng([sc.SEED, 400])
    reads = [ec._rand(rng, n, "ACGT" * 4 + "N") for n in (0, 1, 31, 32, 33, 700, 64)]
    blob, offs, lens = ec.oracle.pack_ascii(reads)
    p = sc.lib.pack(blob, offs, lens)
    q = ec._pack_at(reads, [int(x) for x in p.offsets])
    n = min(len(p.seq2b), len(q.seq2b))
    used = np.zeros(n * 16, dtype=bool)
    for o, r in zip(p.offsets, reads):
        used[int(o):int(o) + len(r)] = True
    uw = used.reshape(n, 16).all(axis=1)
    assert uw.sum() > 40 and (p.seq2b[:n][uw] == q.seq2b[:n][uw]).all()
    host_p = sc.lib.ends_host(["ACGTAC"], [ec.BACKX], p, True, 0.2, 3)
    host_q = sc.lib.ends_host(["ACGTAC"], [ec.BACKX], q, True, 0.2, 3)
    assert len(ec.same_records(host_p, host_q)) == 0
