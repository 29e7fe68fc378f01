"""The random-panel parity slice on the host (sweep_cases.py; no GPU).

The census re-derives every fixed case's class from the library's host accessors
(dmx_panel_pieces / dmx_panel_near_shared / dmx_panel_reach) and asserts the strata table: it is
what keeps the slice on the screen paths when the generator or build_pieces changes (a uniform
draw spends 9 cases of 10 on the plain full scan).  If a case leaves its stratum, fix the recipe
that shapes its draw in sweep_cases.py, never the quota.  The other tests are statements about the
inputs, made with the oracle alone: every case matches reads, the piece-screen cases match
through K-edit copies on both strands, the cases are replayable one by one, and the two
formulations of the oracle agree on these panel shapes."""
import collections

import numpy as np
import pytest

import oracle
import pyref
import sweep_cases as sw
from dmx import lib

TABLE = {"plain": 6, "filter": 6, "step1": 4, "step2": 4, "step4": 4, "near": 4, "near_off": 2,
         "mixed": 3, "pair2": 4, "linked": 3}
STEPS = ("step1", "step2", "step4")


@pytest.fixture(scope="module")
def cases():
    return sw.fixed_cases()


@pytest.fixture(scope="module")
def answers(cases):
    return {c["id"]: sw.expected(c) for c in cases}


def _host(case):
    """(near_shared info, piece info, entries, reach status) of the case's first panel."""
    seqs, wh = case["panels"][0], case["wheres"][0]
    lw = [lib.DMX_FRONT if w == oracle.FRONT else lib.DMX_BACK for w in wh]
    mixed = len(set(lw)) > 1
    flags = (lib.DMX_FRONT if mixed else lw[0]) | (lib.DMX_RC if case["rc"] else 0)
    a = (seqs, flags, case["e"], case["min_overlap"])
    r1, near = lib.panel_near_shared(*a, wheres=lw if mixed else None)
    r2, _ = lib.panel_reach(*a, wheres=lw if mixed else None)
    assert r1 == 0 and r2 == 0, case["id"]
    if mixed:
        return near, {"step": 0, "part_max": 0}, [], lw
    r3, info, ents = lib.panel_pieces(*a)
    assert r3 == 0, case["id"]
    return near, info, ents, lw


def test_census(cases):
    assert collections.Counter(c["stratum"] for c in cases) == TABLE
    assert len({c["id"] for c in cases}) == len(cases) == sum(TABLE.values())
    first_off = {}    # case id: the largest first sampled offset j0 of a piece
    for c in cases:
        near, info, ents, lw = _host(c)
        st, cid = c["stratum"], c["id"]
        front = lw[0] == lib.DMX_FRONT
        uniform = len(set(lw)) == 1
        if st == "plain":
            assert uniform and near["filter_len"] == 0 and info["step"] == 0, cid
        elif st == "filter":
            assert uniform and near["filter_len"] > 0 and info["step"] == 0, cid
            wild = any(ch not in "ACGT" for s in c["panels"][0] for ch in s)
            short = any(sw.min_piece(len(s), c["e"], c["min_overlap"]) < 8 for s in c["panels"][0])
            assert wild or short, cid
        elif st in STEPS:
            assert info["step"] == int(st[4:]) and near["filter_len"] > 0, cid
            assert 64 <= info["part_max"] <= 768 and info["entries"] == len(ents) > 0, cid
            j0 = {}
            for e in ents:
                key = (e["val"], e["len"], e["o"])
                j0[key] = min(j0.get(key, 9), e["off"])
            first_off[cid] = (max(j0.values()), max(e["off"] for e in ents))
        elif st == "near":
            assert uniform and front and near["near_shared"] >= 0, cid
        elif st == "near_off":
            assert uniform and front and near["filter_len"] > 0 and near["near_shared"] == -1, cid
        elif st == "mixed":
            assert set(lw) == {lib.DMX_FRONT, lib.DMX_BACK} and near["filter_len"] == 0, cid
        else:
            assert len(c["panels"]) == 2 and c["kind"] == ("pair" if st == "pair2" else "linked")
            assert set(c["wheres"][0]) == {oracle.FRONT} and set(c["wheres"][1]) == {oracle.BACK}
    plain = [c for c in cases if c["stratum"] == "plain"]
    assert any(c["e"] in (1.0, 2.0, 3.0, 4.0) for c in plain)
    assert any(c["e"] == 0.0 for c in plain)
    assert {1, 12} <= {c["min_overlap"] for c in plain}
    assert {w for c in plain for w in c["wheres"][0]} == {oracle.FRONT, oracle.BACK}
    steps = [c for c in cases if c["stratum"] in STEPS]
    # a piece whose sampled window starts past offset 0 (it straddles a shared block), and, with
    # a step below 4 (whose windows are 0 .. 3 anyway), one that reaches offset 3: the branch
    # of the sweep's seed-56 table bug
    assert sum(j0 > 0 for j0, _ in first_off.values()) >= 3, first_off
    assert sum(top == 3 and not cid.startswith("step4") for cid, (_, top) in first_off.items()) \
        >= 2, first_off
    assert any(c["e"] == 0.0 for c in steps)
    assert any(c["wheres"][0][0] == oracle.BACK for c in steps)
    assert all(c["rc"] for c in steps)
    # the near and pair2 cases that the piece-screen variants of test_sweep.py count on
    assert sum(sw.classify(c)[0]["step"] > 0 for c in cases if c["stratum"] == "near") >= 2
    assert any(all(x["step"] > 0 for x in sw.classify(c)) for c in cases
               if c["stratum"] == "pair2")
    # the index screen (a shared prefix and suffix: jsplit > 0) is in reach of its variants
    for st in ("filter", "step2", "near"):
        assert any(sw.classify(c)[0]["jsplit"] > 0 for c in cases if c["stratum"] == st), st


def test_reads_of_every_case(cases):
    for c in cases:
        reads, cid = c["reads"], c["id"]
        assert 300 <= len(reads) <= 500, cid
        assert "" in reads and any(len(r) == 1 for r in reads), cid
        ads = [s for p in c["panels"] for s in p]
        assert any(r in (a[:7] for a in ads) for r in reads), cid
        assert any(r in (a[-7:] for a in ads) for r in reads), cid
        if c["stratum"] in STEPS:
            pmax = _host(c)[1]["part_max"]
            assert np.mean([len(r) > 2 * pmax for r in reads]) >= 0.2, cid


def test_every_case_matches_reads(cases, answers):
    """Computed from the oracle alone.  plain-4 (an absolute -e over a panel with 20 % IUPAC)
    fell short of the quarter with reads_for's 0 .. 2 copies per read and takes 1 .. 2
    (sweep_cases.MORE_COPIES)."""
    for c in cases:
        exp = answers[c["id"]]
        hit = exp["bin1" if c["kind"] == "single" else "bin2"] >= 0
        assert hit.any(), c["id"]
        if c["e"] >= 0.05:
            assert hit.mean() >= 0.25, (c["id"], hit.mean())


def test_step_cases_match_k_edit_copies_on_both_strands(cases, answers):
    for c in cases:
        if c["stratum"] not in STEPS:
            continue
        exp = answers[c["id"]]
        assert c["k_copies"], c["id"]
        assert any(exp["bin1"][i] == a and exp["m1_errors"][i] == K
                   for i, _, a, K, _ in c["k_copies"]), c["id"]
        hit = exp["bin1"] >= 0
        assert (hit & (exp["rc1"] == 0)).any() and (hit & (exp["rc1"] == 1)).any(), c["id"]
        for place in range(3):   # start, middle, end of the read: each adapter has all three
            assert {a for n, (_, _, a, _, _) in enumerate(c["k_copies"]) if n % 3 == place} == \
                set(range(len(c["panels"][0]))), c["id"]
        assert {s for *_, s in c["k_copies"]} == {0, 1}, c["id"]


def test_cases_are_replayable(cases):
    again = sw.fixed_cases()
    assert [c["id"] for c in again] == [c["id"] for c in cases] == sw.fixed_ids()
    for a, b in zip(cases, again):
        assert a["panels"] == b["panels"] and a["wheres"] == b["wheres"], a["id"]
        assert "\n".join(a["reads"]).encode() == "\n".join(b["reads"]).encode(), a["id"]
    for i in (0, 7, 13, 19, 27, 33, 39):   # a case alone, before any other draw of its stratum
        alone = sw.case_by_id(cases[i]["id"])
        assert alone == cases[i]
    rng_free = sw.sweep_case(5, 3)
    assert rng_free["reads"] == sw.sweep_case(5, 3)["reads"] and rng_free["id"] == "5:3"


def _cut(read, exp_row, width=120):
    """The read cut to `width` nt around the oracle's match (its start, when there is none)."""
    n = len(read)
    if n <= width:
        return read
    lo = 0
    if exp_row["bin1"] >= 0:
        a, b = int(exp_row["m1_rstart"]), int(exp_row["m1_rstop"])
        if exp_row["rc1"]:
            a, b = n - b, n - a
        lo = min(max(0, (a + b) // 2 - width // 2), n - width)
    return read[lo:lo + width]


@pytest.mark.parametrize("stratum", ["filter", "step2", "near", "mixed"])
def test_oracle_formulations_agree_on_these_shapes(stratum, cases, answers):
    """tests/test_oracle.py compares oracle.locate with pyref.locate on single unrelated adapters
    only (no shared flanks, no mixed panel, no --rc round), so nothing here repeats it: one case
    of the stratum, at most 40 reads cut to 120 nt around the match, every result field of the C
    oracle's round against the full-matrix restatement."""
    c = next(x for x in cases if x["stratum"] == stratum)
    exp = answers[c["id"]]
    seqs, wh = c["panels"][0], c["wheres"][0]
    cells = sum(len(s) for s in seqs) * 120 * (2 if c["rc"] else 1)
    n = int(min(40, max(8, 1_500_000 // cells)))
    pick = np.random.default_rng(1).permutation(len(c["reads"]))[:n]
    sub = [_cut(c["reads"][i], exp[i]) for i in pick]
    blob, offs, lens = oracle.pack_ascii(sub)
    got = oracle.run_batch(oracle.Panel(seqs, wh, max_errors=c["e"], min_overlap=c["min_overlap"]),
                           None, blob, offs, lens, mode=0, use_rc=c["rc"])
    matched = 0
    for s, g in zip(sub, got):
        a, is_rc, mt, _ = pyref.demux_round(seqs, wh, s, c["rc"], c["e"], c["min_overlap"])
        mt = mt if a >= 0 else (0,) * 6
        want = (a, -1, int(is_rc), 0, 0, 0, mt[2], mt[3], mt[0], mt[1], mt[4], mt[5]) + (0,) * 6
        assert tuple(int(x) for x in g.tolist()) == want, (c["id"], s)
        matched += a >= 0
    assert matched >= n // 4, (c["id"], matched, n)
