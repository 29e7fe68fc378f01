"""The chop kernels' structure cases (tests/chop_seam_cases.py) are in the classes
they claim: shown on the CPU from the oracle (oracle/chopper.py) and a plain numpy column DP.
The GPU half is tests/test_chop_seams.py."""
import math

import numpy as np

import chop_seam_cases as cc
import chopper as ochop


def test_column_dp_matches_the_python_oracle():
    rng = np.random.default_rng(5)
    seen = 0
    for _ in range(300):
        m = int(rng.integers(1, 12))
        pat = cc.rand(rng, m, "ACGTACGTRYSWKMBDHVN")
        read = cc.rand(rng, rng.integers(0, 40), "ACGTACGTACGTNacgt")
        if rng.random() < 0.5:
            p = int(rng.integers(0, len(read) + 1))
            read = read[:p] + "".join(ochop._IUPAC[c][0] for c in pat) + read[p:]
        cutoff = float(rng.choice([0.0, 0.2, 0.5, 0.9]))
        D = cc.dp_cols(pat, read)
        assert D[0] == m and len(D) == len(read) + 1
        k = int(cutoff * m)
        best = int(D[1:].min()) if len(read) else m + 1
        exp = [(int(j), best) for j in np.flatnonzero(D[1:] == best) + 1] if best <= k else []
        assert [(b, d) for _, b, d in ochop.hits_py(pat, read, cutoff)] == exp, (pat, read)
        seen += bool(exp)
        # a start no earlier than column f: the DP of the read's tail
        f = int(rng.integers(0, len(read) + 1))
        assert cc.dp_cols(pat, read, f)[f:].tolist() == cc.dp_cols(pat, read[f:]).tolist()
    assert seen > 100


def test_cases_are_rebuilt_alone_from_their_ids():
    assert len(set(cc.NAMES)) == len(cc.NAMES)
    ids = [cc.a_id(s) for s in cc.a_specs()]
    assert len(set(ids)) == len(ids)
    for idx in (0, 101, len(ids) - 1):
        assert cc.a_case.__wrapped__(idx)[0] == cc.a_case(idx)[0]
    for name in ("B/nstretch", "C/513", "G/redo"):
        assert cc.batch.__wrapped__(name)["seqs"] == cc.batch(name)["seqs"]
    for letter in "ABCDEFG":
        assert cc.stratum(letter)


def test_seam_cases_hit_their_columns():
    """Stratum A, every case: the DP puts the label's minimum on the designed column at the
    designed cost, the oracle reports that hit, and no column further than k from it has
    D <= k.  The census: every panel reaches its chop_kernel<HB> variant, every kind, seam,
    offset and edit kind occurs, and the cases that tell the two seam mutations apart exist."""
    specs = cc.a_specs()
    kinds = {}
    wu_witness = {}
    for idx, spec in enumerate(specs):
        panel, cutoff, kind, lab, s0, d, e, ek = spec
        read, pat, k, stop, D = cc.a_case(idx)
        m = len(pat)
        assert k == int(cutoff * m) and len(read) <= 1100
        assert int(D[stop]) == e == int(D[1:].min()) <= k, cc.a_id(spec)
        assert stop in [b for _, b, dd in ochop.hits_c(pat, read, cutoff) if dd == e], cc.a_id(spec)
        low = np.flatnonzero(D[1:] <= k) + 1
        assert int(np.abs(low - stop).max()) <= k, cc.a_id(spec)
        if kind in ("stop", "left", "right"):
            assert stop == s0 + d
        if kind == "warm":
            assert stop - (m + k) == s0 - (m + k) + d and e == k
            # the lane of (s0, s0 + 512] warms up from s0 - (m + k); from s0 - m alone it
            # would read a higher cost on its first column
            if stop == s0 + 1 and int(cc.dp_cols(pat, read, s0 - m)[stop]) > k:
                wu_witness.setdefault(panel, []).append(cc.a_id(spec))
        if kind in ("left", "right"):
            assert k >= 2 and D[s0] <= k and D[s0 + 1] <= k
            at_min = np.flatnonzero(D[1:] == e) + 1
            assert (at_min <= s0).all() if kind == "left" else (at_min > s0).all()
        if kind == "last":
            assert stop == len(read) == s0
        if kind == "first":
            assert stop <= m + k and len(read) == s0
        kinds.setdefault((panel, cutoff), set()).add(kind)
    for panel, lens in cc.A_PANELS:
        assert [len(s) for _, s in cc.a_primers(panel)] == list(lens)
        assert kinds[(panel, 0.0)] >= {"stop", "warm", "last", "first"}
        if max(lens) >= 10:
            assert kinds[(panel, 0.2)] >= {"stop", "warm", "left", "right", "last", "first"}
        assert wu_witness.get(panel), panel     # tells `wu = m` from `m + k`
    hb = {p: {m > 32 for m in lens} for p, lens in cc.A_PANELS}
    assert hb["low"] == {False} and hb["high"] == {True}
    assert hb["mix32"] == hb["mix1"] == {False, True}
    stops = {(s[4], s[5]) for s in specs if s[2] == "stop"}
    assert stops == {(s0, d) for s0 in cc.SEAMS for d in cc.A_STOPS}
    warm = {(s[4], s[5]) for s in specs if s[2] == "warm"}
    assert warm == {(s0, d) for s0 in cc.SEAMS for d in cc.A_WARM}
    assert {s[7] for s in specs if s[6] > 0} == set(cc.EDITS)
    assert {s[6] for s in specs if s[0] == "high" and s[1] == 0.2} >= set(range(0, 12))
    assert {s[4] for s in specs if s[2] == "last"} == set(cc.A_ENDS)
    assert {s[4] for s in specs if s[2] == "first"} == set(cc.A_ENDS)
    for name in cc.stratum("A"):      # the batch holds exactly its cases' reads
        b = cc.batch(name)
        assert b["seqs"] == [cc.a_case(i)[0] for i in b["cases"]]


def _longest_run(stops):
    best = cur = 0
    prev = None
    for s in sorted(stops):
        cur = cur + 1 if prev is not None and s == prev + 1 else 1
        best, prev = max(best, cur), s
    return best


def test_long_run_cases_hold_64_columns_at_one_cost():
    """Stratum B: every batch holds a run of >= 64 consecutive hit columns of one label, in a
    block of the first launch and in a block that the redo takes; the all-N reads end their
    runs on the offsets 62, 63, 64 and 65 of the flush mask."""
    for name in cc.stratum("B"):
        b = cc.batch(name)
        H, _ = cc.expected(name)
        runs = {}
        for r, lab, _, _, stop in H:
            runs.setdefault((r, lab), []).append(stop)
        longest = {key: _longest_run(v) for key, v in runs.items()}
        bh = cc.block_hits(name)
        over = set(np.flatnonzero(bh > cc.HIT_CAP).tolist())
        assert any(v >= 64 and key[0] // cc.READS in over for key, v in longest.items()), name
        assert any(v >= 64 and key[0] // cc.READS not in over for key, v in longest.items()), name
        assert len(over) == b["big"] and (cc.low_cols_blocks(name)[bh <= cc.HIT_CAP]
                                          <= cc.HIT_CAP).all(), name
    runs = {}
    for r, lab, _, _, stop in cc.expected("B/alln")[0]:
        runs.setdefault((r, lab), []).append(stop)
    assert {len(v) for v in runs.values()} >= {63, 64, 65, 66, 131}
    seqs = cc.batch("B/nstretch")["seqs"]
    assert all("N" * 200 in s and s.index("N") < 512 < s.rindex("N") for s in seqs if len(s) > 100)


def test_capacity_cases_hold_512_and_513_hits():
    """Stratum C: block 1 of 3 holds exactly 512 / 513 hits, all at D = 0 with cutoff 0.0, so
    the kernel stores exactly what the oracle counts."""
    for name, count in (("C/512", 512), ("C/513", 513)):
        b = cc.batch(name)
        H, _ = cc.expected(name)
        assert b["cutoff"] == 0.0 and all(h[2] == 0 for h in H)
        bh = cc.block_hits(name)
        assert len(bh) == 3 and int(bh[1]) == count and bh[0] < 100 and bh[2] < 100
        assert b["big"] == int(count > cc.HIT_CAP)
    a, b = cc.batch("C/512")["seqs"], cc.batch("C/513")["seqs"]
    assert [i for i in range(len(a)) if a[i] != b[i]] == [cc.READS + 17]


def test_redo_cases_overflow_the_blocks_they_name():
    """Strata D, E and G: the oracle's hits per block (all at D = 0: the stored count) say which
    blocks the redo takes; D/five also overflows the hit staging of a new context (4n + 4096)
    and ends in a block of fewer than 64 reads, E overflows the segment staging (2n + 4096)."""
    want = {"D/five": [1, 3, 4], "D/reuse": [0], "D/none": [], "E/keep": [0], "E/trim": [0],
            "G/plain": [], "G/redo": [0]}
    for name, blocks in want.items():
        b = cc.batch(name)
        H, S = cc.expected(name)
        assert b["cutoff"] == 0.0 and all(h[2] == 0 for h in H)
        bh = cc.block_hits(name)
        assert np.flatnonzero(bh > cc.HIT_CAP).tolist() == blocks, name
        assert b["big"] == len(blocks)
    n = len(cc.batch("D/five")["seqs"])
    bh = cc.block_hits("D/five")
    assert len(bh) >= 5 and 0 < n % cc.READS < cc.READS
    assert len({int(bh[i]) for i in (1, 3, 4)}) == 3
    assert int(bh.sum()) > 4 * n + 4096
    assert len(cc.batch("D/reuse")["seqs"]) < n
    assert bh[[1, 3, 4]].sum() > cc.block_hits("D/reuse")[0]   # the redo's buffers are reused
    for name in ("E/keep", "E/trim"):
        b = cc.batch(name)
        assert len(cc.expected(name)[1]) > 2 * len(b["seqs"]) + 4096
        assert len(b["seqs"]) == 10
    assert cc.batch("E/keep")["keep"] and not cc.batch("E/trim")["keep"]
    assert cc.batch("E/keep")["seqs"] == cc.batch("E/trim")["seqs"]


def test_equal_interval_cases_order_by_label():
    """Stratum G (and D's blocks): the palindromic primer's two labels hit the same intervals;
    the oracle lists them in label order."""
    for name in ("G/plain", "G/redo", "D/five"):
        H, _ = cc.expected(name)
        twins = [(a, b) for a, b in zip(H, H[1:])
                 if (a[0], a[3], a[4]) == (b[0], b[3], b[4])]
        assert len(twins) >= 20 and all((a[1], b[1]) == (2, 3) for a, b in twins), name
    over = cc.block_hits("D/five") > cc.HIT_CAP
    H, _ = cc.expected("D/five")
    assert {bool(over[h[0] // cc.READS]) for h in H if h[1] == 2} == {False, True}


def test_many_block_cases_cross_the_scan_ranges():
    """Stratum F: 70,001 reads are 1,094 blocks, two per thread of chop_blkscan_kernel; blocks
    with hits lie on both sides of the threads' range boundaries and in the last, partial
    block.  The small batches sit on the block edges of the read count."""
    n = len(cc.batch("F/70001")["seqs"])
    nb = math.ceil(n / cc.READS)
    assert n == 70001 and nb == 1094 and math.ceil(nb / 1024) == 2
    bh = cc.block_hits("F/70001")
    assert all(bh[2 * t - 1] > 0 and bh[2 * t] > 0 for t in (1, 2, 100, 273, 546))
    assert bh[nb - 1] > 0 and len({len(s) for s in cc.batch("F/70001")["seqs"]}) >= 13
    assert sum(1 for s in cc.batch("F/70001")["seqs"] if not s) > 10000
    assert (cc.low_cols_blocks("F/70001") <= cc.HIT_CAP).all()
    for name, size in (("F/1", 1), ("F/63", 63), ("F/64", 64), ("F/65", 65)):
        assert len(cc.batch(name)["seqs"]) == size and len(cc.expected(name)[0]) > 0
    assert len(cc.expected("F/65")[0]) > len(cc.expected("F/64")[0])   # the 65th read hits
    empty = cc.batch("F/empty")["seqs"]
    assert len(empty) > cc.READS and not any(empty) and cc.expected("F/empty") == ([], [])
    tail = cc.batch("F/tail")["seqs"]
    assert len(tail) > cc.READS and not any(tail[cc.READS:]) and cc.block_hits("F/tail")[0] > 0
