"""dmx_pairdist_host (the full-matrix DP behind the GPU kernel's parity tests) against a numpy DP
written here, and the pure-Python parts of dmx.sorter: read selection, pair generation and the
identity caps (amplicon_sorter.py:225-235, 550-623, 669-683).  No GPU."""
import numpy as np
import pytest

import pairdist_cases as pc
from dmx import lib, sorter


def host(reads, q, t, mode, flags=None, caps=None, n_threads=4):
    return lib.pairdist_host(pc.pack_reads(reads), q, t, mode, flags, caps, n_threads)


@pytest.mark.parametrize("mode", [lib.PD_NW, lib.PD_HW])
def test_host_dp_matches_numpy_on_random_pairs(mode):
    """~600 pairs, both RC flag values in one call; then caps 0, d - 1, d, d + 1."""
    reads, q, t, flags, exp = pc.random_set()
    assert 0 < flags.sum() < len(flags)
    got = host(reads, q, t, mode, flags)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, exp[mode])
    caps, capped = pc.cap_cycle(exp[mode])
    np.testing.assert_array_equal(host(reads, q, t, mode, flags, caps), capped)
    # one thread or many: the same
    np.testing.assert_array_equal(host(reads, q, t, mode, flags, n_threads=1), got)


def test_hand_cases():
    rng = np.random.default_rng(3)
    s = pc.rand_seq(rng, 57, p_n=0.0)
    big = pc.rand_seq(rng, 200, p_n=0.0)
    reads = [s, s, b"A" * 7, b"C" * 12, b"N", b"N", b"A",
             s + big, big[:100] + s + big[100:], big + s,      # 7, 8, 9: s planted
             b"AAAATTTT", b"TTTTCCCC",                         # 10, 11
             b"ACNGT", b"GGACNGTAA"]                           # 12, 13: odd length, with N
    nw = lambda a, b, f=0: int(host(reads, [a], [b], lib.PD_NW, [f])[0])
    hw = lambda a, b, f=0: int(host(reads, [a], [b], lib.PD_HW, [f])[0])
    assert nw(0, 1) == 0 and hw(0, 1) == 0                     # identical
    assert nw(2, 3) == 12 and nw(3, 2) == 12                   # A*n / C*m: max(n, m)
    assert hw(2, 3) == 7 and hw(3, 2) == 12                    # ... and n in HW
    assert nw(4, 5) == 0 and nw(4, 6) == 1 and nw(6, 4) == 1   # N == N, N != A
    assert hw(0, 7) == 0 and hw(0, 8) == 0 and hw(0, 9) == 0   # planted: start, middle, end
    assert nw(0, 8) == 200
    assert hw(10, 11) == 4 and nw(10, 11) == 8
    # RC of an odd-length sequence containing N: ACNGT -> ACNGT reversed and complemented
    assert pc.revcomp(reads[12]) == b"ACNGT"
    assert nw(12, 12, 1) == 0
    rc13 = pc.revcomp(reads[13])
    assert nw(12, 13, 1) == int(pc.np_dist([reads[12]], [rc13], lib.PD_NW)[0])
    assert hw(12, 13, 1) == 0                                  # ACNGT is its own RC: still planted
    assert nw(3, 3) == 0 and hw(8, 8) == 0                     # a pair (i, i)
    # HW against the empty substring: never more than the query's length
    assert hw(2, 4) == 7


def test_hw_is_not_symmetric_on_an_equal_length_pair():
    """An equal-length pair with HW(q, t) != HW(t, q), found with the numpy DP."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        a, b = pc.rand_seq(rng, 8, 0.0), pc.rand_seq(rng, 8, 0.0)
        exp = [int(pc.np_dist([a], [b], lib.PD_HW)[0]), int(pc.np_dist([b], [a], lib.PD_HW)[0])]
        if exp[0] != exp[1]:
            break
    assert exp[0] != exp[1]
    assert host([a, b], [0, 1], [1, 0], lib.PD_HW).tolist() == exp


def test_host_refusals():
    reads = [b"ACGT", b"", b"A" * (lib.PD_MAX_LEN + 1), b"ACGT" * 10]
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        host(reads, [0], [4], lib.PD_NW)
    with pytest.raises(lib.DmxError, match=r"\(-4\)"):
        host(reads, [0], [1], lib.PD_NW)
    with pytest.raises(lib.DmxError, match=r"\(-4\)"):
        host(reads, [2], [0], lib.PD_NW)
    with pytest.raises(lib.DmxError, match=r"\(-1\)"):
        host(reads, [0], [3], 7)
    assert len(host(reads, [], [], lib.PD_NW)) == 0
    assert lib.PD_MAX_LEN >= 16384
    sizes = lib.pairdist_group_sizes()
    assert sizes == sorted(set(sizes)) and sizes[0] >= 1 and sizes[-1] == 64


# ---- read selection and pair generation ---------------------------------------------------------

def ref_groups(n_usable, maxreads, allreads):
    """The reference's selection on a list of n_usable reads, as plain slicing."""
    lst = list(range(n_usable))
    if allreads and n_usable <= maxreads:
        maxreads = n_usable
    if n_usable < 1000:
        return [lst]
    out, n = [], 0
    while maxreads > 1000:
        out.append(lst[n:n + 1000])
        maxreads -= 1000
        n += 1000
    out.append(lst[n:n + maxreads])
    return [g for g in out if g]


@pytest.mark.parametrize("n_usable", [999, 1000, 2350])
@pytest.mark.parametrize("maxreads", [500, 1000, 1500, 2000, 10000])
@pytest.mark.parametrize("allreads", [False, True])
def test_select_groups(n_usable, maxreads, allreads):
    rng = np.random.default_rng(n_usable)
    # usable reads (300..2000 nt) with too-short and too-long ones mixed in
    lengths = list(rng.integers(300, 2001, n_usable)) + [299] * 40 + [2001] * 40
    rng.shuffle(lengths)
    got = sorter.select_groups(lengths, 300, 2000, maxreads, allreads)
    exp = ref_groups(n_usable, maxreads, allreads)
    assert [list(g) for g in got] == exp
    if n_usable >= 1000:
        assert all(len(g) == 1000 for g in got[:-1])
        assert sum(len(g) for g in got) == min(maxreads, n_usable)
    else:
        assert len(got) == 1 and len(got[0]) == n_usable
    assert len(sorter.usable(lengths, 300, 2000)) == n_usable
    assert len(sorter.usable(lengths, 300)) == n_usable + 40


def test_select_groups_too_few_reads():
    with pytest.raises(lib.DmxError):
        sorter.select_groups([400, 500, 600, 700, 100, 200], 300)
    assert len(sorter.select_groups([400, 500, 600, 700, 800, 200], 300)[0]) == 5


def ref_pairs(groups, lengths):
    out = []
    for g in groups:
        d = sorted(g, key=lambda i: lengths[i])   # stable, as list.sort is
        for p in range(len(d) - 1):
            for p2 in range(p + 1, len(d)):
                if lengths[d[p]] * 1.05 < lengths[d[p2]]:
                    continue
                out.append((d[p], d[p2]))
    return out


def test_pairs_order_ties_and_the_five_percent_rule():
    rng = np.random.default_rng(8)
    lengths = [int(x) for x in rng.integers(300, 360, 150)] + [400, 420, 421, 400, 380, 399]
    groups = [np.arange(0, 100), np.arange(100, len(lengths))]
    q, t = sorter.pairs(groups, lengths)
    exp = ref_pairs([list(g) for g in groups], lengths)
    assert list(zip(q.tolist(), t.tolist())) == exp
    assert len(exp) < sum(len(g) * (len(g) - 1) // 2 for g in groups)   # the rule dropped some
    # ties keep input order: equal lengths pair (earlier, later)
    q, t = sorter.pairs([np.arange(4)], [300, 300, 300, 300])
    assert list(zip(q.tolist(), t.tolist())) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    # exactly at len * 1.05 == len2 (400 * 1.05 == 420.0 in doubles): kept; just past it: dropped
    assert 400 * 1.05 == 420.0
    q, t = sorter.pairs([np.arange(3)], [400, 420, 421])
    assert list(zip(q.tolist(), t.tolist())) == [(0, 1), (1, 2)]
    # a product that is not exact in doubles follows the doubles
    for a, b in [(300, 315), (340, 357), (1000, 1050), (1137, 1194)]:
        q, t = sorter.pairs([np.arange(2)], [a, b])
        assert (len(q) == 1) == (not a * 1.05 < b), (a, b)
    q, t = sorter.pairs([np.arange(1)], [300])
    assert len(q) == 0 and len(t) == 0


@pytest.mark.parametrize("thr", [0.5, 80.0 / 100, 96.0 / 100])
def test_identity_caps_against_a_scan(thr):
    """For every length 1..5000 the cap (the forward pass's 0.5, and -sg 80 and 96) equals a
    brute-force scan over d = 0, 1, .. with built-in round, up to the first d that fails; that
    nothing passes after the first failure is scanned in full on a sample of lengths."""
    for L in range(1, 5001):
        d = 0
        while d <= L and round(1 - d / L, 3) >= thr:
            d += 1
        assert sorter.identity_cap(L, thr) == d - 1, L
    for L in list(range(1, 300)) + [1199, 1200, 4999, 5000]:
        ok = [d for d in range(L + 1) if round(1 - d / L, 3) >= thr]
        assert ok == list(range(len(ok)))
    assert sorter.identity_cap(10, 1.5) == -1


def test_unsupported_alphabet_names_the_read():
    with pytest.raises(lib.DmxError, match="read 2"):
        sorter.similarity(None, ["ACGT" * 100, "acgtn" * 80, "ACGR" * 100, "A" * 400, "C" * 400,
                                 "G" * 400])
