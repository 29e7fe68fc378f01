"""dmx_rowpairdist_host / dmx_rowhits_host (csrc/dmx_pairdist.hip) against an
in-test numpy DP written from the contract (rowpair_cases.np_rowpair): the distances are
integers, so every comparison is exact."""
import numpy as np
import pytest

import pairdist_cases as pc
import rowpair_cases as rp
from dmx import lib


@pytest.fixture(scope="module")
def host():
    """The CPU set with the library's exact distances per mode (computed once)."""
    rows, q, t, flags = rp.host_set()
    got = {m: lib.rowpairdist_host(rows, q, t, m, flags=flags, n_threads=8)
           for m in (lib.PD_NW, lib.PD_HW)}
    return rows, q, t, flags, got


@pytest.mark.parametrize("mode", [lib.PD_NW, lib.PD_HW])
def test_distances_equal_the_numpy_dp(host, mode):
    rows, q, t, flags, got = host
    ql = np.array([len(rows[i]) for i in q])
    tl = np.array([len(rows[j]) for j in t])
    assert {1, 64, 65, 70, 1200} <= set(ql.tolist()) | set(tl.tolist())
    assert (ql > tl).any() and (ql < tl).any() and flags.any() and not flags.all()
    used = "".join(rows[i] for i in set(q.tolist()))
    assert set("-RN") <= set(used) and set("-RN") <= set("".join(rows[j] for j in set(t.tolist())))
    exp = rp.expected(rows, q, t, flags, mode)
    bad = np.flatnonzero(got[mode] != exp)
    assert not [(int(ql[i]), int(tl[i]), int(flags[i]), int(got[mode][i]), int(exp[i]))
                for i in bad[:10]]


def test_caps_threads_and_mask_rows(host):
    rows, q, t, flags, got = host
    for mode in (lib.PD_NW, lib.PD_HW):
        caps, capped = pc.cap_cycle(got[mode])
        np.testing.assert_array_equal(
            lib.rowpairdist_host(rows, q, t, mode, flags=flags, caps=caps, n_threads=3), capped)
    # rows given as masks, no flags: the forward distances; one thread
    masks = [lib.mask_row(x) for x in rows]
    fwd = lib.rowpairdist_host(masks, q[:60], t[:60], lib.PD_HW)
    np.testing.assert_array_equal(
        fwd, rp.expected(rows, q[:60], t[:60], np.zeros(60, dtype=np.uint8), lib.PD_HW))
    assert len(lib.rowpairdist_host(rows, [], [], lib.PD_NW)) == 0


def test_intersect_equality_by_hand():
    rows = ["ACGT", "ANGT", "A-GT", "ARGT", "AYGT", "AMGT", "ACGTACGT", "TTTTACGTTT", "-", "N"]

    def d(a, b, mode=lib.PD_NW, rc=0):
        return int(lib.rowpairdist_host(rows, [a], [b], mode,
                                        flags=np.array([rc], dtype=np.uint8))[0])
    assert d(0, 0) == 0 and d(0, 1) == 1 and d(1, 1) == 0      # N equals N only
    assert d(0, 2) == 1 and d(2, 2) == 1 and d(2, 0) == 1      # a gap equals nothing, itself too
    assert d(0, 3) == 1 and d(0, 4) == 0 and d(4, 0) == 0      # C is in Y, not in R
    assert d(4, 5) == 0 and d(3, 4) == 1                       # Y and M share C; R and Y nothing
    assert d(8, 8) == 1 and d(9, 9) == 0
    assert d(0, 6) == 4 and d(0, 6, lib.PD_HW) == 0            # HW: any substring of the target
    assert d(6, 0, lib.PD_HW) == 4                             # HW with the longer query
    assert d(0, 7, lib.PD_HW) == 0 and d(0, 7, lib.PD_HW, 1) == 0   # ACGT is its own rc
    assert d(7, 7, lib.PD_NW, 1) == int(rp.np_rowpair(
        [lib.mask_row(rows[7])], [lib.mask_rc(lib.mask_row(rows[7]))], lib.PD_NW)[0])


def np_hits(df, dr, cap):
    d = np.minimum(df, dr).astype(np.int64)
    hit = (cap >= 0) & (d <= cap)
    k = np.flatnonzero(hit)
    return k.astype(np.uint32), d[k].astype(np.uint32), (dr < df)[k].astype(np.uint8)


@pytest.mark.parametrize("mode", [lib.PD_NW, lib.PD_HW])
def test_rowhits_is_the_decision_over_both_strands(host, mode):
    rows, q, t, _, _ = host
    n = len(q)
    df = lib.rowpairdist_host(rows, q, t, mode, n_threads=8).astype(np.int64)
    dr = lib.rowpairdist_host(rows, q, t, mode, flags=np.full(n, lib.PD_RC, dtype=np.uint8),
                              n_threads=8).astype(np.int64)
    d = np.minimum(df, dr)
    assert (dr < df).any() and (dr > df).any() and (dr == df).any()
    k = np.arange(n) % 5   # caps: never, 0, d - 1, d, d + 1
    cap = np.where(k == 0, -1, np.where(k == 1, 0, np.where(k == 2, d - 1,
                                                            np.where(k == 3, d, d + 1))))
    pair, dd, rev = lib.rowhits_host(rows, q, t, cap, mode, n_threads=4)
    ep, ed, er = np_hits(df, dr, cap)
    np.testing.assert_array_equal(pair, ep)
    np.testing.assert_array_equal(dd, ed)
    np.testing.assert_array_equal(rev, er)
    assert not np.isin(np.flatnonzero(k == 0), pair).any()          # cap -1 is never a hit
    ties = np.flatnonzero(dr == df)
    assert np.isin(ties, pair).any() and not rev[np.isin(pair, ties)].any()   # ties go forward
    # no hit at all, every pair a hit
    assert len(lib.rowhits_host(rows, q, t, np.full(n, -1), mode)[0]) == 0
    allp, alld, _ = lib.rowhits_host(rows, q, t, np.full(n, 20000), mode, n_threads=4)
    np.testing.assert_array_equal(allp, np.arange(n))
    np.testing.assert_array_equal(alld, d)


def test_refusals_by_their_messages():
    big = "A" * (lib.PD_MAX_LEN + 1)
    for code, match, rows, q, t, kw in (
            (-1, "mode must be", ["ACGT"], [0], [0], {"mode": 2}),
            (-1, "pair 1 names a row outside the 2 given", ["ACGT", "AC"], [0, 0], [1, 2], {}),
            (-1, "pair 0 names a row outside", ["ACGT"], [1], [0], {}),
            (-1, "pair 1 has an unknown flag", ["ACGT"], [0, 0], [0, 0], {"flags": [1, 2]}),
            (-1, "row 1: column 2 has a mask bit",
             ["ACGT", np.array([1, 2, 32], dtype=np.uint8)], [0], [0], {}),
            (-4, "pair 1: row 1 has 0 columns", ["ACGT", ""], [0, 0], [0, 1], {}),
            (-4, "pair 0: row 1 has 0 columns", ["ACGT", ""], [1], [0], {}),
            (-4, "pair 0: row 0 has", [big], [0], [0], {})):
        mode = kw.pop("mode", lib.PD_NW)
        with pytest.raises(lib.DmxError, match=rf"dmx_rowpairdist_host failed \({code}\).*{match}"):
            lib.rowpairdist_host(rows, q, t, mode, **kw)
    # an unused empty row is no error
    assert lib.rowpairdist_host(["ACGT", ""], [0], [0], lib.PD_NW).tolist() == [0]
    with pytest.raises(lib.DmxError, match=r"dmx_rowhits_host failed \(-1\).*pair 1: a cap is"):
        lib.rowhits_host(["ACGT"], [0, 0], [0, 0], [0, -2])
    with pytest.raises(lib.DmxError, match=r"dmx_rowhits_host failed \(-1\).*mode must be"):
        lib.rowhits_host(["ACGT"], [0], [0], [0], mode=7)
    L = lib.load()
    one = np.zeros(1, dtype=np.uint32)
    assert L.dmx_rowpairdist_host(0, 1, None, None, one.ctypes.data, one.ctypes.data, None, None,
                                  1, one.ctypes.data, 1) == -1
    assert b"null" in L.dmx_last_error(None)
    # room below the hit count: the count is set, nothing is written, the call is refused
    import ctypes
    masks, off = lib.mask_row("ACGT"), np.array([0, 4], dtype=np.uint64)
    z = np.zeros(3, dtype=np.uint32)
    cap = np.zeros(3, dtype=np.int32)
    pair = np.full(3, 77, dtype=np.uint32)
    n = ctypes.c_size_t(0)
    rc = L.dmx_rowhits_host(1, 1, masks.ctypes.data, off.ctypes.data, z.ctypes.data, z.ctypes.data,
                            cap.ctypes.data, 3, pair.ctypes.data, pair.ctypes.data, None, 2,
                            ctypes.byref(n), 1)
    assert rc == -1 and n.value == 3 and pair.tolist() == [77, 77, 77]
    assert b"room for 2 hits, 3 to return" in L.dmx_last_error(None)
