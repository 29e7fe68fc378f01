"""dmx_rowdist_host (csrc/dmx_pairdist.hip; include/dmx.h dmx_rowdist) against the
in-test numpy DP of rowdist_cases.py, written from the contract; its refusals; lib.mask_rc.
No GPU: the kernel is held to this host reference by test_rowdist.py."""
import numpy as np
import pytest

import pairdist_cases as pc
import rowdist_cases as rc
from dmx import lib


@pytest.mark.parametrize("n_threads", [1, 16])
def test_host_equals_the_numpy_dp(n_threads):
    reads, rows, q, r, exp = rc.host_set()
    # the set has what it is meant to have
    assert any("-" in x for x in rows) and any(set(x) & set("RYMKSW") for x in rows)
    assert any("N" in x for x in rows) and any(b"N" in x for x in reads)
    assert np.bincount(r).max() > 60 and {0, len(rows) - 1} <= set(r.tolist())
    assert (np.diff(q.astype(np.int64)) < 0).any() and (np.diff(r.astype(np.int64)) < 0).any()
    p = pc.pack_reads(reads)
    got = lib.rowdist_host(p, rows, q, r, n_threads=n_threads)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, exp)
    # caps 0, d - 1, d, d + 1 in turn
    caps, capped = pc.cap_cycle(exp)
    np.testing.assert_array_equal(lib.rowdist_host(p, rows, q, r, caps, n_threads=n_threads),
                                  capped)
    # rows given as mask arrays are the same rows
    np.testing.assert_array_equal(
        lib.rowdist_host(p, [lib.mask_row(x) for x in rows], q, r, n_threads=n_threads), exp)


def test_small_cases_by_hand():
    p = pc.pack_reads([b"ACGT", b"ANGT", b"A"])
    d = lib.rowdist_host(p, ["ACGT", "AC-GT", "RYKM", "ANGT", "----"],
                         [0, 0, 0, 0, 1, 1, 0, 2], [0, 1, 2, 3, 3, 0, 4, 4])
    #  equal; one gap column to step over; A~R C~Y G~K but T!~M; N equals N only; all gaps
    assert d.tolist() == [0, 1, 1, 1, 0, 1, 4, 4]
    assert len(lib.rowdist_host(p, ["ACGT"], [], [])) == 0
    assert len(lib.rowdist_host(p, [], [], [])) == 0


def test_refusals_name_the_pair_or_the_row():
    reads = [b"ACGT" * 5, b"", b"A" * (lib.PD_MAX_LEN + 1)]
    p = pc.pack_reads(reads)
    with pytest.raises(lib.DmxError, match=r"\(-1\).*pair 1 names a read outside the batch"):
        lib.rowdist_host(p, ["ACGT"], [0, 3], [0, 0])
    with pytest.raises(lib.DmxError, match=r"\(-1\).*pair 2 names a row outside"):
        lib.rowdist_host(p, ["ACGT", "AC"], [0, 0, 0], [0, 1, 2])
    with pytest.raises(lib.DmxError, match=r"\(-4\).*pair 1: reads of 1\.\."):
        lib.rowdist_host(p, ["ACGT"], [0, 1], [0, 0])
    with pytest.raises(lib.DmxError, match=r"\(-4\).*pair 0: reads of 1\.\."):
        lib.rowdist_host(p, ["ACGT"], [2], [0])
    with pytest.raises(lib.DmxError, match=r"\(-4\).*pair 1: row 1 has 0 columns"):
        lib.rowdist_host(p, ["ACGT", ""], [0, 0], [0, 1])
    with pytest.raises(lib.DmxError, match=rf"\(-4\).*pair 0: row 0 has {lib.PD_MAX_LEN + 1} col"):
        lib.rowdist_host(p, ["A" * (lib.PD_MAX_LEN + 1)], [0], [0])
    with pytest.raises(lib.DmxError, match=r"\(-1\).*row 1: column 2 has a mask bit"):
        lib.rowdist_host(p, ["ACGT", np.array([1, 2, 32], dtype=np.uint8)], [0], [0])
    L = lib.load()
    one = np.zeros(1, dtype=np.uint32)
    assert L.dmx_rowdist_host(p.seq2b.ctypes.data, p.nmask.ctypes.data, p.offsets.ctypes.data,
                              p.lengths.ctypes.data, p.n_reads, 1, None, None, one.ctypes.data,
                              one.ctypes.data, None, 1, one.ctypes.data, 1) == -1
    assert b"null" in L.dmx_last_error(None)
    # the same pointers with no pairs: nothing to refuse
    assert L.dmx_rowdist_host(None, None, None, None, 0, 0, None, None, None, None, None, 0, None,
                              1) == 0
    with pytest.raises(lib.DmxError, match="one entry per pair"):
        lib.rowdist_host(p, ["ACGT"], [0], [0], caps=[1, 2])
    assert lib.rowdist_host(p, ["ACGT"], [0], [0]).tolist() == [16]


def test_mask_rc():
    rng = np.random.default_rng(83)
    for n in (0, 1, 2, 17, 300):
        s = "".join(rng.choice(list("ACGTNRYMKSW-"), n))
        m = lib.mask_row(s)
        np.testing.assert_array_equal(lib.mask_rc(m), lib.mask_row(rc.revcomp_row(s)))
        np.testing.assert_array_equal(lib.mask_rc(lib.mask_rc(m)), m)
    # on plain sequences it is the reads' reverse complement
    assert lib.mask_symbols(lib.mask_rc(lib.mask_row("AACGTN-"))) == "-NACGTT"
    every = np.arange(32, dtype=np.uint8)
    np.testing.assert_array_equal(lib.mask_rc(lib.mask_rc(every)), every)
    assert (lib.mask_rc(every) & 16).tolist() == (every[::-1] & 16).tolist()
    with pytest.raises(lib.DmxError):
        lib.mask_rc(np.array([32], dtype=np.uint8))
