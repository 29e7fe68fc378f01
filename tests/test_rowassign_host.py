"""dmx_rowassign_host (csrc/dmx_pairdist.hip) against the in-test oracle of
rowassign_cases.py, written from the contract alone: the numpy DP of rowdist_cases.py for the
distances, then a literal Python loop for the pair rule, the stop, the retry and the best line
per place.  All five outputs must be equal.  No GPU."""
import numpy as np
import pytest

import pairdist_cases as pc
import rowassign_cases as ra
from dmx import lib


@pytest.fixture(scope="module")
def case():
    return ra.host_set()


@pytest.fixture(scope="module")
def packed(case):
    return pc.pack_reads(case[0])


def test_the_set_covers_every_branch(case):
    ra.coverage(case)


def test_host_equals_the_oracle(case, packed):
    reads, rows, sel, tb, exp, _ = case
    for n_threads in (1, 5):
        ra.same(lib.rowassign_host(packed, rows, sel, *tb, n_threads=n_threads), exp)
    # rows given as masks, the same
    ra.same(lib.rowassign_host(packed, [lib.mask_row(x) for x in rows], sel, *tb), exp)


def test_stop_after_max_chunks_full_chunks(case, packed):
    reads, rows, sel, tb, full, _ = case
    exp = ra.oracle(reads, rows, sel, *tb, chunk=50, max_chunks=2)
    k = exp["stopped_at"]
    assert k is not None and 100 <= exp["n_pairs"] < 150 < full["n_pairs"]
    assert (exp["best_row"][k + 1:] == ra.NONE).all() and (full["best_row"][k + 1:] != ra.NONE).any()
    ra.same(lib.rowassign_host(packed, rows, sel, *tb, chunk=50, max_chunks=2, n_threads=4), exp)


def test_a_place_that_jumps_over_the_value_stops_nothing(case, packed):
    reads, rows, sel, tb, _, _ = case
    rows7 = [rows[g] for g in (0, 1, 2, 3, 5, 6, 7)]
    fam = np.arange(6, 30, dtype=np.uint32)
    exp = ra.oracle(reads, rows7, fam, *tb, chunk=3, max_chunks=1)
    free = ra.oracle(reads, rows7, fam, *tb)
    per_place = np.bincount([p[0] for p in free["pairs"]], minlength=len(fam))
    ends = np.cumsum(per_place) // 3
    assert per_place[0] >= 6 and ends[0] >= 2 and not (ends == 1).any()
    assert exp["stopped_at"] is None and exp["n_pairs"] == free["n_pairs"] == per_place.sum()
    ra.same(lib.rowassign_host(packed, rows7, fam, *tb, chunk=3, max_chunks=1), exp)


def test_nothing_to_compare(case, packed):
    reads, rows, sel, tb, _, _ = case
    row, d, cls, n_pairs, n_lines = lib.rowassign_host(packed, rows, [], *tb)
    assert len(row) == len(d) == len(cls) == 0 and (n_pairs, n_lines) == (0, 0)
    row, d, cls, n_pairs, n_lines = lib.rowassign_host(packed, [], sel[:5], *tb)
    assert (row == ra.NONE).all() and (d == ra.NONE).all() and (cls == 0).all()
    assert len(row) == 5 and (n_pairs, n_lines) == (0, 0)
    # reads and rows that the 5 % rule keeps apart
    row, _, _, n_pairs, _ = lib.rowassign_host(packed, ["ACGTACGTAC"], [0, 1], *tb)
    assert (row == ra.NONE).all() and n_pairs == 0


REFUSALS = (
    # code, message, rows, reads, changes to (cap_hit, cap_half, bin_off, bins, chunk)
    (-1, "chunk must be at least 1", ["ACGT"], [0], dict(chunk=0)),
    (-1, "place 1 names a read outside the batch", ["ACGT"], [0, 9], {}),
    (-1, "row 1: column 2 has a mask bit", ["ACGT", np.array([1, 2, 32, 4], dtype=np.uint8)], [0], {}),
    (-1, r"length 3: a cap is a distance, or -1", ["ACGT"], [0], dict(cap_hit={3: -2})),
    (-1, r"length 2: a cap is a distance, or -1", ["ACGT"], [0], dict(cap_half={2: -7})),
    (-1, r"place 1, row 0: length 5 is outside the 5 entries", ["ACGTA"], [0, 1], dict(n_len=5)),
    (-1, r"length 4: its classes end outside the 3 entries", ["ACGT"], [0], dict(n_bins=3)),
    (-4, r"place 2: reads of 1\.\.", ["ACGT", ""], [0, 0, 2], {}),
    (-4, r"place 1: reads of 1\.\.", ["ACGT", "A" * 16385], [0, 3], {}),
    (-4, r"place 1: row 1 has 16385 columns", ["ACGT", "A" * 16385], [0, 4], {}),
)


@pytest.mark.parametrize("code,match,rows,sel,change", REFUSALS)
def test_refusals_leave_the_outputs_untouched(code, match, rows, sel, change):
    reads = [b"ACGT", b"ACGTA", b"", b"A" * 16385, b"A" * 16384]
    p = pc.pack_reads(reads)
    n_len = change.get("n_len", 16386)
    cap_hit = np.full(n_len, 1, dtype=np.int32)
    cap_half = np.full(n_len, 2, dtype=np.int32)
    bin_off = np.zeros(n_len, dtype=np.uint32)
    bins = np.full(change.get("n_bins", 4), 7, dtype=np.uint16)
    if "n_bins" in change:
        cap_hit[4] = 3
    for L, v in change.get("cap_hit", {}).items():
        cap_hit[L] = v
    for L, v in change.get("cap_half", {}).items():
        cap_half[L] = v
    with pytest.raises(lib.DmxError, match=rf"dmx_rowassign_host failed \({code}\).*{match}") as e:
        lib.rowassign_host(p, rows, sel, cap_hit, cap_half, bin_off, bins,
                           chunk=change.get("chunk", 10))
    row, d, cls = e.value.outputs
    assert (row == 0xDEADBEEF).all() and (d == 0xDEADBEEF).all() and (cls == 0xBEEF).all()
    assert len(row) == len(sel)
    # the accepted form of the same call
    row, d, cls, n_pairs, n_lines = lib.rowassign_host(
        p, ["ACGT"], [0], np.full(5, 1, dtype=np.int32), np.full(5, 2, dtype=np.int32),
        np.zeros(5, dtype=np.uint32), np.full(2, 7, dtype=np.uint16))
    assert (row.tolist(), d.tolist(), cls.tolist(), n_pairs, n_lines) == ([0], [0], [7], 1, 1)


def test_wrapper_argument_checks(packed):
    with pytest.raises(lib.DmxError, match="of equal length"):
        lib.rowassign_host(packed, ["ACGT"], [0], [1, 1], [1], [0, 0], [1])
    with pytest.raises(lib.DmxError, match="must not be negative"):
        lib.rowassign_host(packed, ["ACGT"], [0], [1], [1], [0], [1], chunk=-1)
