"""dmx_groupalign_host (the sequential reference of dmx_groupalign) against the
in-test model of groupalign_cases.py, hand cases of the mask alphabet and the merge, every
refusal, and sorter.alignment_rows on the returned paths."""
import numpy as np
import pytest

import groupalign_cases as gc
import pairdist_cases as pc
from dmx import lib, sorter


def run(reads, seeds, groups, **kw):
    kw.setdefault("paths", True)
    return lib.groupalign_host(pc.pack_reads([r if isinstance(r, bytes) else r.encode()
                                              for r in reads]), seeds, groups, **kw)


def check_against_model(reads, seeds, groups, res):
    for g, (seed, mem) in enumerate(zip(seeds, groups)):
        rows, dists, paths = gc.model_alignment(seed, [reads[i] for i in mem])
        mask, count, first, dist, got_paths = gc.group_slices(res, g)
        emask, ecount, efirst = gc.model_columns(rows)
        assert dist.tolist() == dists, g
        assert [p.tolist() for p in got_paths] == paths, g
        np.testing.assert_array_equal(mask, emask, str(g))
        np.testing.assert_array_equal(count, ecount, str(g))
        np.testing.assert_array_equal(first, efirst, str(g))
        # the rows rebuilt from the paths are the model's, and the counts are theirs
        built = sorter.alignment_rows(seed, [reads[i] for i in mem], got_paths)
        assert built == ["".join(z) for z in rows], g
        # invariants: the ops that are no match are the distance; a path spans what it met
        n = len(seed)
        for r, ops in zip(mem, got_paths):
            assert int((ops != lib.PA_DELETE).sum()) == len(reads[r])
            assert int((ops != lib.PA_INSERT).sum()) == n
            n = len(ops)
        for d, ops in zip(dists, got_paths):
            assert int((ops != lib.PA_MATCH).sum()) == d
        assert n == len(mask)


def test_mask_row_alphabet():
    m = lib.mask_row("acgtN-RYMKSW")
    assert m.tolist() == [1, 2, 4, 8, 16, 0, 5, 10, 3, 12, 6, 9]
    assert lib.mask_symbols(m[:6]) == "ACGTN-"
    assert lib.mask_row(b"").tolist() == []
    for bad in ("B", "ACGU", "A C"):
        with pytest.raises(lib.DmxError, match="mask_row"):
            lib.mask_row(bad)
    with pytest.raises(lib.DmxError, match="several"):
        lib.mask_symbols(m)


def test_random_groups_equal_the_model():
    rng = np.random.default_rng(5)
    reads, seeds, groups = [], [], []
    for g in range(14):
        base = pc.rand_seq(rng, int(rng.integers(1, 201)))
        seeds.append(gc.plant(rng, base))
        mem = []
        for _ in range(int(rng.integers(1, 8))):
            r = pc.mutate(rng, base, float(rng.uniform(0.02, 0.3)))[:200] if rng.random() < 0.8 \
                else pc.rand_seq(rng, int(rng.integers(1, 201)))
            mem.append(len(reads))
            reads.append(r)
        groups.append(mem)
    res = run(reads, seeds, groups, n_threads=4)
    check_against_model(reads, seeds, groups, res)
    # one thread, no paths: the same columns
    plain = run(reads, seeds, groups, paths=False)
    assert "ops" not in plain
    for name in ("col_off", "mask", "count", "first", "dist"):
        np.testing.assert_array_equal(plain[name], res[name])


def test_gap_iupac_and_n_columns():
    # '-' equals nothing, and stepping over it costs 1
    res = run([b"ACGT"], ["AC-GT"], [[0]])
    assert res["dist"].tolist() == [1] and res["ops"].tolist() == [0, 0, 2, 0, 0]
    res = run([b"A"], ["-"], [[0]])
    assert res["dist"].tolist() == [1] and res["ops"].tolist() == [lib.PA_MISMATCH]
    # R equals A and G, not C
    res = run([b"A", b"G", b"C"], ["R", "R", "R"], [[0], [1], [2]])
    assert res["dist"].tolist() == [0, 0, 1]
    # N equals a masked base only
    res = run([b"N", b"A", b"N"], ["N", "N", "A"], [[0], [1], [2]])
    assert res["dist"].tolist() == [0, 1, 1]
    check_against_model([b"ACGT", b"NACG", b"GGCC"], ["AC-GT", "NWSK", "RYMK"], [[0], [1], [2]],
                        run([b"ACGT", b"NACG", b"GGCC"], ["AC-GT", "NWSK", "RYMK"],
                            [[0], [1], [2]]))


def test_merge_hand_cases():
    # a homopolymer surplus goes to the end: up before the diagonal on the way back
    res = run([b"AAAA"], ["AAA"], [[0]])
    assert res["ops"].tolist() == [0, 0, 0, 1] and res["mask"].tolist() == [1, 1, 1, 0]
    assert res["count"][:, 0].tolist() == [1, 1, 1, 1] and res["first"][3].tolist() == [1, 0, 0, 0, 0]
    # an insertion in round k (0-based) is a 0-mask column with count 1 and first = k + 1;
    # a deletion leaves the column's counts untouched
    reads = [b"ACGT", b"ACGGT", b"ACT"]
    res = run(reads, ["ACGT"], [[0, 1, 2]])
    assert res["dist"].tolist() == [0, 1, 2]
    assert lib.mask_symbols(res["mask"]) == "ACG-T"
    assert res["count"].tolist() == [[3, 0, 0, 0, 0], [0, 3, 0, 0, 0], [0, 0, 2, 0, 0],
                                     [0, 0, 1, 0, 0], [0, 0, 0, 3, 0]]
    assert res["first"][3].tolist() == [0, 0, 2, 0, 0]
    assert res["first"][0].tolist() == [1, 0, 0, 0, 0]
    assert res["ops"][int(res["op_off"][2]):].tolist() == [0, 0, 2, 2, 0]
    check_against_model(reads, ["ACGT"], [[0, 1, 2]], res)
    # a group without members: its seed row, zero counts
    res = run([b"ACGT"], ["AC-R", "ACGT"], [[], [0]])
    assert res["col_off"].tolist() == [0, 4, 8] and res["mask"][:4].tolist() == [1, 2, 0, 5]
    assert not res["count"][:4].any() and not res["first"][:4].any()
    assert res["op_off"].tolist() == [0, 4]
    # no groups at all
    res = run([b"ACGT"], [], [])
    assert res["col_off"].tolist() == [0] and len(res["mask"]) == 0 and len(res["dist"]) == 0


def test_refusals_name_the_group():
    reads = [b"ACGT" * 5, b"", b"A" * (lib.PD_MAX_LEN + 1), b"ACGTACGTAC" + b"TTTTT" + b"ACGTACGTAC"]
    seed20 = "ACGTACGTACACGTACGTAC"
    with pytest.raises(lib.DmxError, match=r"\(-1\).*group 1.*outside the batch"):
        run(reads, ["ACGT", "ACGT"], [[0], [0, 4]])
    with pytest.raises(lib.DmxError, match=r"\(-4\).*group 0.*member 1"):
        run(reads, ["ACGT"], [[0, 1]])
    with pytest.raises(lib.DmxError, match=r"\(-4\).*group 0"):
        run(reads, ["ACGT"], [[2]])
    with pytest.raises(lib.DmxError, match=r"\(-4\).*group 1.*seed"):
        run(reads, ["ACGT", ""], [[0], [0]])
    with pytest.raises(lib.DmxError, match=r"\(-4\).*group 0.*seed"):
        run(reads, ["ACGTA"], [[0]], max_cols=4)
    with pytest.raises(lib.DmxError, match=r"\(-1\).*group 1.*mask bit"):
        run(reads, ["ACGT", np.array([1, 2, 32], dtype=np.uint8)], [[0], [0]])
    with pytest.raises(lib.DmxError, match=r"\(-4\).*max_cols"):
        run(reads, ["ACGT"], [[0]], max_cols=lib.PD_MAX_LEN + 1)
    with pytest.raises(lib.DmxError, match=r"\(-1\).*cols_cap"):
        run(reads, ["ACGT"], [[0]], cols_cap=23)
    with pytest.raises(lib.DmxError, match=r"\(-1\).*ops_cap"):
        run(reads, ["ACGT"], [[0]], ops_cap=23)
    assert len(run(reads, ["ACGT"], [[0]], cols_cap=24, ops_cap=24)["mask"]) == 20
    # null arguments
    L = lib.load()
    assert L.dmx_groupalign_host(None, None, None, None, 0, 1, None, None, None, None, 0, None,
                                 None, None, None, 0, None, None, None, 0, 1) == -1
    assert b"null" in L.dmx_last_error(None)
    # a row that would grow past max_cols: seed 20, a member that inserts 5, max_cols 24
    with pytest.raises(lib.DmxError, match=r"\(-4\).*group 1, round 0.*25.*max_cols 24"):
        run(reads, ["ACGT", seed20], [[], [3]], max_cols=24)
    ok = run(reads, ["ACGT", seed20], [[], [3]], max_cols=25)
    assert ok["dist"].tolist() == [5] and ok["col_off"].tolist() == [0, 4, 29]
