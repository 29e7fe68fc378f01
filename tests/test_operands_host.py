"""Operand tables on the host (include/dmx.h dmx_result_operands_host, dmx_operands_check_host;
DESIGN.md §3.18): the table of a demultiplexer run against a string model, its order and
bin_first, and the argument checks of dmx_set_operands.  No GPU."""
import numpy as np
import pytest

import operands_cases as oc
from dmx import lib

F, B = oc.F, oc.B
SEED = 31801


def _reads(rng, n, lo=120, hi=400):
    return [oc.rand_seq(rng, rng.integers(lo, hi + 1)) for _ in range(n)]


def _rand_views(rng, reads, n):
    out = []
    for _ in range(n):
        r = int(rng.integers(len(reads)))
        L = len(reads[r])
        a = int(rng.integers(0, L - 100))
        b = int(rng.integers(a + 100, L + 1))
        out.append((r, a, b, int(rng.integers(2))))
    return oc.table_arrays(out)


def _check(reads, res, views, mode, w0, w1, keep, min_len):
    lens = np.array([len(r) for r in reads], np.uint32)
    got, first = lib.result_operands_host(res, lens, mode, w0, w1, views=views, keep=keep,
                                          min_len=min_len)
    exp, efirst = oc.model_table(reads, res, views, mode, w0, w1, keep, min_len)
    np.testing.assert_array_equal(first, efirst)
    for g, e, name in zip(got, exp, ("read", "start", "stop", "strand")):
        np.testing.assert_array_equal(g, e, err_msg=name)
    return got, first


@pytest.mark.parametrize("w0,w1", [([F, F, F], [B, B]), ([B, B, B], [F, F]), ([F, B, F], [B, F]),
                                   ([B, F, B], [F, B])])
@pytest.mark.parametrize("with_views", [False, True])
def test_two_round_table_equals_the_string_model(w0, w1, with_views):
    rng = np.random.default_rng([SEED, len(w0) + w0[0], int(with_views)])
    reads = _reads(rng, 60)
    views = _rand_views(rng, reads, 90) if with_views else None
    lens = (views[2] - views[1]) if with_views else [len(r) for r in reads]
    res = oc.synthetic_results(rng, len(lens), lens, w0, w1, lib.MODE_TWO_ROUND)
    # all four (rc1, rc2) combinations occur among the items matched in both rounds
    both = (res["bin1"] >= 0) & (res["bin2"] >= 0)
    assert {(int(a), int(b)) for a, b in zip(res["rc1"][both], res["rc2"][both])} == \
        {(0, 0), (0, 1), (1, 0), (1, 1)}
    _check(reads, res, views, lib.MODE_TWO_ROUND, w0, w1, None, 1)
    # every bin kept: the unmatched items give their untrimmed (but oriented) records
    n_bins = (len(w0) + 1) * (len(w1) + 1)
    got, first = _check(reads, res, views, lib.MODE_TWO_ROUND, w0, w1, np.ones(n_bins, np.uint8), 1)
    assert int(first[-1]) == len(res) == len(got[0])


@pytest.mark.parametrize("w0", [[F, F], [B, B], [F, B]])
def test_single_mode_table_equals_the_string_model(w0):
    rng = np.random.default_rng([SEED, 7, w0[0], w0[1]])
    reads = _reads(rng, 50)
    res = oc.synthetic_results(rng, len(reads), [len(r) for r in reads], w0, [], lib.MODE_SINGLE)
    _check(reads, res, None, lib.MODE_SINGLE, w0, None, None, 1)
    got, first = _check(reads, res[:0], _rand_views(rng, reads, 0), lib.MODE_SINGLE, w0, None,
                        None, 1)   # an empty view run
    assert len(got[0]) == 0 and not first.any()


def test_order_and_bin_first():
    rng = np.random.default_rng([SEED, 11])
    w0, w1 = [F, F, F], [B, B, B]
    reads = _reads(rng, 40)
    lens = [len(r) for r in reads]
    # bins (0, 1) and (2, 2) only; the others stay empty
    bins = [((0, 1) if k % 3 else (2, 2)) for k in range(len(reads))]
    res = oc.synthetic_results(rng, len(reads), lens, w0, w1, lib.MODE_TWO_ROUND, bins=bins)
    got, first = _check(reads, res, None, lib.MODE_TWO_ROUND, w0, w1, None, 1)
    ix = lambda b1, b2: (b1 + 1) * 4 + (b2 + 1)   # noqa: E731
    counts = np.diff(first.astype(np.int64))
    assert counts[ix(0, 1)] == sum(1 for k in range(40) if k % 3) and counts[ix(2, 2)] == 14
    assert counts.sum() == 40 and (counts > 0).sum() == 2
    # inside a bin the operands come in item order (whole reads: the read index)
    for b in (ix(0, 1), ix(2, 2)):
        r = got[0][int(first[b]):int(first[b + 1])]
        assert (np.diff(r.astype(np.int64)) > 0).all()
    # everything in one bin
    res1 = oc.synthetic_results(rng, 40, lens, w0, w1, lib.MODE_TWO_ROUND, bins=[(1, 0)] * 40)
    got, first = _check(reads, res1, None, lib.MODE_TWO_ROUND, w0, w1, None, 1)
    np.testing.assert_array_equal(got[0], np.arange(40))
    assert first[ix(1, 0)] == 0 and first[ix(1, 0) + 1] == 40
    # keep drops bins
    keep = np.zeros(16, np.uint8)
    keep[ix(2, 2)] = 1
    got, first = _check(reads, res, None, lib.MODE_TWO_ROUND, w0, w1, keep, 1)
    assert len(got[0]) == 14 and first[-1] == 14


def test_min_len_boundary():
    rng = np.random.default_rng([SEED, 13])
    w0, w1 = [F], [B]
    reads = _reads(rng, 30)
    res = oc.synthetic_results(rng, 30, [len(r) for r in reads], w0, w1, lib.MODE_TWO_ROUND,
                               bins=[(0, 0)] * 30)
    got, _ = _check(reads, res, None, lib.MODE_TWO_ROUND, w0, w1, None, 1)
    final = (got[2] - got[1]).astype(np.int64)
    m = int(np.sort(final)[10])
    got, _ = _check(reads, res, None, lib.MODE_TWO_ROUND, w0, w1, None, m)
    assert len(got[0]) == int((final >= m).sum()) and (got[2] - got[1]).min() == m   # m is kept
    got, _ = _check(reads, res, None, lib.MODE_TWO_ROUND, w0, w1, None, m + 1)
    assert len(got[0]) == int((final > m).sum())                                    # m is dropped


def test_builder_refusals():
    res = np.zeros(2, dtype=lib.RESULT_DTYPE)
    lens = [50, 60]

    def code(**kw):
        a = dict(mode=lib.MODE_SINGLE, wheres0=[F], wheres1=None, keep=None, min_len=1)
        a.update(kw)
        with pytest.raises(lib.DmxError) as e:
            lib.result_operands_host(res, lens, a["mode"], a["wheres0"], a["wheres1"],
                                     keep=a["keep"], min_len=a["min_len"])
        return e.value.code

    assert code(mode=lib.MODE_LINKED) == -4          # DMX_E_UNSUPPORTED
    assert code(min_len=0) == -1                      # DMX_E_INVALID
    assert code(keep=[1, 1, 1]) == -1                 # two bins
    assert code(mode=lib.MODE_TWO_ROUND) == -1        # no second panel


@pytest.mark.parametrize("bad,why", [
    (dict(read=[3]), "outside the batch"),
    (dict(start=[-1]), "start < 0"),
    (dict(start=[31], stop=[30]), "start > stop"),
    (dict(stop=[41]), "past its read"),
    (dict(strand=[2]), "strand"),
])
def test_set_operands_argument_checks(bad, why):
    lens = [40, 40, 40]
    good = dict(read=[0, 1, 2, 1], start=[0, 40, 5, 5], stop=[40, 40, 5, 30], strand=[0, 1, 1, 0])
    lib.operands_check_host(lens, **good)          # whole, empty, repeated, overlapping: all fine
    lib.operands_check_host(lens, [], [], [], [])
    args = {k: list(v) for k, v in good.items()}
    for k, v in bad.items():
        args[k][2] = v[0]
    with pytest.raises(lib.DmxError) as e:
        lib.operands_check_host(lens, **args)
    assert e.value.code == -1 and "operand 2" in str(e.value) and why in str(e.value)


def test_geometry_covers_what_it_claims():
    reads, tab, pairs = oc.geometry()
    ln, st = (tab[2] - tab[1]).astype(int), tab[3]
    assert set(oc.GEOMETRY_LENS) <= set(ln.tolist()) and 180 <= 2 * len(pairs) <= 300   # both ways
    assert {int(x) % 32 for x in tab[1]} >= set(oc.START_MODS)
    assert {int(x) % 64 for x in ln[st == 1]} >= {0, 1, 63}
    assert ((tab[0] == 0) & (tab[1] == 0)).any() and ((tab[0] == 0) & (tab[2] == len(reads[0]))).any()
    lr = len(reads) - 1
    assert ((tab[0] == lr) & (tab[1] == 0)).any() and ((tab[0] == lr) & (tab[2] == len(reads[lr]))).any()
    assert len(tab[0]) > len(reads) // 2 and set(st.tolist()) == {0, 1}
    # N bases inside operands on both strands, and next to them
    strs = oc.extract(reads, tab)
    assert {int(s) for s, x in zip(st, strs) if "N" in x} == {0, 1}
    assert any(reads[int(r)][int(b)] == "N" for r, b in zip(tab[0], tab[2]) if b < len(reads[int(r)]))
    assert any(reads[int(r)][int(a) - 1] == "N" for r, a in zip(tab[0], tab[1]) if a > 0)
