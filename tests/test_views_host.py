"""View runs, the part that needs no GPU: dmx_chop_views_host, the plain C++
statement of pychopper's PASS rule on dmx_chop_fetch's arrays, against the Python model of
views_cases.py; the composition model against string slicing; and the cases' own shape.
dmx_set_views needs a context (a HIP device), so its refusals are in tests/test_views.py."""
import numpy as np
import pytest

import views_cases as vc
from dmx import lib, loop


def _host(nseg, segs, qc, min_len, cap=None):
    L = lib.load()
    n = len(nseg)
    cap = n if cap is None else cap
    out = (np.zeros(cap, np.uint32), np.zeros(cap, np.int32), np.zeros(cap, np.int32),
           np.zeros(cap, np.uint8))
    nseg = np.ascontiguousarray(nseg, dtype=np.uint32)
    segs = np.ascontiguousarray(segs, dtype=lib.CHOP_SEG_DTYPE)
    q = None if qc is None else np.ascontiguousarray(qc, dtype=np.uint8)
    k = L.dmx_chop_views_host(nseg.ctypes.data if n else None,
                              segs.ctypes.data if len(segs) else None,
                              q.ctypes.data if q is not None and n else None, int(min_len), n,
                              *[a.ctypes.data if cap else None for a in out], cap)
    return k, out


def _table(rng, n, min_len):
    """0, 1 and 2 segments per read, lengths at min_len - 1, min_len, min_len + 1 and random."""
    nseg = rng.integers(0, 3, size=n).astype(np.uint32)
    segs = np.zeros(int(nseg.sum()), dtype=lib.CHOP_SEG_DTYPE)
    si = 0
    for r in range(n):
        for _ in range(int(nseg[r])):
            a = int(rng.integers(0, 300))
            ln = int(rng.choice([max(0, min_len - 1), min_len, min_len + 1,
                                 int(rng.integers(0, 400))]))
            segs[si] = (r, a, a + ln, int(rng.integers(2)), int(rng.integers(4)))
            si += 1
    return nseg, segs


@pytest.mark.parametrize("min_len", [0, 1, 50])
@pytest.mark.parametrize("qc_kind", ["null", "ones", "zeros", "mixed"])
def test_chop_views_host_equals_the_model(min_len, qc_kind):
    rng = np.random.default_rng([vc.SEED, min_len, len(qc_kind)])
    n = 700
    nseg, segs = _table(rng, n, min_len)
    qc = {"null": None, "ones": np.ones(n, np.uint8), "zeros": np.zeros(n, np.uint8),
          "mixed": (rng.random(n) < 0.6).astype(np.uint8) * 7}[qc_kind]   # any nonzero byte passes
    want = vc.pass_model(nseg, segs, qc, min_len)
    k, out = _host(nseg, segs, qc, min_len)
    assert k == len(want)
    got = list(zip(*[a[:k].tolist() for a in out]))
    assert got == want
    if qc_kind == "zeros":
        assert k == 0
    else:
        assert k > 0
        # the three boundary lengths all occur among single-segment reads
        single = segs[np.repeat(nseg, nseg) == 1]
        lens = set((single["stop"] - single["start"]).tolist())
        assert {min_len, min_len + 1} <= lens and (min_len == 0 or min_len - 1 in lens)


def test_chop_views_host_empty_batch_and_small_cap():
    k, _ = _host(np.zeros(0, np.uint32), np.zeros(0, lib.CHOP_SEG_DTYPE), None, 50)
    assert k == 0
    rng = np.random.default_rng(vc.SEED)
    nseg, segs = _table(rng, 200, 10)
    want = vc.pass_model(nseg, segs, None, 10)
    k, out = _host(nseg, segs, None, 10, cap=5)     # the length comes back, 5 views are written
    assert k == len(want) > 5
    assert list(zip(*[a.tolist() for a in out])) == want[:5]
    k0, _ = _host(nseg, segs, None, 10, cap=0)
    assert k0 == k


def test_composition_model_is_string_slicing():
    """compose(), the model of the rule the finalize kernels apply (their own use of it is
    checked through round 1's results, strata M and O of tests/test_views.py), and
    dmx.loop.view_coords, which renders the loop's records: orient(orient(read[s:e], t), o)[a:b]
    is the view both name."""
    rng = np.random.default_rng(vc.SEED + 1)
    read = vc.sw.rand_seq(rng, 300)
    for _ in range(500):
        s = int(rng.integers(0, 301))
        e = int(rng.integers(s, 301))
        t, o = int(rng.integers(2)), int(rng.integers(2))
        a = int(rng.integers(0, e - s + 1))
        b = int(rng.integers(a, e - s + 1))
        v = read[s:e]
        v = vc.revcomp(v) if t else v
        w = vc.revcomp(v) if o else v
        cs, ce, ct = vc.compose(s, e, t, a, b, o)
        x = read[cs:ce]
        assert (vc.revcomp(x) if ct else x) == w[a:b]
        arr = [np.array([v]) for v in (s, e, t, a, b, o)]     # the loop's rule for its sinks
        assert [int(v[0]) for v in loop.view_coords(*arr)] == [cs, ce, ct]


@pytest.mark.parametrize("name", vc.STRATA)
def test_cases_have_the_shape_their_stratum_names(name):
    c = vc.case(name)
    read, start, stop, strand = c.views
    lens = np.array([len(s) for s in c.reads])
    assert len(read) == len(start) == len(stop) == len(strand)
    if len(read):
        assert (read < len(c.reads)).all() and (start >= 0).all() and (start <= stop).all()
        assert (stop <= lens[read]).all() and (strand <= 1).all()
    assert lens.min() >= 150
    vl = stop - start
    if name == "M":
        assert len(read) == 3 * len(c.reads)
        assert set(strand[1::3].tolist()) == {1} and (stop[2::3] == lens[read[2::3]]).all()
    if name == "S":
        assert len(read) < len(c.reads) and len(set(zip(*[a.tolist() for a in c.views]))) < len(read)
    if name == "Z":
        assert set(vl.tolist()) == {0, 1, vc.MIN_OVERLAP - 1, vc.MIN_OVERLAP}
    if name == "E":
        assert (start > 0).all() and (stop < lens[read]).all() and c.restricted
    if name == "G":
        assert len(read) == 5000
    if name == "N":
        assert len(read) == 0
    if name == "O":
        exp = c.expected()
        assert ((exp["rc1"] == 0) & (exp["rc2"] == 1) & (exp["bin2"] >= 0)).sum() > 20
        assert (strand == 1).all()
    if name in ("B", "Bb"):
        exp = c.expected()     # some copies are found (cut or whole), some must not be
        assert (exp["bin1"] >= 0).sum() > 40 and (exp["bin1"] < 0).sum() > 40
