"""dmx_chop_views on the GPU: pychopper's PASS segments become the
demultiplexer's view list on the device.  After chop_exec; chop_views the list must equal
dmx_chop_views_host on the chop_fetch arrays element for element (and the Python model), and
exec must equal (a) the oracle on the extracted strings and (b) the merged path."""
import numpy as np
import pytest

import oracle
import views_cases as vc
from dmx import chop, lib, synth

pytestmark = pytest.mark.gpu


def _setup():
    primers = chop.load_primers(chop.PRIMERS_FASTA)
    with open(chop.CONFIG_FILE) as fh:
        rules = chop.parse_config(fh.read(), [p[0] for p in primers])
    return primers, rules


def _reads(rng, n):
    """tests/test_chop.py's batch: primer - insert - primer on both strands (config 2's
    generator), fused reads with two segments, reads cut before their second primer or without
    any, N runs, padding across the 512-column segments."""
    d = synth.generate("c2", n=n, seed=int(rng.integers(1 << 30)))
    out = []
    for s in synth.to_strings(d):
        u = rng.random()
        if u < 0.10 and out:
            s = s + out[-1]
        elif u < 0.15:
            s = s[:int(rng.integers(0, 130))]
        elif u < 0.20:
            p = int(rng.integers(0, len(s)))
            s = s[:p] + "N" * int(rng.integers(1, 6)) + s[p:]
        elif u < 0.25:
            s = vc.sw.rand_seq(rng, rng.integers(150, 400))
        elif u < 0.35:
            s = vc.sw.rand_seq(rng, rng.integers(380, 530)) + s
        out.append(s)
    return out


def _short_pool(rng, primers, min_len):
    """Short reads, exact primers: SP5 + insert + revcomp(SP27) on either strand with the kept
    segment min_len - 1, min_len, min_len + 1 nt and random; fused pairs; reads without primers."""
    p5, p27 = primers[0][1], primers[1][1]
    fixed = len(p5) + len(p27)
    pool = []
    for i in range(600):
        ins = (min_len - fixed - 1, min_len - fixed, min_len - fixed + 1,
               int(rng.integers(5, 60)))[i % 4]
        s = p5 + vc.sw.rand_seq(rng, ins) + vc.revcomp(p27)
        if i % 3 == 1:
            s = vc.revcomp(s)
        k = i % 10
        if k == 7:
            s = s + s                                   # two segments
        elif k == 8:
            s = vc.sw.rand_seq(rng, 100 + i % 40)       # none
        pool.append(s)
    return pool


def _chop(cx, reads, primers, rules, cutoff=0.2):
    cx.load(lib.pack(*oracle.pack_ascii(reads)))
    cx.chop_set([p[1] for p in primers], rules, cutoff, True)
    cx.chop_exec()
    nseg, _, segs, _ = cx.chop_fetch()
    return nseg, segs


def _host_views(nseg, segs, qc, min_len):
    L = lib.load()
    n = len(nseg)
    out = (np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32),
           np.zeros(n, np.uint8))
    q = None if qc is None else np.ascontiguousarray(qc, dtype=np.uint8)
    k = L.dmx_chop_views_host(nseg.ctypes.data, segs.ctypes.data if len(segs) else None,
                              q.ctypes.data if q is not None else None, int(min_len), n,
                              *[a.ctypes.data for a in out], n)
    assert k >= 0
    return tuple(a[:k] for a in out)


@pytest.mark.parametrize("qc_kind", ["null", "mixed"])
def test_chop_views_equal_the_host_twin_and_exec_equals_both_references(qc_kind):
    rng = np.random.default_rng([vc.SEED, 50, len(qc_kind)])
    primers, rules = _setup()
    reads = _reads(rng, 900)
    qc = None if qc_kind == "null" else (rng.random(len(reads)) < 0.7)
    with lib.Context(0) as cx:
        nseg, segs = _chop(cx, reads, primers, rules)
        # -z at the boundary: the median single segment's length, so lengths on both sides occur
        single = segs[np.repeat(nseg, nseg) == 1]
        min_len = int(np.median(single["stop"] - single["start"]))
        nv = cx.chop_views(qc, min_len)
        got = cx.views()
        want = _host_views(nseg, segs, qc, min_len)
        assert nv == len(want[0]) and 0 < nv < len(reads)
        for a, b in zip(got, want):
            assert a.tolist() == b.tolist()
        assert list(zip(*[a.tolist() for a in got])) == vc.pass_model(nseg, segs, qc, min_len)
        assert {0, 1, 2} <= set(nseg.tolist()) and set(got[3].tolist()) == {0, 1}
        c = vc.Case("chop", reads, got, *vc._bench_rounds())
        c.set_panels(cx)
        cx.exec()
        res, counts, flags = cx.fetch(), cx.counts(), cx.stats()["flags"]
        exp = c.expected()
        assert len(res) == nv
        assert len(vc.differing(res, exp)) == 0
        a0, a1 = c.n_adapters()
        assert counts.tolist() == vc.counts_of(exp, a0, a1, True).tolist()
        assert flags == 0
        # the run is not vacuous: some views carry a barcode of each round
        assert (exp["bin1"] >= 0).sum() > 0 and (exp["bin2"] >= 0).sum() > 0
        merged = vc.run_merged(cx, c)                       # (b); dmx_run drops the list
        ab = vc.differing(merged, exp)
        assert len(ab) == 0, f"references (a) and (b) disagree on {len(ab)} views"
        with pytest.raises(lib.DmxError, match=r"\(-5\)"):  # the batch chop_exec saw is gone
            cx.chop_views(None, min_len)


def test_chop_views_scan_over_more_than_1024_blocks():
    """66,000 short reads: 1,032 blocks of 64 reads, so the scan over the block counts gives
    several blocks to one thread.  The reads tile a pool of 600, so both references are computed
    on the pool's views and shared."""
    rng = np.random.default_rng([vc.SEED, 51])
    primers, rules = _setup()
    min_len = len(primers[0][1]) + len(primers[1][1]) + 30
    pool = _short_pool(rng, primers, min_len)
    n = 66000
    pick = rng.integers(0, len(pool), size=n)
    pick[:len(pool)] = np.arange(len(pool))
    reads = [pool[i] for i in pick]
    qc = rng.random(n) < 0.8
    with lib.Context(0) as cx:
        nseg, segs = _chop(cx, reads, primers, rules, cutoff=0.1)
        nv = cx.chop_views(qc, min_len)
        got = cx.views()
        want = _host_views(nseg, segs, qc, min_len)
        assert nv == len(want[0]) and n // 4 < nv < n
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        lens = (got[2] - got[1])
        assert lens.min() == min_len and (lens == min_len + 1).any()
        c = vc.Case("big", reads, got, *vc._bench_rounds())
        c.set_panels(cx)
        cx.exec()
        res, flags = cx.fetch(), cx.stats()["flags"]
        assert flags == 0 and len(res) == nv
        # the references on one view per distinct (pool read, view): equal strings, equal results
        keys = np.stack([pick[got[0]].astype(np.int64), got[1], got[2], got[3]], axis=1)
        uniq, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
        u = vc.Case("pool", reads, tuple(a[first] for a in got), c.r0, c.r1)
        exp = u.expected()
        assert len(vc.differing(res, exp[inv.reshape(-1)])) == 0
        assert len(vc.differing(vc.run_merged(cx, u), exp)) == 0
