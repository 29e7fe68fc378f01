"""The piece screen's pair table on the CPU: dmx_panel_piece_pairs returns the
4096-row table, the rank bases and the keys the kernels hold; a Python model of the paired lookup
(piece_pairs_cases.py) must agree with single lookups, and the key index must address each key's
own entries.  Also confirms, with the oracle and the host model alone, that the slot reads of the
GPU test (test_piece_pairs.py) are what they claim to be.
"""
import functools

import numpy as np
import pytest

import oracle
import piece_pairs_cases as pp
import pieces_seam_cases as sc
import test_pieces_host as tph
from dmx import lib, synth


def _panel(name):
    if name == "sp27":
        return tuple(synth.panels(24, 24)[3]), lib.DMX_BACK, 0.1
    return sc.panel(name)


PANELS = ("sp5", "sp27", "flank3", "stride2")


@functools.lru_cache(maxsize=None)
def _tables(name):
    seqs, where, rate = _panel(name)
    rc, info, ents = lib.panel_pieces(list(seqs), where | lib.DMX_RC, rate)
    assert rc == 0 and info["step"] > 0, (name, rc, info)
    rc, pair, rank, keys = lib.panel_piece_pairs(list(seqs), where | lib.DMX_RC, rate)
    assert rc == 0
    return info, ents, pair, rank, keys


def test_strides():
    """The panels cover both paired strides."""
    assert _tables("sp5")[0]["step"] == 2 and _tables("stride2")[0]["step"] == 2
    assert _tables("flank3")[0]["step"] == 1


@pytest.mark.parametrize("name", PANELS)
def test_both_halves_hold_the_sampled_8mers(name):
    info, ents, pair, rank, keys = _tables(name)
    ks = pp.key_set(ents)
    assert len(ks) == info["keys"]
    K = np.arange(65536)
    member = np.isin(K, np.fromiter(ks, dtype=np.int64, count=len(ks))).astype(np.int64)
    assert np.array_equal(pp.single(pair, K), member)
    assert np.array_equal(pp.single_b(pair, K), member)


def _overlapped(ks):
    """Every 20-bit word built from two keys that overlap by 6 nt, and around every key the words
    with each possible 2 nt before and after it."""
    by_head = {}
    for k in ks:
        by_head.setdefault(k & 0xFFF, []).append(k)
    out = []
    for k1 in ks:
        out += [k1 | (k2 >> 12) << 16 for k2 in by_head.get(k1 >> 4, [])]
        out += [k1 | b << 16 for b in range(16)]              # k1 first, any trailing 2 nt
        out += [(k1 << 4 | a) & 0xFFFFF for a in range(16)]   # k1 second, any leading 2 nt
    return np.array(sorted(set(out)), dtype=np.int64)


@pytest.mark.parametrize("name", PANELS)
def test_paired_lookup_equals_two_single_lookups(name):
    info, ents, pair, rank, keys = _tables(name)
    ks = sorted(pp.key_set(ents))
    rng = np.random.default_rng(7)
    words = np.concatenate([rng.integers(0, 1 << 20, size=100_000), _overlapped(ks)])
    a, b = pp.paired(pair, words)
    assert np.array_equal(a, pp.single(pair, words & 0xFFFF))
    assert np.array_equal(b, pp.single(pair, (words >> 4) & 0xFFFF))
    assert a.sum() >= 16 * len(ks) and b.sum() >= 16 * len(ks)   # the words do hold hits


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("name", PANELS)
def test_step_words_of_each_pairing(name, S):
    """ps_lookups<S> as the kernel computes it (pairs q, q + 1 at S = 2; q, q + 2 in groups of
    four at S = 1; accumulators and the interleave) on 96-nt streams that hold a 20-bit word of
    the set above at every nt in turn, against one single lookup per sample."""
    info, ents, pair, rank, keys = _tables(name)
    ks = sorted(pp.key_set(ents))
    rng = np.random.default_rng(8 + S)
    words = np.concatenate([rng.integers(0, 1 << 20, size=2000), _overlapped(ks)[:6000]])
    codes = rng.integers(0, 4, size=(len(words), 96))
    at = 8 + np.arange(len(words)) % 79            # the word's first nt: 8 .. 86
    for i in range(10):
        codes[np.arange(len(words)), at + i] = (words >> (2 * i)) & 3
    got = pp.step_hits_paired(pair, codes, S)
    exp = pp.step_hits_single(pair, codes, S)
    assert [int(g) for g in got] == exp
    assert sum(1 for e in exp if e) > len(words) // 8   # the streams do hold hits


@pytest.mark.parametrize("name", PANELS)
def test_key_index_addresses_the_keys_own_entries(name):
    info, ents, pair, rank, keys = _tables(name)
    ks = sorted(pp.key_set(ents))
    seen = 0
    for i, k in enumerate(ks):
        idx = pp.key_index(pair, rank, k)
        assert idx == i
        first, count = int(keys[idx]) & 0xFFFF, int(keys[idx]) >> 16
        own = [e for e in ents if (e["val"] >> (2 * e["off"])) & 0xFFFF == k]
        assert count == len(own) and ents[first:first + count] == own
        seen += count
    assert seen == info["entries"]


def test_interleave():
    x = np.array([0x0000FFFF, 0xFFFF0000, 0x00010001, 0x80000000, 0x00008000], dtype=np.int64)
    assert pp.interleave(x).tolist() == [0x55555555, 0xAAAAAAAA, 0x3, 0x80000000, 0x40000000]


@pytest.mark.parametrize("name", ["sp5", "stride2", "flank3"])
def test_slot_reads_cover_every_sample_slot(name):
    """The GPU test's inputs: every (d, seam, strand) has a read whose copy ends in a column the
    host model marks and which the oracle assigns; at most 10 % of the cases are skipped."""
    seqs, where, rate = sc.panel(name)
    info, ents, pair, rank, keys = _tables(name)
    reads, ends, meta, stats = pp.slot_reads(np.random.default_rng(500), seqs, rate)
    assert stats["skipped"] <= 0.1 * stats["cases"], stats
    assert {(d, jj, s) for _, d, jj, s in meta} == \
        {(d, jj, s) for d in pp.SLOT_D for jj in (0, 1) for s in (0, 1)}
    for read, end, (nt, d, jj, s) in zip(reads, ends, meta):
        assert nt % 64 == d
        assert end in tph.model_marks(read, ents, info["step"], 2)[s], (d, jj, s)
    blob, offs, lens = oracle.pack_ascii(reads)
    p = lib.pack(blob, offs, lens)
    for (nt, d, jj, s), o, n in zip(meta, p.offsets.tolist(), p.lengths.tolist()):
        assert o + 24 <= nt < o + n
    w = oracle.FRONT if where == lib.DMX_FRONT else oracle.BACK
    exp = oracle.run_batch(oracle.Panel(list(seqs), w, max_errors=rate), None, blob, offs, lens,
                           mode=0, use_rc=True, threads=8)
    assert (exp["bin1"] >= 0).mean() > 0.7


def test_two_round_reads_demultiplex():
    n1, s5, n2, s27 = synth.panels(24, 24)
    reads, meta, stats = pp.two_round_reads(np.random.default_rng(501), s5, s27, 0.1)
    assert stats["skipped"] <= 0.1 * stats["cases"], stats
    assert {(d, s) for _, _, d, s in meta} == {(d, s) for d in pp.SLOT_D for s in (0, 1)}
    blob, offs, lens = oracle.pack_ascii(reads)
    p = lib.pack(blob, offs, lens)
    for (nt5, nt27, d, s), o, n in zip(meta, p.offsets.tolist(), p.lengths.tolist()):
        assert o <= nt5 < o + n and o <= nt27 < o + n
        assert nt5 % 64 == d and nt27 % 64 == (d + 32) % 64
    exp = oracle.run_batch(oracle.Panel(s5, oracle.FRONT), oracle.Panel(s27, oracle.BACK), blob,
                           offs, lens, mode=1, threads=8)
    assert (exp["bin2"] >= 0).mean() > 0.7
