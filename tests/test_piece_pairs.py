"""GPU parity of the piece screen's paired lookups against the oracle.

The kernels answer two sampled 8-mers 2 nt apart from one LDS read.  piece_pairs_cases.slot_reads
puts the surviving piece of a K-edit adapter copy at batch nt 64 j + d for every d in 0 .. 63 and
two lane seams j, on both strands, so the piece's sampled 8-mers pass through every sample slot of
a flat-scan lane: as the first and as the second member of a pair, in the pairs whose second
8-mer takes its trailing nt from the next code word, and in the lane's last pair.  The flat scan
(packed and permuted order), the per-part screen (DMX_NO_FLAT=1) and the full filter
(DMX_NO_PIECES=1) must equal the oracle on every result byte, with neither the capacity flag nor
the mask-overflow flag set.  test_piece_pairs_host.py confirms on the CPU that the inputs are what
they claim to be.
"""
import functools

import numpy as np
import pytest

import oracle
import piece_pairs_cases as pp
import pieces_seam_cases as sc
from dmx import lib, synth

pytestmark = pytest.mark.gpu

VARIANTS = {"flat": {}, "permuted": {}, "no_flat": {"DMX_NO_FLAT": "1"},
            "no_pieces": {"DMX_NO_PIECES": "1"}}


def _assert_same(got, exp):
    got = got.view(np.uint8).reshape(len(got), -1)
    exp = exp.view(np.uint8).reshape(len(exp), -1)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} reads differ, first {bad[:10]}"


def _run(reads, panels, variant, monkeypatch):
    """Results in read order and the filter tasks of one run in a context of its own; panels:
    one (adapters, where, rate) per round."""
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    blob, offs, lens = oracle.pack_ascii(reads)
    p = lib.pack(blob, offs, lens)
    perm = None
    if variant == "permuted":
        perm = np.random.default_rng(3).permutation(p.n_reads)
        p = lib.Packed(p.seq2b, p.nmask, p.offsets[perm].copy(), p.lengths[perm].copy())
    with lib.Context(0) as c:
        for r, (seqs, where, rate) in enumerate(panels):
            c.set_panel(r, list(seqs), where | lib.DMX_RC, rate)
        c.set_mode(lib.MODE_TWO_ROUND if len(panels) == 2 else lib.MODE_SINGLE)
        got = c.run(p)
        tasks = c.stats()["filter_tasks"]
        flags = int(c.debug_fetch(lib.DBG_FLAGS, 0)[0])
    assert flags & (16 | 4) == 0, flags   # no cell outside a part's mask, no full list
    if perm is not None:
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        got = got[inv]
    return got, tasks


@functools.lru_cache(maxsize=None)
def _single_case(name):
    seqs, where, rate = sc.panel(name)
    reads, ends, meta, stats = pp.slot_reads(np.random.default_rng(500), seqs, rate)
    assert stats["skipped"] <= 0.1 * stats["cases"], stats
    assert {(d, jj, s) for _, d, jj, s in meta} == \
        {(d, jj, s) for d in pp.SLOT_D for jj in (0, 1) for s in (0, 1)}
    blob, offs, lens = oracle.pack_ascii(reads)
    w = oracle.FRONT if where == lib.DMX_FRONT else oracle.BACK
    exp = oracle.run_batch(oracle.Panel(list(seqs), w, max_errors=rate), None, blob, offs, lens,
                           mode=0, use_rc=True, threads=8)
    exp.flags.writeable = False
    assert (exp["bin1"] >= 0).mean() > 0.7
    return reads, exp


@functools.lru_cache(maxsize=None)
def _two_round_case():
    n1, s5, n2, s27 = synth.panels(24, 24)
    reads, meta, stats = pp.two_round_reads(np.random.default_rng(501), s5, s27, 0.1)
    assert stats["skipped"] <= 0.1 * stats["cases"], stats
    assert {(d, s) for _, _, d, s in meta} == {(d, s) for d in pp.SLOT_D for s in (0, 1)}
    blob, offs, lens = oracle.pack_ascii(reads)
    exp = oracle.run_batch(oracle.Panel(s5, oracle.FRONT), oracle.Panel(s27, oracle.BACK), blob,
                           offs, lens, mode=1, threads=8)
    exp.flags.writeable = False
    assert (exp["bin2"] >= 0).mean() > 0.7
    return reads, exp, ((tuple(s5), lib.DMX_FRONT, 0.1), (tuple(s27), lib.DMX_BACK, 0.1))


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["sp5", "stride2", "flank3"])
def test_every_sample_slot(name, variant, monkeypatch):
    """SP5 (stride 2), the stride-2 shared-flank panel (sampled offsets {2, 3}) and flank3
    (stride 1: samples q and q + 2 pair up): the surviving piece at every nt of a lane."""
    reads, exp = _single_case(name)
    got, tasks = _run(reads, [sc.panel(name)], variant, monkeypatch)
    _assert_same(got, exp)
    assert (tasks[0] == 0) == (variant == "no_pieces")   # the piece screen ran, or was off


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_two_rounds_one_combined_table(variant, monkeypatch):
    """Both M13 panels in a two-round run: the flat scan holds one pair table with both panels'
    keys and round-tagged entries; every read carries an SP5 and an SP27 copy, their surviving
    pieces at batch nt d and d + 32 (mod 64) for every d."""
    reads, exp, panels = _two_round_case()
    got, tasks = _run(reads, panels, variant, monkeypatch)
    _assert_same(got, exp)
    for r in (0, 1):
        assert (tasks[r] == 0) == (variant == "no_pieces")
