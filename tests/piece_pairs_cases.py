"""Shared inputs and the Python model of the piece screen's paired lookups (test_piece_pairs_host.py
on the CPU, test_piece_pairs.py on the GPU).  No GPU code.

The kernels answer two sampled 8-mers 2 nt apart from one row of a 4096-row pair table.  In the
flat scan a lane holds batch nt [64 l, 64 l + 64), so the sample at batch nt x is sample
(x mod 64) / S of its lane: slot_reads puts the surviving piece of a K-edit adapter copy at batch
nt 64 j + d for every d in 0 .. 63, which moves the piece's sampled 8-mers through every sample
slot of a lane, as the first and as the second member of a pair.
"""
import numpy as np

import pieces_seam_cases as sc
import test_pieces_host as tph
from dmx import lib

READ_NT = 256                  # a copy of <= 47 nt fits at every slot of two lane seams
SLOT_D = tuple(range(64))      # the piece's first nt, modulo the lane's 64 nt


# ---------------------------------------------------------------------------------------------
# The lookup model (csrc/dmx_kernels.hip ps_lookups, ps_key)
# ---------------------------------------------------------------------------------------------
def key_set(ents):
    """The sampled 8-mers of dmx_panel_pieces' entries."""
    return {(e["val"] >> (2 * e["off"])) & 0xFFFF for e in ents}


def single(pair, k):
    """One lookup of the 8-mer(s) k: bit k & 15 of pair[k >> 4]."""
    k = np.asarray(k, dtype=np.int64)
    return (pair[k >> 4].astype(np.int64) >> (k & 15)) & 1


def single_b(pair, k):
    """The same 8-mer through the high halves: bit 16 + (k >> 12) of pair[k & 0xFFF]."""
    k = np.asarray(k, dtype=np.int64)
    return (pair[k & 0xFFF].astype(np.int64) >> (16 + (k >> 12))) & 1


def paired(pair, K):
    """ps_row_bits on 20-bit code words K: (hit of the 8-mer at nt 0, hit of the 8-mer at nt 2)
    from ONE row; each half of the row is shifted by 4 bits of K (v_pk_lshrrev_b16)."""
    K = np.asarray(K, dtype=np.int64)
    row = pair[(K >> 4) & 0xFFF].astype(np.int64)
    lo = (row & 0xFFFF) >> (K & 15)
    hi = (row >> 16) >> ((K >> 16) & 15)
    return lo & 1, hi & 1


def interleave(x):
    """ps_interleave: bits 0..15 to the even bits, bits 16..31 to the odd ones."""
    x = np.asarray(x, dtype=np.int64)
    for sh, m in ((8, 0x0000FF00), (4, 0x00F000F0), (2, 0x0C0C0C0C), (1, 0x22222222)):
        t = (x ^ (x >> sh)) & m
        x = (x ^ t ^ (t << sh)) & 0xFFFFFFFF
    return x


def _k20(codes, u):
    """20 bits of codes from nt u of every stream (codes: [N, 96] 2-bit codes)."""
    K = np.zeros(len(codes), dtype=np.int64)
    for i in range(10):
        K |= codes[:, u + i].astype(np.int64) << (2 * i)
    return K


def step_hits_paired(pair, codes, S):
    """ps_lookups<S> on streams of 96 nt (positions C - 16 .. C + 80): the hits word, bit q =
    sample C + q S, computed as the kernel does (pair accumulators, one interleave per word)."""
    if S == 4:
        hits = np.zeros(len(codes), dtype=np.int64)
        for q in range(16):
            hits |= single(pair, _k20(codes, 16 + 4 * q) & 0xFFFF) << q
        return hits
    acc = [np.zeros(len(codes), dtype=np.int64) for _ in range(2)]
    for p in range(16):
        for j in range(2 // S):
            a, b = paired(pair, _k20(codes, 16 + 4 * p + j))
            acc[j] |= (a | (b << 16)) << p
    if S == 2:
        return interleave(acc[0])
    e0, e1 = interleave(acc[0]), interleave(acc[1])   # bit i of e[j] = sample 2i + j
    lo = interleave((e0 & 0xFFFF) | ((e1 << 16) & 0xFFFFFFFF))
    hi = interleave((e0 >> 16) | (e1 & 0xFFFF0000))
    return [int(h) << 32 | int(l) for h, l in zip(hi.tolist(), lo.tolist())]


def step_hits_single(pair, codes, S):
    """The same word from one single lookup per sample."""
    out = [0] * len(codes)
    for q in range(64 // S):
        h = single(pair, _k20(codes, 16 + q * S) & 0xFFFF).tolist()
        out = [o | (b << q) for o, b in zip(out, h)]
    return out


def key_index(pair, rank, k):
    """ps_key: the number of sampled 8-mers below k (k is sampled)."""
    r, a = k >> 4, k & 15
    idx = int(rank[r >> 2])
    for rr in range(r & ~3, r):
        idx += bin(int(pair[rr]) & 0xFFFF).count("1")
    return idx + bin(int(pair[r]) & ((1 << a) - 1)).count("1")


# ---------------------------------------------------------------------------------------------
# Reads with the surviving piece in every sample slot of a lane
# ---------------------------------------------------------------------------------------------
def _offsets(lens):
    lens = np.asarray(lens, dtype=np.uint32)
    offs = np.zeros(len(lens), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return lib.pack(np.full(int(lens.sum()), ord("A"), dtype=np.uint8), offs, lens).offsets


def _pairs(seqs, rate):
    out = []
    for ad in seqs:
        pcs = tph.pieces_of(len(ad), tph.full_k(len(ad), rate))
        out += [(ad, pcs, s) for s in range(len(pcs))]
    return out


class _Turns:
    """(adapter, surviving piece) in a shuffled round robin; counts the cases (placements where
    the copy fits the read) and those skipped because the piece's text is not unique."""

    def __init__(self, rng, seqs, rate):
        self.rng, self.pairs = rng, _pairs(seqs, rate)
        self.order = rng.permutation(len(self.pairs)).tolist()
        self.turn = 0
        self.stats = {"cases": 0, "skipped": 0, "unfit": 0}

    def put(self, n, t, rc_read):
        for _ in range(4 * len(self.pairs)):
            ad, pcs, s = self.pairs[self.order[self.turn % len(self.pairs)]]
            self.turn += 1
            read, end = sc.place(self.rng, ad, pcs, s, n, t, rc_read)
            if read is None:
                self.stats[end] += 1
                self.stats["cases"] += end == "skipped"
                continue
            self.stats["cases"] += 1
            return read, end
        raise AssertionError("no adapter copy fits")


def slot_reads(rng, seqs, rate):
    """One read of READ_NT nt per (d, lane seam, strand): the surviving piece of a K-edit copy
    starts at batch nt 64 j + d, d in SLOT_D, for the first two lane starts j at least 24 nt into
    the read (dmx_pack's offsets, learnt by packing the lengths once), forward and reverse
    complemented.  Returns (reads, ends, meta, stats): ends[i] = the alignment's end column in the
    adapter's view, meta[i] = (batch nt of the piece, d, which seam, strand)."""
    n_reads = len(SLOT_D) * 2 * 2
    offsets = _offsets([READ_NT] * n_reads).tolist()
    turns = _Turns(rng, seqs, rate)
    reads, ends, meta = [], [], []
    i = 0
    for d in SLOT_D:
        for jj in (0, 1):
            for strand in (0, 1):
                o = int(offsets[i])
                nt = ((o + 24 + 63) // 64 + jj) * 64 + d
                read, end = turns.put(READ_NT, nt - o, bool(strand))
                reads.append(read)
                ends.append(end)
                meta.append((nt, d, jj, strand))
                i += 1
    return reads, ends, meta, turns.stats


def two_round_reads(rng, sp5, sp27, rate):
    """Reads with a K-edit SP5 copy and, downstream on the same strand, a K-edit SP27 copy: the
    SP5 copy's surviving piece starts at batch nt 64 j + d and the SP27 copy's at 64 j' + d + 32
    (mod 64), d in SLOT_D, both strands.  Both panels' keys are in the one combined table the
    flat scan holds for a two-round run."""
    half = READ_NT
    n_reads = len(SLOT_D) * 2
    offsets = _offsets([2 * half] * n_reads).tolist()
    t5, t27 = _Turns(rng, sp5, rate), _Turns(rng, sp27, rate)
    reads, meta = [], []
    i = 0
    for d in SLOT_D:
        for strand in (0, 1):
            o = int(offsets[i])
            # streamed order: the SP5 half first on strand 0, last on strand 1
            o5, o27 = (o, o + half) if strand == 0 else (o + half, o)
            nt5 = ((o5 + 24 + 63) // 64) * 64 + d
            nt27 = ((o27 + 24 + 63) // 64) * 64 + (d + 32) % 64
            a, _ = t5.put(half, nt5 - o5, bool(strand))
            b, _ = t27.put(half, nt27 - o27, bool(strand))
            reads.append(a + b if strand == 0 else b + a)
            meta.append((nt5, nt27, d, strand))
            i += 1
    stats = {k: t5.stats[k] + t27.stats[k] for k in t5.stats}
    return reads, meta, stats
