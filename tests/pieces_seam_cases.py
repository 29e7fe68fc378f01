"""Shared inputs and the part model of the piece screen's seam tests (test_pieces_host.py on the
CPU, test_pieces.py on the GPU).  No GPU code.

The per-part screen gives every lane one part [a, b) of a view and the copies that START in it.
A copy starting at g is found through a sampled 8-mer at x = g + off, off <= kPieceMaxOff = 3, so
a copy that starts just before b has its sample past b: the seam reads put the one surviving
piece of a K-edit adapter copy at b + d, d = -3 .. 1, at the first and last interior part
boundary, on both strands, and model_marks_parts restates the kernel's ownership and sampling
rule with the sampling reach as a parameter.
"""
import functools

import numpy as np

import test_pieces_host as tph
from dmx import lib, synth

PIECE_MAX_OFF = 3            # kPieceMaxOff (csrc/dmx_device.h): an entry's 8-mer offset, 2 bits
SEAM_D = (-3, -2, -1, 0, 1)  # the surviving piece's start relative to the part boundary

# Frozen: test_pieces_host._shared_flank_panel(default_rng(0), 12, 9, 12, 0, 30), the first seed
# whose table at -e 0.05 has stride 2 (the 21-nt adapter gives pieces of 10 and 11 nt) and pieces
# with the sampled offsets {2, 3}: their 8-mers at offsets 0 and 1 lie in the shared 9-nt prefix,
# which every adapter's first piece holds.  Literals, so that the generator may change.
STRIDE2_RATE = 0.05
STRIDE2_PANEL = [
    "TGGCCAAAATAGACCCCAAAAGGGCGTCCTTTCTGTGGTGGGGTC", "TGGCCAAAAGTGTGGCTAGGTGCCCCGTATGTGGTGGGGTC",
    "TGGCCAAAATGTGGTGGGGTC", "TGGCCAAAATGCGGCCGGGCTGTGGTGGGGTC",
    "TGGCCAAAATCCTCAGGAACTCTCATTAAGCGATTGTGGTGGGGTC", "TGGCCAAAACTTGATAGCTATAGGTTGTGGTGGGGTC",
    "TGGCCAAAACTGTGGTGGGGTC", "TGGCCAAAATGTATTACGAGGTTCCCTACACTGTGGTGGGGTC",
    "TGGCCAAAATGCTGTACTTCCCGATACCGGTGTGGTGGGGTC", "TGGCCAAAAGTTAAAGTTGTTAATATTTCAGTCTTGTGGTGGGGTC",
    "TGGCCAAAACTACCTGTGGTGGGGTC", "TGGCCAAAAATTGTGGTGGGGTC",
]


@functools.lru_cache(maxsize=None)
def panel(name):
    """(adapters, DMX_FRONT / DMX_BACK, error rate) of a seam-test panel."""
    if name == "flank3":       # stride 1, pieces with sampled offset >= 1
        _, seqs, where, rate = next(c for c in tph._flank_cases() if c[0] == "flank3")
        return tuple(seqs), where, rate
    if name == "stride2":      # stride 2, a piece with sampled offsets {2, 3}
        return tuple(STRIDE2_PANEL), lib.DMX_FRONT, STRIDE2_RATE
    if name == "sp5":          # stride 2, windows {0, 1} and {1, 2} only: the control
        return tuple(synth.panels(24, 24)[1]), lib.DMX_FRONT, 0.1
    raise KeyError(name)


PANELS = ("flank3", "stride2", "sp5")


def part_len(n, part_max):
    """Positions per part of a view of n positions (ps_part_len, csrc/dmx_kernels.hip)."""
    np_ = (n + part_max - 1) // part_max
    return (n + 15) & ~15 if np_ <= 1 else ((n + np_ - 1) // np_ + 15) & ~15


def boundaries(n, part_max):
    """The interior part boundaries of a view of n positions."""
    pl = part_len(n, part_max)
    return list(range(pl, n, pl))


def _rand(rng, k):
    return "".join(rng.choice(list("ACGT"), size=int(k)))


def seam_reads(rng, seqs, rate, info, ents, part_max, n):
    """Reads of n nt, each holding one K-edit copy of an adapter whose one surviving piece starts,
    in view 0 (the strand the kernel streams), at b + d for d in SEAM_D, at the first and the last
    interior part boundary b, forward and (when the table holds orientation 1) as the reverse
    complement.  Returns (reads, ends, strands, stats): ends[i] is the K-edit alignment's end
    column in the view that holds the adapter (view 1 when strands[i]).  stats counts the cases,
    those skipped because the piece's text occurs more than once in the mutated copy (an indel
    next to it, or a repeat), and the placements that are no case at all because the whole copy
    does not fit into [0, n) there."""
    bs = boundaries(n, part_max)
    assert len(bs) >= 2 and info["part_max"] == part_max, (n, part_max, info)
    table = {(e["val"], e["len"], e["o"]) for e in ents}
    both = any(e["o"] == 1 for e in ents)
    reads, ends, strands = [], [], []
    stats = {"cases": 0, "skipped": 0, "unfit": 0}
    for ad in seqs:
        K = tph.full_k(len(ad), rate)
        pcs = tph.pieces_of(len(ad), K)
        for survive, (r0, r1) in enumerate(pcs):
            piece = ad[r0:r1]
            for rc_read in ((False, True) if both else (False,)):
                txt = tph.revcomp(piece) if rc_read else piece
                val = sum(tph.CODE[c] << (2 * i) for i, c in enumerate(txt))
                assert (val, len(piece), int(rc_read)) in table, (ad, survive, rc_read)
                for b in (bs[0], bs[-1]):
                    for d in SEAM_D:
                        read, end = place(rng, ad, pcs, survive, n, b + d, rc_read)
                        if read is None:
                            stats[end] += 1
                            stats["cases"] += end == "skipped"
                            continue
                        stats["cases"] += 1
                        reads.append(read)
                        ends.append(end)
                        strands.append(int(rc_read))
    return reads, ends, strands, stats


def place(rng, ad, pcs, survive, n, t, rc_read):
    """A read of n nt with a copy of `ad` edited once in every piece but `survive`, whose
    surviving piece starts at position t of view 0 (of the read as it is streamed; rc_read: the
    read is the reverse complement of the text that holds the adapter).  Returns (read, the
    alignment's end column in the adapter's view), or (None, "unfit") when the whole copy does not
    fit into the read there, or (None, "skipped") when the piece's text is not found exactly once
    in the copy."""
    r0, r1 = pcs[survive]
    piece = ad[r0:r1]
    copy = tph.mutate(rng, ad, pcs, survive) if len(pcs) > 1 else ad
    ps = max(0, copy.find(piece))
    # view-0 start of the piece's copy: left + ps forward, n - (left + ps + len) reversed
    left = n - t - ps - len(piece) if rc_read else t - ps
    if left < 0 or left + len(copy) > n:
        return None, "unfit"
    if copy.count(piece) != 1 or copy.find(piece, ps + 1) >= 0:
        return None, "skipped"
    view = _rand(rng, left) + copy + _rand(rng, n - left - len(copy))
    return (tph.revcomp(view) if rc_read else view), left + len(copy)


def model_marks_parts(read, ents, step, part_max, n_orient, reach):
    """test_pieces_host.model_marks with the per-part screen's rules: the view is cut into parts
    [a, b) of part_len positions, part [a, b) samples x = a, a + step, ... < b + reach and owns
    the copies that start in it (a <= g < b) and lie inside the view (g + len <= n).  The
    kernel's rule is reach = PIECE_MAX_OFF."""
    n = len(read)
    by_key = {}
    for e in ents:
        by_key.setdefault((e["val"] >> (2 * e["off"])) & 0xFFFF, []).append(e)
    marks = [set(), set()]
    if n < 8:
        return marks
    codes = np.array([tph.CODE.get(c, 0) for c in read], dtype=np.int64)   # N read as A
    keys = np.zeros(n - 7, dtype=np.int64)
    for i in range(8):
        keys |= codes[i:n - 7 + i] << (2 * i)
    hit = np.isin(keys, np.fromiter(by_key, dtype=np.int64, count=len(by_key)))
    pl = part_len(n, part_max)
    for a in range(0, n, pl):
        b = min(n, a + pl)
        xs = np.arange(a, min(b + reach, n - 7), step)
        for x in xs[hit[xs]].tolist():
            for e in by_key[int(keys[x])]:
                g, ln = x - e["off"], e["len"]
                if g < a or g >= b or g + ln > n or e["o"] >= n_orient:
                    continue
                if any(int(codes[g + i]) != (e["val"] >> (2 * i)) & 3 for i in range(ln)):
                    continue
                pe = g + ln if e["o"] == 0 else n - g
                marks[e["o"]].update(range(max(1, pe + e["dlo"]), min(n, pe + e["dhi"]) + 1))
    return marks


FLAT_D = tuple(range(-19, 4))   # piece start relative to a flat-scan seam: the check's code
                                # window is nt [X - 3, X + 29) around the sampled nt X


def flat_seam_reads(rng, seqs, rate, flip):
    """A batch for the flat scan (64-nt lanes, 4096-nt superblocks of the packed batch): reads of
    1024 nt after a first read of 448 nt, so that with dmx_pack's offsets (learnt by packing the
    lengths once) every fourth read holds a superblock seam in its middle.  Such a read gets its
    copy's surviving piece at batch nt 4096 s + d, every other read at 64 j + d for a lane seam j
    of its own, d cycling through FLAT_D and the strand alternating (`flip` swaps the strands of
    the whole batch), adapters and surviving pieces in turn.  The first read's copy starts at the
    batch's first read nt and the last read's copy ends at its last.  Returns (reads, meta), meta[i]
    = (kind, batch nt of the piece, d, strand)."""
    n_reads = 2 + 4 * 2 * len(FLAT_D)
    lens = np.array([448] + [1024] * (n_reads - 2) + [1000], dtype=np.uint32)
    offs = np.zeros(n_reads, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    offsets = lib.pack(np.full(int(lens.sum()), ord("A"), dtype=np.uint8), offs, lens).offsets
    pairs = []
    for ad in seqs:
        pcs = tph.pieces_of(len(ad), tph.full_k(len(ad), rate))
        pairs += [(ad, pcs, s) for s in range(len(pcs))]
    order = rng.permutation(len(pairs)).tolist()
    turn = [0]

    def put(n, t, rc_read):   # the next (adapter, piece) whose mutated copy is unambiguous
        for _ in range(4 * len(pairs)):
            ad, pcs, s = pairs[order[turn[0] % len(pairs)]]
            turn[0] += 1
            read, _ = place(rng, ad, pcs, s, n, t, rc_read)
            if read is not None:
                return read
        raise AssertionError("no adapter copy fits")

    reads, meta = [], []
    n_sb = n_lane = 0
    for i in range(n_reads):
        o, n = int(offsets[i]), int(lens[i])
        if i == 0:                      # the copy starts at the first nt of the first read
            ad, pcs, s = next(p for p in pairs if p[2] == (len(p[1]) - 1 if flip else 0))
            copy = tph.mutate(rng, ad, pcs, s)
            view = _rand(rng, n - len(copy)) + copy if flip else copy + _rand(rng, n - len(copy))
            reads.append(tph.revcomp(view) if flip else view)
            meta.append(("first", o, 0, int(flip)))
            continue
        if i == n_reads - 1:            # the copy ends at the last nt of the last read
            ad, pcs, s = next(p for p in pairs if p[2] == (0 if flip else len(p[1]) - 1))
            copy = tph.mutate(rng, ad, pcs, s)
            view = copy + _rand(rng, n - len(copy)) if flip else _rand(rng, n - len(copy)) + copy
            reads.append(tph.revcomp(view) if flip else view)
            meta.append(("last", o + n - 1, 0, int(flip)))
            continue
        seam = (o + n // 2) // 4096 * 4096
        if o + 100 <= seam <= o + n - 100:
            d, strand = FLAT_D[n_sb % len(FLAT_D)], (n_sb // len(FLAT_D)) & 1
            kind, n_sb = "superblock", n_sb + 1
        else:
            d, strand = FLAT_D[n_lane % len(FLAT_D)], (n_lane // len(FLAT_D)) & 1
            seam = (o // 64 + 2 + n_lane % 12) * 64
            kind, n_lane = "lane", n_lane + 1
        strand ^= int(flip)
        reads.append(put(n, seam + d - o, bool(strand)))
        meta.append((kind, seam + d, d, strand))
    return reads, meta
