"""Shared inputs of the strand-aware group alignment tests (dmx_groupalign_strands; DESIGN.md
§8g): test_groupalign_strands_host.py on the CPU, test_groupalign_strands.py on the GPU.

No new model: a flagged member must give exactly what the unflagged, unchanged code gives on a
second pack in which that member is physically its reverse complement.  turned() makes that
second input: every flagged membership points at a reverse-complemented copy appended to the
reads (a copy, not a replacement, so that one read can be forward in one group and reversed in
another), and no flags are passed.

A case is (reads, seeds, groups, strands); packed(case, kind) lays the reads out with the normal
packer or with bounds_cases.tight_pack (read 0 at nt offset 16, no pads: the 64 source positions
of a reversed query's last word then begin before the packed buffer)."""
import functools

import numpy as np

import bounds_cases as bc
import groupalign_cases as gc
import pairdist_cases as pc
from dmx import lib

LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)


def with_n(s: bytes) -> bytes:
    """s with N at its first and last position and on both sides of every 64-nt word boundary."""
    a = bytearray(s)
    for k in (0, len(a) - 1, 63, 64, 127, 128):
        if 0 <= k < len(a):
            a[k] = ord("N")
    return bytes(a)


def lengths_case():
    """Reversed members of every length of LENGTHS, N at the first, last and word-boundary
    positions; each is the first member of its group, followed by a forward mutated copy that
    meets the gapped row.  Read 0 (1 nt) and the last read are reversed members: the layout
    edges.  The seeds are related to the reverse complement, so the paths are not trivial."""
    rng = np.random.default_rng(171)
    reads, seeds, groups, strands = [], [], [], []
    fwd = []
    for m in LENGTHS:
        r = with_n(pc.rand_seq(rng, m))
        seeds.append(gc.plant(rng, pc.mutate(rng, pc.revcomp(r), 0.08)))
        fwd.append(pc.mutate(rng, pc.revcomp(r), 0.08))
        reads.append(r)
    n = len(LENGTHS)
    reads += fwd
    for k in range(n):
        groups.append([k, n + k])
        strands.append([1, 0])
    # the last read of the batch: a reversed 65-nt member of group 0, third in line
    reads.append(with_n(pc.rand_seq(rng, 65)))
    groups[0].append(len(reads) - 1)
    strands[0].append(1)
    return reads, seeds, groups, strands


def stripe_case():
    """Reversed members of more than one stripe (over 64 words: 4,200 nt and 2 * 4096 + 70 nt)
    against short seeds, each followed by a short reversed member that meets the long row."""
    rng = np.random.default_rng(172)
    a = pc.rand_seq(rng, 4200)
    b = pc.rand_seq(rng, 2 * 4096 + 70)
    ra, rb = pc.revcomp(a), pc.revcomp(b)
    reads = [a, pc.revcomp(pc.mutate(rng, ra[2000:2300], 0.05)), b,
             pc.revcomp(pc.mutate(rng, rb[3000:3100], 0.05))]
    seeds = [gc.plant(rng, pc.mutate(rng, ra[2000:2300], 0.05)),
             pc.mutate(rng, rb[3000:3100], 0.05).decode()]
    return reads, seeds, [[0, 1], [2, 3]], [[1, 1], [1, 0]]


def both_case():
    """One read forward in one group and reversed in another (and in a third, both at once)."""
    rng = np.random.default_rng(173)
    x = pc.rand_seq(rng, 150)
    reads = [x, pc.mutate(rng, x, 0.1), pc.revcomp(pc.mutate(rng, x, 0.1))]
    seeds = [pc.mutate(rng, x, 0.1).decode(), pc.mutate(rng, pc.revcomp(x), 0.1).decode(),
             gc.plant(rng, x, 0.1)]
    return reads, seeds, [[0, 1, 2], [0, 2, 1], [0, 0]], [[0, 0, 1], [1, 0, 1], [0, 1]]


def uneven_case():
    """Groups of 0, 1, 2 and 7 members with mixed flags, read 3 a member of two groups; seeds
    with '-', IUPAC and N columns."""
    rng = np.random.default_rng(174)
    base = [pc.rand_seq(rng, n, p_n=0.1) for n in (90, 150, 33, 260)]
    reads = [pc.mutate(rng, base[k % 4], 0.1) for k in range(10)]
    for k in (1, 2, 4, 5, 9):
        reads[k] = pc.revcomp(reads[k])
    seeds = [gc.plant(rng, b, 0.15) for b in base]
    return (reads, seeds, [[], [1], [3, 2], [3, 7, 0, 4, 5, 6, 9]],
            [[], [1], [0, 1], [1, 0, 0, 1, 1, 0, 1]])


def budget_case():
    """Eight groups of two members of about 1,000 nt (16 words) against seeds as long, flags
    mixed: a round's traces (about 18 bytes per word and column, 290 KB per member) come to
    more than 2 MiB, so DMX_PA_TRACE_MB=1 cuts every round into several launches."""
    rng = np.random.default_rng(175)
    reads, seeds, groups, strands = [], [], [], []
    for k in range(8):
        base = pc.rand_seq(rng, 1000 + 7 * k)
        seeds.append(gc.plant(rng, base, 0.02))
        f = [k % 2, (k // 2) % 2]
        groups.append([len(reads), len(reads) + 1])
        strands.append(f)
        reads += [pc.revcomp(pc.mutate(rng, base, 0.06)) if x else pc.mutate(rng, base, 0.06)
                  for x in f]
    return reads, seeds, groups, strands


CASES = {"lengths": lengths_case, "stripes": stripe_case, "both": both_case,
         "uneven": uneven_case, "budget": budget_case}
# (case, layout): every case on the normal pack, the short ones on the tight pack as well
RUNS = [(name, "normal") for name in CASES] + [(name, "tight") for name in CASES
                                               if name not in ("stripes", "budget")]


def turned(case):
    """(reads + reverse-complemented copies, groups pointing the flagged memberships at them)."""
    reads, _, groups, strands = case
    extra, where, out = [], {}, []
    for g, s in zip(groups, strands):
        row = []
        for r, f in zip(g, s):
            if f:
                if r not in where:
                    where[r] = len(reads) + len(extra)
                    extra.append(pc.revcomp(reads[r]))
                r = where[r]
            row.append(r)
        out.append(row)
    return list(reads) + extra, out


def packed(case, kind):
    reads = case[0]
    if kind == "tight":
        return bc.tight_pack([r.decode() for r in reads])
    return pc.pack_reads(reads)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The case, and the unflagged host result on the turned reads (paths included): what every
    flagged run must equal byte for byte.  Computed once per process; callers leave it as it is."""
    case = CASES[name]()
    reads2, groups2 = turned(case)
    exp = lib.groupalign_host(pc.pack_reads(reads2), case[1], groups2, paths=True, n_threads=16)
    return case, exp
