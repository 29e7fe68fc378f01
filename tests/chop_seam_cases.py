"""Shared inputs of the chop kernels' structure tests (test_chop_seams_host.py on the CPU,
test_chop_seams.py on the GPU).  No GPU code.

csrc/dmx_chop.hip gives a lane the columns (s0, s0 + 512] of one read for one label, after a
warm-up of m + k columns, keeps the minimum columns of every run of D <= k as a first column and
a 64-bit offset mask, stores a 64-read block's hits in a 512-entry LDS list and has the blocks
that overflow it redone by chop_big_kernel.  Every case here aims at one of those edges:

  A  copies whose stop lies on chosen columns around the seams 512 and 1024, copies that start
     at the warm-up limit, copies on a read's first and last column, and runs of D <= k that
     straddle a seam with their minimum on a known side; primer lengths on both sides of the
     32-bit word seam (the three chop_kernel<HB> variants)
  B  runs of 64 and more columns at one cost (the mid-run flush)
  C  a block with exactly 512 and 513 stored hits
  D  several redone blocks among plain ones, a last block with fewer than 64 reads, a hit
     staging overflow, and smaller batches afterwards on the same context
  E  a segment staging overflow
  F  more than 1024 blocks (chop_blkscan_kernel with two blocks per thread) and block edges in
     the read count
  G  hits of two labels on the same interval (a palindromic primer), in a plain and a redone block

One generator, deterministic: every case is rebuilt alone from its id with its own
default_rng([SEED, k]), k = the case's position in its list.
"""
import functools

import numpy as np

import chopper as ochop

SEED = 8804
SEG = 512        # kChopSeg: columns owned by one scan lane
READS = 64       # kChopReads: reads per block
HIT_CAP = 512    # kChopHitCap: LDS hit list per block
SEAMS = (512, 1024)
DRAWS = 50       # background draws per case before the generator gives up

_BITS = {"A": 1, "C": 2, "G": 4, "T": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3,
         "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}


def rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), size=int(n)))


# ---- the column DP -------------------------------------------------------------------------

def dp_cols(pat, read, first=0):
    """D(j) for j = 0 .. len(read): the least edit distance of `pat` (IUPAC) to a piece of
    `read` that ends at column j (after read[j - 1]) and starts at column `first` or later; a
    read character outside ACGT matches anything.  D(j) = m for j <= first.  Plain numpy, one
    column at a time: tmp = min(prev[i-1] + cost, prev[i] + 1), then the running minimum along
    the column (cur[i] = min over i' <= i of tmp[i'] + i - i')."""
    m, n = len(pat), len(read)
    ar = np.arange(m + 1, dtype=np.int64)
    bits = np.array([_BITS[c] for c in pat.upper()], dtype=np.int64)
    cost = np.ones((5, m), dtype=np.int64)
    for c in range(4):
        cost[c] = 1 - ((bits >> c) & 1)
    cost[4] = 0
    codes = ["ACGT".find(c) for c in read.upper()]
    D = np.full(n + 1, m, dtype=np.int64)
    prev = ar.copy()
    tmp = np.zeros(m + 1, dtype=np.int64)
    for j in range(first + 1, n + 1):
        np.minimum(prev[:-1] + cost[codes[j - 1]], prev[1:] + 1, out=tmp[1:])
        prev = ar + np.minimum.accumulate(tmp - ar)
        D[j] = prev[m]
    return D


# ---- stratum A: seams ----------------------------------------------------------------------

A_PANELS = (("low", (5, 31, 32)), ("high", (33, 58, 64)), ("mix32", (32, 33)), ("mix1", (1, 64)))
A_CUTOFFS = (0.0, 0.2)
A_ENDS = (511, 512, 513, 1024, 1025)
A_STOPS = (-1, 0, 1, 2)       # the planted stop relative to the seam
A_WARM = (-1, 0, 1)           # the copy's first column relative to s0 - (m + k)
EDITS = ("sub", "ins", "del")


@functools.lru_cache(maxsize=None)
def a_primers(panel):
    """Primers of a stratum-A panel.  The short ones (< 20 nt) are over AT, so that a CG
    background holds no column with D <= k for them."""
    lens = dict(A_PANELS)[panel]
    rng = np.random.default_rng([SEED, 900 + [p for p, _ in A_PANELS].index(panel)])
    return tuple((f"P{i}", rand(rng, m, "AT" if m < 20 else "ACGT")) for i, m in enumerate(lens))


def a_rules(panel):
    nl = 2 * len(a_primers(panel))
    return [(a, (a + 3) % nl, a & 1) for a in range(0, nl, 2)] + [(1, 1, 0)]


@functools.lru_cache(maxsize=None)
def a_specs():
    """Every stratum-A case: (panel, cutoff, kind, label, seam, delta, edits, edit kind).
    kind stop: the copy's stop at seam + delta; warm: a copy of m + k columns (k insertions)
    whose first column is seam - (m + k) + delta; left / right: an exact copy whose run of
    D <= k covers seam and seam + 1, its minimum at seam + delta on the named side (k >= 2);
    last / first: a copy on the last / first column of a read of `seam` nt."""
    out = []
    turn = 0
    for panel, _ in A_PANELS:
        labs = ochop.labels(a_primers(panel))
        for cutoff in A_CUTOFFS:
            for lab, (_, s) in enumerate(labs):
                k = int(cutoff * len(s))
                for s0 in SEAMS:
                    for d in A_STOPS:
                        e = turn % (k + 1)
                        out.append((panel, cutoff, "stop", lab, s0, d, e, EDITS[turn % 3]))
                        turn += 1
                    for d in A_WARM:
                        out.append((panel, cutoff, "warm", lab, s0, d, k, "ins"))
                    if k >= 2:
                        out += [(panel, cutoff, "left", lab, s0, d, 0, "sub") for d in (-1, 0)]
                        out += [(panel, cutoff, "right", lab, s0, d, 0, "sub") for d in (1, 2)]
                n = A_ENDS[len([o for o in out if o[2] == "last"]) % len(A_ENDS)]
                for kind in ("last", "first"):
                    if n >= len(s) + k:
                        out.append((panel, cutoff, kind, lab, n, 0, turn % (k + 1),
                                    EDITS[turn % 3]))
                    turn += 1
    return tuple(out)


def a_id(spec):
    panel, cutoff, kind, lab, s0, d, e, ek = spec
    return f"A/{panel}/{cutoff}/{kind}/L{lab}/s{s0}{d:+d}/{e}{ek}"


def _edited(rng, lab, e, kind, alphabet):
    """`lab` (over ACGT) with e edits of one kind at interior positions."""
    s = list(lab)
    if e == 0:
        return lab
    pos = sorted(rng.choice(np.arange(2, len(s) - 1), size=e, replace=False).tolist(),
                 reverse=True)
    for p in pos:
        if kind == "del":
            del s[p]
            continue
        near = {s[p], s[p - 1]}
        pick = [c for c in alphabet if c not in near] or [c for c in "ACGT" if c not in near]
        c = pick[int(rng.integers(len(pick)))]
        if kind == "sub":
            s[p] = c
        else:
            s.insert(p, c)
    return "".join(s)


@functools.lru_cache(maxsize=None)
def a_case(idx):
    """Case idx of a_specs(), built alone: (read, label sequence, k, stop, D).  The background
    is redrawn until the label's only columns with D <= k are those within k of the planted
    stop and the stop is a minimum of the read at the designed cost (left / right: the one
    minimum)."""
    panel, cutoff, kind, lab, s0, d, e, ek = a_specs()[idx]
    pat = ochop.labels(a_primers(panel))[lab][1]
    m = len(pat)
    k = int(cutoff * m)
    bg = "CG" if m < 20 else "ACGT"
    rng = np.random.default_rng([SEED, idx])
    for _ in range(DRAWS):
        copy = _edited(rng, pat, e, ek, bg)
        if kind == "warm":
            left = s0 - (m + k) + d
        elif kind == "first":
            left = 0
        elif kind == "last":
            left = s0 - len(copy)
        else:
            left = s0 + d - len(copy)
        stop = left + len(copy)
        n = s0 if kind in ("first", "last") else stop + int(rng.integers(0, 70))
        if left < 0:
            raise AssertionError(f"{a_id(a_specs()[idx])}: the copy does not fit")
        read = rand(rng, left, bg) + copy + rand(rng, n - stop, bg)
        D = dp_cols(pat, read)
        low = np.flatnonzero(D[1:] <= k) + 1
        one = kind not in ("left", "right") or int((D[1:] == e).sum()) == 1
        if int(D[stop]) == e and int(D[1:].min()) == e and one \
                and int(np.abs(low - stop).max()) <= k:
            return read, pat, k, stop, D
    raise AssertionError(f"{a_id(a_specs()[idx])}: no background in {DRAWS} draws")


# ---- batches -------------------------------------------------------------------------------

def _blocks(rng, blocks, filler=12):
    """Reads laid out block by block: every list of `blocks` but the last is filled up to 64
    reads with empty and short (<= `filler` nt) reads."""
    out = []
    for i, b in enumerate(blocks):
        out += list(b)
        if i + 1 < len(blocks):
            out += [rand(rng, rng.integers(0, filler + 1)) if j % 3 else ""
                    for j in range(READS - len(b))]
    return out


def _batch(primers, rules, cutoff, keep, seqs, big=None, **more):
    return dict(primers=list(primers), rules=list(rules), cutoff=cutoff, keep=keep,
                seqs=list(seqs), big=big, **more)


def _a_batch(panel, cutoff):
    idx = [i for i, s in enumerate(a_specs()) if s[0] == panel and s[1] == cutoff]
    return _batch(a_primers(panel), a_rules(panel), cutoff, bool(len(idx) & 1),
                  [a_case(i)[0] for i in idx], cases=idx)


def _tandem(rng, unit, n):
    return (unit * (int(n) // len(unit) + 1))[:int(n)]


def _b_alln(rng):
    m = 20
    p = [("P0", rand(rng, m))]
    own = [["N" * (m + x)] for x in (62, 63, 64, 65, 130)]
    return _batch(p, [(0, 1, 0), (1, 0, 1)], 0.2, True,
                  _blocks(rng, own + [["N" * (m + 130)] * 3]), big=1)


def _b_nprimer(rng):
    m = 20
    own = [[rand(rng, m + x)] for x in (62, 63, 64, 65, 130)]
    return _batch([("PN", "N" * m)], [(0, 1, 0)], 0.0, False,
                  _blocks(rng, own + [[rand(rng, 300)]]), big=1)


def _b_nstretch(rng):
    def read(a):
        return rand(rng, a) + "N" * 200 + rand(rng, 700 - a - 200)
    return _batch([("P0", rand(rng, 20))], [(0, 1, 0), (1, 0, 1)], 0.2, True,
                  _blocks(rng, [[read(412)], [read(450), read(400)]], filler=10), big=1)


def _b_homo(rng):
    m = 16
    own = [["A" * (m + x)] for x in (62, 63, 64, 65)] + [["T" * (m + 64)]]
    return _batch([("PA", "A" * m)], [(0, 0, 0), (1, 1, 1)], 0.2, True,
                  _blocks(rng, own + [["A" * 600]], filler=8), big=1)


def _c(rng, extra):
    """Block 1 of 3 holds 64 reads of 8 exact primer copies each: 512 hits, all with D = 0
    (cutoff 0.0), so the kernel stores as many hits as the oracle counts; `extra` adds a ninth
    copy to one read."""
    primers = [(f"P{i}", rand(rng, 20)) for i in range(4)]
    labs = ochop.labels(primers)

    def plain():
        s = rand(rng, rng.integers(0, 200))
        return s + labs[int(rng.integers(8))][1] if rng.random() < 0.3 else s

    def full(n):
        return "".join(rand(rng, rng.integers(10, 31)) + labs[int(rng.integers(8))][1]
                       for _ in range(n)) + rand(rng, rng.integers(0, 20))
    b0 = [plain() for _ in range(READS)]
    b1 = [full(8) for _ in range(READS)]
    b2 = [plain() for _ in range(40)]
    tail = rand(rng, 15) + labs[int(rng.integers(8))][1]
    if extra:
        b1[17] += tail
    return _batch(primers, [(0, 3, 0), (2, 1, 1)], 0.0, True, b0 + b1 + b2, big=int(extra))


PAL = "ACGTACGTACGT"   # its own reverse complement: labels 2p and 2p + 1 hit the same intervals


def _d_panel(rng):
    return [("T6", "ACCTGA"), ("PAL", PAL)], [(0, 0, 0), (2, 3, 0), (3, 2, 1), (0, 2, 1)]


def _pal_read(rng):
    s = rand(rng, rng.integers(0, 60))
    for _ in range(int(rng.integers(1, 4))):
        s += PAL * int(rng.integers(1, 3)) + rand(rng, rng.integers(0, 40))
    return s


def _d(rng, shape):
    """shape: per block (reads, tandem reads of the 6-nt primer among them); the rest are plain
    reads, every fifth with copies of the palindromic primer."""
    primers, rules = _d_panel(rng)
    seqs = []
    for nr, nt in shape:
        blk = [_tandem(rng, "ACCTGA", rng.integers(600, 1201)) for _ in range(nt)]
        blk += [_pal_read(rng) if j % 5 == 0 else rand(rng, rng.integers(0, 200))
                for j in range(nr - nt)]
        seqs += [blk[i] for i in rng.permutation(nr)]
    return _batch(primers, rules, 0.0, True, seqs, big=sum(1 for _, nt in shape if nt))


D_SHAPES = {"D/five": ((64, 0), (64, 14), (64, 0), (64, 18), (20, 15)),
            "D/reuse": ((64, 6), (30, 0)),
            "D/none": ((50, 0),)}


def _e(rng, keep):
    primers = [("T6", "ACCTGA")]
    seqs = [rand(rng, rng.integers(0, 200)) for _ in range(10)]
    for i in (1, 4, 8):
        seqs[i] = _tandem(rng, "ACCTGA", rng.integers(20000, 20400))
    return _batch(primers, [(0, 0, 0)], 0.0, keep, seqs, big=1)


def _amplicons(rng, primers, n, pool=300, every=37):
    """n reads: empty or one of `pool` reads of 1..12 nt, every `every`-th a short amplicon of
    the two primers around a 20-nt insert, on either strand."""
    short = [""] * (pool // 3) + [rand(rng, rng.integers(1, 13)) for _ in range(pool - pool // 3)]
    pick = rng.integers(0, len(short), size=n)
    seqs = [short[i] for i in pick.tolist()]
    for r in range(every - 1, n, every):
        s = primers[0][1] + rand(rng, 20) + ochop.revcomp(primers[1][1])
        seqs[r] = ochop.revcomp(s) if rng.random() < 0.5 else s
    return seqs


def _f(rng, n, tail_empty=0):
    primers = [("F0", rand(rng, 12)), ("F1", rand(rng, 12))]
    seqs = _amplicons(rng, primers, n, every=37 if n > 100 else min(5, n))
    if tail_empty:
        seqs += [""] * tail_empty
    return _batch(primers, [(0, 3, 0), (2, 1, 1)], 0.1, True, seqs, big=0)


def _f_empty(rng):
    return _batch([("F0", rand(rng, 12))], [(0, 1, 0)], 0.1, True, [""] * 70, big=0)


def _g(rng, redo):
    primers, rules = _d_panel(rng)
    seqs = [_pal_read(rng) if j % 2 == 0 else rand(rng, rng.integers(0, 200)) for j in range(40)]
    if redo:
        for j in (3, 9, 15, 21, 27, 33):
            seqs[j] = _tandem(rng, "ACCTGA", rng.integers(600, 1201))
    return _batch(primers, rules + [(2, 2, 0), (3, 3, 1)], 0.0, True, seqs, big=int(redo))


BATCHES = tuple(
    [(f"A/{p}/{c}", functools.partial(lambda rng, p, c: _a_batch(p, c), p=p, c=c))
     for p, _ in A_PANELS for c in A_CUTOFFS] +
    [("B/alln", _b_alln), ("B/nprimer", _b_nprimer), ("B/nstretch", _b_nstretch),
     ("B/homo", _b_homo),
     ("C/512", functools.partial(_c, extra=False)), ("C/513", functools.partial(_c, extra=True))] +
    [(name, functools.partial(_d, shape=shape)) for name, shape in D_SHAPES.items()] +
    [("E/keep", functools.partial(_e, keep=True)), ("E/trim", functools.partial(_e, keep=False)),
     ("F/70001", functools.partial(_f, n=70001)), ("F/1", functools.partial(_f, n=1)),
     ("F/63", functools.partial(_f, n=63)), ("F/64", functools.partial(_f, n=64)),
     ("F/65", functools.partial(_f, n=65)), ("F/empty", _f_empty),
     ("F/tail", functools.partial(_f, n=64, tail_empty=10)),
     ("G/plain", functools.partial(_g, redo=False)), ("G/redo", functools.partial(_g, redo=True))])
NAMES = tuple(n for n, _ in BATCHES)
# C/513 is C/512 with one more copy: the two are built from the same draws
_SAME_DRAWS = {"C/513": "C/512", "E/trim": "E/keep", "G/redo": "G/plain"}


def stratum(letter):
    return [n for n in NAMES if n.startswith(letter + "/")]


@functools.lru_cache(maxsize=None)
def batch(name):
    """A batch by its id, built alone: primers, rules, cutoff, keep, seqs, and big = the number
    of blocks chop_big_kernel must redo where that is fixed by the input (None: it depends on
    the timing of the cross-lane pruning)."""
    k = NAMES.index(_SAME_DRAWS.get(name, name))
    return dict(BATCHES)[name](np.random.default_rng([SEED, 10000 + k]))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's (hits, segments) of a batch as (read, label, dist, start, stop) and
    (read, start, stop, strand, rule), in read order; the oracle runs once per distinct read."""
    b = batch(name)
    labs = ochop.labels(b["primers"])
    cache = {}
    H, S = [], []
    for r, s in enumerate(b["seqs"]):
        if s not in cache:
            hs = ochop.read_hits(labs, s, b["cutoff"]) if s else []
            cache[s] = (hs, ochop.segments(hs, b["rules"], b["keep"]))
        hs, sg = cache[s]
        H += [(r, lab, d, a, z) for a, z, lab, d in hs]
        S += [(r, a, z, st, ri) for a, z, st, ri in sg]
    return H, S


def block_hits(name):
    """The oracle's hit count per 64-read block."""
    n = len(batch(name)["seqs"])
    return np.bincount([h[0] // READS for h in expected(name)[0]],
                       minlength=(n + READS - 1) // READS)


def low_cols_blocks(name):
    """Per 64-read block, the columns with D <= k over all reads and labels (numpy DP): no
    lane can store more hits than that, whatever the timing of the cross-lane pruning."""
    b = batch(name)
    labs = ochop.labels(b["primers"])
    n = len(b["seqs"])
    out = np.zeros((n + READS - 1) // READS, dtype=np.int64)
    cache = {}
    for r, s in enumerate(b["seqs"]):
        if s not in cache:
            cache[s] = sum(int((dp_cols(p, s)[1:] <= int(b["cutoff"] * len(p))).sum())
                           for _, p in labs if len(s) >= len(p) - int(b["cutoff"] * len(p)))
        out[r // READS] += cache[s]
    return out
