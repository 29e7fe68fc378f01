"""Shared inputs of the end-window stage's structure tests (test_ends_struct_host.py on the CPU,
test_ends_struct.py on the GPU).  No GPU code.

csrc/dmx_ends.hip gives a lane one (view, orientation, restricted adapter) triple per step of a
grid-stride loop, queues the prefilter's survivors in an LDS queue of 2 * kEndsBlock entries,
drains the top kEndsBlock of them whenever the queue holds that many and the rest after the loop.
ends_cases.py pins `locate` on single short reads; every stratum here aims at the structure
around it:

  Q  queue drains: a 24-adapter panel with a shared 25-nt prefix over a batch in which every
     block makes 12 loop steps and most triples of a carrier survive the prefilter, in a band
     round (-e 0.2) and a ring round (-e 0.3); batches whose last block-step holds 1, 127, 128
     and 129 triples
  R  round 1 over the item views round 0 left (DMX_MODE_TWO_ROUND): regular and non-internal
     round 0, XA / AX and mixed panels in round 1, a ring round 1, one winner slot per
     orientation, views of 0, 1 and 2 nt
  W  panel width: 48 adapters that share a prefix, 64 restricted adapters, 32 regular among 32
     restricted ones, a tie between indices 0 and 63
  L  reads of 255 .. 200,003 nt at chosen offsets, window starts j0 = 0, 1 and 16

Chain of trust: the GPU is compared with dmx_ends_host on all 40 bytes of every record; the CPU
half compares dmx_ends_host with the Python demux oracle on the distinct reads of every stratum.
Every stratum draws from its own default_rng([SEED, k]).
"""
from __future__ import annotations

import functools
import json
import os
from dataclasses import dataclass, field

import numpy as np

import ends_cases as ec
from ends_cases import BACKX, FRONTX, PREFIX, RESTRICTED, SUFFIX, _place, _rand, _sub, revcomp
from dmx import lib

F, B = ec.F, ec.B
SEED = 6116
# mirrored from csrc/dmx_ends.hip; test_ends_struct_host.py reads both constexpr lines there
ENDS_BLOCK = 128     # kEndsBlock: triples per block-step, and the size of one mid-loop drain
ENDS_GRID = 2048     # kEndsGrid: the largest grid
QUEUE_CAP = 2 * ENDS_BLOCK   # s_qi / s_qs

NAMES = {PREFIX: "prefix", FRONTX: "frontx", SUFFIX: "suffix", BACKX: "backx"}


def panel_kk(e: float, m: int) -> int:
    return int(ec.rate_of(e, m) * m)


@functools.lru_cache(maxsize=None)
def shared_panel() -> tuple:
    """24 adapters of 30 nt: one random 25-nt prefix, 24 5-nt tails that differ within their
    first four characters (the shape of the benchmark's and the workflow's panel; an AX copy
    without its last character still names its adapter)."""
    rng = np.random.default_rng([SEED, 0])
    prefix = _rand(rng, 25)
    tails = {}
    while len(tails) < 24:
        t = _rand(rng, 5)
        tails.setdefault(t[:4], t)
    return tuple(prefix + t for t in sorted(tails.values()))


# ---- stratum Q: queue drains ---------------------------------------------------------------

Q_E = (0.2, 0.3)          # m = 30: k = 6, a band round / k = 9, a ring round
Q_BASE = 600
Q_STEPS = 12              # loop steps of every block in the large batch
Q_SPECS = tuple((w, e) for w in RESTRICTED for e in Q_E)
Q_TAILS = (1, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def q_base(where: int, e: float) -> tuple:
    """600 distinct reads of 45-90 nt.  Seven of every ten carry one adapter of the shared
    panel, with 0-1 substitutions in the shared prefix, at the end `where` needs; half of the
    carriers are stored reverse-complemented.  Carriers and random reads alternate in a fixed
    pattern, so every block-step of the tiled batch meets about the same share of survivors.
    Under -e 0.3 ten carriers have 8 substitutions: a band round would flag their cost."""
    rng = np.random.default_rng([SEED, 10 + Q_SPECS.index((where, e))])
    seqs = shared_panel()
    reads = []
    carriers = 0
    for i in range(Q_BASE):
        n = int(rng.integers(45, 91))
        if i % 10 < 7:
            ad = seqs[int(rng.integers(24))]
            nsub = int(rng.integers(0, 2))
            if e > 0.25 and carriers % 40 == 7:
                nsub = 8
            piece = _sub(rng, ad[:25], nsub) + ad[25:]
            r = _place(where, piece, _rand(rng, n - 30))
            reads.append(revcomp(r) if rng.random() < 0.5 else r)
            carriers += 1
        else:
            reads.append(_rand(rng, n))
    return tuple(reads)


def q_reps(steps: int = Q_STEPS) -> int:
    """Copies of the base so that every block of a full grid makes `steps` loop steps."""
    need = steps * ENDS_GRID * ENDS_BLOCK
    return -(-need // (Q_BASE * 48))


@functools.lru_cache(maxsize=None)
def q_host(where: int, e: float) -> np.ndarray:
    return ec.host_round(list(shared_panel()), [where] * 24, list(q_base(where, e)), True, e, 3)


@functools.lru_cache(maxsize=None)
def q_accepted(where: int, e: float) -> np.ndarray:
    """acc[read, o, adapter]: the exact DP accepts this triple (dmx_ends_host with one-adapter
    panels, on the reads and on their reverse complements).  Accepted implies that the
    prefilter passes: a lower bound on what reaches the queue."""
    base = list(q_base(where, e))
    flip = [revcomp(r) for r in base]
    acc = np.zeros((len(base), 2, 24), dtype=bool)
    for a, s in enumerate(shared_panel()):
        for o, reads in enumerate((base, flip)):
            acc[:, o, a] = ec.host_round([s], [where], reads, False, e, 3)["bin1"] >= 0
    return acc


def q_plan(acc: np.ndarray, reps: int) -> dict:
    """The queue of every block on the accepted arrivals alone, laid out as the kernel does:
    triple ti = item * T + o * nE + e runs in block (ti / 128) % grid at step ti / (128 * grid);
    a step's arrivals join the queue, then 128 are drained if it holds that many."""
    flat = np.tile(acc.reshape(len(acc), -1), (reps, 1)).reshape(-1)
    total = len(flat)
    chunks = -(-total // ENDS_BLOCK)
    grid = min(chunks, ENDS_GRID)
    steps = -(-chunks // grid)
    arr = np.zeros(steps * grid * ENDS_BLOCK, dtype=np.int64)
    arr[:total] = flat
    arr = arr.reshape(steps, grid, ENDS_BLOCK).sum(axis=2)
    q = np.zeros(grid, dtype=np.int64)
    peak = np.zeros(grid, dtype=np.int64)
    drains = np.zeros(grid, dtype=np.int64)
    partial = np.zeros(grid, dtype=bool)       # some drain left 1..127 entries below it
    for s in range(steps):
        q += arr[s]
        peak = np.maximum(peak, q)
        d = q >= ENDS_BLOCK
        q[d] -= ENDS_BLOCK
        drains += d
        partial |= d & (q > 0)
    return {"total": total, "grid": grid, "steps": steps, "accepted": int(flat.sum()),
            "per_block": arr.sum(axis=0), "peak": peak, "drains": drains, "partial": partial}


def q_tail_case(where: int, r: int) -> tuple:
    """(seqs, rc, n_reads): a batch whose triples are full block-steps and a last one of r
    (129: a full one and a single triple), on fewer blocks than ENDS_GRID.  T = 48 only reaches
    multiples of 16, so the odd values take 23 adapters and one orientation."""
    seqs = list(shared_panel())
    if r % 16 == 0:
        rc, T = True, 48
    else:
        seqs, rc, T = seqs[:23], False, 23
    for n in range(20, 2000):
        total = n * T
        if total % ENDS_BLOCK == r % ENDS_BLOCK and total > 2 * ENDS_BLOCK + r:
            return seqs, rc, n
    raise AssertionError((where, r))


def q_tail_reads(where: int, n: int) -> list:
    base = q_base(where, 0.2)
    return [base[i % len(base)] for i in range(n)]


# ---- two-round and single-round cases ------------------------------------------------------

@dataclass
class Case:
    """One batch: round 0's panel, for stratum R round 1's too.  rN = (seqs, wheres, rc, e, -O)."""
    name: str
    r0: tuple
    r1: tuple = None
    reads: list = field(default_factory=list)
    labels: list = field(default_factory=list)
    offsets: list = None          # stratum L: the batch is packed with ec._pack_at

    def add(self, label, read):
        self.reads.append(read)
        self.labels.append(label)

    def packed(self):
        if self.offsets is not None:
            return ec._pack_at(self.reads, self.offsets)
        blob, offs, lens = ec.oracle.pack_ascii(self.reads)
        return lib.pack(blob, offs, lens)

    def _expected(self, single):
        if self.r1 is not None:
            return ec.two_round_expected(self.reads, self.r0, self.r1, single)
        s, w, rc, e, o = self.r0
        if single is ec.host_round and self.offsets is not None:
            return lib.ends_host(s, w, self.packed(), rc, e, o)
        return single(s, w, self.reads, rc, e, o)

    def host(self) -> np.ndarray:
        if getattr(self, "_host", None) is None:
            self._host = self._expected(ec.host_round)
        return self._host

    def oracle(self) -> np.ndarray:
        return self._expected(ec.demux)


def _shuffled(rng, c: Case) -> Case:
    order = rng.permutation(len(c.reads))
    c.reads = [c.reads[i] for i in order]
    c.labels = [c.labels[i] for i in order]
    return c


# ---- stratum R: round 1 over item views ----------------------------------------------------

R_NAMES = ("reg_suffix", "reg_backx", "noni_both", "mixed", "ring", "oslot", "tiny_e1",
           "tiny_e01")


def _r_view(rng, w, ad, n_body, nsub=0, keep=None):
    """A round-1 view with `ad` (or, for the non-internal types, the `keep` characters next to
    the view's end) where type w looks for it."""
    piece = _sub(rng, ad, nsub) if nsub else ad
    if keep is not None:
        piece = piece[len(piece) - keep:] if w & F else piece[:keep]
    return _place(w, piece, _rand(rng, n_body))


@functools.lru_cache(maxsize=None)
def r_case(name: str) -> Case:
    rng = np.random.default_rng([SEED, 100 + R_NAMES.index(name)])
    a0 = [_rand(rng, 24) for _ in range(3)]
    reg0 = (a0, [F] * 3, True, 0.1, 3)
    pre0 = (a0, [PREFIX] * 3, True, 0.1, 3)

    def front(i, view, regular=True, nsub=None):
        """A read that round 0 trims to `view`: its adapter i % 3 in front (after up to 15 nt
        when round 0 is regular), stored reverse-complemented for every second i."""
        ad = _sub(rng, a0[i % 3], i % 3 if nsub is None else nsub)
        r = (_rand(rng, i % 16) if regular else "") + ad + view
        return revcomp(r) if i % 2 else r

    if name in ("reg_suffix", "reg_backx"):
        w1 = SUFFIX if name == "reg_suffix" else BACKX
        a1 = [_rand(rng, 18) for _ in range(3)]
        c = Case(name, reg0, (a1, [w1] * 3, True, 0.1, 3))
        for i in range(300):
            keep = None if w1 == SUFFIX or i % 4 else (9, 3, 2)[(i // 4) % 3]
            v = _r_view(rng, w1, a1[(i // 3) % 3], 40 + i % 37, (i // 2) % 2, keep)
            if i % 5 == 1:
                v = revcomp(v)             # round 1 takes the view's reverse complement
            if i % 11 == 0:
                v = v + "ACGT"             # round 1's adapter is no longer at the end
            c.add("plain", front(i, v))
        return c
    if name == "noni_both":
        a1 = [_rand(rng, 20) for _ in range(3)]
        c = Case(name, (a0, [FRONTX] * 3, True, 0.1, 3), (a1, [BACKX] * 3, True, 0.1, 3))
        for i in range(300):
            k0 = (24, 24, 10, 3, 2)[i % 5]           # round 0's copy: full, cut, -O, -O - 1
            k1 = (20, 11, 3, 2)[(i // 5) % 4]
            v = _r_view(rng, BACKX, a1[i % 3], 35 + i % 41, i % 2 if k1 > 3 else 0, k1)
            if i % 7 == 3:
                v = revcomp(v)
            r = a0[(i // 2) % 3][24 - k0:] + v
            c.add(f"cut_{k0}_{k1}", revcomp(r) if i % 2 else r)
        return c
    if name == "mixed":
        x, y, z = (_rand(rng, 22) for _ in range(3))
        c = Case(name, reg0, ([x, y, y, z], [B, SUFFIX, B, BACKX], True, 0.1, 3))
        for i in range(320):
            kind = ("regular_beats", "restricted_beats", "tie", "inner_y", "only_x", "only_z",
                    "suffix_sub", "none")[i % 8]
            if kind == "regular_beats":        # x exact inside, z with two errors at the end
                v = _rand(rng, 30) + x + _rand(rng, 12) + _sub(rng, z, 2)
            elif kind == "restricted_beats":   # x with two errors inside, z exact at the end
                v = _rand(rng, 30) + _sub(rng, x, 2) + _rand(rng, 12) + z
            elif kind == "tie":                # y at the end: A$ (index 1) and -a (index 2) tie
                v = _rand(rng, 40 + i % 9) + y
            elif kind == "inner_y":            # y inside: only the regular adapter (index 2)
                v = _rand(rng, 25) + _sub(rng, y, i % 3) + _rand(rng, 20 + i % 5)
            elif kind == "only_x":
                v = _rand(rng, 20 + i % 7) + _sub(rng, x, i % 2) + _rand(rng, i % 30)
            elif kind == "only_z":
                v = _rand(rng, 40) + z[:(22, 12, 3)[(i // 8) % 3]]
            elif kind == "suffix_sub":
                v = _rand(rng, 33 + i % 13) + _sub(rng, y, 1 + i % 2)
            else:
                v = _rand(rng, 50 + i % 20)
            if (i // 8) % 4 == 3:
                v = revcomp(v)
            c.add(kind, front(i, v))
        return c
    if name == "ring":
        a1 = [_rand(rng, 40) for _ in range(4)]
        c = Case(name, pre0, (a1, list(RESTRICTED), True, 0.25, 3))
        for i in range(280):
            a = i % 4
            w = RESTRICTED[a]
            keep = None if not w & ec.NONI or i % 3 else (25, 8, 3)[(i // 12) % 3]
            nsub = (0, 3, 10, 11)[(i // 4) % 4] if keep is None else 0
            v = _r_view(rng, w, a1[a], 50 + i % 43, nsub, keep)
            if i % 5 == 2:
                v = revcomp(v)
            c.add(f"ring_{nsub}", front(i, v, regular=False, nsub=i % 3))
        return c
    if name == "oslot":
        a1 = ["ACG", _rand(rng, 6)]
        c = Case(name, pre0, (a1, [BACKX, BACKX], True, 2.0, 3))
        for i in range(320):
            c.add("random", front(i, _rand(rng, 8 + i % 40), regular=False, nsub=i % 3))
        return c
    if name in ("tiny_e1", "tiny_e01"):
        if name == "tiny_e1":   # a 1-nt ^A at -e 1 accepts an empty view with one error
            r1 = (["A", "C", _rand(rng, 4)], [PREFIX, SUFFIX, BACKX], True, 1.0, 1)
        else:
            a1 = [_rand(rng, 18) for _ in range(2)]
            r1 = (a1, [SUFFIX, BACKX], True, 0.1, 3)
        c = Case(name, pre0, r1)
        for i in range(240):
            n = (0, 1, 2, 3, 30)[i % 5]
            if name == "tiny_e01" and n == 30:
                v = _r_view(rng, r1[1][i % 2], r1[0][i % 2], 20 + i % 9, i % 2)
            else:
                v = _rand(rng, n)
            c.add(f"view{n}", front(i, v, regular=False, nsub=(i // 5) % 3))
        return c
    raise KeyError(name)


def r_coverage(names=R_NAMES) -> set:
    """What stratum R exercises, judged from the expected records of its cases."""
    cov = set()
    for name in names:
        c = r_case(name)
        exp = c.host()
        s1, w1, rc1, e1, o1 = c.r1
        regular = [w for w in w1 if w not in RESTRICTED]
        for i, (lab, read) in enumerate(zip(c.labels, c.reads)):
            r = exp[i]
            if r["bin1"] < 0:
                continue
            view = ec.trimmed(read, r, c.r0[1])
            hit = r["bin2"] >= 0
            cov.add(("view_len", min(len(view), 3), bool(hit)))
            if hit:
                w = w1[r["bin2"]]
                if w in RESTRICTED:
                    cov.add(("winner1", w, "rc2" if r["rc2"] else "fwd2"))
                    cov.add(("winner1", w, "strand1" if r["rc1"] else "strand0"))
                    if regular and lab == "restricted_beats":
                        cov.add("restricted_beats_regular")
                    if regular and lab == "tie" and w == SUFFIX:
                        cov.add("tie_lower_index")
                    if panel_kk(e1, len(s1[r["bin2"]])) > 7 and r["m2_errors"] > 7:
                        cov.add(("ring1_errors_gt7", w))
                else:
                    sub = sum(1 for x in w1[:r["bin2"]] if x not in RESTRICTED)
                    if sub != r["bin2"]:
                        cov.add("remapped_regular_winner")
                    if lab == "regular_beats":
                        cov.add("regular_beats_restricted")
            if name == "noni_both" and hit and r["m2_astop"] - r["m2_astart"] == o1:
                cov.add("cut_to_min_overlap_both")
            if name == "noni_both" and lab.endswith("_2") and not hit:
                cov.add("cut_below_min_overlap_1")
            if name == "oslot" and r["rc2"] and not hit:
                bf = ec.best_match(s1, w1, view, e1, o1)
                br = ec.best_match(s1, w1, revcomp(view), e1, o1)
                if bf is not None and bf[1][4] < 0 and br is None:
                    cov.add("nonpositive_forward_loses_to_no_match")
    return cov


def r_required() -> set:
    req = {"restricted_beats_regular", "regular_beats_restricted", "remapped_regular_winner",
           "tie_lower_index", "cut_to_min_overlap_both", "cut_below_min_overlap_1",
           "nonpositive_forward_loses_to_no_match",
           ("view_len", 0, True), ("view_len", 0, False), ("view_len", 1, True),
           ("view_len", 1, False), ("view_len", 2, True), ("view_len", 2, False)}
    for w in RESTRICTED:
        req |= {("winner1", w, x) for x in ("rc2", "fwd2", "strand0", "strand1")}
        req.add(("ring1_errors_gt7", w))
    return req


# ---- stratum W: panel width ----------------------------------------------------------------

W_NAMES = ("shared_front", "shared_back", "wide64", "mixed64")


def _w_reads(rng, c: Case, n_reads: int, back_cut: int = 12):
    """Reads in which every adapter of the panel is planted at least twice (exact and with a
    substitution; non-internal ones also cut), on both strands; the regular ones inside."""
    seqs, wheres, rc, e, o = c.r0
    i = 0
    while len(c.reads) < n_reads:
        a = i % len(seqs)
        turn = i // len(seqs)
        s, w = seqs[a], wheres[a]
        body = _rand(rng, 40 + (i * 7) % 50)
        if w in RESTRICTED:
            piece = _sub(rng, s, 1) if turn % 4 == 2 else s
            if w & ec.NONI and turn % 2:
                piece = piece[len(s) - 12:] if w & F else piece[:back_cut]
            r = _place(w, piece, body)
        else:
            r = _rand(rng, i % 13) + (_sub(rng, s, 1) if turn % 2 else s) + body
        c.add(f"plant_{a}", revcomp(r) if (i // 3) % 2 else r)
        i += 1
    for _ in range(12):
        c.add("unrelated", _rand(rng, 70))
    return c


@functools.lru_cache(maxsize=None)
def w_case(name: str) -> Case:
    rng = np.random.default_rng([SEED, 200 + W_NAMES.index(name)])
    if name in ("shared_front", "shared_back"):
        # every adapter of the shared-prefix panel under both types of one side: 2a anchored,
        # 2a + 1 non-internal; the anchored one wins the ties, the other one the cut copies
        pair = (PREFIX, FRONTX) if name == "shared_front" else (SUFFIX, BACKX)
        seqs = [s for s in shared_panel() for _ in pair]
        wheres = [w for _ in shared_panel() for w in pair]
        return _w_reads(rng, Case(name, (seqs, wheres, True, 0.1, 3)), 480, back_cut=29)
    if name == "wide64":
        # 16 of each type, T = 128: one read per block-step; index 63 repeats index 0
        seqs = [_rand(rng, int(rng.integers(20, 35))) for _ in range(64)]
        wheres = [(PREFIX, SUFFIX, BACKX, FRONTX)[a % 4] for a in range(64)]
        seqs[63] = seqs[0]       # ^A at index 0, XA at index 63
        c = Case(name, (seqs, wheres, True, 0.1, 3))
        for j in range(8):    # full copies: ^A at index 0 and XA at index 63 tie
            r = seqs[0] + _rand(rng, 50 + j)
            c.add("tie_0_63", revcomp(r) if j % 2 else r)
        return _w_reads(rng, c, 500)
    if name == "mixed64":
        seqs = [_rand(rng, int(rng.integers(20, 35))) for _ in range(64)]
        wheres = [RESTRICTED[(a // 2) % 4] if a % 2 == 0 else F for a in range(64)]
        return _w_reads(rng, Case(name, (seqs, wheres, True, 0.1, 3)), 500)
    raise KeyError(name)


# ---- stratum L: long reads -----------------------------------------------------------------

L_E = (0.1, 0.25)
L_LENS = (255, 256, 257, 4095, 4096, 65535, 65536, 65537, 200003)
L_M = (24, 30, 36, 40)    # ^A, XA, A$, AX; the 40-nt adapter makes -e 0.25 a ring round


@functools.lru_cache(maxsize=None)
def l_case(e: float) -> Case:
    """The same reads for both error settings.  Every length with each type's adapter (0-2
    substitutions) at its end, stored forward and reverse-complemented, for XA and AX also cut
    to 12 nt, and once without an adapter; for the 3' types reads of m + k, m + k + 1 and m + k + 16 nt (k of either setting),
    whose window starts at column 0, 1 and 16.  The first read sits where lib.pack would put it,
    the others at offsets = 0, 1, 15 and 16 mod 16 above a 16-nt gap."""
    rng = np.random.default_rng([SEED, 300])
    seqs = [_rand(rng, m) for m in L_M]
    c = Case(f"long_e{e}", (seqs, list(RESTRICTED), True, e, 3), offsets=[])
    for n in L_LENS:
        body = _rand(rng, n, "ACGT" * 8 + "N")
        for a, w in enumerate(RESTRICTED):
            for strand in (0, 1):
                piece = _sub(rng, seqs[a], int(rng.integers(0, 3)))
                r = _place(w, piece, body[:n - len(piece)])
                c.add(f"len_{n}", revcomp(r) if strand else r)
            if w & ec.NONI:    # a cut copy: the 12 characters next to the read's end
                for strand in (0, 1):
                    piece = seqs[a][len(seqs[a]) - 12:] if w & F else seqs[a][:12]
                    r = _place(w, piece, body[:n - 12])
                    c.add(f"cut_{n}", revcomp(r) if strand else r)
        c.add(f"bare_{n}", body)
    for a, w in ((2, SUFFIX), (3, BACKX)):
        m = len(seqs[a])
        for k in sorted({panel_kk(x, m) for x in L_E}):
            for extra in (0, 1, 16):
                for strand in (0, 1):
                    r = _rand(rng, k + extra) + seqs[a]
                    c.add(f"j0_{k}_{extra}", revcomp(r) if strand else r)
    pos = lib.PACK_PAD
    for i, r in enumerate(c.reads):
        if i:
            pos = (pos + 15) // 16 * 16 + 16 + (0, 1, 15, 16)[i % 4]
        c.offsets.append(pos)
        pos += len(r)
    return c


# ---- the bounds-checked build --------------------------------------------------------------

def run_case(ctx, c: Case) -> tuple:
    """(records that differ from the host twin's, records, pipeline flags) of one case on ctx:
    a single round through dmx_run, two rounds through dmx_load / dmx_exec, twice."""
    s, w, rc, e, o = c.r0
    ctx.set_panel_ex(0, s, w, rc, e, o)
    if c.r1 is None:
        ctx.set_mode(lib.MODE_SINGLE)
        got = ctx.run(c.packed())
        return len(ec.same_records(got, c.host())), len(got), ctx.stats()["flags"]
    s, w, rc, e, o = c.r1
    ctx.set_panel_ex(1, s, w, rc, e, o)
    ctx.set_mode(lib.MODE_TWO_ROUND)
    bad = flags = 0
    try:
        ctx.load(c.packed())
        for _ in range(2):      # the second dmx_exec runs on the resident batch
            ctx.exec()
            bad += len(ec.same_records(ctx.fetch(), c.host()))
            flags |= ctx.stats()["flags"]
    finally:
        ctx.set_mode(lib.MODE_SINGLE)
    return bad, len(c.reads), flags


def run_q(ctx, where: int, e: float, reps: int):
    """(records, tiled host records) of stratum Q's batch of `reps` copies of the base."""
    reads = list(q_base(where, e)) * reps
    blob, offs, lens = ec.oracle.pack_ascii(reads)
    ctx.set_panel_ex(0, list(shared_panel()), [where] * 24, True, e, 3)
    ctx.set_mode(lib.MODE_SINGLE)
    return ctx.run(lib.pack(blob, offs, lens)), np.tile(q_host(where, e), reps)


def main():
    """Strata R, W and L, and Q at two loop steps per block, on the library DMX_DEBUG_BOUNDS
    selects (test_ends_struct.py runs this in a child process with the bounds-checked build):
    one JSON line."""
    out = {"lib": os.path.basename(lib.LIB_PATH), "bad": 0, "n": 0, "flags": 0, "err": ""}
    with lib.Context(0) as ctx:
        try:
            cases = [r_case(x) for x in R_NAMES] + [w_case(x) for x in W_NAMES] + \
                [l_case(e) for e in L_E]
            for c in cases:
                bad, n, flags = run_case(ctx, c)
                out["bad"] += bad
                out["n"] += n
                out["flags"] |= flags
            for where, e in Q_SPECS:
                got, exp = run_q(ctx, where, e, q_reps(2))
                out["bad"] += len(ec.same_records(got, exp))
                out["n"] += len(got)
                out["flags"] |= ctx.stats()["flags"]
        except lib.DmxError as err:
            out["bad"], out["err"] = -1, str(err)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
