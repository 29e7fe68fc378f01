"""Shared inputs and the numpy oracle of the pairwise-distance tests (test_pairdist_host.py on
the CPU, test_pairdist.py on the GPU).  Edit distance has one right answer, so a full-matrix DP
is a complete oracle; it is computed once per process and shared."""
import functools

import numpy as np

from dmx import lib

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def np_dist(queries, targets, mode):
    """Edit distances of queries[b] against targets[b] (bytes; symbols compare as bytes, so N
    equals N only) by a full-matrix DP, row by row over all pairs at once; the in-row insertion
    chain D(i, j) = min_k (c[k] + j - k) is resolved by minimum.accumulate.  mode: lib.PD_NW
    (whole sequences) or lib.PD_HW (query against any substring of the target)."""
    B = len(queries)
    if B == 0:
        return np.zeros(0, dtype=np.int64)
    ml = np.array([len(x) for x in queries])
    nl = np.array([len(x) for x in targets])
    M, N = int(ml.max()), int(nl.max())
    Q = np.zeros((B, M), dtype=np.uint8)
    T = np.full((B, N), 255, dtype=np.uint8)
    for b in range(B):
        Q[b, :ml[b]] = np.frombuffer(queries[b], dtype=np.uint8)
        T[b, :nl[b]] = np.frombuffer(targets[b], dtype=np.uint8)
    ar = np.arange(N + 1, dtype=np.int32)
    prev = np.tile(ar, (B, 1)) if mode == lib.PD_NW else np.zeros((B, N + 1), dtype=np.int32)
    res = np.zeros(B, dtype=np.int64)
    inside = ar[None, :] <= nl[:, None]
    c = np.empty((B, N + 1), dtype=np.int32)
    for i in range(1, M + 1):
        neq = Q[:, i - 1:i] != T
        c[:, 0] = i
        np.minimum(prev[:, 1:] + 1, prev[:, :-1] + neq, out=c[:, 1:])
        cur = np.minimum.accumulate(c - ar, axis=1) + ar
        sel = np.flatnonzero(ml == i)
        if len(sel):
            if mode == lib.PD_NW:
                res[sel] = cur[sel, nl[sel]]
            else:
                res[sel] = np.where(inside[sel], cur[sel], np.iinfo(np.int32).max).min(axis=1)
        prev = cur
    return res


def rand_seq(rng, n, p_n=0.04) -> bytes:
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n)
    s[rng.random(n) < p_n] = ord("N")
    return s.tobytes()


def mutate(rng, s: bytes, rate: float) -> bytes:
    out = bytearray()
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(b"ACGTN"[rng.integers(5)])
        elif r < rate:
            ch = b"ACGTN"[rng.integers(5)]
        out.append(ch)
    return bytes(out) or b"A"


def pack_reads(reads) -> lib.Packed:
    blob = np.frombuffer(b"".join(reads), dtype=np.uint8)
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    return lib.pack(blob, offs, lens)


@functools.lru_cache(maxsize=None)
def random_set(n_pairs=600, max_len=400, seed=11):
    """About 600 random pairs, lengths 1..400 over ACGTN: half unrelated, half mutated copies
    (2-30 % substitutions, insertions, deletions); a random RC flag per pair.  Read 2i is pair
    i's query, read 2i + 1 its target.  Returns (reads, q, t, flags, {mode: numpy distances})."""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n_pairs):
        a = rand_seq(rng, int(rng.integers(1, max_len + 1)))
        if i % 2:
            b = mutate(rng, a, float(rng.uniform(0.02, 0.30)))[:max_len]
            if rng.random() < 0.5:
                b = revcomp(b)   # so that RC-flagged pairs see related sequences too
        else:
            b = rand_seq(rng, int(rng.integers(1, max_len + 1)))
        if rng.random() < 0.5:
            a, b = b, a
        reads += [a, b]
    q = np.arange(0, 2 * n_pairs, 2, dtype=np.uint32)
    t = q + 1
    flags = (rng.random(n_pairs) < 0.5).astype(np.uint8)
    qs = [reads[i] for i in q]
    ts = [revcomp(reads[j]) if f else reads[j] for j, f in zip(t, flags)]
    exp = {m: np_dist(qs, ts, m) for m in (lib.PD_NW, lib.PD_HW)}
    return reads, q, t, flags, exp


def cap_cycle(d):
    """Caps 0, d - 1, d, d + 1 in turn over the pairs, and what min(d, cap + 1) then is."""
    d = np.asarray(d, dtype=np.int64)
    k = np.arange(len(d)) % 4
    caps = np.where(k == 0, 0, np.where(k == 1, np.maximum(d - 1, 0), np.where(k == 2, d, d + 1)))
    return caps.astype(np.uint32), np.minimum(d, caps + 1).astype(np.uint32)
