"""Shared inputs and the oracle of the gene-group tests (test_genegroups_host.py on the CPU,
test_genegroups.py and test_genegroups_scale.py on the GPU).

The oracle is a literal restatement of amplicon_sorter.py update_list (:983-1034) and merge_groups
(:1058-1087), fed the lines of a plain restatement of similarity (:777-808) on the numpy DP of
pairdist_cases with built-in round.  It is computed once per process and shared.  The pair
lists of many blocks and tiles (scale_case) have an oracle of their own, in numpy alone."""
import functools
import zlib

import numpy as np

import pairdist_cases as pc
from dmx import lib

NONE = lib.LG_NONE


# ---- the reference, restated ---------------------------------------------------------------------

def restated_lines(reads, sg=80.0, minlength=0):
    """amplicon_sorter.py:550-571, 669-683, 777-808 in plain Python on the numpy DP (one group:
    fewer than 1000 reads): a stable sort by length, the 5 % rule, per pair the forward identity
    and, below 0.5, the identity against the longer read's reverse complement.  Returns (lines,
    hits): hits[k] = (i, j, d, reverse) of line k.  The DP runs per length class, so that short
    pairs are not padded to the longest read."""
    comp = [r.upper().encode() if isinstance(r, str) else bytes(r).upper() for r in reads]
    comp = [r for r in comp if len(r) >= minlength]
    d = sorted(range(len(comp)), key=lambda i: len(comp[i]))
    todo = []
    for p in range(len(d) - 1):
        for p2 in range(p + 1, len(d)):
            if len(comp[d[p]]) * 1.05 < len(comp[d[p2]]):
                continue
            todo.append((d[p], d[p2]))

    def dist(pairs, rc):
        out = np.zeros(len(pairs), dtype=np.int64)
        cls = np.array([len(comp[b]) > 400 for _, b in pairs], dtype=bool)
        for c in (False, True):
            sel = np.flatnonzero(cls == c)
            out[sel] = pc.np_dist([comp[pairs[k][0]] for k in sel],
                                  [pc.revcomp(comp[pairs[k][1]]) if rc else comp[pairs[k][1]]
                                   for k in sel], lib.PD_NW)
        return out

    fwd = dist(todo, False)
    out = []
    for (a, b), df in zip(todo, fwd):
        iden = round(1 - int(df) / len(comp[b]), 3)
        if iden >= sg / 100:
            out.append((a, b, int(df), False))
        elif iden < 0.5:
            out.append((a, b, None, True))   # the reverse complement is tried: filled in below
    again = [(a, b) for a, b, dd, _ in out if dd is None]
    rev = dict(zip(again, dist(again, True)))
    hits = []
    for a, b, dd, r in out:
        if dd is None:
            dd = int(rev[(a, b)])
            if not round(1 - dd / len(comp[b]), 3) >= sg / 100:
                continue
        hits.append((a, b, dd, r))
    lines = [str(a) + ":" + str(b) + ":" + str(round(1 - dd / len(comp[b]), 3)) +
             (":reverse" if r else "") for a, b, dd, r in hits]
    return lines, hits


def merge_groups(grouplist):
    """amplicon_sorter.py:1058-1087 without its prints."""
    a1 = len(grouplist)
    a2 = 0
    if a1 > 1:
        grouplist = [i for i in grouplist if len(i) > 1]
        grouplist = [set(i) for i in grouplist]
        while a1 > a2:
            a1 = len(grouplist)
            position = 0
            for position in range(position, len(grouplist) - 1):
                for position2 in range(position + 1, len(grouplist)):
                    A1 = grouplist[position]
                    A2 = grouplist[position2]
                    if len(A1.intersection(A2)) > 0:
                        grouplist[position] = grouplist[position].union(A2)
                        grouplist[position2].clear()
            grouplist = [i for i in grouplist if len(i) > 0]
            a2 = len(grouplist)
    return grouplist


def update_list(lines):
    """amplicon_sorter.py:983-1034 on a list of lines instead of the temporary file: the dict of
    lists, the string comparison of the identities, the sort with reverse=True, the greedy loop,
    then merge_groups.  Returns (templist, grouplist): the kept lines as [i, j, iden] of str, and
    the groups as sets of str, in the reference's order."""
    templist = []
    tempdict = {}
    for line in lines:
        e = line.strip().split(':')[:3]
        a = e[1]
        if a in tempdict:
            tempdict[a].append(e)
            tempdict[a].sort(key=lambda x: (int(x[1]), float(x[2])))
            for i, j in enumerate(tempdict[a][:-1]):
                if j[1] == tempdict[a][i + 1][1]:
                    if j[2] < tempdict[a][i + 1][2]:
                        j[0] = ''
            tempdict[a] = [i for i in tempdict[a] if i[0] != '']
        else:
            tempdict[a] = [e]
    templist.extend(tempdict.values())
    templist = [x for sublist in templist for x in sublist]
    templist.sort(key=lambda x: (float(x[2]), int(x[1])), reverse=True)
    grouplist = []
    for x in templist:
        for s in grouplist:
            if len({x[0], x[1]}.intersection(s)) > 0:
                s.update({x[0], x[1]})
                break
        else:
            grouplist.append({x[0], x[1]})
    return templist, merge_groups(grouplist)


def as_index_groups(grouplist):
    """The reference's groups (sets of str) as ascending int lists, in its order."""
    return [sorted(int(x) for x in g) for g in grouplist]


def best_lines(lines):
    """Per longer read the lines of the largest identity, ties kept: what DESIGN.md §8i takes
    update_list's filter to keep, as a set of (i, j)."""
    top = {}
    for x in lines:
        i, j, iden = x.split(":")[:3]
        top[j] = max(top.get(j, -1.0), float(iden))
    return {(int(x.split(":")[0]), int(x.split(":")[1])) for x in lines
            if float(x.split(":")[2]) == top[x.split(":")[1]]}


def components(edges, n):
    """Labels as dmx_edgegroups defines them, by repeated relabelling (no union-find: a
    different algorithm from both the kernels' and the host twin's)."""
    lab = np.arange(n, dtype=np.int64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    while len(e):
        lo = np.minimum(lab[e[:, 0]], lab[e[:, 1]])
        new = lab.copy()
        np.minimum.at(new, e[:, 0], lo)
        np.minimum.at(new, e[:, 1], lo)
        if (new == lab).all():
            break
        lab = new
    on = np.zeros(n, dtype=bool)
    on[e.reshape(-1)] = True
    out = np.where(on, lab, NONE).astype(np.uint32)
    return out


def groups_of(labels):
    """The partition a label array stands for: a sorted list of ascending member lists."""
    labels = np.asarray(labels)
    out = {}
    for v in np.flatnonzero(labels != NONE):
        out.setdefault(int(labels[v]), []).append(int(v))
    return sorted(out.values())


# ---- small graphs --------------------------------------------------------------------------------

def small_graphs():
    """name -> (a, b, n_nodes): the shapes of the issue's list."""
    rng = np.random.default_rng(5)
    g = {}
    g["empty"] = ([], [], 6)
    g["no_nodes"] = ([], [], 0)
    g["one_edge"] = ([4], [2], 6)
    g["self_loop_only"] = ([3], [3], 5)
    g["star"] = ([40] * 39, [k for k in range(41) if k not in (40, 17)], 41)   # 17: isolated
    perm = rng.permutation(300)
    g["path_300_shuffled"] = (perm[:-1].tolist(), perm[1:].tolist(), 300)
    c1, c2 = list(range(0, 12)), list(range(20, 33))
    clique = [(x, y) for c in (c1, c2) for x in c for y in c if x < y]
    g["two_cliques_apart"] = ([x for x, _ in clique], [y for _, y in clique], 40)
    g["two_cliques_joined"] = ([x for x, _ in clique] + [31], [y for _, y in clique] + [5], 40)
    g["repeated_edges"] = ([1, 2, 1, 2, 7, 7, 8], [2, 1, 2, 1, 8, 8, 7], 10)
    return g


def big_graphs():
    """The GPU-only sizes: a random graph of 50,000 nodes and 60,000 edges, and one path over
    100,000 nodes in shuffled index order (the most hooking rounds and the longest chains)."""
    rng = np.random.default_rng(6)
    g = {}
    g["random_50k_60k"] = (rng.integers(0, 50000, 60000), rng.integers(0, 50000, 60000), 50000)
    perm = rng.permutation(100000)
    g["path_100k_shuffled"] = (perm[:-1], perm[1:], 100000)
    return g


# ---- the synthetic bin ---------------------------------------------------------------------------

def substitute(rng, s: bytes, k: int) -> bytes:
    """s with exactly k substitutions at places at least 8 apart (so the edit distance is k)."""
    out = bytearray(s)
    step = len(s) // k
    assert step >= 8
    for x in range(k):
        pos = x * step + int(rng.integers(0, step - 7))
        out[pos] = ord("ACGT"[("ACGT".index(chr(out[pos])) + 1 + int(rng.integers(3))) % 4])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def gene_bin():
    """The bin of the gene-group tests (minlength = 0, similar_genes = 80), as str reads:
      A, B  two families of about 15 reads of at most 166 nt.  B's founder is A's with 22 % of
            its places substituted, so reads of A and B do not hit each other (identity near
            0.72, above 0.5: no reverse try either)
      J     the bridge: A's founder with 40 % of those substitutions (13 % from A, 9 % from B)
            and two more nt, the longest read of its length class and so only ever a target.
            Reads of B are its best hits, reads of A hit it too, but never as a best hit: only
            the best-hit filter keeps A and B apart
      T     in A: a read and two shorter copies at the same distance 3 from it (an exact tie)
      C     a family of 15 reads of about 130 nt, unrelated (the 5 % rule keeps it from A, B)
            every fourth read of a family is reverse-complemented
      L     a family of 8 reads of about 1,500 nt; its longest read has two shorter copies at
            distances 31 and 32, which both round to the identity 0.979
      U     two unrelated reads of about 160 nt: no hit at all
    shuffled, so that families and indices do not line up."""
    rng = np.random.default_rng(33)

    def acgt(n):
        return pc.rand_seq(rng, n, p_n=0.0)

    def family(founder, n, lo, hi, most):
        out = []
        for k in range(n):
            r = pc.mutate(rng, founder, float(rng.uniform(lo, hi)))[:most]
            out.append(pc.revcomp(r) if k % 4 == 3 else r)
        return out

    fa = acgt(165)
    where = rng.permutation(165)[:36]                      # 22 % of the places
    fb, fj = bytearray(fa), bytearray(fa)
    for n, pos in enumerate(where):
        new = ord("ACGT"[("ACGT".index(chr(fa[pos])) + 1 + int(rng.integers(3))) % 4])
        fb[pos] = new
        if n < 22:                                         # 13 % from A, 9 % from B
            fj[pos] = new
    fb, fj = bytes(fb), bytes(fj) + b"GT"
    reads = family(fa, 12, 0.02, 0.04, 166) + family(fb, 15, 0.02, 0.04, 166) + [fj]
    tj = pc.mutate(rng, fa, 0.03)[:166]
    reads += [tj, substitute(rng, tj, 2)[:-1], substitute(rng, tj, 2)[:-1]]
    reads += family(acgt(130), 15, 0.02, 0.06, 140)
    lj = acgt(1500)
    reads += [lj, substitute(rng, lj, 30)[:-1], substitute(rng, lj, 30)[:-2]]
    reads += family(lj, 5, 0.03, 0.05, len(lj) - 3)
    reads += [acgt(159), acgt(163)]
    order = rng.permutation(len(reads))
    fam = np.array([0] * 12 + [1] * 15 + [1] + [0] * 3 + [2] * 15 + [3] * 8 + [4, 5])
    return [reads[i].decode() for i in order], fam[order]


@functools.lru_cache(maxsize=None)
def gene_bin_oracle():
    """(lines, hits, templist, groups) of gene_bin()'s reads: the restated similarity lines and their
    (i, j, d, reverse), update_list's kept lines, and its groups as ascending int lists in the
    reference's order."""
    lines, hits = restated_lines(gene_bin()[0])
    templist, grouplist = update_list(lines)
    return lines, hits, templist, as_index_groups(grouplist)


@functools.lru_cache(maxsize=None)
def quiet_bin():
    """Six unrelated reads of one length class: pairs are compared, nothing hits."""
    rng = np.random.default_rng(34)
    return [pc.rand_seq(rng, 150 + k, p_n=0.0).decode() for k in range(6)]


def bin_plan(reads, sg=80.0):
    """What sorter.gene_groups hands to pairhits for `reads` (minlength 0): (packed, lengths, q,
    t, cap_hit, cap_half), from the sorter's own planning."""
    from dmx import sorter
    return sorter._similarity_plan(reads, sg, 0, None, 10000, False)


# ---- pair lists at scale -------------------------------------------------------------------------
# dmx_pairhits' pair list is arbitrary and its caps are per pair, so a list of any length can be
# drawn from the few thousand distinct pairs of a small batch, and the caps of every place chosen
# so that the documented rule (sorter.similarity; the comment above ph_decide_kernel) gives the
# class wanted there.  The numpy DP runs once, over the distinct pairs; everything expected of a
# list is then numpy arithmetic on those distances.

SCALE_SIZES = (255, 256, 257, 16384, 16385, 65536, 65537, 131329)
SCALE_LAYOUTS = ("all_forward", "none", "every_257th", "block_stripes", "tile_heads", "last_only",
                 "mixed", "one_target")
SCALE_TOP = SCALE_SIZES[-1]        # 514 blocks of 256: three tiles of the scan, a ragged last block
SCALE_HOST_N = 65537               # the CPU tests' size: 257 blocks, the second tile holds one
F, R, M, X = 0, 1, 2, 3            # forward hit, reverse hit, miss without a retry, retried miss


def scale_cases():
    """(layout, N) of the GPU tests: every layout at the largest size; at the sizes on either side
    of 64 and 256 blocks (and of one block), `mixed` and `all_forward`."""
    return [(name, SCALE_TOP) for name in SCALE_LAYOUTS] + \
        [(name, n) for n in SCALE_SIZES[:-1] for name in ("all_forward", "mixed")]


@functools.lru_cache(maxsize=None)
def scale_reads():
    """64 reads of 24-60 nt (one 64-row word each): 8 founders, of each two mutated copies (5-10 %)
    and two reverse-complemented mutated copies, 18 unrelated reads and 6 reads with N; shuffled.
    Returns (reads, packed, d_fwd, d_rev): d_fwd[a, b] = NW(a, b), d_rev[a, b] = NW(a, revcomp(b))
    by the numpy DP, int64; the diagonal is not used."""
    rng = np.random.default_rng(41)
    reads = []
    for _ in range(8):
        f = pc.rand_seq(rng, int(rng.integers(30, 56)), p_n=0.0)
        reads.append(f)
        for k in range(4):
            c = pc.mutate(rng, f, float(rng.uniform(0.05, 0.10)))[:60]
            reads.append(pc.revcomp(c) if k >= 2 else c)
    reads += [pc.rand_seq(rng, int(rng.integers(24, 61)), p_n=0.0) for _ in range(18)]
    reads += [pc.rand_seq(rng, int(rng.integers(24, 61)), p_n=0.1) for _ in range(6)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    n = len(reads)
    assert n == 64 and all(24 <= len(r) <= 60 for r in reads)
    assert sum(b"N" in r for r in reads) >= 6
    a, b = [x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    qs = [reads[i] for i in a]
    d_fwd = pc.np_dist(qs, [reads[j] for j in b], lib.PD_NW).reshape(n, n)
    d_rev = pc.np_dist(qs, [pc.revcomp(reads[j]) for j in b], lib.PD_NW).reshape(n, n)
    return reads, pc.pack_reads(reads), d_fwd, d_rev


def _between(rng, lo, hi):
    """Per place an integer of lo .. hi (arrays, lo <= hi): a third each the lower end, the upper
    end and a uniform draw, so that both sides of every comparison of the rule occur often."""
    k = rng.integers(0, 3, len(lo))
    return np.where(k == 0, lo, np.where(k == 1, hi, rng.integers(lo, hi + 1)))


def _class_pattern(layout, n, rng):
    i = np.arange(n)
    if layout == "all_forward":
        return np.full(n, F)
    if layout == "none":
        return np.full(n, M)
    if layout == "every_257th":      # the one hit walks through every lane over consecutive blocks
        return np.where(i % 257 == 0, F, M)
    if layout == "block_stripes":
        return np.where((i // 256) % 2 == 0, F, M)
    if layout == "tile_heads":       # 65,536 pairs = 256 blocks = one tile of the scan
        return np.where((i % 65536 == 0) | (i == n - 1), F, M)
    if layout == "last_only":
        return np.where(i == n - 1, R, M)
    if layout in ("mixed", "one_target"):
        return rng.permutation(i % 4)
    raise KeyError(layout)


class ScaleCase:
    """A pair list and everything expected of it, from numpy alone."""

    def __init__(self, layout, n):
        reads, self.packed, d_fwd, d_rev = scale_reads()
        rng = np.random.default_rng([zlib.crc32(layout.encode()), n])
        self.layout, self.n, self.n_reads = layout, n, len(reads)
        self.cls = cls = _class_pattern(layout, n, rng)
        # the distinct ordered pairs, and which of them can produce which class
        a, b = np.nonzero(~np.eye(self.n_reads, dtype=bool))
        if layout == "one_target":   # three targets with a query for every class
            ok = [r for r in range(self.n_reads) if (d_rev[:, r] < d_fwd[:, r]).sum() >= 2]
            keep = np.isin(b, ok[:3])
            a, b = a[keep], b[keep]
        df, dr = d_fwd[a, b], d_rev[a, b]
        # hits land on reads with a relative only (a read within a quarter of their length, either
        # strand): an unrelated hit there loses against the relative's in the tie filter, so the
        # kept edges fall into several groups and the reads without a relative keep no label
        ln = np.array([len(r) for r in reads])
        near = np.where(np.eye(self.n_reads, dtype=bool), 99, np.minimum(d_fwd, d_rev)).min(axis=0)
        fam = (near <= ln // 4)[b] | (layout == "one_target")
        can = {F: fam, R: fam & (dr < df), M: df >= 1, X: np.minimum(df, dr) >= 1}
        pick = np.zeros(n, dtype=np.int64)
        for c, mask in can.items():
            where = np.flatnonzero(cls == c)
            pick[where] = rng.choice(np.flatnonzero(mask), len(where))
        self.q, self.t = a[pick].astype(np.uint32), b[pick].astype(np.uint32)
        self.d_fwd, self.d_rev = df, dr = df[pick], dr[pick]
        one, any_half = np.ones(n, dtype=np.int64), rng.integers(-1, 70, n)
        # F: d_fwd <= cap_hit, whatever cap_half is
        hit_f = df + rng.choice([0, 0, 1, 5], n)
        # R and X: d_fwd > cap_hit >= 0 and d_fwd > cap_half; R: d_rev <= cap_hit, X: d_rev > cap_hit
        lo_half = _between(rng, -one, np.maximum(df - 1, -1))
        hit_r = _between(rng, dr, np.maximum(df - 1, dr))
        hit_x = _between(rng, 0 * one, np.maximum(np.minimum(df, dr) - 1, 0))
        # M: no hit cap at all (every other M), or cap_hit < d_fwd <= cap_half
        bare = (np.cumsum(cls == M) % 2 == 1)
        hit_m = np.where(bare, -1, _between(rng, 0 * one, np.maximum(df - 1, 0)))
        half_m = np.where(bare, any_half, _between(rng, df, df + 4))
        self.cap_hit = np.select([cls == F, cls == R, cls == X], [hit_f, hit_r, hit_x],
                                 hit_m).astype(np.int32)
        self.cap_half = np.select([cls == F, cls == M], [any_half, half_m], lo_half).astype(np.int32)
        # what the rule gives, restated on the exact distances
        ch, chalf = self.cap_hit.astype(np.int64), self.cap_half.astype(np.int64)
        fwd = df <= ch
        tried = ~fwd & (ch >= 0) & (df > chalf)
        back = tried & (dr <= ch)
        got = np.select([fwd, back, tried], [F, R, X], M)
        assert (got == cls).all(), "the generator missed a class it asked for"
        self.hit = fwd | back
        self.outcome = np.where(fwd, df, np.where(back, dr | lib.LG_REV, NONE)).astype(np.uint32)
        self.pair = np.flatnonzero(self.hit).astype(np.uint32)
        self.d = np.where(fwd, df, dr)[self.pair].astype(np.uint32)
        self.rev = back[self.pair].astype(np.uint8)
        self.n_hits = len(self.pair)
        self.best = np.full(self.n_reads, NONE, dtype=np.uint32)
        np.minimum.at(self.best, self.t[self.pair], self.d)

    def args(self):
        return self.q, self.t, self.cap_hit, self.cap_half

    def ties(self):
        """name -> tie table: the best distance per read, and one more where there is a best."""
        return {"best": self.best,
                "best+1": np.where(self.best != NONE, self.best + np.uint32(1), self.best)}

    def edges(self, tie):
        """The hits dmx_hitgroups keeps for `tie`, as a mask over the hits."""
        return self.d <= np.asarray(tie, dtype=np.uint32)[self.t[self.pair]]

    def labels(self, tie):
        """dmx_hitgroups' labels for `tie` by label propagation over the distinct kept edges."""
        keep = self.pair[self.edges(tie)]
        e = np.unique(np.stack([self.q[keep], self.t[keep]], axis=1), axis=0)
        return components(e, self.n_reads)

    @functools.cached_property
    def host(self):
        """The host twin's state for this list (pinned to the oracle by test_genegroups_host.py)."""
        return lib.pairhits_host(self.packed, *self.args(), n_threads=16)


@functools.lru_cache(maxsize=None)
def scale_case(layout, n):
    return ScaleCase(layout, n)


def first_differences(got, exp, what, most=5):
    """A message naming the first places where two arrays differ (or their lengths), or None."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape:
        return f"{what}: {len(got)} entries, {len(exp)} expected"
    bad = np.flatnonzero(got != exp)
    if not len(bad):
        return None
    return f"{what}: {len(bad)} of {len(exp)} differ, first at " + ", ".join(
        f"[{k}] {got[k]} != {exp[k]}" for k in bad[:most])


def assert_same(got, exp, what):
    msg = first_differences(got, exp, what)
    assert msg is None, msg
