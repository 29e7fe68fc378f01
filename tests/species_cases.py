"""Shared inputs and the oracle of the species-group tests (test_speciesgroups_host.py on the
CPU, test_speciesgroups.py on the GPU).

The oracle is a literal restatement of amplicon_sorter.py SSG (:810-836, float sums in file
order) and of the first half of read_indexes (:1363-1411), per gene group, on the lines of
genegroups_cases.restated_lines with genegroups_cases.merge_groups.  The pair lists of many blocks
(genegroups_cases.scale_case) get their expectations from numpy alone."""
import functools

import numpy as np

import genegroups_cases as gc
import pairdist_cases as pc
from dmx import lib, sorter

NONE = lib.LG_NONE
SSG = 95            # the species threshold of the bin's tests, in percent
EDGE = 1e-6         # how far the float SSG has to stay from each of its comparisons' edges


# ---- the reference, restated ---------------------------------------------------------------------

def ssg_float(simils):
    """amplicon_sorter.py:810-836 on the identities of the lines in file order (floats, as
    float(line.split(':')[2]) gives them): the dict of counts, the float sum, b, the walk.
    Returns (ssg or None, margin): margin = the least distance of a float comparison from its
    edge: totalsimil * 0.06 from the integers on either side, and the running sum from b at the
    crossing and at the step before it."""
    t = 0
    totalsimil = 0
    tempdict = {}
    for simil in simils:
        if simil in tempdict:
            tempdict[simil] += 1
        else:
            tempdict[simil] = 1
        t += 1
        totalsimil += simil
    templist = list(tempdict.keys())
    templist.sort(reverse=True)
    b = int(totalsimil * 0.06)
    margin = min(totalsimil * 0.06 - b, b + 1 - totalsimil * 0.06)
    N6 = 0
    for n, x in enumerate(templist):
        before = N6
        N6 += tempdict[x] * x
        if N6 >= b:
            margin = min(margin, N6 - b) if b else margin   # b = 0: 0 >= 0 holds exactly
            if n:
                margin = min(margin, b - before)
            return int(x * 100), margin
    return None, margin


def line_simils(lines):
    return [float(x.strip().split(':')[2]) for x in lines]


def read_indexes(lines, indexes, ssg):
    """amplicon_sorter.py:1363-1411 for one gene group, on a list of lines instead of the compare
    file: `indexes` is the set of the group's reads as str, ssg the threshold in percent.
    Returns (templist, merged, grouplist): the lines kept by the filter, the groups merge_groups
    leaves, and those of more than 3 reads."""
    similar_species_groups = ssg / 100
    templist = []
    tempdict = {}
    for line in lines:
        e = line.strip().split(':')
        a = e[1]
        if float(e[2]) >= similar_species_groups:
            if len({e[0], e[1]}.intersection(indexes)) > 0:
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
    grouplist = []
    templist.sort(key=lambda x: float(x[2]), reverse=True)
    for x in templist:
        for s in grouplist:
            if len({x[1], x[0]}.intersection(s)) > 0:
                s.update([x[0], x[1]])
                break
        else:
            grouplist.append({x[0], x[1]})
    merged = gc.merge_groups(grouplist)
    return templist, merged, [list(set(i)) for i in merged if len(i) > 3]


def as_sets(grouplist):
    return {frozenset(int(x) for x in g) for g in grouplist}


def best_lines(lines, indexes, ssg):
    """What §8k keeps of a gene group's lines: those at the threshold with a read in the group,
    and of these per longer read the ones of the largest identity, ties kept; as (i, j)."""
    ok = [x.split(":")[:3] for x in lines]
    ok = [e for e in ok if float(e[2]) >= ssg / 100 and (e[0] in indexes or e[1] in indexes)]
    top = {}
    for i, j, iden in ok:
        top[j] = max(top.get(j, -1.0), float(iden))
    return {(int(i), int(j)) for i, j, iden in ok if float(iden) == top[j]}


# ---- the synthetic bin ---------------------------------------------------------------------------

def _change(s: bytes, places, step=1) -> bytes:
    out = bytearray(s)
    for pos in places:
        out[pos] = ord("ACGT"[("ACGT".index(chr(out[pos])) + step) % 4])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def species_bin():
    """The bin of the species-group tests (minlength = 0, similar_genes = 80, ssg = 95): reads of
    about 340 nt, every fourth read of a species reverse-complemented.
      A     gene group 0: species A1 (7 reads), A2 (6) and A3 (3: dropped), whose founders differ
            in 30 places (8.8 %); a read is its founder with 2-3 substitutions
      B     gene group 1: species B1 (6 reads; its founder is A1's with 24 places changed, so A1
            and B1 are similar genes that stay below the species threshold) and B2 (6 reads, up to
            2 nt shorter, 30 places from B1)
      X     one read in no group, half way between A1's and B1's founders and one nt longer: the
            longer read of lines from both groups, foreign to two groups at once
      S     a gene group of 4 reads, too small to be kept (label NONE): 8 places from A2's founder
            and two nt longer, so that reads of A2 hit them above the threshold
      L     gene group 2: a read of 1,500 nt with shorter copies at distances 31, 32 and 32, which
            all round to the identity 0.979 (the rounding tie), and two reads about 4 % away
    shuffled.  Returns (reads as str, role per read, gene groups as index arrays)."""
    rng = np.random.default_rng(77)
    n = 340
    fa = pc.rand_seq(rng, n, p_n=0.0)
    places = rng.permutation(n)
    cut = np.cumsum([0, 15, 15, 15, 24, 30, 8])
    s1, s2, s3, dd, ee, ss = (places[cut[k]:cut[k + 1]] for k in range(6))
    a1, a2, a3 = _change(fa, s1), _change(fa, s2), _change(fa, s3)
    b1 = _change(a1, dd)
    b2 = _change(b1, ee)
    fs = _change(a2, ss)

    def noisy(f, trim=0):
        r = _change(f, rng.permutation(len(f))[:int(rng.integers(2, 4))], step=2)
        return r[:len(r) - trim]

    reads, role = [], []

    def species(name, f, count, trim=0):
        for k in range(count):
            r = noisy(f, int(rng.integers(0, trim + 1)))
            reads.append(pc.revcomp(r) if k % 4 == 3 else r)
            role.append(name)

    species("A1", a1, 7)
    species("A2", a2, 6)
    species("A3", a3, 3)
    species("B1", b1, 6)
    species("B2", b2, 6, trim=2)
    reads.append(_change(a1, dd[:12]) + b"G")
    role.append("X")
    for _ in range(4):
        reads.append(noisy(fs) + b"AC")
        role.append("S")
    lj = pc.rand_seq(rng, 1500, p_n=0.0)
    reads += [lj, gc.substitute(rng, lj, 30)[:-1], gc.substitute(rng, lj, 30)[:-2],
              gc.substitute(rng, lj, 29)[:-3]]
    role += ["L"] * 4
    reads += [gc.substitute(rng, lj, 56)[:-4], gc.substitute(rng, lj, 58)[:-5]]
    role += ["Lo"] * 2
    order = rng.permutation(len(reads))
    reads = [reads[i].decode() for i in order]
    role = np.array(role)[order]
    groups = [np.flatnonzero(np.isin(role, names)) for names in
              (("A1", "A2", "A3"), ("B1", "B2"), ("L", "Lo"))]
    return reads, role, groups


@functools.lru_cache(maxsize=None)
def species_oracle():
    """(lines, hits, per gene group the species groups as a set of frozensets) of species_bin(), by
    the literal restatement; asserts that the bin has the features its tests are about."""
    reads, role, groups = species_bin()
    lines, hits = gc.restated_lines(reads)
    exp = []
    for g in groups:
        idx = {str(int(i)) for i in g}
        templist, merged, grouplist = read_indexes(lines, idx, SSG)
        exp.append(as_sets(grouplist))
        # successor-only leftovers (§8i): every one joins two reads that the best lines join too
        best = best_lines(lines, idx, SSG)
        kept = {(int(e[0]), int(e[1])) for e in templist}
        assert best <= kept
        lab = gc.components(sorted(best), len(reads))
        for i, j in kept - best:
            assert lab[i] == lab[j] != NONE, ("a leftover line joins two groups", i, j)
        assert {frozenset(x) for x in gc.groups_of(lab)} == as_sets(merged)

    def where(name):
        return set(np.flatnonzero(role == name).tolist())

    def group_with(sets, members):
        return [s for s in sets if members & s]

    x = where("X")
    ga, gb = group_with(exp[0], where("A1")), group_with(exp[1], where("B1"))
    assert len(ga) == 1 and len(gb) == 1 and x <= ga[0] and x <= gb[0], "X is foreign to A and B"
    assert not (ga[0] & where("B1")) and not (gb[0] & where("A1"))
    s_in = [s for s in exp[0] if s & where("S")]
    assert len(s_in) == 1 and where("A2") <= s_in[0], "a read of the small group is pulled in"
    assert len(exp[0]) == 2 and len(exp[1]) == 2 and len(exp[2]) == 1
    assert not any(s & where("A3") for s in exp[0]), "the 3-read species is dropped"
    # A3 is a species on its own among the groups before the size filter
    merged0 = as_sets(read_indexes(lines, {str(int(i)) for i in groups[0]}, SSG)[1])
    assert frozenset(where("A3")) in merged0
    assert exp[2] == {frozenset(where("L"))}
    rev_kept = [h for h in hits if h[3] and 1 - h[2] / len(reads[h[1]]) >= SSG / 100]
    assert rev_kept, "reverse hits above the species threshold"
    lj = max(where("L"), key=lambda i: len(reads[i]))
    to_lj = sorted(h[2] for h in hits if h[1] == lj)
    assert to_lj[:3] == [31, 32, 32] and sorter.identity(31, 1500) == sorter.identity(32, 1500)
    ssg, margin = ssg_float(line_simils(lines))
    assert ssg is not None and margin > EDGE, (ssg, margin)
    return lines, hits, exp


@functools.lru_cache(maxsize=None)
def species_plan():
    """What the sorter hands to pairhits for the bin, and the host twin's state."""
    p, ln, q, t, cap_sg, cap_half = gc.bin_plan(species_bin()[0])
    return p, ln, q, t, cap_sg, cap_half, lib.pairhits_host(p, q, t, cap_sg, cap_half, n_threads=16)


# ---- random histograms ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_histograms(count=300, seed=9):
    """`count` histograms over the 1001 identity classes with the float SSG of a shuffled line
    order more than EDGE from every edge (at an edge the reference's answer depends on the order
    of its lines; candidates there are passed over): (hist uint64, the float SSG)."""
    rng = np.random.default_rng(seed)
    out, tried = [], 0
    while len(out) < count:
        tried += 1
        assert tried <= 2 * count, "too many histograms at an edge"
        lo = int(rng.integers(500, 990))
        width = int(rng.integers(1, 1001 - lo))
        n_lines = int(rng.integers(1, 3000))
        shape = rng.integers(0, 3)
        k = rng.integers(lo, lo + width, n_lines)
        if shape == 1:      # a peak near the top and a long tail
            top = lo + width - 1 - rng.integers(0, min(width, 5), n_lines)
            k = np.where(rng.random(n_lines) < 0.7, top, k)
        elif shape == 2:    # few distinct values
            k = lo + (k - lo) // max(width // 3, 1) * max(width // 3, 1)
        hist = np.bincount(k, minlength=sorter.N_CLASSES).astype(np.uint64)
        ssg, margin = ssg_float([float(str(x / 1000)) for x in rng.permutation(k)])
        if margin > EDGE:
            out.append((hist, ssg))
    return out


# ---- expectations from numpy alone ---------------------------------------------------------------

def np_hithist(t, pair, d, bin_off, bins, n_classes):
    at = np.asarray(bin_off, dtype=np.int64)[t[pair]] + d.astype(np.int64)
    return np.bincount(np.asarray(bins)[at], minlength=n_classes).astype(np.uint64)


def np_cross(q, t, pair, d, label, cap2):
    """The mask over the hits that dmx_pairhits_cross keeps."""
    label, cap2 = np.asarray(label), np.asarray(cap2, dtype=np.int64)
    a, b = q[pair], t[pair]
    return (cap2[b] >= 0) & (d.astype(np.int64) <= cap2[b]) & (label[a] != label[b])


def np_within(q, t, pair, d, tie2, label, xa, xb, n_nodes):
    """dmx_hitgroups_within's labels by label propagation (genegroups_cases.components)."""
    tie2, label = np.asarray(tie2, dtype=np.int64), np.asarray(label)
    a, b = q[pair].astype(np.int64), t[pair].astype(np.int64)
    keep = (label[a] == label[b]) & (label[b] != NONE) & (tie2[b] != NONE) & (d <= tie2[b])
    e = np.stack([np.concatenate([a[keep], np.asarray(xa, dtype=np.int64)]),
                  np.concatenate([b[keep], np.asarray(xb, dtype=np.int64)])], axis=1)
    return gc.components(np.unique(e, axis=0), n_nodes)


def flat_table(n_reads, top_d, n_classes, spread, rng):
    """A table for scale_case lists: a row of top_d + 1 classes per read; spread = 1: every
    entry is one class; otherwise classes drawn from 0 .. spread - 1."""
    bin_off = (np.arange(n_reads, dtype=np.uint32) * np.uint32(top_d + 1))
    if spread == 1:
        bins = np.full(n_reads * (top_d + 1), n_classes - 1, dtype=np.uint16)
    else:
        bins = rng.integers(0, spread, n_reads * (top_d + 1)).astype(np.uint16)
    return bin_off, bins
