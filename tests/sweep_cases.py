"""The one generator of random demux cases (no GPU code): the fixed, stratified slice that
test_sweep_host.py (CPU) and test_sweep.py (GPU) run, and the open-ended cases that
tools/parity_sweep.py draws.  DESIGN.md §8c.1 has the measured draw table that motivates the strata.

Every case comes from a random stream of its own, so it can be rebuilt alone from its id:

    fixed slice   "<stratum>-<k>"   default_rng([SEED, STRATA.index(stratum), k])
    sweep         "<seed>:<k>"      default_rng([seed, k])

A case is a dict of inputs (`build_case`, `sweep_case`): kind "single" (panels[0] with a where per
adapter), "pair" (two rounds, FRONT then BACK) or "linked" (-g F...R pairs), e, min_overlap, rc
and the reads.  `expected` is the oracle's answer and `classify` what the library's host accessors
say about the panels; neither touches a GPU.  `set_panels` / `pack` put a case on a context.

The slice is stratified by the path the host says a panel takes: draw k of a stratum is shaped by
recipe k % quota (adapter lengths by build_pieces' own rule: the shortest piece decides the
sampling step), and `fixed_cases` keeps, per recipe, the first draw whose class the host confirms.
"""
import functools

import numpy as np

import oracle
import pieces_seam_cases as sc
import test_pieces_host as tph
from dmx import lib, synth

SEED = 2610
MAX_DRAWS = 60            # draws per recipe before a stratum is declared unreachable
ALPH = np.array(list("ACGT"))
WILD = list("NRYSWKMBDHV")
rc = tph.revcomp


def rand_seq(rng, n):
    return "".join(ALPH[rng.integers(0, 4, size=int(n))])


def mutate(rng, a, err):
    """`a` with a share `err` of its characters edited (60 % substitutions, 20 % deletions, 20 %
    insertions); wildcards are drawn as a base first."""
    out = []
    for c in a:
        if c not in "ACGT":
            c = "ACGT"[int(rng.integers(4))]
        r = rng.random()
        if r < err * 0.6:
            out.append("ACGT"[int(rng.integers(4))])
        elif r < err * 0.8:
            pass
        elif r < err:
            out += [c, "ACGT"[int(rng.integers(4))]]
        else:
            out.append(c)
    return "".join(out)


def random_panel(rng):
    """The sweep's unshaped panel: 1..16 adapters of 3..64 nt, 40 % with shared flanks."""
    n = int(rng.integers(1, 17))
    lo = int(rng.integers(3, 40))
    hi = int(rng.integers(lo, 65))
    wild = float(rng.choice([0.0, 0.0, 0.05, 0.2]))
    shared = rng.random() < 0.4          # common flanks (exercises the window filter path)
    pre, suf = rand_seq(rng, int(rng.integers(0, 25))), rand_seq(rng, int(rng.integers(10, 25)))
    out = []
    for _ in range(n):
        L = int(rng.integers(lo, hi + 1))
        s = rand_seq(rng, L)
        if shared:
            s = (pre + rand_seq(rng, int(rng.integers(3, 29))) + suf)[:64]
        s = "".join(c if rng.random() >= wild else str(rng.choice(WILD)) for c in s)
        out.append(s)
    return out


def reads_for(rng, panel, n, err_hi=0.15, plant_lo=0, maxlen=None):
    """n random reads of 0..maxlen nt (maxlen 40, 150 or 600 unless given), 1 % of them with N,
    each with plant_lo..2 planted adapter copies of 0..err_hi edits per nt: whole inside the read,
    or cut and put at a read end; 30 % of the reads reverse-complemented."""
    seqs = []
    if maxlen is None:
        maxlen = int(rng.choice([40, 150, 600]))
    for _ in range(n):
        s = rand_seq(rng, int(rng.integers(0, maxlen + 1)))
        if rng.random() < 0.01:
            s = "".join(c if rng.random() > 0.05 else "N" for c in s)
        for _k in range(int(rng.integers(plant_lo, 3))):
            frag = mutate(rng, panel[int(rng.integers(len(panel)))], float(rng.uniform(0, err_hi)))
            u = rng.random()
            if u < 0.2 and len(frag) > 1:
                frag = frag[int(rng.integers(1, len(frag))):]
                s = frag + s
            elif u < 0.4 and len(frag) > 1:
                frag = frag[:int(rng.integers(1, len(frag)))]
                s = s + frag
            else:
                p = int(rng.integers(0, len(s) + 1))
                s = s[:p] + frag + s[p:]
        if rng.random() < 0.3:
            s = rc(s)
        seqs.append(s)
    return seqs


# ---------------------------------------------------------------------------------------------
# What the host says about a case
# ---------------------------------------------------------------------------------------------
def _lib_where(w):
    return lib.DMX_FRONT if w == oracle.FRONT else lib.DMX_BACK


def classify(case, use_rc=None):
    """Per panel of the case, from dmx_panel_near_shared / dmx_panel_pieces / dmx_panel_reach:
    filter_len, near_shared, the piece screen's step and part_max, the set of entry offsets, the
    largest first sampled offset of a piece (j0) and the reach status; `mixed` when the panel
    holds FRONT and BACK adapters (the piece accessor has no such form: a mixed panel has no
    filter, so no pieces)."""
    out = []
    f_rc = lib.DMX_RC if (case["rc"] if use_rc is None else use_rc) else 0
    for seqs, wh in zip(case["panels"], case["wheres"]):
        lw = [_lib_where(w) for w in wh]
        mixed = len(set(lw)) > 1
        a = (seqs, (lib.DMX_FRONT if mixed else lw[0]) | f_rc, case["e"], case["min_overlap"])
        r1, near = lib.panel_near_shared(*a, wheres=lw if mixed else None)
        r2, reach = lib.panel_reach(*a, wheres=lw if mixed else None)
        c = dict(near, mixed=mixed, front=lw[0] == lib.DMX_FRONT, status=(r1, r2),
                 step=0, part_max=0, offsets=set(), j0=0,
                 iupac=any(ch not in "ACGT" for s in seqs for ch in s))
        if not mixed:
            r3, info, ents = lib.panel_pieces(*a)
            first = {}
            for e in ents:
                key = (e["val"], e["len"], e["o"])
                first[key] = min(first.get(key, 9), e["off"])
            c.update(step=info["step"], part_max=info["part_max"], status=(r1, r2, r3),
                     offsets={e["off"] for e in ents}, j0=max(first.values(), default=0))
        out.append(c)
    return out


def min_piece(m, e, min_overlap=3):
    """The shortest piece build_pieces cuts from an ACGT adapter of m nt (capped at 16; 99 when
    the whole adapter is never accepted and builds none)."""
    if m < min_overlap:
        return 99
    K = tph.full_k(m, e / m if e >= 1 else e)
    return min(16, m // (K + 1))


STEP_OF = {4: (11, 16), 2: (9, 10), 1: (8, 8), 0: (1, 7)}   # step: the shortest piece's range


def _lengths(rng, n, lo, hi, e, mo, step):
    """n adapter lengths in lo..hi whose shortest pieces give `step` (0: no piece screen): all at
    or above the range's lower end, the first inside it.  None when no length does."""
    need, cap = STEP_OF[step]
    if step == 0:
        ok = tight = [m for m in range(lo, hi + 1) if min_piece(m, e, mo) <= cap]
    else:
        ok = [m for m in range(lo, hi + 1) if need <= min_piece(m, e, mo) <= 16]
        tight = [m for m in ok if min_piece(m, e, mo) <= cap]
    if not tight:
        return None
    return [int(rng.choice(tight))] + [int(rng.choice(ok)) for _ in range(n - 1)]


def _flank_panel(rng, lengths, pre, suf):
    p, s = rand_seq(rng, pre), rand_seq(rng, suf)
    return [p + rand_seq(rng, L - pre - suf) + s for L in lengths]


def _wild_mid(rng, seqs, pre, suf, share=0.1):
    """IUPAC codes in the adapters' own middles (at least one per panel): the flanks stay shared."""
    out = []
    for i, s in enumerate(seqs):
        mid = list(s[pre:len(s) - suf])
        for j in range(len(mid)):
            if rng.random() < share or (i == 0 and j == 0):
                mid[j] = str(rng.choice(WILD))
        out.append(s[:pre] + "".join(mid) + s[len(s) - suf:])
    return out


# ---------------------------------------------------------------------------------------------
# The strata: (cases, recipes).  A recipe shapes the draw; `want` is what the host must confirm
# on top of the stratum's class.
# ---------------------------------------------------------------------------------------------
F, B = oracle.FRONT, oracle.BACK
STRATA = ("plain", "filter", "step1", "step2", "step4", "near", "near_off", "mixed", "pair2",
          "linked")
RECIPES = {
    "plain": [   # unrelated adapters: no shared suffix, no pieces
        dict(where=F, e="abs", mo=3, rc=True), dict(where=B, e=0.0, mo=3, rc=True),
        dict(where=F, e=0.1, mo=1, rc=False, wild=0.05), dict(where=B, e=0.2, mo=12, rc=True),
        dict(where=B, e="abs", mo=5, rc=False, wild=0.2), dict(where=F, e=0.3, mo=3, rc=True),
    ],
    "filter": [  # shared suffix, no pieces: IUPAC in the panel, or pieces shorter than 8 nt
        dict(where=F, e=0.1, mo=3, rc=True, pre=(10, 15), iupac="mid"),
        dict(where=B, e=0.1, mo=3, rc=True, pre=(0, 9), iupac="suf"),
        dict(where=B, e=0.2, mo=3, rc=True, pre=(10, 15), step=0),
        dict(where=F, e=0.15, mo=3, rc=False, pre=(0, 9), step=0),
        dict(where=F, e=2.0, mo=5, rc=True, pre=(10, 15), iupac="mid"),
        dict(where=B, e=0.3, mo=3, rc=True, pre=(0, 9), step=0),
    ],
    "step1": [
        dict(where=F, e=0.1, mo=3, rc=True, pre=(10, 15), step=1),
        dict(where=B, e=0.1, mo=3, rc=True, pre=(4, 10), step=1),
        dict(where=F, e=0.12, mo=3, rc=True, pre=(4, 10), step=1),
        dict(where=B, e=2.0, mo=5, rc=True, pre=(0, 6), step=1),
    ],
    "step2": [   # the benchmark panels' step
        dict(where=F, e=0.1, mo=3, rc=True, pre=(10, 15), step=2),
        dict(where=B, e=0.1, mo=3, rc=True, pre=(10, 15), step=2),
        dict(where=F, e=0.05, mo=3, rc=True, pre=(0, 1), suf=(10, 13), step=2),
        dict(where=B, e=3.0, mo=5, rc=True, pre=(4, 10), step=2),
    ],
    "step4": [
        dict(where=F, e=0.0, mo=3, rc=True, pre=(4, 10), step=4),
        dict(where=B, e=0.05, mo=3, rc=True, pre=(10, 15), step=4),
        dict(where=F, e=0.05, mo=5, rc=True, pre=(0, 6), step=4),
        dict(where=B, e=1.0, mo=3, rc=True, pre=(10, 15), step=4),
    ],
    "near": [    # FRONT, near_shared >= 0: the first two with the piece screen on
        dict(where=F, e=0.1, mo=3, rc=True, pre=(10, 15), step=2, want="pieces"),
        dict(where=F, e=0.05, mo=3, rc=False, pre=(0, 9), step=4, want="pieces"),
        dict(where=F, e=0.15, mo=3, rc=True, pre=(10, 15), iupac="mid"),
        dict(where=F, e=0.2, mo=3, rc=True, pre=(0, 6), suf=(14, 23), step=0),
    ],
    "near_off": [   # FRONT, filter on, near_shared == -1
        dict(where=F, e="abs23", mo=3, rc=True, pre=(0, 9), spread=True),   # unlike acc tables
        dict(where=F, e=0.1, mo=3, rc=True, pre=(0, 1), suffix_adapter=True),   # |adapter| = |S|
    ],
    "mixed": [
        dict(where="mixed", e=0.1, mo=3, rc=True, pre=(0, 9), flank=True),
        dict(where="mixed", e=0.15, mo=3, rc=False, wild=0.05),
        dict(where="mixed", e=2.0, mo=5, rc=True, pre=(10, 15), flank=True),
    ],
    "pair2": [   # two rounds, FRONT then BACK; shapes of (panel 1, panel 2)
        dict(e=0.1, mo=3, rc=True, shapes=("step2", "step2"), want="pieces"),
        dict(e=0.1, mo=3, rc=True, shapes=("iupac", "flank")),
        dict(e=0.15, mo=3, rc=False, shapes=("random", "flank")),
        dict(e=0.05, mo=5, rc=True, shapes=("flank", "flank")),
    ],
    "linked": [
        dict(e=0.1, mo=3, shapes=("random", "random")),
        dict(e=0.15, mo=3, shapes=("flank", "flank")),
        dict(e=2.0, mo=3, shapes=("random", "flank")),
    ],
}
QUOTA = {s: len(r) for s, r in RECIPES.items()}
# cases of the non-vacuity bar (at least a quarter of the reads matched) that needed more planted
# copies than reads_for's 0..2 per read: every read of these gets at least one
MORE_COPIES = {"plain": (4,)}


def _shaped_panel(rng, r, shape=None):
    """One panel of recipe r (or of a pair recipe's shape name)."""
    e, mo = r["e"], r["mo"]
    if shape is not None:
        r = dict(r, **{"step2": dict(pre=(10, 15), step=2), "flank": dict(pre=(0, 12), flank=True),
                       "iupac": dict(pre=(10, 15), iupac="mid"), "random": dict()}[shape])
    n = int(rng.integers(2, 13))
    if "pre" not in r:                                   # unrelated adapters
        lo = int(rng.integers(max(3, mo + 2 if mo > 3 else 3), 40))
        hi = int(rng.integers(lo, 65))
        seqs = [rand_seq(rng, int(rng.integers(lo, hi + 1))) for _ in range(n)]
        w = r.get("wild", 0.0)
        return ["".join(c if rng.random() >= w else str(rng.choice(WILD)) for c in s)
                for s in seqs]
    pre = int(rng.integers(*r["pre"]))
    suf = int(rng.integers(*r.get("suf", (10, 21))))
    lo = pre + suf + 3
    if "step" in r:
        lengths = _lengths(rng, n, lo, 64, e, mo, r["step"])
        if lengths is None:
            return None
    elif r.get("spread"):
        lengths = [lo, 64] + [int(rng.integers(lo, 65)) for _ in range(n - 2)]
    else:
        lengths = [int(rng.integers(lo, min(64, lo + 28) + 1)) for _ in range(n)]
    seqs = _flank_panel(rng, lengths, pre, suf)
    if r.get("iupac") == "mid":
        seqs = _wild_mid(rng, seqs, pre, suf)
    elif r.get("iupac") == "suf":                        # one code inside the shared suffix
        j, ch = int(rng.integers(1, suf)), str(rng.choice(WILD))
        seqs = [s[:len(s) - j] + ch + s[len(s) - j + 1:] for s in seqs]
    if r.get("suffix_adapter"):
        seqs[int(rng.integers(1, n))] = seqs[0][len(seqs[0]) - suf:]
    return seqs


def _draw(stratum, k):
    """(rng, recipe, inputs without reads) of draw k, or inputs None when the shape has no panel."""
    rng = np.random.default_rng([SEED, STRATA.index(stratum), k])
    r = dict(RECIPES[stratum][k % QUOTA[stratum]])
    if r["e"] == "abs":
        r["e"] = float(rng.integers(1, 5))
    elif r["e"] == "abs23":
        r["e"] = float(rng.integers(2, 4))
    case = dict(id=f"{stratum}-{k}", stratum=stratum, e=float(r["e"]), min_overlap=r["mo"],
                rc=bool(r.get("rc", False)))
    if stratum in ("pair2", "linked"):
        p1, p2 = (_shaped_panel(rng, r, s) for s in r["shapes"])
        if p1 is None or p2 is None:
            return rng, r, None
        if stratum == "linked":
            n = min(len(p1), len(p2))
            p1, p2 = p1[:n], p2[:n]
        case.update(kind="pair" if stratum == "pair2" else "linked", panels=[p1, p2],
                    wheres=[[F] * len(p1), [B] * len(p2)])
        return rng, r, case
    seqs = _shaped_panel(rng, r)
    if seqs is None:
        return rng, r, None
    if r["where"] == "mixed":
        wh = [F if rng.random() < 0.5 else B for _ in seqs]
        wh[0], wh[-1] = F, B
    else:
        wh = [r["where"]] * len(seqs)
    case.update(kind="single", panels=[seqs], wheres=[wh])
    return rng, r, case


def in_class(stratum, case, cls, want=None):
    """Does the host put the panel(s) where the stratum says?  (The census of test_sweep_host.py
    asserts exactly this of every fixed case.)"""
    c = cls[0]
    if any(s != 0 for x in cls for s in x["status"]):
        return False
    if want == "pieces" and not all(x["step"] > 0 for x in cls):
        return False
    if stratum == "plain":
        return c["filter_len"] == 0 and c["step"] == 0 and not c["mixed"]
    if stratum == "filter":
        return c["filter_len"] > 0 and c["step"] == 0
    if stratum in ("step1", "step2", "step4"):
        return c["step"] == int(stratum[4:])
    if stratum == "near":
        return c["front"] and not c["mixed"] and c["near_shared"] >= 0
    if stratum == "near_off":
        return c["front"] and not c["mixed"] and c["filter_len"] > 0 and c["near_shared"] == -1
    if stratum == "mixed":
        return c["mixed"]
    return len(cls) == 2 and case["kind"] == ("pair" if stratum == "pair2" else "linked")


# ---------------------------------------------------------------------------------------------
# Reads
# ---------------------------------------------------------------------------------------------
def _k_copy(rng, ad, e, mo):
    """(copy of ACGT adapter `ad` with exactly K = acc[m] edits, one in every piece but one; K)."""
    K = tph.full_k(len(ad), e / len(ad) if e >= 1 else e)
    if len(ad) < mo or len(ad) // (K + 1) < 1:
        return ad, 0
    pcs = tph.pieces_of(len(ad), K)
    return (tph.mutate(rng, ad, pcs, int(rng.integers(K + 1))) if K else ad), K


def _surviving_piece_reads(rng, case, p, other=None):
    """(a): per adapter of ACGT panel p a K-edit copy at the read's start, middle and end, the
    strands alternating where rc is on.  other: the pair's second panel, whose copy a round-1
    read carries after the first (and a round-2 read before it), so that both rounds match."""
    seqs, e, mo = case["panels"][p], case["e"], case["min_overlap"]
    out, meta, turn = [], [], 0
    for a, ad in enumerate(seqs):
        for place in ("start", "middle", "end"):
            copy, K = _k_copy(rng, ad, e, mo)
            L, fl = int(rng.integers(120, 500)), int(rng.integers(0, 5))
            if other is not None:   # FRONT copy first, the BACK copy after it
                o = case["panels"][other]
                oc = mutate(rng, o[int(rng.integers(len(o)))], 0.02)
                first, second = (copy, oc) if p == 0 else (oc, copy)
                pads = {"start": (fl, L, 0), "middle": (L // 2, L, L // 2), "end": (0, L, fl)}
                x, y, z = pads[place]
                s = rand_seq(rng, x) + first + rand_seq(rng, y) + second + rand_seq(rng, z)
            elif place == "start":
                s = rand_seq(rng, fl) + copy + rand_seq(rng, L)
            elif place == "end":
                s = rand_seq(rng, L) + copy + rand_seq(rng, fl)
            else:
                s = rand_seq(rng, L // 2) + copy + rand_seq(rng, L // 2)
            strand = turn & 1 if case["rc"] else 0
            turn += 1
            out.append(rc(s) if strand else s)
            meta.append((p, a, K, strand))
    return out, meta


def _near_start_reads(rng, case, flen):
    """(b): suffixes of 3..|S| nt of an adapter at read offset 0..4, with at most one edit."""
    out = []
    seqs = case["panels"][0]
    for i in range(40):
        ad = seqs[i % len(seqs)]
        frag = ad[len(ad) - int(rng.integers(3, max(flen, 3) + 1)):]
        frag = "".join(c if c in "ACGT" else "ACGT"[int(rng.integers(4))] for c in frag)
        if i & 1:
            j, t = int(rng.integers(len(frag))), int(rng.integers(3))
            frag = frag[:j] + ("ACGT".replace(frag[j], "")[int(rng.integers(3))] if t == 0 else
                               "" if t == 1 else frag[j] + "ACGT"[int(rng.integers(4))]) + \
                frag[j + 1:]
        s = rand_seq(rng, i % 5) + frag + rand_seq(rng, int(rng.integers(60, 300)))
        out.append(rc(s) if case["rc"] and i % 4 >= 2 else s)
    return out


def _long_reads(rng, case, pmax, n):
    """(c): n reads longer than 2 x part_max, so that the per-part screen cuts them into three or
    more parts.  The first six hold a K-edit copy whose surviving piece starts 1..3 nt before an
    interior multiple of part_max and before an interior part boundary (pieces_seam_cases), on
    both strands; the rest one or two copies anywhere."""
    seqs, e, mo = case["panels"][0], case["e"], case["min_overlap"]
    out = []
    for i in range(n):
        L = 2 * pmax + 1 + int(rng.integers(0, 400))
        ad = seqs[int(rng.integers(len(seqs)))]
        K = tph.full_k(len(ad), e / len(ad) if e >= 1 else e)
        s = None
        if i < 6 and len(ad) >= mo:
            marks = [pmax, 2 * pmax] + sc.boundaries(L, pmax)
            pcs = tph.pieces_of(len(ad), K)
            for _ in range(8):
                t = marks[i % len(marks)] - int(rng.integers(1, 4))
                s, _end = sc.place(rng, ad, pcs, int(rng.integers(K + 1)), L, t,
                                   bool(i & 1) and case["rc"])
                if s is not None:
                    break
        if s is None:
            s = rand_seq(rng, L)
            for _ in range(int(rng.integers(1, 3))):
                frag = mutate(rng, ad, float(rng.uniform(0, 0.08)))
                p = int(rng.integers(0, L - len(frag)))
                s = s[:p] + frag + s[p + len(frag):]
            if case["rc"] and rng.random() < 0.5:
                s = rc(s)
        out.append(s)
    return out


def _pair_reads(rng, case, n, err):
    """Reads holding a copy of a panel-1 adapter, a body and a copy of a panel-2 adapter (the
    same index for linked pairs), as the sweep builds them."""
    p1, p2 = case["panels"]
    out = []
    for _ in range(n):
        a = int(rng.integers(len(p1)))
        b = a if case["kind"] == "linked" else int(rng.integers(len(p2)))
        s = (rand_seq(rng, int(rng.integers(0, 20))) + mutate(rng, p1[a], err) +
             rand_seq(rng, int(rng.integers(0, 200))) + mutate(rng, p2[b], err) +
             rand_seq(rng, int(rng.integers(0, 20))))
        out.append(rc(s) if case["rc"] and rng.random() < 0.3 else s)
    return out


def _add_reads(rng, case, cls):
    """The reads of a fixed case (300..500): reads_for's planted copies plus (a)..(d) above."""
    st, e = case["stratum"], case["e"]
    seqs = [s for p in case["panels"] for s in p]
    rate = e / max(len(s) for s in seqs) if e >= 1 else e
    target = int(rng.integers(300, 501))
    extra, meta = [], []
    steps = st.startswith("step")
    if (steps or st in ("near", "pair2")):
        for p, c in enumerate(cls):
            if not c["iupac"]:
                rd, mt = _surviving_piece_reads(rng, case, p, (1 - p) if st == "pair2" else None)
                meta += [(len(extra) + i,) + m for i, m in enumerate(mt)]
                extra += rd
    if st in ("near", "near_off"):
        extra += _near_start_reads(rng, case, cls[0]["filter_len"])
    if steps:
        extra += _long_reads(rng, case, cls[0]["part_max"], -(-target * 22 // 100))
    if case["kind"] != "single":
        extra += _pair_reads(rng, case, target * 6 // 10 - len(extra) // 2,
                             min(0.05, 0.6 * rate))
    ad = seqs[int(rng.integers(len(seqs)))]
    tail = ["", "ACGT"[int(rng.integers(4))], ad[:7], ad[-7:]]
    k = int(case["id"].rsplit("-", 1)[1]) % QUOTA[st]
    base = reads_for(rng, seqs, max(20, target - len(extra) - len(tail)),
                     err_hi=max(0.03, min(0.15, 1.5 * rate)),
                     plant_lo=1 if k in MORE_COPIES.get(st, ()) else 0)
    reads = extra + base + tail
    order = rng.permutation(len(reads))   # every chunk of a chunked run gets reads of every kind
    place = np.empty_like(order)
    place[order] = np.arange(len(order))
    case["reads"] = [reads[i] for i in order]
    # (read, panel, adapter, K, strand) of the (a) copies, in the order they were made
    case["k_copies"] = [(int(place[m[0]]),) + m[1:] for m in meta]


@functools.lru_cache(maxsize=None)
def _accepted(stratum, slot):
    """The first draw k = slot, slot + quota, ... whose class the host confirms."""
    for k in range(slot, slot + MAX_DRAWS * QUOTA[stratum], QUOTA[stratum]):
        _, r, case = _draw(stratum, k)
        if case is not None and in_class(stratum, case, classify(case), r.get("want")):
            return k
    raise RuntimeError(f"sweep_cases: no draw of {stratum} recipe {slot} reaches its class in "
                       f"{MAX_DRAWS} tries; fix the recipe's shape, not the quota")


def fixed_ids():
    return [f"{s}-{_accepted(s, j)}" for s in STRATA for j in range(QUOTA[s])]


def build_case(case_id):
    """The inputs of fixed case "<stratum>-<k>", from that draw's stream alone."""
    stratum, k = case_id.rsplit("-", 1)
    rng, r, case = _draw(stratum, int(k))
    cls = classify(case) if case is not None else None
    if case is None or not in_class(stratum, case, cls, r.get("want")):
        raise KeyError(f"{case_id}: the draw is not in its stratum")
    _add_reads(rng, case, cls)
    return case


def fixed_cases():
    return [build_case(i) for i in fixed_ids()]


# ---------------------------------------------------------------------------------------------
# The sweep's open-ended cases (tools/parity_sweep.py)
# ---------------------------------------------------------------------------------------------
def case_random(rng):
    panel = random_panel(rng)
    e = float(rng.choice([0.0, 0.05, 0.1, 0.15, 0.2, 0.3])) if rng.random() < 0.8 else \
        float(rng.integers(1, 5))
    mo = int(rng.choice([1, 2, 3, 3, 3, 5, 8, 12]))
    use_rc = bool(rng.random() < 0.7)
    kind = str(rng.choice(["front", "back", "mixed"]))
    wh = [F if (kind == "front" or (kind == "mixed" and rng.random() < 0.5)) else B
          for _ in panel]
    return dict(kind="single", panels=[panel], wheres=[wh], e=e, min_overlap=mo, rc=use_rc,
                reads=reads_for(rng, panel, int(rng.integers(200, 3000))))


def case_random_pair(rng):
    """Two random panels as two rounds (FRONT then BACK) or as linked -g F...R pairs."""
    linked = bool(rng.random() < 0.4)
    p1 = random_panel(rng)
    p2 = random_panel(rng)
    if linked:
        k = min(len(p1), len(p2))
        p1, p2 = p1[:k], p2[:k]
    e = float(rng.choice([0.05, 0.1, 0.15, 0.2])) if rng.random() < 0.85 else \
        float(rng.integers(1, 4))
    mo = int(rng.choice([1, 3, 3, 5]))
    use_rc = (not linked) and bool(rng.random() < 0.8)
    seqs = []
    for s in reads_for(rng, p1 + p2, int(rng.integers(200, 2500))):
        if linked and rng.random() < 0.6:
            a = int(rng.integers(len(p1)))
            s = (rand_seq(rng, int(rng.integers(0, 20))) + mutate(rng, p1[a], 0.05) +
                 rand_seq(rng, int(rng.integers(0, 200))) + mutate(rng, p2[a], 0.05) +
                 rand_seq(rng, int(rng.integers(0, 20))))
        seqs.append(s)
    return dict(kind="linked" if linked else "pair", panels=[p1, p2],
                wheres=[[F] * len(p1), [B] * len(p2)], e=e, min_overlap=mo, rc=use_rc, reads=seqs)


def case_synth(rng):
    cfg = str(rng.choice(["c1", "c2", "c2x24", "c4", "c5"]))
    seed = int(rng.integers(1000, 10 ** 6))
    n = int(rng.integers(2000, 20000))
    e = 0.1 if rng.random() < 0.7 else float(rng.choice([0.05, 0.15, 0.2]))
    d = synth.generate(cfg, n=n, seed=seed)
    return dict(kind="linked" if cfg == "c5" else "pair", panels=[d["sp5"], d["sp27"]],
                wheres=[[F] * len(d["sp5"]), [B] * len(d["sp27"])], e=e, min_overlap=3,
                rc=cfg != "c5", packed=(d["blob"], d["offsets"], d["lengths"]),
                synth=dict(config=cfg, seed=seed, n=n))


def sweep_case(seed, k):
    """Case k of the sweep with that seed: half single random panels, 30 % pairs, 20 % the seeded
    synthetic configs."""
    rng = np.random.default_rng([int(seed), int(k)])
    u = rng.random()
    case = (case_random if u < 0.5 else case_random_pair if u < 0.8 else case_synth)(rng)
    return dict(case, id=f"{seed}:{k}", stratum="sweep")


def case_by_id(case_id):
    """A fixed case ("step2-5") or a sweep case ("41:17")."""
    if ":" in case_id:
        return sweep_case(*case_id.split(":"))
    return build_case(case_id)


# ---------------------------------------------------------------------------------------------
# Running a case: the oracle's answer, and the case on a context
# ---------------------------------------------------------------------------------------------
MODE = {"single": 0, "pair": 1, "linked": 2}


def ascii_batch(case):
    return case["packed"] if "packed" in case else oracle.pack_ascii(case["reads"])


def n_reads(case):
    return len(ascii_batch(case)[2])


def expected(case, use_rc=None, threads=8):
    """The oracle's 40 bytes per read (use_rc: the case's own unless given)."""
    blob, offs, lens = ascii_batch(case)
    ps = [oracle.Panel(s, w, max_errors=case["e"], min_overlap=case["min_overlap"])
          for s, w in zip(case["panels"], case["wheres"])]
    return oracle.run_batch(ps[0], ps[1] if len(ps) > 1 else None, blob, offs, lens,
                            mode=MODE[case["kind"]],
                            use_rc=case["rc"] if use_rc is None else use_rc, threads=threads)


def set_panels(ctx, case, use_rc=None):
    use_rc = case["rc"] if use_rc is None else use_rc
    for r, (seqs, wh) in enumerate(zip(case["panels"], case["wheres"])):
        lw = [_lib_where(w) for w in wh]
        if len(set(lw)) > 1:
            ctx.set_panel_mixed(r, seqs, lw, use_rc, case["e"], case["min_overlap"])
        else:
            ctx.set_panel(r, seqs, lw[0] | (lib.DMX_RC if use_rc else 0), case["e"],
                          case["min_overlap"])
    ctx.set_mode((lib.MODE_SINGLE, lib.MODE_TWO_ROUND, lib.MODE_LINKED)[MODE[case["kind"]]])


def pack(case):
    return lib.pack(*ascii_batch(case))


def differing(got, exp):
    g = got.view(np.uint8).reshape(len(got), -1)
    e = exp.view(np.uint8).reshape(len(exp), -1)
    return np.nonzero((g != e).any(axis=1))[0]
