"""The packed index screen's step without its cost (bare groups): a Python model
of `myers_step_pk` on two 16-bit halves of a dword, as `iscreen4_kernel` runs it.

The last-row cost d of a half is redundant: row 0 is free and the padding rows always match, so
d = popcount(pv) - popcount(mv) after every column.  A scan may therefore drop d for any number of
leading columns and take it back from the deltas before the first column that is counted.
"""
import numpy as np
import pytest

H = 0xFFFF


def pk_add(a, b):
    return (((a & H) + (b & H)) & H) | ((((a >> 16) + (b >> 16)) & H) << 16)


def pk_sub(a, b):
    return (((a & H) - (b & H)) & H) | ((((a >> 16) - (b >> 16)) & H) << 16)


def pk_shl(a, n):
    return (((a & H) << n) & H) | ((((a >> 16) << n) & H) << 16)


def pk_shr(a, n):
    return ((a & H) >> n) | (((a >> 16) >> n) << 16)


def pk_min(a, b):
    return min(a & H, b & H) | (min(a >> 16, b >> 16) << 16)


def step_bare(eq, pv, mv):
    """myers_step_pk_bare: two 16-bit blocks, last row = bit 15 of each half."""
    m32 = 0xFFFFFFFF
    xv = eq | mv
    s = pk_add(eq & pv, pv)
    ph = (mv | ~(s | pv | eq)) & m32
    mh = pv & ((s ^ pv) | eq)
    ph2, mh2 = pk_shl(ph, 1), pk_shl(mh, 1)
    return (mh2 | ~(xv | ph2)) & m32, ph2 & xv, ph, mh


def step(eq, pv, mv, d):
    """myers_step_pk: the same with the per-half last-row cost."""
    pv2, mv2, ph, mh = step_bare(eq, pv, mv)
    return pv2, mv2, pk_sub(pk_add(d, pk_shr(ph, 15)), pk_shr(mh, 15))


def cost_from_deltas(pv, mv):
    """pk_cost_from_deltas: popcount(pv half) - popcount(mv half), per half."""
    lo = (bin(pv & H).count("1") - bin(mv & H).count("1")) & H
    hi = (bin(pv >> 16).count("1") - bin(mv >> 16).count("1")) & H
    return lo | (hi << 16)


def half_rows(block, code):
    """Match bits of one half for a read code (0..3, 4 = non-ACGT): the block's rows in the top
    l bits, all-match padding below (non-ACGT matches only the padding)."""
    l = len(block)
    rows = 0
    for r, b in enumerate(block):
        if code < 4 and b == code:
            rows |= 1 << r
    return ((rows << (16 - l)) | ((1 << (16 - l)) - 1)) & H


def initial(l0, l1):
    pv = ((H << (16 - l0)) & H) | (((H << (16 - l1)) & H) << 16)
    return pv, 0, l0 | (l1 << 16)


def dp_last_row(block, codes):
    """Plain DP: D(i, 0) = i, D(0, x) = 0; the last row's cost after every column."""
    col = list(range(len(block) + 1))
    out = []
    for c in codes:
        new = [0]
        for i, b in enumerate(block, 1):
            new.append(min(col[i - 1] + (0 if (c < 4 and b == c) else 1), col[i] + 1,
                           new[i - 1] + 1))
        col = new
        out.append(col[-1])
    return out


def _case(rng):
    l0, l1 = int(rng.integers(1, 17)), int(rng.integers(1, 17))
    b0, b1 = rng.integers(0, 4, l0).tolist(), rng.integers(0, 4, l1).tolist()
    n = int(rng.integers(1, 81))
    codes = rng.choice(5, size=n, p=[0.24, 0.24, 0.24, 0.24, 0.04]).tolist()
    if rng.random() < 0.5:   # a copy of a block inside the read: costs go down to 0
        p = int(rng.integers(0, n))
        codes[p:p + l0] = b0[:max(0, n - p)]
    eqs = [half_rows(b0, c) | (half_rows(b1, c) << 16) for c in codes]
    return l0, l1, b0, b1, codes, eqs


@pytest.mark.parametrize("seed", range(4))
def test_cost_is_sum_of_deltas(seed):
    """After every column d of each half is popcount(pv) - popcount(mv), and it is the plain DP's
    last-row cost of that half's block."""
    rng = np.random.default_rng(4100 + seed)
    for _ in range(150):
        l0, l1, b0, b1, codes, eqs = _case(rng)
        pv, mv, d = initial(l0, l1)
        assert d == cost_from_deltas(pv, mv)
        ref0, ref1 = dp_last_row(b0, codes), dp_last_row(b1, codes)
        for x, eq in enumerate(eqs):
            pv, mv, d = step(eq, pv, mv, d)
            assert d == cost_from_deltas(pv, mv)
            assert (d & H, d >> 16) == (ref0[x], ref1[x])


@pytest.mark.parametrize("seed", range(4))
def test_bare_prefix_gives_the_same_minima(seed):
    """Dropping d for the first c columns and restoring it from the deltas gives the full scan's
    minimum over the counted columns (from qlo >= c on), for every c, and the same final state
    (the partial-I rows at the read end read pv and mv)."""
    rng = np.random.default_rng(4200 + seed)
    for _ in range(60):
        l0, l1, _, _, _, eqs = _case(rng)
        n = len(eqs)
        pv, mv, d = initial(l0, l1)
        full = []
        for eq in eqs:
            pv, mv, d = step(eq, pv, mv, d)
            full.append(d)
        end = (pv, mv, d)
        for c in range(n + 1):
            pv, mv, d = initial(l0, l1)
            for eq in eqs[:c]:
                pv, mv, _, _ = step_bare(eq, pv, mv)
            d = cost_from_deltas(pv, mv)
            got = []
            for eq in eqs[c:]:
                pv, mv, d = step(eq, pv, mv, d)
                got.append(d)
            assert got == full[c:]
            assert (pv, mv, d) == end
            for qlo in {c, (c + n) // 2, n}:   # the minimum a chunk would test
                m = m_ref = 0xFFFFFFFF
                for x in range(qlo, n):
                    m, m_ref = pk_min(m, got[x - c]), pk_min(m_ref, full[x])
                assert m == m_ref
