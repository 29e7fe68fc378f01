// dmx_pairdist.hip — exact edit distance between pairs of reads of the resident batch
// (include/dmx.h dmx_pairdist).  Replaces the edlib.align(task='distance') calls
// of the amplicon-sorting stage's similarity pass (amplicon_sorter.py:225-235, 777-808) and of
// its HW comparisons (:840-852).
//
// Block Myers/Hyyro: the query's rows are cut into 64-row words, one word per lane.  The G lanes
// of a group run as a systolic array: at step t lane w advances column t - w of its word; the
// horizontal delta (-1/0/+1) of the word's last row and the column's target symbol travel to
// lane w + 1 by a one-lane shift.  A query of more than 64 G rows runs in stripes of 64 G rows;
// the last row's horizontal deltas of a stripe wait in a scratch row (one byte per column) for
// the next stripe.  A wave carries floor(64 / G) groups of one size G (kPdSizes), so short pairs
// do not idle 64 lanes.
//
// dmx_pairalign (edlib.align(mode='NW', task='path') of create_alignment,
// amplicon_sorter.py:333-339) runs the same scheme with a trace of every word's Pv / Mv and
// last-row score per column (pairalign_kernel), and a second kernel that walks the edit path
// back through it (pairalign_traceback_kernel).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>

#include "dmx_internal.h"

namespace dmx {

// The group sizes a wave may be cut into: every distinct floor(64 / k).  A pair runs in the
// smallest size that holds its query's words (64 for longer queries, which then run in stripes).
static const int kPdSizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21, 32, 64};
constexpr int kPdNSizes = (int)(sizeof kPdSizes / sizeof *kPdSizes);
constexpr uint32_t kPdWavesPerBlock = 4;
constexpr size_t kPdChunkDefault = 1u << 20;          // pairs per launch (DMX_PD_CHUNK)
constexpr size_t kPdScratchMax = 64u << 20;           // scratch bytes per launch

struct PdPair {
    uint32_t q, t, cap, flags;   // flags: DMX_PD_RC | 0x100 (cap given)
    uint64_t soff;               // the pair's scratch row (queries of more than one stripe)
};
struct PdWave {
    uint32_t first, count, G, steps;   // pairs[first .. first + count), one group of G lanes each
};

struct PdArgs {
    Packed pk;
    const uint64_t* offs;
    const uint32_t* lens;
    const PdPair* pairs;
    const PdWave* waves;
    uint32_t n_waves;
    uint32_t n_pairs;
    int mode;
    uint8_t* scratch;
    uint64_t scratch_bytes;
    uint32_t* out;
};

struct PdState {
    PdPair* d_pairs = nullptr;
    PdWave* d_waves = nullptr;
    uint32_t* d_out = nullptr;
    uint8_t* d_scratch = nullptr;
    size_t pair_cap = 0, wave_cap = 0, scratch_cap = 0;
    hipEvent_t ev[2] = {};
    float ms = 0.f;
};

// ---- dmx_pairalign: the NW distance and the edit path -------------------------
struct PaPair {
    uint32_t q, t, flags, pad;
    uint64_t soff;               // the pair's scratch row (queries of more than one stripe)
    uint64_t toff;               // its trace: word-step (wi, j) is entry toff + wi * n + j
    uint64_t roff;               // its (m + n)-byte op region
};

struct PaArgs {
    Packed pk;
    const uint64_t* offs;
    const uint32_t* lens;
    const PaPair* pairs;
    const PdWave* waves;
    uint32_t n_waves;
    uint32_t n_pairs;
    uint8_t* scratch;
    uint64_t scratch_bytes;
    ulonglong2* pm;              // trace: Pv, Mv of a word after a column
    uint16_t* sc;                // trace: D(word's last row, column)
    uint64_t trace_steps;        // entries of pm / sc
    uint8_t* ops;
    uint64_t ops_bytes;
    uint32_t* out;               // per pair: distance, path length
};

struct PaState {
    PaPair* d_pairs = nullptr;
    PdWave* d_waves = nullptr;
    uint32_t* d_out = nullptr;
    uint8_t* d_scratch = nullptr;
    ulonglong2* d_pm = nullptr;
    uint16_t* d_sc = nullptr;
    uint8_t* d_ops = nullptr;
    size_t pair_cap = 0, wave_cap = 0, scratch_cap = 0, trace_cap = 0, ops_cap = 0;
    hipEvent_t ev[3] = {};
    float ms[2] = {0.f, 0.f};    // forward pass, traceback
    int launches = 0;            // chunks of the last call
};

void pd_release(Ctx* c) {
    if (PdState* s = c->pd) {
        void* bufs[] = {s->d_pairs, s->d_waves, s->d_out, s->d_scratch};
        for (void* b : bufs)
            if (b) hipFree(b);
        for (auto& e : s->ev)
            if (e) hipEventDestroy(e);
        delete s;
        c->pd = nullptr;
    }
    if (PaState* s = c->pa) {
        void* bufs[] = {s->d_pairs, s->d_waves, s->d_out, s->d_scratch, s->d_pm, s->d_sc, s->d_ops};
        for (void* b : bufs)
            if (b) hipFree(b);
        for (auto& e : s->ev)
            if (e) hipEventDestroy(e);
        delete s;
        c->pa = nullptr;
    }
}

// The five match masks (A, C, G, T, N) of query rows 64 wi .. 64 wi + 63, built in registers
// from the packed query.  A masked row is the fifth symbol whatever code it carries: it is kept
// out of the A/C/G/T masks.  Rows past the query's end match nothing.
__device__ __forceinline__ void pd_masks(const Packed& pk, uint64_t qoff, uint32_t m, uint32_t wi,
                                         uint64_t (&peq)[5]) {
    const int64_t g0 = (int64_t)qoff + 64ll * wi;
    const uint32_t rows = min(64u, m - 64u * wi);
    uint32_t cw[4], nw[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) cw[k] = code32(pk, g0 + 16 * k);
#pragma unroll
    for (int k = 0; k < 2; ++k) nw[k] = mask32(pk, g0 + 32 * k);
    const uint64_t valid = rows >= 64u ? ~0ull : ((1ull << rows) - 1ull);
    const uint64_t nb = (((uint64_t)nw[1] << 32) | nw[0]) & valid;
    uint64_t lo = 0, hi = 0;   // bit i: low / high bit of row i's code
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t l = 0, h = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            l |= ((cw[k] >> (2 * i)) & 1u) << i;
            h |= ((cw[k] >> (2 * i + 1)) & 1u) << i;
        }
        lo |= (uint64_t)l << (16 * k);
        hi |= (uint64_t)h << (16 * k);
    }
    const uint64_t acgt = valid & ~nb;
    peq[0] = ~hi & ~lo & acgt;
    peq[1] = ~hi & lo & acgt;
    peq[2] = hi & ~lo & acgt;
    peq[3] = hi & lo & acgt;
    peq[4] = nb;
}

__global__ __launch_bounds__(64 * kPdWavesPerBlock) void pairdist_kernel(PdArgs A) {
    const uint32_t wave = blockIdx.x * kPdWavesPerBlock + (threadIdx.x >> 6);
    if (wave >= A.n_waves) return;   // whole waves leave: the shift below sees full waves
    const uint32_t lane = threadIdx.x & 63u;
    const PdWave W = A.waves[wave];
    const uint32_t G = W.G;
    const uint32_t g = lane / G, w = lane - g * G;
    bool active = g < W.count && (uint64_t)W.first + g < A.n_pairs;

    uint32_t m = 1, n = 1, rc = 0, cap = 0, has_cap = 0;
    uint64_t qoff = 0, toff = 0, soff = 0;
    if (active) {
        const PdPair P = A.pairs[W.first + g];
        if (DMX_BOUND(A.pk.bd, reads, P.q, kBufRead) && DMX_BOUND(A.pk.bd, reads, P.t, kBufRead)) {
            m = A.lens[P.q];
            n = A.lens[P.t];
            qoff = A.offs[P.q];
            toff = A.offs[P.t];
            rc = P.flags & DMX_PD_RC;
            has_cap = P.flags & 0x100u;
            cap = P.cap;
            soff = P.soff;
        } else {
            active = false;
        }
    }
    const uint32_t mw = (m + 63u) >> 6;          // words of the query
    const uint32_t S = (mw + G - 1u) / G;        // stripes
    const uint32_t L = n + G;                    // steps per stripe (n + G - 1, one to spare)

    uint64_t peq[5] = {0, 0, 0, 0, 0};
    uint64_t Pv = 0, Mv = 0;
    uint32_t s = 0, ts = 0, pass = 0, codes = 0, nbits = 0, wi = 0, hb = 63;
    bool last = false, live = false;
    int score = 0, best = 0;

    for (uint32_t step = 0; step < W.steps; ++step) {
        // lane w - 1's (delta + 1) | symbol << 2 of the column this lane takes now
        uint32_t recv = (uint32_t)__shfl_up((int)pass, 1);
        if (!active) continue;
        if (ts == 0) {   // a stripe starts: this lane's word, D(i, 0) = i
            wi = s * G + w;
            live = wi < mw;
            last = wi + 1u == mw;
            if (live) pd_masks(A.pk, qoff, m, wi, peq);
            Pv = ~0ull;
            Mv = 0ull;
            hb = last ? ((m - 1u) & 63u) : 63u;
            if (last) score = best = (int)m;
        }
        if (w == 0) {   // the group's first lane feeds the array: row 0's delta or the stripe
                        // above's, and the target symbol
            uint32_t sym = 0, hin1 = 1;
            if (ts < n) {
                if ((ts & 15u) == 0u) fetch16(A.pk, toff, n, rc, 0u, ts, codes, nbits);
                const uint32_t k = ts & 15u;
                sym = ((nbits >> k) & 1u) ? 4u : ((codes >> (2u * k)) & 3u);
                if (s == 0) {
                    hin1 = A.mode == DMX_PD_NW ? 2u : 1u;   // D(0, j) = j, or 0 in HW
                } else {
                    const uint64_t si = soff + ts;
                    hin1 = bchk(A.pk.bd, (int64_t)si, 0, (int64_t)A.scratch_bytes, kBufPd)
                               ? A.scratch[si] : 1u;
                }
            }
            recv = hin1 | (sym << 2);
        }
        const uint32_t j = ts - w;   // wraps above n for ts < w
        if (live && j < n) {
            const uint32_t sym = recv >> 2;
            const int hin = (int)(recv & 3u) - 1;
            uint64_t Eq = sym == 0 ? peq[0] : sym == 1 ? peq[1] : sym == 2 ? peq[2]
                        : sym == 3 ? peq[3] : peq[4];
            const uint64_t hneg = hin < 0 ? 1ull : 0ull, hpos = hin > 0 ? 1ull : 0ull;
            const uint64_t Xv = Eq | Mv;
            Eq |= hneg;
            const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
            uint64_t Ph = Mv | ~(Xh | Pv);
            uint64_t Mh = Pv & Xh;
            const int hout = (int)((Ph >> hb) & 1ull) - (int)((Mh >> hb) & 1ull);
            Ph = (Ph << 1) | hpos;
            Mh = (Mh << 1) | hneg;
            Pv = Mh | ~(Xv | Ph);
            Mv = Ph & Xv;
            pass = (uint32_t)(hout + 1) | (sym << 2);
            if (last) {
                score += hout;
                best = min(best, score);
            } else if (w + 1u == G) {   // the stripe's last row: kept for the stripe below
                const uint64_t si = soff + j;
                if (bchk(A.pk.bd, (int64_t)si, 0, (int64_t)A.scratch_bytes, kBufPd))
                    A.scratch[si] = (uint8_t)(hout + 1);
            }
        }
        if (++ts == L) {
            ts = 0;
            if (++s == S) {
                active = false;
                if (last) {
                    uint32_t d = (uint32_t)(A.mode == DMX_PD_NW ? score : best);
                    if (has_cap && d > cap) d = cap + 1u;
                    A.out[W.first + g] = d;
                }
            } else {
                __threadfence();   // the scratch row is read back by the group's first lane
            }
        }
    }
}

// dmx_pairalign's forward pass: pairdist_kernel's NW scheme (same groups, stripes, scratch row
// and target fetch), with every live lane also following D(r, j) of its word's last row
// r = min(64 (wi + 1), m) and leaving Pv, Mv and that score of every column in the pair's trace
// at [wi][j] (a lane writes consecutive entries over time).  out[2 k] = the distance.
__global__ __launch_bounds__(64 * kPdWavesPerBlock) void pairalign_kernel(PaArgs A) {
    const uint32_t wave = blockIdx.x * kPdWavesPerBlock + (threadIdx.x >> 6);
    if (wave >= A.n_waves) return;   // whole waves leave: the shift below sees full waves
    const uint32_t lane = threadIdx.x & 63u;
    const PdWave W = A.waves[wave];
    const uint32_t G = W.G;
    const uint32_t g = lane / G, w = lane - g * G;
    bool active = g < W.count && (uint64_t)W.first + g < A.n_pairs;

    uint32_t m = 1, n = 1, rc = 0;
    uint64_t qoff = 0, toff = 0, soff = 0, trace = 0;
    if (active) {
        const PaPair P = A.pairs[W.first + g];
        if (DMX_BOUND(A.pk.bd, reads, P.q, kBufRead) && DMX_BOUND(A.pk.bd, reads, P.t, kBufRead)) {
            m = A.lens[P.q];
            n = A.lens[P.t];
            qoff = A.offs[P.q];
            toff = A.offs[P.t];
            rc = P.flags & DMX_PD_RC;
            soff = P.soff;
            trace = P.toff;
        } else {
            active = false;
        }
    }
    const uint32_t mw = (m + 63u) >> 6;          // words of the query
    const uint32_t S = (mw + G - 1u) / G;        // stripes
    const uint32_t L = n + G;                    // steps per stripe (n + G - 1, one to spare)

    uint64_t peq[5] = {0, 0, 0, 0, 0};
    uint64_t Pv = 0, Mv = 0, tbase = 0;
    uint32_t s = 0, ts = 0, pass = 0, codes = 0, nbits = 0, wi = 0, hb = 63;
    bool last = false, live = false;
    int score = 0;

    for (uint32_t step = 0; step < W.steps; ++step) {
        uint32_t recv = (uint32_t)__shfl_up((int)pass, 1);
        if (!active) continue;
        if (ts == 0) {   // a stripe starts: this lane's word, D(i, 0) = i
            wi = s * G + w;
            live = wi < mw;
            last = wi + 1u == mw;
            if (live) pd_masks(A.pk, qoff, m, wi, peq);
            Pv = ~0ull;
            Mv = 0ull;
            const uint32_t r = min(m, 64u * (wi + 1u));   // the word's last row
            hb = (r - 1u) & 63u;
            score = (int)r;
            tbase = trace + (uint64_t)wi * n;
        }
        if (w == 0) {   // the group's first lane feeds the array (pairdist_kernel, NW)
            uint32_t sym = 0, hin1 = 1;
            if (ts < n) {
                if ((ts & 15u) == 0u) fetch16(A.pk, toff, n, rc, 0u, ts, codes, nbits);
                const uint32_t k = ts & 15u;
                sym = ((nbits >> k) & 1u) ? 4u : ((codes >> (2u * k)) & 3u);
                if (s == 0) {
                    hin1 = 2u;   // D(0, j) = j
                } else {
                    const uint64_t si = soff + ts;
                    hin1 = bchk(A.pk.bd, (int64_t)si, 0, (int64_t)A.scratch_bytes, kBufPd)
                               ? A.scratch[si] : 1u;
                }
            }
            recv = hin1 | (sym << 2);
        }
        const uint32_t j = ts - w;   // wraps above n for ts < w
        if (live && j < n) {
            const uint32_t sym = recv >> 2;
            const int hin = (int)(recv & 3u) - 1;
            uint64_t Eq = sym == 0 ? peq[0] : sym == 1 ? peq[1] : sym == 2 ? peq[2]
                        : sym == 3 ? peq[3] : peq[4];
            const uint64_t hneg = hin < 0 ? 1ull : 0ull, hpos = hin > 0 ? 1ull : 0ull;
            const uint64_t Xv = Eq | Mv;
            Eq |= hneg;
            const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
            uint64_t Ph = Mv | ~(Xh | Pv);
            uint64_t Mh = Pv & Xh;
            const int hout = (int)((Ph >> hb) & 1ull) - (int)((Mh >> hb) & 1ull);
            Ph = (Ph << 1) | hpos;
            Mh = (Mh << 1) | hneg;
            Pv = Mh | ~(Xv | Ph);
            Mv = Ph & Xv;
            pass = (uint32_t)(hout + 1) | (sym << 2);
            score += hout;
            const uint64_t ti = tbase + j;
            if (bchk(A.pk.bd, (int64_t)ti, 0, (int64_t)A.trace_steps, kBufPaTrace)) {
                A.pm[ti] = make_ulonglong2(Pv, Mv);
                A.sc[ti] = (uint16_t)score;
            }
            if (!last && w + 1u == G) {   // the stripe's last row: kept for the stripe below
                const uint64_t si = soff + j;
                if (bchk(A.pk.bd, (int64_t)si, 0, (int64_t)A.scratch_bytes, kBufPd))
                    A.scratch[si] = (uint8_t)(hout + 1);
            }
        }
        if (++ts == L) {
            ts = 0;
            if (++s == S) {
                active = false;
                if (last) A.out[2u * (W.first + g)] = (uint32_t)score;
            } else {
                __threadfence();   // the scratch row is read back by the group's first lane
            }
        }
    }
}

// dmx_pairalign's traceback: one lane per pair walks back from (m, n), preferring up (INSERT),
// then left (DELETE), then the diagonal (include/dmx.h).  Bit b of a word's Pv / Mv at column j
// is D(64 wi + b + 1, j) - D(64 wi + b, j) = +1 / -1, so "up" is one bit test, and D(i, j - 1) is
// the word's score at column j - 1 minus the vertical deltas of the rows below i.  Column j of
// the matrix is trace column j - 1; D(i, 0) = i needs no trace.  Op k goes to
// region[m + n - 1 - k]: the path ends up in forward order at the region's tail.
constexpr uint32_t kPaTbLanes = 64;
__global__ __launch_bounds__(kPaTbLanes) void pairalign_traceback_kernel(PaArgs A) {
    const uint32_t k = blockIdx.x * kPaTbLanes + threadIdx.x;
    if (k >= A.n_pairs) return;
    const PaPair P = A.pairs[k];
    if (!(DMX_BOUND(A.pk.bd, reads, P.q, kBufRead) && DMX_BOUND(A.pk.bd, reads, P.t, kBufRead)))
        return;
    const uint32_t m = A.lens[P.q], n = A.lens[P.t];
    uint32_t i = m, j = n, len = 0;
    int d = (int)A.out[2u * k];
    uint64_t pos = P.roff + m + n;
    while (i > 0 || j > 0) {
        uint32_t op;
        if (j == 0) {
            op = DMX_PA_INSERT;
            --i;
        } else if (i == 0) {
            op = DMX_PA_DELETE;
            --j;
        } else {
            const uint32_t wi = (i - 1u) >> 6, b = (i - 1u) & 63u;
            const uint64_t t1 = P.toff + (uint64_t)wi * n + (j - 1u);
            ulonglong2 c1 = make_ulonglong2(0, 0), c0 = make_ulonglong2(0, 0);
            uint32_t s0 = 0;
            if (bchk(A.pk.bd, (int64_t)t1, 0, (int64_t)A.trace_steps, kBufPaTrace)) c1 = A.pm[t1];
            if (j > 1u && bchk(A.pk.bd, (int64_t)t1 - 1, 0, (int64_t)A.trace_steps, kBufPaTrace)) {
                c0 = A.pm[t1 - 1u];
                s0 = A.sc[t1 - 1u];
            }
            if ((c1.x >> b) & 1ull) {   // D(i - 1, j) + 1 == D(i, j)
                op = DMX_PA_INSERT;
                --i;
                --d;
            } else {
                int dl, dd;   // D(i, j - 1), D(i - 1, j - 1)
                if (j == 1u) {
                    dl = (int)i;
                    dd = (int)i - 1;
                } else {
                    const uint32_t hb = (min(m, 64u * (wi + 1u)) - 1u) & 63u;
                    // rows i + 1 .. the word's last row: bits b + 1 .. hb
                    const uint64_t below = (hb == 63u ? ~0ull : ((1ull << (hb + 1u)) - 1ull)) &
                                           ~((2ull << b) - 1ull);
                    dl = (int)s0 - __popcll(c0.x & below) + __popcll(c0.y & below);
                    dd = dl - (int)((c0.x >> b) & 1ull) + (int)((c0.y >> b) & 1ull);
                }
                if (dl + 1 == d) {
                    op = DMX_PA_DELETE;
                    --j;
                    d = dl;
                } else {   // the diagonal: D(i, j) = D(i - 1, j - 1) + (symbols differ)
                    op = dd == d ? DMX_PA_MATCH : DMX_PA_MISMATCH;
                    --i;
                    --j;
                    d = dd;
                }
            }
        }
        --pos;
        if (bchk(A.pk.bd, (int64_t)pos, 0, (int64_t)A.ops_bytes, kBufPaOps)) A.ops[pos] = (uint8_t)op;
        ++len;
    }
    A.out[2u * k + 1u] = len;
}

}  // namespace dmx

using namespace dmx;

namespace {

#define PD_CK(call)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            c->err = std::string("dmx_pairdist: ") + #call + ": " + hipGetErrorString(e_);   \
            return DMX_E_HIP;                                                                \
        }                                                                                    \
    } while (0)

template <typename T>
hipError_t pd_realloc(T** p, size_t count) {
    if (*p) {
        hipFree(*p);
        *p = nullptr;
    }
    return hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T));
}

int pd_group_size(uint32_t m) {
    const uint32_t mw = std::min<uint32_t>((m + 63u) / 64u, 64u);
    for (int k = 0; k < kPdNSizes; ++k)
        if ((uint32_t)kPdSizes[k] >= mw) return kPdSizes[k];
    return 64;
}

// Arguments every form checks the same way.  0, or the code with *err set.
int pd_validate(int mode, const uint32_t* lens, size_t n_reads, const uint32_t* q,
                const uint32_t* t, const uint8_t* flags, size_t n_pairs, std::string* err) {
    if (mode != DMX_PD_NW && mode != DMX_PD_HW) {
        *err = "dmx_pairdist: mode must be DMX_PD_NW or DMX_PD_HW";
        return DMX_E_INVALID;
    }
    for (size_t i = 0; i < n_pairs; ++i) {
        if (q[i] >= n_reads || t[i] >= n_reads) {
            *err = "dmx_pairdist: pair " + std::to_string(i) + " names a read outside the batch";
            return DMX_E_INVALID;
        }
        if (flags && (flags[i] & ~DMX_PD_RC)) {
            *err = "dmx_pairdist: pair " + std::to_string(i) + " has an unknown flag";
            return DMX_E_INVALID;
        }
    }
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t m = lens[q[i]], n = lens[t[i]];
        if (m < 1 || n < 1 || m > DMX_PD_MAX_LEN || n > DMX_PD_MAX_LEN) {
            *err = "dmx_pairdist: pair " + std::to_string(i) + ": reads of 1.." +
                   std::to_string(DMX_PD_MAX_LEN) + " nt supported";
            return DMX_E_UNSUPPORTED;
        }
    }
    return DMX_OK;
}

// Symbols 0..3 = A/C/G/T, 4 = masked, of read `r` (reverse-complemented when rc).
void pd_decode(const uint32_t* seq2b, const uint32_t* nmask, uint64_t off, uint32_t n, bool rc,
               std::vector<uint8_t>& out) {
    out.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t x = off + i;
        const uint32_t code = (seq2b[x / 16] >> (2 * (x % 16))) & 3u;
        const uint32_t nb = (nmask[x / 32] >> (x % 32)) & 1u;
        const uint8_t sym = nb ? 4 : (uint8_t)(rc ? 3u - code : code);
        out[rc ? n - 1 - i : i] = sym;
    }
}

// Plain full-matrix DP, one row kept: D(i, j) over query rows i and target columns j.
uint32_t pd_dp(int mode, const std::vector<uint8_t>& a, const std::vector<uint8_t>& b,
               std::vector<uint32_t>& row) {
    const size_t m = a.size(), n = b.size();
    row.resize(n + 1);
    for (size_t j = 0; j <= n; ++j) row[j] = mode == DMX_PD_NW ? (uint32_t)j : 0u;
    for (size_t i = 1; i <= m; ++i) {
        uint32_t diag = row[0];
        row[0] = (uint32_t)i;
        const uint8_t ai = a[i - 1];
        for (size_t j = 1; j <= n; ++j) {
            const uint32_t up = row[j];
            const uint32_t sub = diag + (ai == b[j - 1] ? 0u : 1u);
            row[j] = std::min(sub, std::min(up, row[j - 1]) + 1u);
            diag = up;
        }
    }
    if (mode == DMX_PD_NW) return row[n];
    return *std::min_element(row.begin(), row.end());
}

}  // namespace

extern "C" int dmx_pairdist_group_sizes(int* out, int cap) {
    for (int k = 0; k < kPdNSizes && k < cap && out; ++k) out[k] = kPdSizes[k];
    return kPdNSizes;
}

extern "C" float dmx_pairdist_ms(dmx_ctx* c) { return c && c->pd ? c->pd->ms : 0.f; }

extern "C" int dmx_pairdist_host(int mode, const uint32_t* seq2b, const uint32_t* nmask,
                                 const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
                                 const uint32_t* q, const uint32_t* t, const uint8_t* flags,
                                 const uint32_t* caps, size_t n_pairs, uint32_t* out,
                                 int n_threads) {
    if (n_pairs && (!q || !t || !out || !seq2b || !nmask || !offsets || !lens)) return DMX_E_INVALID;
    std::string err;
    if (const int rc = pd_validate(mode, lens, n_reads, q, t, flags, n_pairs, &err)) {
        set_process_error(err);
        return rc;
    }
    const size_t nth = std::max<size_t>(1, std::min<size_t>((size_t)std::max(n_threads, 1),
                                                            std::max<size_t>(n_pairs, 1)));
    auto work = [&](size_t k) {
        std::vector<uint8_t> a, b;
        std::vector<uint32_t> row;
        for (size_t i = k; i < n_pairs; i += nth) {   // interleaved: similar work per thread
            pd_decode(seq2b, nmask, offsets[q[i]], lens[q[i]], false, a);
            pd_decode(seq2b, nmask, offsets[t[i]], lens[t[i]], flags && (flags[i] & DMX_PD_RC), b);
            uint32_t d = pd_dp(mode, a, b, row);
            if (caps && d > caps[i]) d = caps[i] + 1u;
            out[i] = d;
        }
    };
    if (nth == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (size_t k = 0; k < nth; ++k) th.emplace_back(work, k);
        for (auto& x : th) x.join();
    }
    return DMX_OK;
}

extern "C" int dmx_pairdist(dmx_ctx* c, int mode, const uint32_t* q, const uint32_t* t,
                            const uint8_t* flags, const uint32_t* caps, size_t n_pairs,
                            uint32_t* out) {
    if (!c) return DMX_E_INVALID;
    if (n_pairs && (!q || !t || !out)) {
        c->err = "dmx_pairdist: null pair list or output";
        return DMX_E_INVALID;
    }
    if (c->pd) c->pd->ms = 0.f;
    const size_t n_reads = c->d_seq ? c->n_reads : 0;
    // everything is validated on the host before anything is launched: the lengths come back
    // from the resident batch (a copy, no kernel)
    std::vector<uint32_t> lens(n_reads);
    if (n_reads && n_pairs) {
        PD_CK(hipSetDevice(c->device));
        PD_CK(hipMemcpy(lens.data(), c->d_lens, n_reads * 4, hipMemcpyDeviceToHost));
    }
    if (const int rc = pd_validate(mode, lens.data(), n_reads, q, t, flags, n_pairs, &c->err))
        return rc;
    if (!n_pairs) return DMX_OK;
    if (!c->pd) {
        c->pd = new PdState();
        for (auto& e : c->pd->ev) PD_CK(hipEventCreate(&e));
    }
    PdState* s = c->pd;
    hipStream_t st = c->stream;
    size_t chunk = kPdChunkDefault;
    if (const char* e = std::getenv("DMX_PD_CHUNK")) {
        const size_t v = (size_t)std::strtoull(e, nullptr, 10);
        if (v) chunk = v;
    }
    chunk = std::min<size_t>(chunk, 1u << 24);

    std::vector<uint64_t> keys;
    std::vector<PdPair> pairs;
    std::vector<PdWave> waves;
    std::vector<uint32_t> res;
    float total_ms = 0.f;
    for (size_t lo = 0; lo < n_pairs;) {
        // the chunk: up to `chunk` pairs, fewer when their scratch rows fill the bound
        size_t hi = lo, scratch = 0;
        keys.clear();
        while (hi < n_pairs && hi - lo < chunk) {
            const uint32_t m = lens[q[hi]], n = lens[t[hi]];
            const size_t need = m > 64u * 64u ? n : 0;
            if (hi > lo && scratch + need > kPdScratchMax) break;
            scratch += need;
            // sort key: group size, then target length (similar step counts share a wave),
            // longest first; the low bits are the pair's place in the chunk
            keys.push_back(((uint64_t)pd_group_size(m) << 48) | ((uint64_t)n << 24) |
                           (uint64_t)(hi - lo));
            ++hi;
        }
        const size_t np = hi - lo;
        std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
        pairs.resize(np);
        waves.clear();
        size_t soff = 0;
        for (size_t k = 0; k < np;) {
            const uint32_t G = (uint32_t)(keys[k] >> 48);
            const uint32_t per = 64u / G;
            PdWave W{(uint32_t)k, 0, G, 0};
            while (k < np && W.count < per && (uint32_t)(keys[k] >> 48) == G) {
                const size_t i = lo + (size_t)(keys[k] & 0xFFFFFFu);
                const uint32_t m = lens[q[i]], n = lens[t[i]];
                const uint32_t mw = (m + 63u) / 64u, S = (mw + G - 1u) / G;
                PdPair& P = pairs[k];
                P.q = q[i];
                P.t = t[i];
                P.cap = caps ? caps[i] : 0u;
                P.flags = (flags ? (flags[i] & DMX_PD_RC) : 0u) | (caps ? 0x100u : 0u);
                P.soff = soff;
                if (S > 1) soff += n;
                W.steps = std::max(W.steps, S * (n + G));
                ++W.count;
                ++k;
            }
            waves.push_back(W);
        }
        if (s->pair_cap < np || !s->d_pairs) {
            PD_CK(pd_realloc(&s->d_pairs, np));
            PD_CK(pd_realloc(&s->d_out, np));
            s->pair_cap = np;
        }
        if (s->wave_cap < waves.size() || !s->d_waves) {
            PD_CK(pd_realloc(&s->d_waves, waves.size()));
            s->wave_cap = waves.size();
        }
        if (s->scratch_cap < soff || !s->d_scratch) {
            PD_CK(pd_realloc(&s->d_scratch, soff));
            s->scratch_cap = std::max<size_t>(soff, 1);
        }
        PD_CK(hipMemcpyAsync(s->d_pairs, pairs.data(), np * sizeof(PdPair), hipMemcpyHostToDevice,
                             st));
        PD_CK(hipMemcpyAsync(s->d_waves, waves.data(), waves.size() * sizeof(PdWave),
                             hipMemcpyHostToDevice, st));
        PD_CK(bounds_reset(c, st));
        PdArgs A;
        A.pk.seq = c->d_seq;
        A.pk.nmask = c->d_nmask;
        A.pk.bd = make_bounds(c, kKerPairdist);
        A.offs = c->d_offs;
        A.lens = c->d_lens;
        A.pairs = s->d_pairs;
        A.waves = s->d_waves;
        A.n_waves = (uint32_t)waves.size();
        A.n_pairs = (uint32_t)np;
        A.mode = mode;
        A.scratch = s->d_scratch;
        A.scratch_bytes = s->scratch_cap;
        A.out = s->d_out;
        const uint32_t nb = (A.n_waves + kPdWavesPerBlock - 1u) / kPdWavesPerBlock;
        PD_CK(hipEventRecord(s->ev[0], st));
        hipLaunchKernelGGL(pairdist_kernel, dim3(nb), dim3(64 * kPdWavesPerBlock), 0, st, A);
        PD_CK(hipGetLastError());
        PD_CK(hipEventRecord(s->ev[1], st));
        res.resize(np);
        PD_CK(hipMemcpyAsync(res.data(), s->d_out, np * 4, hipMemcpyDeviceToHost, st));
        PD_CK(hipStreamSynchronize(st));
        if (const int brc = bounds_check(c, "dmx_pairdist")) return brc;
        float ms = 0.f;
        hipEventElapsedTime(&ms, s->ev[0], s->ev[1]);
        total_ms += ms;
        for (size_t k = 0; k < np; ++k) out[lo + (size_t)(keys[k] & 0xFFFFFFu)] = res[k];
        lo = hi;
    }
    s->ms = total_ms;
    return DMX_OK;
}

// ---- dmx_pairalign: the NW distance and the edit path (include/dmx.h) -----------

namespace {

#define PA_CK(call)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            c->err = std::string("dmx_pairalign: ") + #call + ": " + hipGetErrorString(e_);  \
            return DMX_E_HIP;                                                                \
        }                                                                                    \
    } while (0)

constexpr size_t kPaTraceEntry = sizeof(ulonglong2) + sizeof(uint16_t);   // bytes per word-step
constexpr size_t kPaTraceMbDefault = 1024;                                // DMX_PA_TRACE_MB

// pd_validate with dmx_pairalign's name in the message, and the room the paths may need.
int pa_validate(const uint32_t* lens, size_t n_reads, const uint32_t* q, const uint32_t* t,
                const uint8_t* flags, size_t n_pairs, size_t ops_cap, std::string* err) {
    if (const int rc = pd_validate(DMX_PD_NW, lens, n_reads, q, t, flags, n_pairs, err)) {
        if (err->rfind("dmx_pairdist", 0) == 0) err->replace(0, 12, "dmx_pairalign");
        return rc;
    }
    size_t need = 0;
    for (size_t i = 0; i < n_pairs; ++i) need += (size_t)lens[q[i]] + lens[t[i]];
    if (ops_cap < need) {
        *err = "dmx_pairalign: ops_cap " + std::to_string(ops_cap) + " is below the " +
               std::to_string(need) + " bytes the paths may take (sum of both lengths)";
        return DMX_E_INVALID;
    }
    return DMX_OK;
}

// The whole (m + 1) x (n + 1) matrix, then the walk back from (m, n) by the contract's rule:
// up (INSERT) before left (DELETE) before the diagonal.  The ops come out last first in `rev`.
uint32_t pa_dp_path(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b,
                    std::vector<uint16_t>& D, std::vector<uint8_t>& rev) {
    const size_t m = a.size(), n = b.size(), W = n + 1;
    D.resize((m + 1) * W);
    for (size_t j = 0; j <= n; ++j) D[j] = (uint16_t)j;
    for (size_t i = 1; i <= m; ++i) {
        uint16_t* row = &D[i * W];
        const uint16_t* up = row - W;
        row[0] = (uint16_t)i;
        const uint8_t ai = a[i - 1];
        for (size_t j = 1; j <= n; ++j) {
            const uint32_t sub = up[j - 1] + (ai == b[j - 1] ? 0u : 1u);
            row[j] = (uint16_t)std::min<uint32_t>(sub, std::min<uint32_t>(up[j], row[j - 1]) + 1u);
        }
    }
    rev.clear();
    size_t i = m, j = n;
    while (i > 0 || j > 0) {
        if (j == 0) {
            rev.push_back(DMX_PA_INSERT), --i;
        } else if (i == 0) {
            rev.push_back(DMX_PA_DELETE), --j;
        } else if (D[(i - 1) * W + j] + 1u == D[i * W + j]) {
            rev.push_back(DMX_PA_INSERT), --i;
        } else if (D[i * W + j - 1] + 1u == D[i * W + j]) {
            rev.push_back(DMX_PA_DELETE), --j;
        } else {
            rev.push_back(a[i - 1] == b[j - 1] ? DMX_PA_MATCH : DMX_PA_MISMATCH), --i, --j;
        }
    }
    return D[m * W + n];
}

}  // namespace

extern "C" float dmx_pairalign_ms(dmx_ctx* c) {
    return c && c->pa ? c->pa->ms[0] + c->pa->ms[1] : 0.f;
}

extern "C" int dmx_pairalign_stats(dmx_ctx* c, float* ms, int n_ms) {
    if (!c) return DMX_E_INVALID;
    for (int k = 0; k < n_ms && k < 2 && ms; ++k) ms[k] = c->pa ? c->pa->ms[k] : 0.f;
    return c->pa ? c->pa->launches : 0;
}

extern "C" int dmx_pairalign_host(const uint32_t* seq2b, const uint32_t* nmask,
                                  const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
                                  const uint32_t* q, const uint32_t* t, const uint8_t* flags,
                                  size_t n_pairs, uint32_t* dist, uint64_t* op_off, uint8_t* ops,
                                  size_t ops_cap, int n_threads) {
    if (!op_off || (n_pairs && (!q || !t || !dist || !ops || !seq2b || !nmask || !offsets || !lens))) {
        set_process_error("dmx_pairalign_host: null argument");
        return DMX_E_INVALID;
    }
    std::string err;
    if (const int rc = pa_validate(lens, n_reads, q, t, flags, n_pairs, ops_cap, &err)) {
        set_process_error(err);
        return rc;
    }
    // every pair's path first goes to the tail of its own (m + n)-byte region, so the threads
    // need not know each other's lengths; then the regions are closed up in place
    std::vector<uint64_t> roff(n_pairs + 1, 0);
    for (size_t i = 0; i < n_pairs; ++i) roff[i + 1] = roff[i] + lens[q[i]] + lens[t[i]];
    std::vector<uint32_t> plen(n_pairs, 0);
    const size_t nth = std::max<size_t>(1, std::min<size_t>((size_t)std::max(n_threads, 1),
                                                            std::max<size_t>(n_pairs, 1)));
    auto work = [&](size_t k) {
        std::vector<uint8_t> a, b, rev;
        std::vector<uint16_t> D;
        for (size_t i = k; i < n_pairs; i += nth) {
            pd_decode(seq2b, nmask, offsets[q[i]], lens[q[i]], false, a);
            pd_decode(seq2b, nmask, offsets[t[i]], lens[t[i]], flags && (flags[i] & DMX_PD_RC), b);
            dist[i] = pa_dp_path(a, b, D, rev);
            plen[i] = (uint32_t)rev.size();
            std::reverse_copy(rev.begin(), rev.end(), ops + roff[i + 1] - rev.size());
        }
    };
    if (nth == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (size_t k = 0; k < nth; ++k) th.emplace_back(work, k);
        for (auto& x : th) x.join();
    }
    uint64_t at = 0;
    for (size_t i = 0; i < n_pairs; ++i) {
        op_off[i] = at;
        std::memmove(ops + at, ops + roff[i + 1] - plen[i], plen[i]);
        at += plen[i];
    }
    op_off[n_pairs] = at;
    return DMX_OK;
}

extern "C" int dmx_pairalign(dmx_ctx* c, const uint32_t* q, const uint32_t* t, const uint8_t* flags,
                             size_t n_pairs, uint32_t* dist, uint64_t* op_off, uint8_t* ops,
                             size_t ops_cap) {
    if (!c) return DMX_E_INVALID;
    if (!op_off || (n_pairs && (!q || !t || !dist || !ops))) {
        c->err = "dmx_pairalign: null pair list or output";
        return DMX_E_INVALID;
    }
    if (c->pa) {
        c->pa->ms[0] = c->pa->ms[1] = 0.f;
        c->pa->launches = 0;
    }
    const size_t n_reads = c->d_seq ? c->n_reads : 0;
    // everything is validated on the host before anything is launched (dmx_pairdist)
    std::vector<uint32_t> lens(n_reads);
    if (n_reads && n_pairs) {
        PA_CK(hipSetDevice(c->device));
        PA_CK(hipMemcpy(lens.data(), c->d_lens, n_reads * 4, hipMemcpyDeviceToHost));
    }
    if (const int rc = pa_validate(lens.data(), n_reads, q, t, flags, n_pairs, ops_cap, &c->err))
        return rc;
    op_off[0] = 0;
    if (!n_pairs) return DMX_OK;
    if (!c->pa) {
        c->pa = new PaState();
        for (auto& e : c->pa->ev) PA_CK(hipEventCreate(&e));
    }
    PaState* s = c->pa;
    hipStream_t st = c->stream;
    size_t budget = kPaTraceMbDefault;
    if (const char* e = std::getenv("DMX_PA_TRACE_MB")) {
        const size_t v = (size_t)std::strtoull(e, nullptr, 10);
        if (v) budget = v;
    }
    budget = std::min<size_t>(budget, (size_t)1 << 20) << 20;   // bytes

    std::vector<uint64_t> keys;
    std::vector<PaPair> pairs;
    std::vector<PdWave> waves;
    std::vector<uint32_t> res, place;
    std::vector<uint8_t> region;
    float ms_fwd = 0.f, ms_tb = 0.f;
    uint64_t at = 0;   // bytes of `ops` filled
    for (size_t lo = 0; lo < n_pairs;) {
        // the chunk: pairs while their traces fit the budget and their scratch rows the bound,
        // one pair at least
        size_t hi = lo, scratch = 0, trace = 0;
        keys.clear();
        while (hi < n_pairs && hi - lo < kPdChunkDefault) {
            const uint32_t m = lens[q[hi]], n = lens[t[hi]];
            const size_t need = m > 64u * 64u ? n : 0;
            const size_t steps = (size_t)((m + 63u) / 64u) * n;
            if (hi > lo && (scratch + need > kPdScratchMax ||
                            (trace + steps) * kPaTraceEntry > budget))
                break;
            scratch += need;
            trace += steps;
            keys.push_back(((uint64_t)pd_group_size(m) << 48) | ((uint64_t)n << 24) |
                           (uint64_t)(hi - lo));
            ++hi;
        }
        const size_t np = hi - lo;
        std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
        pairs.resize(np);
        waves.clear();
        size_t soff = 0, toff = 0, roff = 0;
        for (size_t k = 0; k < np;) {
            const uint32_t G = (uint32_t)(keys[k] >> 48);
            const uint32_t per = 64u / G;
            PdWave W{(uint32_t)k, 0, G, 0};
            while (k < np && W.count < per && (uint32_t)(keys[k] >> 48) == G) {
                const size_t i = lo + (size_t)(keys[k] & 0xFFFFFFu);
                const uint32_t m = lens[q[i]], n = lens[t[i]];
                const uint32_t mw = (m + 63u) / 64u, S = (mw + G - 1u) / G;
                PaPair& P = pairs[k];
                P.q = q[i];
                P.t = t[i];
                P.flags = flags ? (flags[i] & DMX_PD_RC) : 0u;
                P.pad = 0;
                P.soff = soff;
                P.toff = toff;
                P.roff = roff;
                if (S > 1) soff += n;
                toff += (size_t)mw * n;
                roff += (size_t)m + n;
                W.steps = std::max(W.steps, S * (n + G));
                ++W.count;
                ++k;
            }
            waves.push_back(W);
        }
        if (s->pair_cap < np || !s->d_pairs) {
            PA_CK(pd_realloc(&s->d_pairs, np));
            PA_CK(pd_realloc(&s->d_out, 2 * np));
            s->pair_cap = np;
        }
        if (s->wave_cap < waves.size() || !s->d_waves) {
            PA_CK(pd_realloc(&s->d_waves, waves.size()));
            s->wave_cap = waves.size();
        }
        if (s->scratch_cap < soff || !s->d_scratch) {
            PA_CK(pd_realloc(&s->d_scratch, soff));
            s->scratch_cap = std::max<size_t>(soff, 1);
        }
        if (s->trace_cap < toff || !s->d_pm) {
            PA_CK(pd_realloc(&s->d_pm, toff));
            PA_CK(pd_realloc(&s->d_sc, toff));
            s->trace_cap = std::max<size_t>(toff, 1);
        }
        if (s->ops_cap < roff || !s->d_ops) {
            PA_CK(pd_realloc(&s->d_ops, roff));
            s->ops_cap = std::max<size_t>(roff, 1);
        }
        PA_CK(hipMemcpyAsync(s->d_pairs, pairs.data(), np * sizeof(PaPair), hipMemcpyHostToDevice,
                             st));
        PA_CK(hipMemcpyAsync(s->d_waves, waves.data(), waves.size() * sizeof(PdWave),
                             hipMemcpyHostToDevice, st));
        PA_CK(bounds_reset(c, st));
        PaArgs A;
        A.pk.seq = c->d_seq;
        A.pk.nmask = c->d_nmask;
        A.pk.bd = make_bounds(c, kKerPairalign);
        A.offs = c->d_offs;
        A.lens = c->d_lens;
        A.pairs = s->d_pairs;
        A.waves = s->d_waves;
        A.n_waves = (uint32_t)waves.size();
        A.n_pairs = (uint32_t)np;
        A.scratch = s->d_scratch;
        A.scratch_bytes = s->scratch_cap;
        A.pm = s->d_pm;
        A.sc = s->d_sc;
        A.trace_steps = s->trace_cap;
        A.ops = s->d_ops;
        A.ops_bytes = s->ops_cap;
        A.out = s->d_out;
        const uint32_t nb = (A.n_waves + kPdWavesPerBlock - 1u) / kPdWavesPerBlock;
        PA_CK(hipEventRecord(s->ev[0], st));
        hipLaunchKernelGGL(pairalign_kernel, dim3(nb), dim3(64 * kPdWavesPerBlock), 0, st, A);
        PA_CK(hipGetLastError());
        PA_CK(hipEventRecord(s->ev[1], st));
        set_kid(A.pk.bd, kKerPairalignTb);
        hipLaunchKernelGGL(pairalign_traceback_kernel, dim3((A.n_pairs + kPaTbLanes - 1u) / kPaTbLanes),
                           dim3(kPaTbLanes), 0, st, A);
        PA_CK(hipGetLastError());
        PA_CK(hipEventRecord(s->ev[2], st));
        res.resize(2 * np);
        region.resize(roff);
        PA_CK(hipMemcpyAsync(res.data(), s->d_out, 2 * np * 4, hipMemcpyDeviceToHost, st));
        PA_CK(hipMemcpyAsync(region.data(), s->d_ops, roff, hipMemcpyDeviceToHost, st));
        PA_CK(hipStreamSynchronize(st));
        if (const int brc = bounds_check(c, "dmx_pairalign")) return brc;
        float ms = 0.f;
        hipEventElapsedTime(&ms, s->ev[0], s->ev[1]);
        ms_fwd += ms;
        hipEventElapsedTime(&ms, s->ev[1], s->ev[2]);
        ms_tb += ms;
        ++s->launches;
        // the chunk's paths in the caller's pair order: pair lo + x ran at sorted place[x]
        place.resize(np);
        for (size_t k = 0; k < np; ++k) place[(size_t)(keys[k] & 0xFFFFFFu)] = (uint32_t)k;
        for (size_t x = 0; x < np; ++x) {
            const size_t k = place[x];
            const uint32_t m = lens[q[lo + x]], n = lens[t[lo + x]];
            const uint32_t len = res[2 * k + 1];
            if (len > m + n || len < std::max(m, n)) {
                c->err = "dmx_pairalign: pair " + std::to_string(lo + x) + ": path of " +
                         std::to_string(len) + " ops for reads of " + std::to_string(m) + " and " +
                         std::to_string(n) + " nt";
                return DMX_E_STATE;
            }
            dist[lo + x] = res[2 * k];
            op_off[lo + x] = at;
            std::memcpy(ops + at, region.data() + pairs[k].roff + (m + n - len), len);
            at += len;
        }
        lo = hi;
    }
    op_off[n_pairs] = at;
    s->ms[0] = ms_fwd;
    s->ms[1] = ms_tb;
    return DMX_OK;
}
