// dmx_ends.hip — the end-window stage: cutadapt 4.9's four restricted adapter
// types, whose matches touch one end of the read view,
//   ^ADAPTER  PrefixAdapter            flags QUERY_STOP                 (kEndPrefix)
//   XADAPTER  NonInternalFrontAdapter  flags REF_START | QUERY_STOP     (kEndFrontX)
//   ADAPTER$  SuffixAdapter            flags QUERY_START                (kEndSuffix)
//   ADAPTERX  NonInternalBackAdapter   flags QUERY_START | REF_END      (kEndBackX)
// (adapters.py; Aligner.locate of _align.pyx as restated in oracle/cutadapt_oracle.c).  Without
// QUERY_START locate stops at column max_n = min(n, m + k); without QUERY_STOP it starts at column
// min_n = max(0, n - m - k): the DP of a restricted adapter lives in the first or the last m + k
// columns of the view, with locate's own boundary column.  Per (view, orientation, restricted
// adapter):
//   1. a Myers bit-vector pass over that window with the type's boundary conditions gives the exact
//      unit cost of every end cell locate would test; the triple goes on only if one of them is
//      within its acceptance limit (most triples stop here);
//   2. the survivors are queued in LDS and run cutadapt's DP column by column (cost, score and
//      origin with locate's tie rules, §3.5), the column held in LDS, lanes side by side;
//   3. an accepted best cell goes into the view's winner slot with the internal pipeline's key.
// Also here: the host twin dmx_ends_host (a full-matrix DP for every adapter type).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "dmx_internal.h"

namespace dmx {

namespace {

constexpr int kEndsBlock = 128;
constexpr int kEndsGrid = 256 * 8;
constexpr int kEndsRows = kMaxLen + 1;

struct EndsArgs {
    Packed pk;
    const uint64_t* offs;
    const uint32_t* lens;
    const ItemView* items;        // round 1: the views round 0 left; round 0: the view list of a
                                  // view run, else nullptr (whole reads)
    const uint32_t* n_items_dev;  // device count of items (with items)
    uint32_t n_items;             // host count / upper bound
    const DevEnds* E;
    unsigned long long* winner;
    int32_t* origin;              // ring rounds: per slot
    int32_t oslot;                // one winner slot per (item, orientation)
    int32_t okey;                 // band round: the key carries its origin (make_key_o)
    uint32_t* flags;              // d_counters + 3
    uint32_t* n_dp;               // exact DPs run
    uint32_t* n_seen;             // triples whose view holds min_overlap columns
};

// fetch16 (dmx_device.h) under the stage's own buffer ids
__device__ __forceinline__ void fetch16e(const Packed& pk, uint64_t off, uint32_t n,
                                         uint32_t strand, uint32_t start, uint32_t p,
                                         uint32_t& codes, uint32_t& nbits) {
    if (strand == 0) {
        const int64_t g = (int64_t)off + start + p;
        codes = window32(pk.seq, 2 * g, pk.bd, kBufEndsSeq);
        nbits = window32(pk.nmask, g, pk.bd, kBufEndsMask) & 0xFFFFu;
    } else {
        const int64_t b = (int64_t)off + (int64_t)n - 1 - start - (int64_t)p - 15;
        codes = ~rev_pairs(window32(pk.seq, 2 * b, pk.bd, kBufEndsSeq));
        nbits = __brev(window32(pk.nmask, b, pk.bd, kBufEndsMask)) >> 16;
    }
}

struct EndView {
    uint64_t off;
    uint32_t n, strand, start, len;
    bool ok;
};

// The oriented view of (item, o): task_view's rules (dmx_kernels.hip).
__device__ __forceinline__ EndView end_view(const EndsArgs& A, uint32_t item, int o) {
    EndView v{kMinOffset, 0, 0, 0, 0, false};
    uint32_t read = item;
    if (A.items) {
        if (!DMX_BOUND(A.pk.bd, items, item, kBufEndsItem)) return v;
        const ItemView iv = A.items[item];
        read = iv.read;
        v.start = iv.start;
        v.len = iv.len;
        v.strand = iv.strand;
    }
    if (!DMX_BOUND(A.pk.bd, reads, read, kBufEndsRead)) return v;
    v.n = A.lens[read];
    v.off = A.offs[read];
    if (!A.items) v.len = v.n;
    if (o) {
        v.start = v.n - v.start - v.len;
        v.strand ^= 1u;
    }
    v.ok = true;
    return v;
}

// The window of view columns a type's DP covers: columns j0 + 1 .. j1 after boundary column j0.
__device__ __forceinline__ void end_window(int type, int m, int k, uint32_t len, uint32_t& j0,
                                           uint32_t& j1) {
    const uint32_t w = (uint32_t)(m + k);
    if (type <= kEndFrontX) {
        j0 = 0;
        j1 = len < w ? len : w;
    } else {
        j0 = len > w ? len - w : 0u;
        j1 = len;
    }
}

// One Myers / Hyyro column step with the row-0 horizontal delta `hin` (0: free start in the read,
// 1: D(0, j) = j).  Plain 64-bit form: this pass is a small part of a small stage.
__device__ __forceinline__ void myers_col(uint64_t eq, uint64_t& pv, uint64_t& mv, uint64_t hin) {
    const uint64_t xv = eq | mv;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    ph = (ph << 1) | hin;
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}

// Step 1: can locate accept any end cell of this triple?  Exact unit costs, so a necessary and
// (up to the aligned length, which only the DP knows for kEndFrontX) sufficient test.
__device__ __forceinline__ bool ends_prefilter(const EndsArgs& A, const EndView& v, int type, int m,
                                               const uint64_t* peq, const int8_t* acc,
                                               const int8_t* pacc, uint32_t j0, uint32_t j1) {
    const bool front = type <= kEndFrontX;
    const uint64_t full = m >= 64 ? ~0ull : ((1ull << m) - 1ull);
    uint64_t pv = type == kEndFrontX ? 0ull : ~0ull, mv = 0ull;   // D(i, j0) = 0 / i
    const uint64_t hin = front ? 1ull : 0ull;
    // an empty view: locate still tests cell (m, 0), whose cost is m (kEndFrontX: length 0)
    bool hit = front && j1 == 0 && type == kEndPrefix && m <= (int)acc[m];
    for (uint32_t p = j0; p < j1; p += 16) {
        uint32_t codes, nb;
        fetch16e(A.pk, v.off, v.n, v.strand, v.start, p, codes, nb);
        const uint32_t cnt = min(16u, j1 - p);
        for (uint32_t x = 0; x < cnt; ++x) {
            const uint32_t c = (codes >> (2 * x)) & 3u;
            const uint64_t eq = ((nb >> x) & 1u) ? 0ull : peq[c];
            myers_col(eq, pv, mv, hin);
            if (front) {   // last-row cell (m, j), j = p + x + 1
                const int j = (int)(p + x + 1);
                const int d = j + __popcll(pv & full) - __popcll(mv & full);
                const int L = min(m, j + d);
                hit |= type == kEndPrefix ? d <= (int)acc[m] : d <= (int)pacc[L];
            }
        }
    }
    if (front) return hit;
    if (type == kEndSuffix)
        return __popcll(pv & full) - __popcll(mv & full) <= (int)acc[m];
    int d = 0;   // kEndBackX: cells (i, n), aligned length i
    for (int i = 1; i <= m; ++i) {
        d += (int)((pv >> (i - 1)) & 1ull) - (int)((mv >> (i - 1)) & 1ull);
        hit |= d <= (int)acc[i];
    }
    return hit;
}

// A DP cell in one LDS word: cost (8 bits), origin relative to the boundary column + 128 (8),
// score (16, signed).  cost <= m + m + k < 256; the relative origin lies in [-m, m + k].
struct Cell {
    int cost, origin, score;
};
__device__ __forceinline__ uint32_t cell_pack(const Cell& c) {
    return (uint32_t)(c.cost & 255) | ((uint32_t)((c.origin + 128) & 255) << 8) |
           ((uint32_t)(uint16_t)(int16_t)c.score << 16);
}
__device__ __forceinline__ Cell cell_unpack(uint32_t w) {
    return Cell{(int)(w & 255u), (int)((w >> 8) & 255u) - 128, (int)(int16_t)(w >> 16)};
}

struct EndBest {
    int score, cost, origin, iend;   // origin relative to j0
    uint32_t j;
    bool any;
};

__device__ __forceinline__ void end_offer(EndBest& b, const Cell& c, int iend, uint32_t j,
                                          int j0, const int8_t* acc) {
    const int oabs = c.origin + j0;
    const int length = iend + (oabs < 0 ? oabs : 0);
    if (length < 0 || c.cost > (int)acc[length]) return;
    if (!b.any || c.score > b.score || (c.score == b.score && c.cost < b.cost)) {
        b = EndBest{c.score, c.cost, c.origin, iend, j, true};
    }
}

// Step 2: locate's DP over the window, one column in LDS (col[i * kEndsBlock], this lane's word of
// row i), full columns (no Ukkonen cut-off: the cells it would leave stale cost more than k and
// never reach an accepted cell, §3.5).
__device__ __forceinline__ EndBest ends_dp(const EndsArgs& A, const EndView& v, int type, int m,
                                           const uint64_t* peq, const int8_t* acc, uint32_t j0,
                                           uint32_t j1, uint32_t* col) {
    const bool front = type <= kEndFrontX;
    for (int i = 0; i <= m; ++i) {
        Cell c;
        if (type == kEndFrontX) c = Cell{0, -i, 0};
        else if (type == kEndPrefix) c = Cell{i, 0, -2 * i};
        else c = Cell{i, max(0, (int)j0 - i) - (int)j0, -2 * i};
        col[i * kEndsBlock] = cell_pack(c);
    }
    EndBest best{0, 0, 0, 0, 0, false};
    for (uint32_t p = j0; p < j1; p += 16) {
        uint32_t codes, nb;
        fetch16e(A.pk, v.off, v.n, v.strand, v.start, p, codes, nb);
        const uint32_t cnt = min(16u, j1 - p);
        for (uint32_t x = 0; x < cnt; ++x) {
            const uint32_t j = p + x + 1;
            const uint32_t c = (codes >> (2 * x)) & 3u;
            const uint64_t eq = ((nb >> x) & 1u) ? 0ull : peq[c];
            Cell diag = cell_unpack(col[0]);
            Cell prev = diag;
            if (front) {
                prev.cost = (int)j;
                prev.score = -2 * (int)j;
            } else {
                prev.origin = (int)(j - j0);
            }
            col[0] = cell_pack(prev);
            for (int i = 1; i <= m; ++i) {
                const Cell cur = cell_unpack(col[i * kEndsBlock]);
                Cell nw;
                if ((eq >> (i - 1)) & 1ull) {
                    nw = Cell{diag.cost, diag.origin, diag.score + 1};
                } else {
                    const int cd = diag.cost + 1, cdel = cur.cost + 1, cins = prev.cost + 1;
                    if (cd <= cdel && cd <= cins) nw = Cell{cd, diag.origin, diag.score - 1};
                    else if (cins <= cdel) nw = Cell{cins, prev.origin, prev.score - 2};
                    else nw = Cell{cdel, cur.origin, cur.score - 2};
                }
                diag = cur;
                prev = nw;
                col[i * kEndsBlock] = cell_pack(nw);
            }
            if (front) end_offer(best, prev, m, j, 0, acc);   // prev = cell (m, j)
        }
    }
    if (front && j1 == 0) {   // locate's last-column test of an empty view: cell (m, 0)
        end_offer(best, cell_unpack(col[m * kEndsBlock]), m, 0, 0, acc);
    }
    if (!front) {
        for (int i = type == kEndBackX ? 0 : m; i <= m; ++i)
            end_offer(best, cell_unpack(col[i * kEndsBlock]), i, j1, (int)j0, acc);
    }
    return best;
}

// PHASE 0: offer the keys.  PHASE 1 (ring rounds, after phase 0 has drained): the triple whose key
// won its slot writes the origin, as select_kernel does for the internal pipeline.
template <int PHASE>
__global__ __launch_bounds__(kEndsBlock) void ends_kernel(EndsArgs A) {
    __shared__ uint64_t s_peq[4 * kMaxAdapters];
    __shared__ int8_t s_acc[72 * kMaxAdapters];
    __shared__ int8_t s_pacc[72 * kMaxAdapters];
    __shared__ uint32_t s_meta[kMaxAdapters];       // m | k << 8 | type << 16 | orig << 24
    __shared__ uint32_t s_col[kEndsRows * kEndsBlock];
    __shared__ uint32_t s_qi[2 * kEndsBlock], s_qs[2 * kEndsBlock];   // queued (item, sub)
    __shared__ uint32_t s_nq, s_ndp, s_nseen;
    const DevEnds* E = A.E;
    const int nE = E->n, T = nE * E->n_orient;
    for (int x = threadIdx.x; x < nE; x += kEndsBlock) {
        const EndAdapter& e = E->ad[x];
        s_meta[x] = (uint32_t)e.m | ((uint32_t)e.k << 8) | ((uint32_t)e.type << 16) |
                    ((uint32_t)e.orig << 24);
    }
    for (int x = threadIdx.x; x < 4 * nE; x += kEndsBlock) s_peq[x] = E->ad[x >> 2].peq[x & 3];
    for (int x = threadIdx.x; x < 72 * nE; x += kEndsBlock) {
        s_acc[x] = E->ad[x / 72].acc[x % 72];
        s_pacc[x] = E->ad[x / 72].pacc[x % 72];
    }
    if (threadIdx.x == 0) s_nq = s_ndp = s_nseen = 0;
    __syncthreads();
    const uint32_t n_items = A.items ? min(*A.n_items_dev, A.n_items) : A.n_items;
    const uint64_t total = (uint64_t)n_items * (uint64_t)T;

    // the exact DP of the top `cnt` (<= kEndsBlock) queued triples (block-uniform call)
    auto dp_pass = [&](uint32_t cnt) {
        const uint32_t lo = s_nq - cnt;
        __syncthreads();
        if (threadIdx.x < cnt) {
            const uint32_t item = s_qi[lo + threadIdx.x];
            const int sub = (int)s_qs[lo + threadIdx.x];
            const int o = sub / nE, e = sub % nE;
            const uint32_t mt = s_meta[e];
            const int m = (int)(mt & 255u), k = (int)((mt >> 8) & 255u);
            const int type = (int)((mt >> 16) & 255u), orig = (int)(mt >> 24);
            const EndView v = end_view(A, item, o);
            uint32_t j0, j1;
            end_window(type, m, k, v.len, j0, j1);
            const EndBest b = ends_dp(A, v, type, m, s_peq + 4 * e, s_acc + 72 * e, j0, j1,
                                      s_col + threadIdx.x);
            const uint32_t slot = A.oslot ? 2u * item + (uint32_t)o : item;
            if (b.any && DMX_BOUND(A.pk.bd, slots, slot, kBufEndsSlot)) {
                const int origin = b.origin + (int)j0;
                // last-row cells by their column, last-column cells after them by their row
                const uint64_t t = type <= kEndFrontX ? (uint64_t)b.j
                                                      : (uint64_t)v.len + 1 + (uint64_t)b.iend;
                const int delta = origin - ((int)b.j - b.iend);
                uint64_t key;
                if (A.okey) {
                    // the path leaves its end cell's diagonal by at most its cost <= kk <= 7
                    if (abs(delta) > kBandMaxCost || b.cost > kBandMaxCost) atomicOr(A.flags, 2u);
                    key = make_key_o(b.score, o, b.cost, orig, t, delta);
                } else {
                    key = make_key(b.score, o, b.cost, orig, t);
                }
                if (PHASE == 0) atomicMin(&A.winner[slot], (unsigned long long)key);
                else if (A.winner[slot] == key) A.origin[slot] = origin;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            s_nq = lo;
            s_ndp += cnt;
        }
        __syncthreads();
    };

    for (uint64_t base = (uint64_t)blockIdx.x * kEndsBlock; base < total;
         base += (uint64_t)gridDim.x * kEndsBlock) {
        const uint64_t ti = base + threadIdx.x;
        if (ti < total) {
            const uint32_t item = (uint32_t)(ti / (uint32_t)T);
            const int sub = (int)(ti % (uint32_t)T);
            const int o = sub / nE, e = sub % nE;
            const uint32_t mt = s_meta[e];
            const int m = (int)(mt & 255u), k = (int)((mt >> 8) & 255u);
            const int type = (int)((mt >> 16) & 255u);
            const EndView v = end_view(A, item, o);
            // An alignment over L adapter characters takes at least L - len edits in a view of
            // len columns: a view too short for every accepted length holds no match (with
            // -e 0.1 that is every view below min_overlap; absolute -e values admit shorter ones)
            bool room = false;
            for (int L = 0; L <= m && !room; ++L)
                room = (int)s_acc[72 * e + L] >= max(0, L - (int)min(v.len, 64u));
            if (v.ok && room) {
                atomicAdd(&s_nseen, 1u);
                uint32_t j0, j1;
                end_window(type, m, k, v.len, j0, j1);
                if (ends_prefilter(A, v, type, m, s_peq + 4 * e, s_acc + 72 * e, s_pacc + 72 * e,
                                   j0, j1)) {
                    const uint32_t q = atomicAdd(&s_nq, 1u);
                    s_qi[q] = item;
                    s_qs[q] = (uint32_t)sub;
                }
            }
        }
        __syncthreads();
        if (s_nq >= (uint32_t)kEndsBlock) dp_pass(kEndsBlock);   // the queue ends below a block
        __syncthreads();
    }
    if (s_nq) dp_pass(s_nq);
    if (PHASE == 0 && threadIdx.x == 0) {
        if (s_ndp) atomicAdd(A.n_dp, s_ndp);
        if (s_nseen) atomicAdd(A.n_seen, s_nseen);
    }
}

// The internal pipeline numbered the unrestricted adapters by their place in the sub-panel; the
// winner slots meet the restricted adapters' keys under the whole panel's numbering.  The map is
// increasing, so the order of the keys already in a slot does not change.
__global__ void ends_remap_kernel(EndsArgs A) {
    const uint32_t n_items = A.items ? min(*A.n_items_dev, A.n_items) : A.n_items;
    const uint64_t slots = (uint64_t)n_items * (A.oslot ? 2u : 1u);
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots;
         s += (uint64_t)gridDim.x * blockDim.x) {
        if (!DMX_BOUND(A.pk.bd, slots, s, kBufEndsSlot)) continue;
        const uint64_t key = A.winner[s];
        if (key == ~0ull) continue;
        const uint64_t a = A.E->remap[key_adapter(key) & (kMaxAdapters - 1)];
        A.winner[s] = (key & ~(255ull << 40)) | (a << 40);
    }
}

}  // namespace

int launch_ends(Ctx* c, int round, hipStream_t st) {
    EndsArgs A;
    A.pk.seq = c->d_seq;
    A.pk.nmask = c->d_nmask;
    A.pk.bd = make_bounds(c, kKerEnds);
    A.offs = c->in.offs.p;
    A.lens = c->in.lens.p;
    if (round == 0 && c->views_on) {   // a view run: round 0's items like round 1's
        A.items = c->d_views.p;
        A.n_items_dev = c->d_view_n.p;
        A.n_items = (uint32_t)c->n_views;
#ifdef DMX_DEBUG_BOUNDS
        A.pk.bd.items = c->d_views.cap;
#endif
    } else if (round == 0) {
        A.items = nullptr;
        A.n_items_dev = nullptr;
        A.n_items = (uint32_t)c->n_reads;
    } else {
        A.items = c->d_items.p;
        A.n_items_dev = c->d_counters.p + kCntItems;
        A.n_items = (uint32_t)c->item_cap;
    }
    A.E = c->d_ends[round].p;
    A.winner = c->d_winner[round].p;
    A.origin = c->d_origin[round].p;
    A.oslot = c->orient_slot[round] ? 1 : 0;
    A.okey = band_round(c, round) ? 1 : 0;
    A.flags = c->d_counters.p + kCntFlags;
    A.n_dp = c->d_counters.p + kCntEndsDp + round;
    A.n_seen = c->d_counters.p + kCntEndsSeen + round;
    hipEventRecord(c->ev[ev_of(kEvEndsIn, round)], st);
    if (A.n_items) {
        if (c->ends_remap[round] && c->panel[round].n > 0) {
            set_kid(A.pk.bd, kKerEndsRemap);
            const uint32_t g = std::min<uint32_t>((A.n_items + 255u) / 256u, 2048u);
            hipLaunchKernelGGL(ends_remap_kernel, dim3(g), dim3(256), 0, st, A);
        }
        const uint64_t total = (uint64_t)A.n_items * (uint64_t)c->ends_n[round] *
                               (uint64_t)c->panel[round].n_orient;
        const uint32_t grid =
            (uint32_t)std::min<uint64_t>((total + kEndsBlock - 1) / kEndsBlock, kEndsGrid);
        set_kid(A.pk.bd, kKerEnds);
        hipLaunchKernelGGL(ends_kernel<0>, dim3(grid), dim3(kEndsBlock), 0, st, A);
        if (!A.okey) {
            set_kid(A.pk.bd, kKerEndsOrigin);
            hipLaunchKernelGGL(ends_kernel<1>, dim3(grid), dim3(kEndsBlock), 0, st, A);
        }
    }
    hipEventRecord(c->ev[ev_of(kEvEndsOut, round)], st);
    return hipGetLastError() == hipSuccess ? DMX_OK : DMX_E_HIP;
}

// ---------------------------------------------------------------------------------------------
// Host twin: Aligner.locate by a full matrix, best_match, ReverseComplementer.
// ---------------------------------------------------------------------------------------------
namespace {

uint8_t host_iupac(char ch) {
    switch (ch) {
        case 'A': return 1;
        case 'C': return 2;
        case 'G': return 4;
        case 'T': return 8;
        case 'R': return 5;
        case 'Y': return 10;
        case 'S': return 6;
        case 'W': return 9;
        case 'K': return 12;
        case 'M': return 3;
        case 'B': return 14;
        case 'D': return 13;
        case 'H': return 11;
        case 'V': return 7;
        case 'N': return 15;
        default: return 0;
    }
}

struct HostAdapter {
    std::vector<uint8_t> mask;   // IUPAC mask per character
    std::vector<int> ncount;     // N's in the first i characters
    int m = 0, min_overlap = 0, eff_len = 0;
    bool wild = false, front = false;
    bool start_in_ref = false, start_in_query = false, stop_in_ref = false, stop_in_query = false;
    double rate = 0.0;
};

struct HostMatch {
    bool any = false;
    int astart = 0, astop = 0, rstart = 0, rstop = 0, score = 0, errors = 0;
};

struct HCell {
    int cost, score, origin;
};

// Aligner.locate on view codes q[0 .. n) (0..3 = A, C, G, T; 4 = matches nothing): every column
// of locate's range kept, every row computed.
HostMatch host_locate(const HostAdapter& ad, const std::vector<uint8_t>& q) {
    const int m = ad.m, n = (int)q.size();
    const int k = (int)(ad.rate * m);
    int max_n = n, min_n = 0;
    if (!ad.start_in_query) max_n = std::min(n, m + k);
    if (!ad.stop_in_query) min_n = std::max(0, n - m - k);
    const int cols = max_n - min_n + 1;
    std::vector<HCell> M((size_t)(m + 1) * (size_t)cols);
    auto at = [&](int i, int j) -> HCell& { return M[(size_t)i * cols + (size_t)(j - min_n)]; };
    for (int i = 0; i <= m; ++i) {
        HCell& c = at(i, min_n);
        if (!ad.start_in_ref && !ad.start_in_query) c = HCell{std::max(i, min_n), -2 * std::max(i, min_n), 0};
        else if (ad.start_in_ref && !ad.start_in_query) c = HCell{min_n, 0, std::min(0, min_n - i)};
        else if (!ad.start_in_ref && ad.start_in_query) c = HCell{i, -2 * i, std::max(0, min_n - i)};
        else c = HCell{std::min(i, min_n), 0, min_n - i};
    }
    auto acceptable = [&](const HCell& c, int iend) {
        const int length = iend + std::min(c.origin, 0);
        int eff = length;
        if (ad.wild) eff = length < m ? length - ad.ncount[std::max(length, 0)] : ad.eff_len;
        return length >= ad.min_overlap && (double)c.cost <= (double)eff * ad.rate;
    };
    bool any = false;
    HCell best{0, INT_MIN, 0};
    int best_i = m, best_j = n;
    auto offer = [&](const HCell& c, int i, int j) {
        if (!acceptable(c, i)) return;
        if (!any || c.score > best.score || (c.score == best.score && c.cost < best.cost)) {
            any = true;
            best = c;
            best_i = i;
            best_j = j;
        }
    };
    for (int j = min_n + 1; j <= max_n; ++j) {
        HCell& top = at(0, j);
        top = at(0, j - 1);
        if (ad.start_in_query) top.origin = j;
        else top = HCell{j, -2 * j, top.origin};
        for (int i = 1; i <= m; ++i) {
            const HCell &dg = at(i - 1, j - 1), &del = at(i, j - 1), &ins = at(i - 1, j);
            const bool eq = q[j - 1] < 4 && (ad.mask[i - 1] >> q[j - 1]) & 1;
            HCell& c = at(i, j);
            if (eq) {
                c = HCell{dg.cost, dg.score + 1, dg.origin};
            } else if (dg.cost + 1 <= del.cost + 1 && dg.cost + 1 <= ins.cost + 1) {
                c = HCell{dg.cost + 1, dg.score - 1, dg.origin};
            } else if (ins.cost + 1 <= del.cost + 1) {
                c = HCell{ins.cost + 1, ins.score - 2, ins.origin};
            } else {
                c = HCell{del.cost + 1, del.score - 2, del.origin};
            }
        }
        if (ad.stop_in_query) offer(at(m, j), m, j);
    }
    if (max_n == n)
        for (int i = ad.stop_in_ref ? 0 : m; i <= m; ++i) offer(at(i, n), i, n);
    HostMatch r;
    if (!any) return r;
    r.any = true;
    r.astart = best.origin >= 0 ? 0 : -best.origin;
    r.rstart = best.origin >= 0 ? best.origin : 0;
    r.astop = best_i;
    r.rstop = best_j;
    r.score = best.score;
    r.errors = best.cost;
    return r;
}

// AdapterCutter.best_match: greater score, then fewer errors, then the earlier adapter.
int host_best(const std::vector<HostAdapter>& ads, const std::vector<uint8_t>& q, HostMatch& bm) {
    int best = -1;
    for (size_t a = 0; a < ads.size(); ++a) {
        const HostMatch r = host_locate(ads[a], q);
        if (!r.any) continue;
        if (best < 0 || r.score > bm.score || (r.score == bm.score && r.errors < bm.errors)) {
            best = (int)a;
            bm = r;
        }
    }
    return best;
}

}  // namespace
}  // namespace dmx

using namespace dmx;

extern "C" int dmx_ends_host(const char* const* seqs, const int* lens, const int* wheres,
                             const int* min_overlaps, int n_adapters, double max_errors,
                             int min_overlap, int rc, const uint32_t* seq2b, const uint32_t* nmask,
                             const uint64_t* offsets, const uint32_t* read_lens, size_t n_reads,
                             dmx_result* out) {
    auto fail = [](int code, const std::string& msg) {
        set_process_error("dmx_ends_host: " + msg);
        return code;
    };
    if (!seqs || !lens || !wheres || (n_reads && (!seq2b || !nmask || !offsets || !read_lens || !out)))
        return fail(DMX_E_INVALID, "null argument");
    if (n_adapters <= 0 || n_adapters > kMaxAdapters)
        return fail(DMX_E_INVALID, "panel must hold 1..64 adapters");
    if (!(max_errors >= 0.0)) return fail(DMX_E_INVALID, "max_errors must be >= 0");
    std::vector<HostAdapter> ads((size_t)n_adapters);
    for (int a = 0; a < n_adapters; ++a) {
        HostAdapter& ad = ads[(size_t)a];
        const int w = wheres[a], side = w & (DMX_FRONT | DMX_BACK);
        const int restrict_bits = w & (DMX_ANCHORED | DMX_NONINTERNAL);
        if ((w & ~(DMX_FRONT | DMX_BACK | DMX_ANCHORED | DMX_NONINTERNAL)) ||
            (side != DMX_FRONT && side != DMX_BACK) ||
            restrict_bits == (DMX_ANCHORED | DMX_NONINTERNAL))
            return fail(DMX_E_INVALID, "adapter " + std::to_string(a) + ": bad where");
        const int m = lens[a];
        if (m <= 0 || m > kMaxLen)
            return fail(DMX_E_UNSUPPORTED, "adapter length must be 1..64");
        ad.m = m;
        ad.front = side == DMX_FRONT;
        ad.mask.resize((size_t)m);
        ad.ncount.assign((size_t)m + 1, 0);
        int nc = 0;
        for (int i = 0; i < m; ++i) {
            const char ch = seqs[a][i];
            ad.mask[(size_t)i] = host_iupac(ch);
            if (!ad.mask[(size_t)i])
                return fail(DMX_E_INVALID, std::string("adapter character not IUPAC uppercase: ") + ch);
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') ad.wild = true;
            ad.ncount[(size_t)i] = nc;
            if (ch == 'N') ++nc;
        }
        ad.ncount[(size_t)m] = nc;
        ad.eff_len = ad.wild ? m - nc : m;
        if (ad.eff_len == 0) return fail(DMX_E_INVALID, "adapter consists only of N wildcards");
        ad.rate = max_errors >= 1.0 ? max_errors / (double)m : max_errors;
        ad.min_overlap = (w & DMX_ANCHORED) ? m : (min_overlaps ? min_overlaps[a] : min_overlap);
        // adapters.py: the EndSkip flags of the six single-adapter classes
        if (ad.front) {
            ad.stop_in_query = true;
            ad.start_in_query = !restrict_bits;
            ad.start_in_ref = !(w & DMX_ANCHORED);
        } else {
            ad.start_in_query = true;
            ad.stop_in_query = !restrict_bits;
            ad.stop_in_ref = !(w & DMX_ANCHORED);
        }
    }
    std::vector<uint8_t> fw, rv;
    for (size_t r = 0; r < n_reads; ++r) {
        const uint64_t off = offsets[r];
        const uint32_t n = read_lens[r];
        fw.resize(n);
        rv.resize(n);
        for (uint32_t x = 0; x < n; ++x) {
            const uint64_t g = off + x;
            const uint8_t code = (uint8_t)((seq2b[g >> 4] >> (2 * (g & 15))) & 3u);
            const bool masked = (nmask[g >> 5] >> (g & 31)) & 1u;
            fw[x] = masked ? 4 : code;
            rv[n - 1 - x] = masked ? 4 : (uint8_t)(3 - code);
        }
        dmx_result res;
        memset(&res, 0, sizeof(res));
        res.bin1 = res.bin2 = -1;
        HostMatch mf, mr;
        const int af = host_best(ads, fw, mf);
        const int ar = rc ? host_best(ads, rv, mr) : -1;
        const int fs = af >= 0 ? mf.score : 0, rs = ar >= 0 ? mr.score : 0;
        const bool use_rc = rc && rs > fs;   // ReverseComplementer: strictly greater only
        const int a = use_rc ? ar : af;
        const HostMatch& mt = use_rc ? mr : mf;
        res.rc1 = use_rc ? 1 : 0;
        if (a >= 0) {
            res.bin1 = (int16_t)a;
            res.m1.rstart = mt.rstart;
            res.m1.rstop = mt.rstop;
            res.m1.astart = (int16_t)mt.astart;
            res.m1.astop = (int16_t)mt.astop;
            res.m1.score = (int16_t)mt.score;
            res.m1.errors = (int16_t)mt.errors;
        }
        out[r] = res;
    }
    return DMX_OK;
}
