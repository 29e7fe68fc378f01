// dmx_groups.hip — gene groups on the device (include/dmx.h dmx_edgegroups, dmx_pairhits,
// dmx_pairhits_fetch, dmx_hitgroups).  Replaces the best-hit filter and the
// grouping of the amplicon-sorting stage (amplicon_sorter.py update_list :983-1034, merge_groups
// :1058-1087): of the similarity pass only one label per read comes back.
//
// Three pieces:
//   outcomes    what becomes of a launch of dmx_pairhits' distances (ph_decide_kernel): per input
//               pair a distance and a reverse bit, or none; per read the least distance of the
//               hits it is the target of (atomicMin); a bitmap of the pairs to try reversed.
//   compaction  order-preserving: a flag per pair, the flags counted per block of 256
//               (lg_count_kernel), the counts scanned by one block (lg_scan_kernel), and every
//               kept pair written at its block's offset plus its rank in the block
//               (lg_scatter_kernel).  It makes dmx_pairhits_fetch's hit list and dmx_hitgroups'
//               edge list (the hits with d <= tie[t]).
//   components  of an edge list over n nodes: parent[v] = v; rounds of hooking (every edge whose
//               ends have different roots sets the larger root's parent to the smaller root,
//               atomicMin) and pointer jumping (parent[v] = v's root), until a round hooks
//               nothing; a last pass writes labels.  parent[v] <= v always holds, so there are no
//               cycles, a root is the smallest node of its tree, and the result (the smallest
//               node of the component) does not depend on the order the atomics land in.
// The species groups (dmx_hithist, dmx_pairhits_cross, dmx_hitgroups_within; DESIGN.md §8k;
// amplicon_sorter.py SSG :810-836, read_indexes :1363-1411) read the same outcomes: a histogram
// of the hits' identity classes (lg_hist_kernel), and the compaction with two more predicates.
// The forward pass itself is dmx_pairdist's (dmx_pairdist.hip dmx_pairhits).
#include <cstring>
#include <numeric>

#include "dmx_internal.h"

namespace dmx {

constexpr uint32_t kLgBlock = 256;                 // threads per block, one pair / edge / node each
constexpr uint32_t kLgWaves = kLgBlock / 64;
constexpr uint32_t kLgDist = ~(uint32_t)DMX_LG_REV;   // an outcome's distance bits

struct LgState {
    // the last dmx_pairhits: its pair list, and per pair the outcome (d | DMX_LG_REV, or
    // DMX_LG_NONE); valid until the next dmx_load, dmx_pairhits or dmx_close
    DevBuf<uint32_t> q, t, outc;
    DevBuf<int32_t> cap_hit, cap_half;
    DevBuf<uint32_t> best;           // per read of the batch
    DevBuf<uint32_t> orig, need;     // per launch: sorted pair -> input pair; the retry bitmap
    DevBuf<unsigned long long> cnt;  // hits
    size_t n_pairs = 0, n_reads = 0;
    uint64_t n_hits = 0;
    bool valid = false;
    // compaction: per-block counts / offsets, and what it writes (hits: pair, d, rev; edges: a, b)
    DevBuf<uint32_t> blk, sel_a, sel_b;
    DevBuf<uint8_t> sel_rev;
    // components
    DevBuf<uint32_t> parent, labels, tie, flag;
    // species groups: per read its gene group and second cap; the histogram's table and counters
    DevBuf<uint32_t> label, bin_off, hbad;
    DevBuf<int32_t> cap2;
    DevBuf<uint16_t> bins;
    DevBuf<unsigned long long> hist;
    hipEvent_t ev[2] = {};
    // dmx_pairhits' forward launches, compaction, components, histogram
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    int rounds = 0;                  // hooking rounds of the last components run
    ~LgState() {
        for (auto& e : ev)
            if (e) hipEventDestroy(e);
    }
};

void lg_release(Ctx* c) {
    delete c->lg;
    c->lg = nullptr;
}

void lg_invalidate(Ctx* c) {
    if (c->lg) c->lg->valid = false;   // the outcomes name reads of the previous resident batch
}

// ---- outcomes ----------------------------------------------------------------------------------

struct PhDecide {
    const uint32_t* dist;    // the launch's distances, min(d, cap + 1), in sorted order
    const uint32_t* orig;    // sorted pair k is input pair orig[k]
    uint32_t np, pass, lo;   // pass 0: forward, bit orig[k] - lo of need; pass 1: reverse
    const int32_t* cap_hit;
    const int32_t* cap_half;
    const uint32_t* t;
    uint32_t n_pairs, n_reads;
    uint32_t* outc;
    uint32_t* best;
    uint32_t* need;
    uint32_t need_words;
    unsigned long long* cnt;
};

// The decisions of sorter.similarity on one launch's distances.  Forward: d <= cap_hit is a hit;
// otherwise cap_hit >= 0 and d > cap_half asks for the reverse complement.  Reverse: d <= cap_hit
// is a hit with the reverse bit.  The forward cap is max(cap_hit, cap_half, 0), so the clamped
// distance compares against both caps as the exact one would.
__global__ __launch_bounds__(kLgBlock) void ph_decide_kernel(PhDecide A) {
    const uint32_t k = blockIdx.x * kLgBlock + threadIdx.x;
    bool hit = false;
    if (k < A.np) {
        const uint32_t i = A.orig[k];
        if (i < A.n_pairs) {
            const int64_t d = A.dist[k], ch = A.cap_hit[i], chalf = A.cap_half[i];
            hit = d <= ch;
            if (A.pass == 0) {
                A.outc[i] = hit ? (uint32_t)d : DMX_LG_NONE;
                if (!hit && ch >= 0 && d > chalf) {
                    const uint32_t b = i - A.lo;
                    if ((b >> 5) < A.need_words) atomicOr(&A.need[b >> 5], 1u << (b & 31u));
                }
            } else if (hit) {
                A.outc[i] = (uint32_t)d | DMX_LG_REV;
            }
            if (hit) {
                const uint32_t r = A.t[i];
                if (r < A.n_reads) atomicMin(&A.best[r], (uint32_t)d);
            }
        }
    }
    const uint64_t bal = __ballot(hit);   // every lane of the wave is here
    if ((threadIdx.x & 63u) == 0 && bal) atomicAdd(A.cnt, (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(kLgBlock) void lg_fill_kernel(uint32_t* p, uint32_t n, uint32_t v) {
    const uint32_t i = blockIdx.x * kLgBlock + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- compaction --------------------------------------------------------------------------------

struct LgCompact {
    const uint32_t* outc;
    const uint32_t* q;
    const uint32_t* t;
    const uint32_t* tie;     // edges: per read, the largest distance kept (within: NONE = no edge)
    const uint32_t* label;   // cross, within: per read, its gene group or DMX_LG_NONE
    const int32_t* cap2;     // cross: per read, the largest distance of the second threshold
    uint32_t n_pairs, n_reads;
    uint32_t* blk;           // [block]: its count, then its offset; [n_blocks]: the total
    uint32_t* out_a;         // hits: the pair's place in the input; edges: q
    uint32_t* out_b;         // hits: d; edges: t
    uint8_t* out_rev;        // hits: the reverse bit
    uint32_t out_cap;
};

// What a compaction keeps, and what it writes: hits and cross hits (place, d, reverse bit), edges
// and within-group edges (q, t).
enum LgKind : int { kLgHits = 0, kLgEdges = 1, kLgCross = 2, kLgWithin = 3 };
constexpr bool lg_writes_edges(int kind) { return kind == kLgEdges || kind == kLgWithin; }

// Is pair i kept?  Hits: every pair with an outcome.  Edges: those with d <= tie[t].  Cross: the
// hits within the second threshold of their target (cap2[t] >= 0, d <= cap2[t]) whose ends carry
// different labels (so one of the two is a group).  Within: the hits whose ends carry the same
// group and d <= tie[t], where tie[t] = DMX_LG_NONE keeps nothing.  Every read index is tested
// against n_reads before it indexes a per-read table.
template <int kKind>
__device__ __forceinline__ bool lg_keep(const LgCompact& A, uint32_t i) {
    if (i >= A.n_pairs) return false;
    const uint32_t o = A.outc[i];
    if (o == DMX_LG_NONE) return false;
    if constexpr (kKind == kLgEdges) {
        const uint32_t r = A.t[i];
        return r < A.n_reads && (o & kLgDist) <= A.tie[r];
    } else if constexpr (kKind == kLgCross) {
        const uint32_t x = A.q[i], r = A.t[i];
        if (x >= A.n_reads || r >= A.n_reads) return false;
        const int64_t c2 = A.cap2[r];
        return c2 >= 0 && (int64_t)(o & kLgDist) <= c2 && A.label[x] != A.label[r];
    } else if constexpr (kKind == kLgWithin) {
        const uint32_t x = A.q[i], r = A.t[i];
        if (x >= A.n_reads || r >= A.n_reads) return false;
        const uint32_t lr = A.label[r], tr = A.tie[r];
        return lr != DMX_LG_NONE && A.label[x] == lr && tr != DMX_LG_NONE && (o & kLgDist) <= tr;
    } else {
        return true;
    }
}

// The flagged threads of the block before this one; *total: of the whole block.  Every thread of
// the block calls it.
__device__ __forceinline__ uint32_t lg_block_rank(bool f, uint32_t* total) {
    __shared__ uint32_t wsum[kLgWaves];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t bal = __ballot(f);
    if (lane == 0) wsum[w] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLgWaves; ++k) {
        if (k < w) before += wsum[k];
        tot += wsum[k];
    }
    *total = tot;
    return before;
}

template <int kKind>
__global__ __launch_bounds__(kLgBlock) void lg_count_kernel(LgCompact A) {
    uint32_t tot;
    lg_block_rank(lg_keep<kKind>(A, blockIdx.x * kLgBlock + threadIdx.x), &tot);
    if (threadIdx.x == 0) A.blk[blockIdx.x] = tot;
}

// One block: blk[b] becomes the sum of the counts before b, blk[nb] the total.
__global__ __launch_bounds__(kLgBlock) void lg_scan_kernel(uint32_t* blk, uint32_t nb) {
    __shared__ uint32_t wsum[kLgWaves];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kLgBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? blk[i] : 0u;
        uint32_t x = v;   // the wave's inclusive scan
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63u) wsum[w] = x;
        __syncthreads();
        uint32_t off = 0, tot = 0;
#pragma unroll
        for (uint32_t k = 0; k < kLgWaves; ++k) {
            if (k < w) off += wsum[k];
            tot += wsum[k];
        }
        if (i < nb) blk[i] = carry + off + x - v;
        carry += tot;
        __syncthreads();   // wsum is written again in the next tile
    }
    if (threadIdx.x == 0) blk[nb] = carry;
}

template <int kKind>
__global__ __launch_bounds__(kLgBlock) void lg_scatter_kernel(LgCompact A) {
    const uint32_t i = blockIdx.x * kLgBlock + threadIdx.x;
    const bool f = lg_keep<kKind>(A, i);
    uint32_t tot;
    const uint32_t pos = A.blk[blockIdx.x] + lg_block_rank(f, &tot);
    if (!f || pos >= A.out_cap) return;
    if constexpr (lg_writes_edges(kKind)) {
        A.out_a[pos] = A.q[i];
        A.out_b[pos] = A.t[i];
    } else {
        const uint32_t o = A.outc[i];
        A.out_a[pos] = i;
        A.out_b[pos] = o & kLgDist;
        A.out_rev[pos] = (uint8_t)(o >> 31);
    }
}

// ---- identity histogram ------------------------------------------------------------------------

constexpr uint32_t kLgHistClasses = 1024;   // the most classes: the block's LDS counters
constexpr uint32_t kLgHistBlocks = 1024;    // the most blocks of a launch (grid-stride beyond)
enum LgHistBad : uint32_t { kLgBadRead = 1, kLgBadBin = 2, kLgBadClass = 4 };

struct LgHist {
    const uint32_t* outc;
    const uint32_t* t;
    const uint32_t* bin_off;   // per read: where its length's row of the table starts
    const uint16_t* bins;      // the table: the class of distance d at bins[bin_off[t] + d]
    uint64_t n_bins;
    uint32_t n_pairs, n_reads, n_classes;
    unsigned long long* hist;  // n_classes counters, zeroed before the launch
    uint32_t* bad;             // LgHistBad bits: an index formed from data was outside its extent
    Bounds bd;
};

// hist[class of the hit] += 1 over the hits of the outcomes: a thread per pair, grid-stride; the
// block counts in LDS and adds its nonzero counters to the global ones once.  A block sees fewer
// than 2^31 pairs, so its 32-bit counters cannot wrap.  A target outside the reads, a table index
// outside the bins or a class outside the classes is not followed: it sets its bit of *bad and
// the host discards the counts.
__global__ __launch_bounds__(kLgBlock) void lg_hist_kernel(LgHist A) {
    __shared__ uint32_t h[kLgHistClasses];
    for (uint32_t k = threadIdx.x; k < kLgHistClasses; k += kLgBlock) h[k] = 0u;
    __syncthreads();
    uint32_t bad = 0u;
    const uint32_t stride = gridDim.x * kLgBlock;
    for (uint32_t base = blockIdx.x * kLgBlock; base < A.n_pairs; base += stride) {
        const uint32_t i = base + threadIdx.x;
        uint32_t cls = DMX_LG_NONE;
        if (i < A.n_pairs) {
            const uint32_t o = A.outc[i];
            if (o != DMX_LG_NONE) {
                const uint32_t r = A.t[i];
                if (r >= A.n_reads) {
                    bad |= kLgBadRead;
                } else {
                    const uint64_t at = (uint64_t)A.bin_off[r] + (o & kLgDist);
                    if (at >= A.n_bins) {
                        bad |= kLgBadBin;
                    } else if (bchk(A.bd, (int64_t)at, 0, (int64_t)A.n_bins, kBufHistBins)) {
                        const uint32_t x = A.bins[at];
                        if (x >= A.n_classes || x >= kLgHistClasses) bad |= kLgBadClass;
                        else cls = x;
                    }
                }
            }
        }
        // (one LDS add per hit; per-wave aggregation of equal classes was slower)
        if (cls != DMX_LG_NONE) atomicAdd(&h[cls], 1u);
    }
    if (bad) atomicOr(A.bad, bad);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < A.n_classes && k < kLgHistClasses; k += kLgBlock)
        if (h[k]) atomicAdd(&A.hist[k], (unsigned long long)h[k]);
}

// ---- components --------------------------------------------------------------------------------

// v's root.  parent[x] <= x for every x, so the walk only descends; a value another thread is
// writing meanwhile is an ancestor either way.  n bounds the walk whatever the array holds.
__device__ __forceinline__ uint32_t lg_root(const uint32_t* parent, uint32_t v, uint32_t n) {
    for (uint32_t it = 0; it < n; ++it) {
        const uint32_t p = parent[v];
        if (p >= v) break;
        v = p;
    }
    return v;
}

__global__ __launch_bounds__(kLgBlock) void lg_init_kernel(uint32_t* parent, uint32_t* labels,
                                                           uint32_t n) {
    const uint32_t v = blockIdx.x * kLgBlock + threadIdx.x;
    if (v >= n) return;
    parent[v] = v;
    labels[v] = DMX_LG_NONE;
}

// A node on an edge (a self-loop too) gets a label; which one, lg_flatten_kernel says.
__global__ __launch_bounds__(kLgBlock) void lg_mark_kernel(const uint32_t* a, const uint32_t* b,
                                                           uint32_t ne, uint32_t n,
                                                           uint32_t* labels) {
    const uint32_t e = blockIdx.x * kLgBlock + threadIdx.x;
    if (e >= ne) return;
    const uint32_t x = a[e], y = b[e];
    if (x >= n || y >= n) return;
    labels[x] = 0u;
    labels[y] = 0u;
}

// Hooking.  The larger root's parent becomes at most the smaller root: were it lowered further by
// another edge meanwhile, this edge's union is not recorded, but the flag is set and the next
// round sees the edge again.  The first atomicMin of a round lands on a true root and lowers it,
// so every round that sets the flag lowers some parent: the rounds end.
__global__ __launch_bounds__(kLgBlock) void lg_hook_kernel(const uint32_t* a, const uint32_t* b,
                                                           uint32_t ne, uint32_t n,
                                                           uint32_t* parent, uint32_t* flag) {
    const uint32_t e = blockIdx.x * kLgBlock + threadIdx.x;
    if (e >= ne) return;
    const uint32_t x = a[e], y = b[e];
    if (x >= n || y >= n) return;
    const uint32_t rx = lg_root(parent, x, n), ry = lg_root(parent, y, n);
    if (rx == ry) return;
    atomicMin(&parent[max(rx, ry)], min(rx, ry));
    *flag = 1u;
}

// Pointer jumping, all the way: every tree becomes a star.
__global__ __launch_bounds__(kLgBlock) void lg_jump_kernel(uint32_t* parent, uint32_t n) {
    const uint32_t v = blockIdx.x * kLgBlock + threadIdx.x;
    if (v >= n) return;
    const uint32_t r = lg_root(parent, v, n);
    if (r != parent[v]) parent[v] = r;
}

__global__ __launch_bounds__(kLgBlock) void lg_flatten_kernel(const uint32_t* parent,
                                                              uint32_t* labels, uint32_t n) {
    const uint32_t v = blockIdx.x * kLgBlock + threadIdx.x;
    if (v >= n) return;
    if (labels[v] != DMX_LG_NONE) labels[v] = lg_root(parent, v, n);
}

}  // namespace dmx

using namespace dmx;

namespace {

#define LG_CK(who, call)                                                                     \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            c->err = std::string(who) + ": " + #call + ": " + hipGetErrorString(e_);         \
            return DMX_E_HIP;                                                                \
        }                                                                                    \
    } while (0)

inline uint32_t lg_blocks(size_t n) { return (uint32_t)((n + kLgBlock - 1) / kLgBlock); }

int lg_state(Ctx* c, const char* who) {
    LG_CK(who, hipSetDevice(c->device));
    if (!c->lg) {
        c->lg = new LgState();
        for (auto& e : c->lg->ev) LG_CK(who, hipEventCreate(&e));
    }
    return DMX_OK;
}

// The compaction of the last dmx_pairhits' outcomes into sel_a / sel_b (/ sel_rev), room for
// `cap` entries; *total = how many are kept.  Synchronises; ms[1] = its device time.
template <int kKind>
int lg_compact(Ctx* c, const char* who, size_t cap, uint32_t* total) {
    LgState* s = c->lg;
    hipStream_t st = c->stream;
    *total = 0;
    s->ms[1] = 0.f;
    if (!s->n_pairs) return DMX_OK;
    const uint32_t nb = lg_blocks(s->n_pairs);
    LG_CK(who, s->blk.reserve((size_t)nb + 1));
    LG_CK(who, s->sel_a.reserve(cap));
    LG_CK(who, s->sel_b.reserve(cap));
    if (!lg_writes_edges(kKind)) LG_CK(who, s->sel_rev.reserve(cap));
    LgCompact A;
    A.outc = s->outc.p, A.q = s->q.p, A.t = s->t.p, A.tie = s->tie.p;
    A.label = s->label.p, A.cap2 = s->cap2.p;
    A.n_pairs = (uint32_t)s->n_pairs, A.n_reads = (uint32_t)s->n_reads;
    A.blk = s->blk.p, A.out_a = s->sel_a.p, A.out_b = s->sel_b.p, A.out_rev = s->sel_rev.p;
    A.out_cap = (uint32_t)cap;
    LG_CK(who, hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(lg_count_kernel<kKind>, dim3(nb), dim3(kLgBlock), 0, st, A);
    hipLaunchKernelGGL(lg_scan_kernel, dim3(1), dim3(kLgBlock), 0, st, s->blk.p, nb);
    hipLaunchKernelGGL(lg_scatter_kernel<kKind>, dim3(nb), dim3(kLgBlock), 0, st, A);
    LG_CK(who, hipGetLastError());
    LG_CK(who, hipEventRecord(s->ev[1], st));
    LG_CK(who, hipMemcpyAsync(total, s->blk.p + nb, 4, hipMemcpyDeviceToHost, st));
    LG_CK(who, hipStreamSynchronize(st));
    hipEventElapsedTime(&s->ms[1], s->ev[0], s->ev[1]);
    return DMX_OK;
}

// The components of the device edge list (d_a, d_b) over n nodes into s->labels.  ms[2] = the
// time from the first kernel to the last, the flag's trips to the host between the rounds
// included.  Synchronises.
int lg_components(Ctx* c, const char* who, const uint32_t* d_a, const uint32_t* d_b, uint32_t ne,
                  uint32_t n) {
    LgState* s = c->lg;
    hipStream_t st = c->stream;
    s->ms[2] = 0.f;
    s->rounds = 0;
    if (!n) return DMX_OK;
    const uint32_t vb = lg_blocks(n), eb = lg_blocks(ne);
    LG_CK(who, s->parent.reserve(n));
    LG_CK(who, s->labels.reserve(n));
    LG_CK(who, s->flag.reserve(1));
    LG_CK(who, hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(lg_init_kernel, dim3(vb), dim3(kLgBlock), 0, st, s->parent.p, s->labels.p, n);
    if (ne) {
        hipLaunchKernelGGL(lg_mark_kernel, dim3(eb), dim3(kLgBlock), 0, st, d_a, d_b, ne, n,
                           s->labels.p);
        // every round that goes on lowers a parent, so n rounds are never reached (lg_hook_kernel)
        for (uint32_t round = 0;; ++round) {
            uint32_t changed = 0;
            LG_CK(who, hipMemsetAsync(s->flag.p, 0, 4, st));
            hipLaunchKernelGGL(lg_hook_kernel, dim3(eb), dim3(kLgBlock), 0, st, d_a, d_b, ne, n,
                               s->parent.p, s->flag.p);
            LG_CK(who, hipGetLastError());
            LG_CK(who, hipMemcpyAsync(&changed, s->flag.p, 4, hipMemcpyDeviceToHost, st));
            LG_CK(who, hipStreamSynchronize(st));
            s->rounds = (int)round + 1;
            if (!changed) break;
            if (round >= n) {
                c->err = std::string(who) + ": the hooking rounds did not end";
                return DMX_E_STATE;
            }
            hipLaunchKernelGGL(lg_jump_kernel, dim3(vb), dim3(kLgBlock), 0, st, s->parent.p, n);
        }
        hipLaunchKernelGGL(lg_flatten_kernel, dim3(vb), dim3(kLgBlock), 0, st, s->parent.p,
                           s->labels.p, n);
    }
    LG_CK(who, hipGetLastError());
    LG_CK(who, hipEventRecord(s->ev[1], st));
    LG_CK(who, hipStreamSynchronize(st));
    hipEventElapsedTime(&s->ms[2], s->ev[0], s->ev[1]);
    return DMX_OK;
}

// The sequential union-find of the host twins: the root of a tree is its smallest node.
struct HostSets {
    std::vector<uint32_t> parent;
    explicit HostSets(size_t n) : parent(n) { std::iota(parent.begin(), parent.end(), 0u); }
    uint32_t find(uint32_t v) {
        uint32_t r = v;
        while (parent[r] != r) r = parent[r];
        while (parent[v] != r) {
            const uint32_t up = parent[v];
            parent[v] = r;
            v = up;
        }
        return r;
    }
    void join(uint32_t x, uint32_t y) {
        const uint32_t rx = find(x), ry = find(y);
        if (rx != ry) parent[std::max(rx, ry)] = std::min(rx, ry);
    }
};

// 0, or DMX_E_INVALID with *err naming the first edge with an end outside the nodes.
int lg_validate_edges(const char* who, const uint32_t* a, const uint32_t* b, size_t n_edges,
                      uint32_t n_nodes, std::string* err) {
    for (size_t e = 0; e < n_edges; ++e)
        if (a[e] >= n_nodes || b[e] >= n_nodes) {
            *err = std::string(who) + ": edge " + std::to_string(e) + " names a node outside the " +
                   std::to_string(n_nodes) + " given";
            return DMX_E_INVALID;
        }
    return DMX_OK;
}

void lg_host_labels(const uint32_t* a, const uint32_t* b, size_t n_edges, size_t n_nodes,
                    uint32_t* labels) {
    HostSets hs(n_nodes);
    std::vector<uint8_t> on(n_nodes, 0);
    for (size_t e = 0; e < n_edges; ++e) {
        on[a[e]] = on[b[e]] = 1;
        hs.join(a[e], b[e]);
    }
    for (size_t v = 0; v < n_nodes; ++v) labels[v] = on[v] ? hs.find((uint32_t)v) : DMX_LG_NONE;
}

}  // namespace

// ---- dmx_pairhits' device-side bookkeeping (dmx_internal.h) ------------------------------------

namespace dmx {

int lg_hits_begin(Ctx* c, const char* who, const uint32_t* q, const uint32_t* t,
                  const int32_t* cap_hit, const int32_t* cap_half, size_t n_pairs, size_t n_reads) {
    if (const int rc = lg_state(c, who)) return rc;
    LgState* s = c->lg;
    hipStream_t st = c->stream;
    s->valid = false;
    s->n_pairs = n_pairs;
    s->n_reads = n_reads;
    s->n_hits = 0;
    s->ms[0] = 0.f;
    LG_CK(who, s->q.reserve(n_pairs));
    LG_CK(who, s->t.reserve(n_pairs));
    LG_CK(who, s->outc.reserve(n_pairs));
    LG_CK(who, s->cap_hit.reserve(n_pairs));
    LG_CK(who, s->cap_half.reserve(n_pairs));
    LG_CK(who, s->best.reserve(n_reads));
    LG_CK(who, s->cnt.reserve(1));
    if (n_pairs) {
        LG_CK(who, hipMemcpyAsync(s->q.p, q, n_pairs * 4, hipMemcpyHostToDevice, st));
        LG_CK(who, hipMemcpyAsync(s->t.p, t, n_pairs * 4, hipMemcpyHostToDevice, st));
        LG_CK(who, hipMemcpyAsync(s->cap_hit.p, cap_hit, n_pairs * 4, hipMemcpyHostToDevice, st));
        LG_CK(who, hipMemcpyAsync(s->cap_half.p, cap_half, n_pairs * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lg_fill_kernel, dim3(lg_blocks(n_pairs)), dim3(kLgBlock), 0, st,
                           s->outc.p, (uint32_t)n_pairs, (uint32_t)DMX_LG_NONE);
    }
    if (n_reads)
        hipLaunchKernelGGL(lg_fill_kernel, dim3(lg_blocks(n_reads)), dim3(kLgBlock), 0, st,
                           s->best.p, (uint32_t)n_reads, (uint32_t)DMX_LG_NONE);
    LG_CK(who, hipGetLastError());
    LG_CK(who, hipMemsetAsync(s->cnt.p, 0, sizeof(unsigned long long), st));
    LG_CK(who, hipStreamSynchronize(st));   // the caller's arrays are pageable
    return DMX_OK;
}

int lg_hits_decide(Ctx* c, const char* who, const uint32_t* d_dist, const uint32_t* orig, size_t np,
                   int pass, size_t lo, std::vector<uint32_t>* need) {
    LgState* s = c->lg;
    hipStream_t st = c->stream;
    const size_t words = (np + 31) / 32;
    LG_CK(who, s->orig.reserve(np));
    LG_CK(who, s->need.reserve(words));
    LG_CK(who, hipMemcpyAsync(s->orig.p, orig, np * 4, hipMemcpyHostToDevice, st));
    if (pass == 0) LG_CK(who, hipMemsetAsync(s->need.p, 0, words * 4, st));
    PhDecide A;
    A.dist = d_dist, A.orig = s->orig.p;
    A.np = (uint32_t)np, A.pass = (uint32_t)pass, A.lo = (uint32_t)lo;
    A.cap_hit = s->cap_hit.p, A.cap_half = s->cap_half.p, A.t = s->t.p;
    A.n_pairs = (uint32_t)s->n_pairs, A.n_reads = (uint32_t)s->n_reads;
    A.outc = s->outc.p, A.best = s->best.p, A.need = s->need.p;
    A.need_words = pass == 0 ? (uint32_t)words : 0u;
    A.cnt = s->cnt.p;
    hipLaunchKernelGGL(ph_decide_kernel, dim3(lg_blocks(np)), dim3(kLgBlock), 0, st, A);
    LG_CK(who, hipGetLastError());
    if (pass == 0 && need) {
        need->resize(words);
        LG_CK(who, hipMemcpyAsync(need->data(), s->need.p, words * 4, hipMemcpyDeviceToHost, st));
    }
    LG_CK(who, hipStreamSynchronize(st));
    return DMX_OK;
}

int lg_hits_end(Ctx* c, const char* who, float forward_ms, uint32_t* best, uint64_t* n_hits) {
    LgState* s = c->lg;
    hipStream_t st = c->stream;
    unsigned long long cnt = 0;
    LG_CK(who, hipMemcpyAsync(&cnt, s->cnt.p, sizeof cnt, hipMemcpyDeviceToHost, st));
    if (s->n_reads)
        LG_CK(who, hipMemcpyAsync(best, s->best.p, s->n_reads * 4, hipMemcpyDeviceToHost, st));
    LG_CK(who, hipStreamSynchronize(st));
    s->n_hits = cnt;
    s->ms[0] = forward_ms;
    s->valid = true;
    *n_hits = cnt;
    return DMX_OK;
}

int lg_compact_outcomes(Ctx* c, const char* who, const uint32_t* d_outc, size_t n_pairs,
                        size_t hits_cap, uint32_t* pair, uint32_t* d, uint8_t* rev, size_t* n_hits,
                        float* ms) {
    *n_hits = 0;
    *ms = 0.f;
    if (!n_pairs) return DMX_OK;
    if (const int rc = lg_state(c, who)) return rc;
    LgState* s = c->lg;
    hipStream_t st = c->stream;
    const size_t room = std::min(hits_cap, n_pairs);   // the scatter writes no place at or past it
    const uint32_t nb = lg_blocks(n_pairs);
    LG_CK(who, s->blk.reserve((size_t)nb + 1));
    LG_CK(who, s->sel_a.reserve(room));
    LG_CK(who, s->sel_b.reserve(room));
    LG_CK(who, s->sel_rev.reserve(room));
    LgCompact A;
    A.outc = d_outc, A.q = nullptr, A.t = nullptr, A.tie = nullptr;   // hits: the outcomes alone
    A.label = nullptr, A.cap2 = nullptr;
    A.n_pairs = (uint32_t)n_pairs, A.n_reads = 0;
    A.blk = s->blk.p, A.out_a = s->sel_a.p, A.out_b = s->sel_b.p, A.out_rev = s->sel_rev.p;
    A.out_cap = (uint32_t)room;
    uint32_t total = 0;
    LG_CK(who, hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(lg_count_kernel<kLgHits>, dim3(nb), dim3(kLgBlock), 0, st, A);
    hipLaunchKernelGGL(lg_scan_kernel, dim3(1), dim3(kLgBlock), 0, st, s->blk.p, nb);
    hipLaunchKernelGGL(lg_scatter_kernel<kLgHits>, dim3(nb), dim3(kLgBlock), 0, st, A);
    LG_CK(who, hipGetLastError());
    LG_CK(who, hipEventRecord(s->ev[1], st));
    LG_CK(who, hipMemcpyAsync(&total, s->blk.p + nb, 4, hipMemcpyDeviceToHost, st));
    LG_CK(who, hipStreamSynchronize(st));
    hipEventElapsedTime(ms, s->ev[0], s->ev[1]);
    *n_hits = total;
    if (!total) return DMX_OK;
    if (hits_cap < total || !pair || !d || !rev) {
        c->err = std::string(who) + ": room for " + std::to_string(hits_cap) + " hits, " +
                 std::to_string(total) + " to return";
        return DMX_E_INVALID;
    }
    LG_CK(who, hipMemcpy(pair, s->sel_a.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    LG_CK(who, hipMemcpy(d, s->sel_b.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    LG_CK(who, hipMemcpy(rev, s->sel_rev.p, (size_t)total, hipMemcpyDeviceToHost));
    return DMX_OK;
}

}  // namespace dmx

// ---- the entry points (include/dmx.h) -----------------------------------------------------------

extern "C" int dmx_edgegroups_host(const uint32_t* a, const uint32_t* b, size_t n_edges,
                                   uint32_t n_nodes, uint32_t* labels) {
    const char* const who = "dmx_edgegroups_host";
    if ((n_edges && (!a || !b)) || (n_nodes && !labels)) {
        set_process_error(std::string(who) + ": null argument");
        return DMX_E_INVALID;
    }
    std::string err;
    if (const int rc = lg_validate_edges(who, a, b, n_edges, n_nodes, &err)) {
        set_process_error(err);
        return rc;
    }
    lg_host_labels(a, b, n_edges, n_nodes, labels);
    return DMX_OK;
}

extern "C" int dmx_edgegroups(dmx_ctx* c, const uint32_t* a, const uint32_t* b, size_t n_edges,
                              uint32_t n_nodes, uint32_t* labels) {
    const char* const who = "dmx_edgegroups";
    if (!c) return DMX_E_INVALID;
    if ((n_edges && (!a || !b)) || (n_nodes && !labels)) {
        c->err = "dmx_edgegroups: null edge list or output";
        return DMX_E_INVALID;
    }
    if (n_edges > DMX_LG_MAX_PAIRS) {
        c->err = "dmx_edgegroups: at most " + std::to_string(DMX_LG_MAX_PAIRS) + " edges supported";
        return DMX_E_UNSUPPORTED;
    }
    if (const int rc = lg_validate_edges(who, a, b, n_edges, n_nodes, &c->err)) return rc;
    if (!n_nodes) return DMX_OK;
    if (const int rc = lg_state(c, who)) return rc;
    LgState* s = c->lg;
    hipStream_t st = c->stream;
    LG_CK(who, s->sel_a.reserve(n_edges));
    LG_CK(who, s->sel_b.reserve(n_edges));
    if (n_edges) {
        LG_CK(who, hipMemcpyAsync(s->sel_a.p, a, n_edges * 4, hipMemcpyHostToDevice, st));
        LG_CK(who, hipMemcpyAsync(s->sel_b.p, b, n_edges * 4, hipMemcpyHostToDevice, st));
    }
    if (const int rc = lg_components(c, who, s->sel_a.p, s->sel_b.p, (uint32_t)n_edges, n_nodes))
        return rc;
    LG_CK(who, hipMemcpy(labels, s->labels.p, (size_t)n_nodes * 4, hipMemcpyDeviceToHost));
    return DMX_OK;
}

extern "C" int dmx_pairhits_host(const uint32_t* seq2b, const uint32_t* nmask,
                                 const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
                                 const uint32_t* q, const uint32_t* t, const int32_t* cap_hit,
                                 const int32_t* cap_half, size_t n_pairs, uint32_t* outcome,
                                 uint32_t* best, uint64_t* n_hits, int n_threads) {
    const char* const who = "dmx_pairhits_host";
    if (!n_hits || (n_reads && !best) || (n_pairs && (!q || !t || !cap_hit || !cap_half || !outcome))) {
        set_process_error(std::string(who) + ": null argument");
        return DMX_E_INVALID;
    }
    for (size_t i = 0; i < n_pairs; ++i)
        if (cap_hit[i] < -1 || cap_half[i] < -1) {
            set_process_error(std::string(who) + ": pair " + std::to_string(i) +
                              ": a cap is a distance, or -1 for none");
            return DMX_E_INVALID;
        }
    std::vector<uint32_t> fcap(n_pairs), df(n_pairs);
    for (size_t i = 0; i < n_pairs; ++i)
        fcap[i] = (uint32_t)std::max(std::max(cap_hit[i], cap_half[i]), 0);
    if (const int rc = dmx_pairdist_host(DMX_PD_NW, seq2b, nmask, offsets, lens, n_reads, q, t,
                                         nullptr, fcap.data(), n_pairs, df.data(), n_threads))
        return rc;
    std::vector<uint32_t> rq, rt, rcap, ri;
    for (size_t i = 0; i < n_pairs; ++i) {
        const int64_t d = df[i];
        outcome[i] = d <= cap_hit[i] ? df[i] : DMX_LG_NONE;
        if (d > cap_hit[i] && cap_hit[i] >= 0 && d > cap_half[i]) {
            ri.push_back((uint32_t)i);
            rq.push_back(q[i]);
            rt.push_back(t[i]);
            rcap.push_back((uint32_t)cap_hit[i]);
        }
    }
    std::vector<uint8_t> rflags(ri.size(), DMX_PD_RC);
    std::vector<uint32_t> dr(ri.size());
    if (const int rc = dmx_pairdist_host(DMX_PD_NW, seq2b, nmask, offsets, lens, n_reads, rq.data(),
                                         rt.data(), rflags.data(), rcap.data(), ri.size(),
                                         dr.data(), n_threads))
        return rc;
    for (size_t k = 0; k < ri.size(); ++k)
        if (dr[k] <= rcap[k]) outcome[ri[k]] = dr[k] | DMX_LG_REV;
    for (size_t r = 0; r < n_reads; ++r) best[r] = DMX_LG_NONE;
    uint64_t hits = 0;
    for (size_t i = 0; i < n_pairs; ++i)
        if (outcome[i] != DMX_LG_NONE) {
            ++hits;
            best[t[i]] = std::min(best[t[i]], outcome[i] & kLgDist);
        }
    *n_hits = hits;
    return DMX_OK;
}

extern "C" int dmx_hitgroups_host(const uint32_t* q, const uint32_t* t, const uint32_t* outcome,
                                  size_t n_pairs, const uint32_t* tie, size_t n_reads,
                                  uint32_t* labels) {
    const char* const who = "dmx_hitgroups_host";
    if ((n_pairs && (!q || !t || !outcome)) || (n_reads && (!tie || !labels))) {
        set_process_error(std::string(who) + ": null argument (no dmx_pairhits_host outcomes?)");
        return DMX_E_INVALID;
    }
    if (n_reads > DMX_LG_NONE) {
        set_process_error(std::string(who) + ": too many reads");
        return DMX_E_UNSUPPORTED;
    }
    std::string err;
    if (const int rc = lg_validate_edges(who, q, t, n_pairs, (uint32_t)n_reads, &err)) {
        set_process_error(err);
        return rc;
    }
    std::vector<uint32_t> a, b;
    for (size_t i = 0; i < n_pairs; ++i)
        if (outcome[i] != DMX_LG_NONE && (outcome[i] & kLgDist) <= tie[t[i]]) {
            a.push_back(q[i]);
            b.push_back(t[i]);
        }
    lg_host_labels(a.data(), b.data(), a.size(), n_reads, labels);
    return DMX_OK;
}

extern "C" int dmx_pairhits_fetch(dmx_ctx* c, uint32_t* pair, uint32_t* d, uint8_t* rev, size_t cap,
                                  size_t* n) {
    const char* const who = "dmx_pairhits_fetch";
    if (!c) return DMX_E_INVALID;
    if (!n) {
        c->err = "dmx_pairhits_fetch: null count";
        return DMX_E_INVALID;
    }
    *n = 0;
    if (!c->lg || !c->lg->valid) {
        c->err = "dmx_pairhits_fetch: no dmx_pairhits since the last dmx_load";
        return DMX_E_INVALID;
    }
    LgState* s = c->lg;
    *n = (size_t)s->n_hits;
    if (!s->n_hits) return DMX_OK;
    if (cap < s->n_hits || !pair || !d || !rev) {
        c->err = "dmx_pairhits_fetch: room for " + std::to_string(cap) + " hits, " +
                 std::to_string(s->n_hits) + " to return";
        return DMX_E_INVALID;
    }
    LG_CK(who, hipSetDevice(c->device));
    uint32_t total = 0;
    if (const int rc = lg_compact<kLgHits>(c, who, (size_t)s->n_hits, &total)) return rc;
    if (total != s->n_hits) {
        c->err = "dmx_pairhits_fetch: the compaction kept " + std::to_string(total) + " of " +
                 std::to_string(s->n_hits) + " hits";
        return DMX_E_STATE;
    }
    LG_CK(who, hipMemcpy(pair, s->sel_a.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    LG_CK(who, hipMemcpy(d, s->sel_b.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    LG_CK(who, hipMemcpy(rev, s->sel_rev.p, (size_t)total, hipMemcpyDeviceToHost));
    return DMX_OK;
}

extern "C" int dmx_hitgroups(dmx_ctx* c, const uint32_t* tie, uint32_t* labels) {
    const char* const who = "dmx_hitgroups";
    if (!c) return DMX_E_INVALID;
    if (!c->lg || !c->lg->valid) {
        c->err = "dmx_hitgroups: no dmx_pairhits since the last dmx_load";
        return DMX_E_INVALID;
    }
    LgState* s = c->lg;
    if (!s->n_reads) return DMX_OK;
    if (!tie || !labels) {
        c->err = "dmx_hitgroups: null tie table or output";
        return DMX_E_INVALID;
    }
    LG_CK(who, hipSetDevice(c->device));
    LG_CK(who, s->tie.reserve(s->n_reads));
    LG_CK(who, hipMemcpyAsync(s->tie.p, tie, s->n_reads * 4, hipMemcpyHostToDevice, c->stream));
    uint32_t n_edges = 0;
    if (const int rc = lg_compact<kLgEdges>(c, who, (size_t)s->n_hits, &n_edges)) return rc;
    if (n_edges > s->n_hits) {
        c->err = "dmx_hitgroups: the compaction kept more edges than there are hits";
        return DMX_E_STATE;
    }
    if (const int rc = lg_components(c, who, s->sel_a.p, s->sel_b.p, n_edges, (uint32_t)s->n_reads))
        return rc;
    LG_CK(who, hipMemcpy(labels, s->labels.p, s->n_reads * 4, hipMemcpyDeviceToHost));
    return DMX_OK;
}

// ---- species groups -------------------------------------------------------------

namespace {

const char* lg_hist_bad_name(uint32_t bad) {
    return (bad & kLgBadRead)  ? "a target outside the reads"
           : (bad & kLgBadBin) ? "a table index (bin_off[t] + d) outside the n_bins entries"
                               : "a class outside n_classes";
}

// The first hit of the outcomes that the histogram cannot follow, as LgHistBad (0: none).
uint32_t lg_hist_host_bad(const uint32_t* t, const uint32_t* outcome, size_t n_pairs,
                          size_t n_reads, const uint32_t* bin_off, const uint16_t* bins,
                          size_t n_bins, uint32_t n_classes, size_t* where) {
    for (size_t i = 0; i < n_pairs; ++i) {
        if (outcome[i] == DMX_LG_NONE) continue;
        *where = i;
        if (t[i] >= n_reads) return kLgBadRead;
        const uint64_t at = (uint64_t)bin_off[t[i]] + (outcome[i] & kLgDist);
        if (at >= n_bins) return kLgBadBin;
        if (bins[at] >= n_classes) return kLgBadClass;
    }
    return 0;
}

// 0, or DMX_E_INVALID: the arguments every species-group call checks before it does anything.
int lg_within_args(const char* who, size_t n_reads, const uint32_t* xa, const uint32_t* xb,
                   size_t n_extra, uint32_t n_nodes, std::string* err) {
    if (n_nodes < n_reads) {
        *err = std::string(who) + ": " + std::to_string(n_nodes) + " nodes for " +
               std::to_string(n_reads) + " reads";
        return DMX_E_INVALID;
    }
    if (n_extra && (!xa || !xb)) {
        *err = std::string(who) + ": null extra edges";
        return DMX_E_INVALID;
    }
    return lg_validate_edges(who, xa, xb, n_extra, n_nodes, err);
}

}  // namespace

extern "C" int dmx_hithist_host(const uint32_t* t, const uint32_t* outcome, size_t n_pairs,
                                size_t n_reads, const uint32_t* bin_off, const uint16_t* bins,
                                size_t n_bins, uint32_t n_classes, uint64_t* hist) {
    const char* const who = "dmx_hithist_host";
    if ((n_pairs && (!t || !outcome)) || (n_reads && !bin_off) || (n_bins && !bins) || !hist ||
        !n_classes || n_classes > kLgHistClasses) {
        set_process_error(std::string(who) + ": null argument, or n_classes outside 1.." +
                          std::to_string(kLgHistClasses));
        return DMX_E_INVALID;
    }
    size_t where = 0;
    if (const uint32_t bad = lg_hist_host_bad(t, outcome, n_pairs, n_reads, bin_off, bins, n_bins,
                                              n_classes, &where)) {
        set_process_error(std::string(who) + ": pair " + std::to_string(where) + ": " +
                          lg_hist_bad_name(bad));
        return DMX_E_INVALID;
    }
    for (size_t i = 0; i < n_pairs; ++i)
        if (outcome[i] != DMX_LG_NONE) ++hist[bins[(uint64_t)bin_off[t[i]] + (outcome[i] & kLgDist)]];
    return DMX_OK;
}

extern "C" int dmx_hithist(dmx_ctx* c, const uint32_t* bin_off, const uint16_t* bins, size_t n_bins,
                           uint32_t n_classes, uint64_t* hist) {
    const char* const who = "dmx_hithist";
    if (!c) return DMX_E_INVALID;
    if (!c->lg || !c->lg->valid) {
        c->err = "dmx_hithist: no dmx_pairhits since the last dmx_load";
        return DMX_E_INVALID;
    }
    LgState* s = c->lg;
    s->ms[3] = 0.f;
    if (!hist || !n_classes || n_classes > kLgHistClasses || (s->n_reads && !bin_off) ||
        (n_bins && !bins)) {
        c->err = "dmx_hithist: null argument, or n_classes outside 1.." +
                 std::to_string(kLgHistClasses);
        return DMX_E_INVALID;
    }
    if (!s->n_pairs || !s->n_hits) return DMX_OK;
    hipStream_t st = c->stream;
    LG_CK(who, hipSetDevice(c->device));
    LG_CK(who, s->bin_off.reserve(s->n_reads));
    LG_CK(who, s->bins.reserve(n_bins));
    LG_CK(who, s->hist.reserve(n_classes));
    LG_CK(who, s->hbad.reserve(1));
    LG_CK(who, hipMemcpyAsync(s->bin_off.p, bin_off, s->n_reads * 4, hipMemcpyHostToDevice, st));
    if (n_bins)
        LG_CK(who, hipMemcpyAsync(s->bins.p, bins, n_bins * 2, hipMemcpyHostToDevice, st));
    LG_CK(who, hipMemsetAsync(s->hist.p, 0, (size_t)n_classes * sizeof(unsigned long long), st));
    LG_CK(who, hipMemsetAsync(s->hbad.p, 0, 4, st));
    LG_CK(who, bounds_reset(c, st));
    LgHist A;
    A.outc = s->outc.p, A.t = s->t.p, A.bin_off = s->bin_off.p, A.bins = s->bins.p;
    A.n_bins = n_bins, A.n_pairs = (uint32_t)s->n_pairs, A.n_reads = (uint32_t)s->n_reads;
    A.n_classes = n_classes, A.hist = s->hist.p, A.bad = s->hbad.p;
    A.bd = make_bounds(c, kKerHithist);
    const uint32_t nb = std::min(lg_blocks(s->n_pairs), kLgHistBlocks);
    LG_CK(who, hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(lg_hist_kernel, dim3(nb), dim3(kLgBlock), 0, st, A);
    LG_CK(who, hipGetLastError());
    LG_CK(who, hipEventRecord(s->ev[1], st));
    std::vector<unsigned long long> got(n_classes);
    uint32_t bad = 0;
    LG_CK(who, hipMemcpyAsync(got.data(), s->hist.p, (size_t)n_classes * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, st));
    LG_CK(who, hipMemcpyAsync(&bad, s->hbad.p, 4, hipMemcpyDeviceToHost, st));
    LG_CK(who, hipStreamSynchronize(st));
    hipEventElapsedTime(&s->ms[3], s->ev[0], s->ev[1]);
    if (bad) {
        c->err = std::string(who) + ": " + lg_hist_bad_name(bad);
        return DMX_E_INVALID;
    }
    if (const int brc = bounds_check(c, who)) return brc;
    for (uint32_t k = 0; k < n_classes; ++k) hist[k] += got[k];
    return DMX_OK;
}

extern "C" int dmx_pairhits_cross_host(const uint32_t* q, const uint32_t* t,
                                       const uint32_t* outcome, size_t n_pairs, size_t n_reads,
                                       const uint32_t* label, const int32_t* cap2, uint32_t* pair,
                                       uint32_t* d, uint8_t* rev, size_t cap, size_t* n) {
    const char* const who = "dmx_pairhits_cross_host";
    if (!n || (n_pairs && (!q || !t || !outcome)) || (n_reads && (!label || !cap2))) {
        set_process_error(std::string(who) + ": null argument");
        return DMX_E_INVALID;
    }
    *n = 0;
    std::string err;
    if (const int rc = lg_validate_edges(who, q, t, n_pairs, (uint32_t)std::min<size_t>(
                                             n_reads, DMX_LG_NONE), &err)) {
        set_process_error(err);
        return rc;
    }
    std::vector<size_t> keep;
    for (size_t i = 0; i < n_pairs; ++i) {
        if (outcome[i] == DMX_LG_NONE) continue;
        const int64_t c2 = cap2[t[i]];
        if (c2 >= 0 && (int64_t)(outcome[i] & kLgDist) <= c2 && label[q[i]] != label[t[i]])
            keep.push_back(i);
    }
    *n = keep.size();
    if (keep.empty()) return DMX_OK;
    if (cap < keep.size() || !pair || !d || !rev) {
        set_process_error(std::string(who) + ": room for " + std::to_string(cap) + " hits, " +
                          std::to_string(keep.size()) + " to return");
        return DMX_E_INVALID;
    }
    for (size_t k = 0; k < keep.size(); ++k) {
        pair[k] = (uint32_t)keep[k];
        d[k] = outcome[keep[k]] & kLgDist;
        rev[k] = (uint8_t)(outcome[keep[k]] >> 31);
    }
    return DMX_OK;
}

extern "C" int dmx_pairhits_cross(dmx_ctx* c, const uint32_t* label, const int32_t* cap2,
                                  uint32_t* pair, uint32_t* d, uint8_t* rev, size_t cap, size_t* n) {
    const char* const who = "dmx_pairhits_cross";
    if (!c) return DMX_E_INVALID;
    if (!n) {
        c->err = "dmx_pairhits_cross: null count";
        return DMX_E_INVALID;
    }
    *n = 0;
    if (!c->lg || !c->lg->valid) {
        c->err = "dmx_pairhits_cross: no dmx_pairhits since the last dmx_load";
        return DMX_E_INVALID;
    }
    LgState* s = c->lg;
    if (s->n_reads && (!label || !cap2)) {
        c->err = "dmx_pairhits_cross: null label or cap table";
        return DMX_E_INVALID;
    }
    if (!s->n_hits) return DMX_OK;
    hipStream_t st = c->stream;
    LG_CK(who, hipSetDevice(c->device));
    LG_CK(who, s->label.reserve(s->n_reads));
    LG_CK(who, s->cap2.reserve(s->n_reads));
    LG_CK(who, hipMemcpyAsync(s->label.p, label, s->n_reads * 4, hipMemcpyHostToDevice, st));
    LG_CK(who, hipMemcpyAsync(s->cap2.p, cap2, s->n_reads * 4, hipMemcpyHostToDevice, st));
    // the scatter writes no place at or past the room; the count is of all that are kept
    const size_t room = std::min<size_t>(cap, (size_t)s->n_hits);
    uint32_t total = 0;
    if (const int rc = lg_compact<kLgCross>(c, who, room, &total)) return rc;
    *n = total;
    if (!total) return DMX_OK;
    if (cap < total || !pair || !d || !rev) {
        c->err = "dmx_pairhits_cross: room for " + std::to_string(cap) + " hits, " +
                 std::to_string(total) + " to return";
        return DMX_E_INVALID;
    }
    LG_CK(who, hipMemcpy(pair, s->sel_a.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    LG_CK(who, hipMemcpy(d, s->sel_b.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    LG_CK(who, hipMemcpy(rev, s->sel_rev.p, (size_t)total, hipMemcpyDeviceToHost));
    return DMX_OK;
}

extern "C" int dmx_hitgroups_within_host(const uint32_t* q, const uint32_t* t,
                                         const uint32_t* outcome, size_t n_pairs, size_t n_reads,
                                         const uint32_t* tie2, const uint32_t* label,
                                         const uint32_t* xa, const uint32_t* xb, size_t n_extra,
                                         uint32_t n_nodes, uint32_t* labels_out) {
    const char* const who = "dmx_hitgroups_within_host";
    if ((n_pairs && (!q || !t || !outcome)) || (n_reads && (!tie2 || !label)) ||
        (n_nodes && !labels_out)) {
        set_process_error(std::string(who) + ": null argument (no dmx_pairhits_host outcomes?)");
        return DMX_E_INVALID;
    }
    std::string err;
    int rc = lg_within_args(who, n_reads, xa, xb, n_extra, n_nodes, &err);
    if (!rc) rc = lg_validate_edges(who, q, t, n_pairs, (uint32_t)n_reads, &err);
    if (rc) {
        set_process_error(err);
        return rc;
    }
    std::vector<uint32_t> a, b;
    for (size_t i = 0; i < n_pairs; ++i) {
        if (outcome[i] == DMX_LG_NONE) continue;
        const uint32_t lr = label[t[i]], tr = tie2[t[i]];
        if (lr != DMX_LG_NONE && label[q[i]] == lr && tr != DMX_LG_NONE &&
            (outcome[i] & kLgDist) <= tr) {
            a.push_back(q[i]);
            b.push_back(t[i]);
        }
    }
    a.insert(a.end(), xa, xa + n_extra);
    b.insert(b.end(), xb, xb + n_extra);
    lg_host_labels(a.data(), b.data(), a.size(), n_nodes, labels_out);
    return DMX_OK;
}

extern "C" int dmx_hitgroups_within(dmx_ctx* c, const uint32_t* tie2, const uint32_t* label,
                                    const uint32_t* xa, const uint32_t* xb, size_t n_extra,
                                    uint32_t n_nodes, uint32_t* labels_out) {
    const char* const who = "dmx_hitgroups_within";
    if (!c) return DMX_E_INVALID;
    if (!c->lg || !c->lg->valid) {
        c->err = "dmx_hitgroups_within: no dmx_pairhits since the last dmx_load";
        return DMX_E_INVALID;
    }
    LgState* s = c->lg;
    if (const int rc = lg_within_args(who, s->n_reads, xa, xb, n_extra, n_nodes, &c->err)) return rc;
    if (!n_nodes) return DMX_OK;
    if ((s->n_reads && (!tie2 || !label)) || !labels_out) {
        c->err = "dmx_hitgroups_within: null tie table, labels or output";
        return DMX_E_INVALID;
    }
    if (s->n_hits + n_extra > DMX_LG_MAX_PAIRS) {
        c->err = "dmx_hitgroups_within: at most " + std::to_string(DMX_LG_MAX_PAIRS) + " edges";
        return DMX_E_UNSUPPORTED;
    }
    hipStream_t st = c->stream;
    LG_CK(who, hipSetDevice(c->device));
    if (s->n_reads) {
        LG_CK(who, s->tie.reserve(s->n_reads));
        LG_CK(who, s->label.reserve(s->n_reads));
        LG_CK(who, hipMemcpyAsync(s->tie.p, tie2, s->n_reads * 4, hipMemcpyHostToDevice, st));
        LG_CK(who, hipMemcpyAsync(s->label.p, label, s->n_reads * 4, hipMemcpyHostToDevice, st));
    }
    // one edge buffer: the kept hits first, the caller's edges behind them
    const size_t room = (size_t)s->n_hits + n_extra;
    LG_CK(who, s->sel_a.reserve(room));
    LG_CK(who, s->sel_b.reserve(room));
    uint32_t n_edges = 0;
    if (const int rc = lg_compact<kLgWithin>(c, who, room, &n_edges)) return rc;
    if (n_edges > s->n_hits) {
        c->err = "dmx_hitgroups_within: the compaction kept more edges than there are hits";
        return DMX_E_STATE;
    }
    if (n_extra) {
        LG_CK(who, hipMemcpyAsync(s->sel_a.p + n_edges, xa, n_extra * 4, hipMemcpyHostToDevice, st));
        LG_CK(who, hipMemcpyAsync(s->sel_b.p + n_edges, xb, n_extra * 4, hipMemcpyHostToDevice, st));
    }
    if (const int rc = lg_components(c, who, s->sel_a.p, s->sel_b.p, n_edges + (uint32_t)n_extra,
                                     n_nodes))
        return rc;
    LG_CK(who, hipMemcpy(labels_out, s->labels.p, (size_t)n_nodes * 4, hipMemcpyDeviceToHost));
    return DMX_OK;
}

extern "C" int dmx_hitgroups_stats(dmx_ctx* c, float* ms, int n_ms) {
    if (!c) return DMX_E_INVALID;
    for (int k = 0; k < n_ms && k < 4 && ms; ++k) ms[k] = c->lg ? c->lg->ms[k] : 0.f;
    return c->lg ? c->lg->rounds : 0;
}
