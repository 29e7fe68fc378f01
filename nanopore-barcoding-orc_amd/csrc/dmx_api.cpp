// dmx_api.cpp — C-ABI of libdmx (include/dmx.h): context, panels, packing, batch execution.
//
// Panel rules restate cutadapt 4.9 adapter construction (parser.py / adapters.py, not vendored
// in /root/reference): name/sequence come from the FASTA, sequences are
// uppercase with U->T, adapter wildcards are enabled iff a non-ACGT character is present,
// k = int(max_error_rate * m), acceptance `cost <= effective_length * max_error_rate` in IEEE
// double with effective length excluding adapter N's, minimum overlap -O (default 3).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "dmx_internal.h"
#include "pack.h"

using namespace dmx;

#define CK(call)                                                                        \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            c->err = std::string(#call) + ": " + hipGetErrorString(e_);                 \
            return DMX_E_HIP;                                                           \
        }                                                                               \
    } while (0)

namespace {

constexpr int kMinFilterLen = 10; // shortest shared suffix worth a filter pass
// kGuardWords (dmx_device.h): zeroed words before/after the packed device buffers

uint8_t iupac_mask(char ch) {
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

// (A0+1)(A1+1) per-bin counts + 2 RC counts (include/dmx.h dmx_counts)
size_t counts_size(const Ctx* c) {
    const size_t a1 = c->mode == DMX_MODE_SINGLE ? 0 : (size_t)c->panel[1].n_all;
    return ((size_t)c->panel[0].n_all + 1) * (a1 + 1) + 2;
}

// dmx_stats' flag bits (include/dmx.h): lists that overflowed are grown and the pipeline run again
// (exec_checked); the other two are internal errors.
enum StatFlag {
    kFlagClusters = 1, kFlagTraceback = 2, kFlagWindows = 4, kFlagCands = 8, kFlagFilter = 16,
    kFlagsOverflow = kFlagClusters | kFlagWindows | kFlagCands,
    kFlagsInternal = kFlagTraceback | kFlagFilter
};

// The window list and what is sized with it: the verified windows, 4 screen tasks per window
// record, the filter tasks.
int reserve_windows(Ctx* c, size_t n) {
    CK(c->d_win.reserve(n));
    CK(c->d_win2.reserve(n));
    CK(c->d_tasks.reserve(4 * n));
    CK(c->d_ftask.reserve(n));
    return DMX_OK;
}

int reserve_cands(Ctx* c, size_t n) {
    for (int r = 0; r < 2; ++r)
        for (int l = 0; l < 2; ++l) CK(c->d_cand[r][l].reserve(n));
    return DMX_OK;
}

int reserve_clusters(Ctx* c, size_t n) {
    for (int r = 0; r < 2; ++r) {
        CK(c->d_cl[r].reserve(n));
        CK(c->d_outc[r].reserve(n));
    }
    return DMX_OK;
}

// Room for the current batch, mode and panels.  Every capacity is read from its buffers, so a
// buffer whose allocation failed in an earlier call is allocated again here.
int ensure_pipeline(Ctx* c) {
    // a view run has one item, winner slot and result per view, and views may outnumber the reads
    const size_t n = c->views_on ? std::max(c->n_reads, c->n_views) : c->n_reads;
    const bool linked = c->mode == DMX_MODE_LINKED;
    const size_t slots0 = linked ? n * (size_t)std::max(1, c->panel[0].n) : n;
    const size_t items = linked ? slots0 : n;
    // non-linked rounds may need one winner slot per (item, orientation): see orient_slot
    const size_t need = std::max(slots0, items) * (linked ? 1 : 2);
    CK(c->in.res.reserve(n));   // the resident input set's result array
    for (int r = 0; r < 2; ++r) {
        CK(c->d_winner[r].reserve(need));
        CK(c->d_lb[r].reserve(need));
    }
    CK(c->d_linked.reserve(n));
    // per-slot origins: only for the rounds this mode runs in ring mode (a band round's winner
    // key carries its origin), sized like the winner slots
    for (int r = 0; r < 2; ++r) {
        if ((r == 1 && c->mode == DMX_MODE_SINGLE) || band_round(c, r)) continue;
        CK(c->d_origin[r].reserve(slot_cap(c)));
    }
    // The item list is sized by its own need: a linked batch has reads x pairs items, which can
    // exceed what an earlier two-round batch needed (reads) while its winner slots (2 x reads)
    // still suffice.
    CK(c->d_items.reserve(items));
    c->item_cap = items;
    if (c->views_on && c->mode != DMX_MODE_SINGLE) CK(c->d_item_src.reserve(items));
    int rc;
    if ((rc = reserve_clusters(c, 4 * std::max(slots0, n) + 65536))) return rc;
    if ((rc = reserve_cands(c, 4 * std::max(slots0, n) + 65536))) return rc;
    if ((rc = reserve_windows(c, 4 * 2 * std::max(slots0, n) + 65536))) return rc;
    const size_t nc = counts_size(c);
    c->n_counts = 0;   // until there is room: dmx_counts and the all-reduce copy n_counts words
    CK(c->d_counts.reserve(nc));
    c->n_counts = nc;
    return DMX_OK;
}

// The pipeline counters (dmx_device.h CounterSlot) with the sharded lists' totals (records kept,
// over every shard) folded into their slots.  *ovf: flag bits of overflowed lists.
hipError_t read_counters(Ctx* c, uint32_t* cnt, int* ovf) {
    hipError_t e =
        hipMemcpy(cnt, c->d_counters.p, kCntCount * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    std::vector<uint32_t> sh((size_t)kShLists * kShards * kShardStride);
    e = hipMemcpy(sh.data(), c->d_shard.p, sh.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    // each list of ShardList: where its run of lists starts, the slot that takes the first of
    // them, its capacity and the flag an overflow raises
    const struct {
        int first, slot;
        size_t cap;
        int flag;
    } lists[] = {{kShWin, kCntWindows, win_cap(c), kFlagWindows},
                 {kShWin2, kCntVerified, win_cap(c), kFlagWindows},
                 {kShTasks, kCntTasks, task_cap(c), kFlagWindows},
                 {kShCand, kCntCands, cand_cap(c), kFlagCands},
                 {kShFtask, kCntFtasks, win_cap(c), kFlagWindows}};
    constexpr int n_lists = (int)(sizeof lists / sizeof *lists);
    static_assert(kShWin == 0 && kShWin < kShWin2 && kShWin2 < kShTasks && kShTasks < kShCand &&
                      kShCand < kShFtask && kShFtask < kShLists,
                  "lists[] follows ShardList in ascending order");
    int o = 0;
    for (int x = 0; x < kShLists; ++x) {
        int k = 0;
        while (k + 1 < n_lists && x >= lists[k + 1].first) ++k;
        const uint32_t scap = (uint32_t)(lists[k].cap / kShards);
        uint64_t t = 0;
        for (int s = 0; s < kShards; ++s) {
            const uint32_t v = sh[(size_t)(x * kShards + s) * kShardStride];
            t += std::min(v, scap);
            if (v > scap) o |= lists[k].flag;
        }
        cnt[lists[k].slot + (x - lists[k].first)] = (uint32_t)t;
    }
    if (ovf) *ovf = o;
    return hipSuccess;
}

// An overflowed list doubles (exec_checked).
int grow_cands(Ctx* c) { return reserve_cands(c, cand_cap(c) * 2); }
int grow_windows(Ctx* c) { return reserve_windows(c, win_cap(c) * 2); }
int grow_clusters(Ctx* c) { return reserve_clusters(c, cl_cap(c) * 2); }

}  // namespace

namespace dmx {

namespace {
std::mutex g_proc_err_mu;
std::string g_proc_err;
}  // namespace

void set_process_error(const std::string& msg) {
    std::lock_guard<std::mutex> lk(g_proc_err_mu);
    g_proc_err = msg;
}

std::string process_error() {
    std::lock_guard<std::mutex> lk(g_proc_err_mu);
    return g_proc_err;
}

// The kernels' reach around a view, per panel.  A 16-position gather at view
// position p physically loads two aligned u32 words, i.e. view positions [p - 16, p + 32) on
// either strand; whole-block loads (ViewBlocks: filter, verify) cover [p - 63, p + 64 s + 127]
// for s 64-position stretches from p.  Per kernel, the first gather position before the view:
//   filter, verify, window scan, scan, resolve, chop: >= 0 (their ranges start at column 0);
//   index screen: x1 - 15 >= -(m_max - pre_len) - kf - 15 (the I_a band's warm-up, both the
//     last-row test and the 3' last-column test; D' only lowers D there);
//   edge bands: dx - H >= -(m + 7) (end cell (i, j) with j >= 0, H <= 7 diagonals);
// and past the view end: ViewBlocks' in-flight block (<= 190 nt), fetch16 prefetches (<= 54).
// Positions before -kViewReachPre are read at -kViewReachPre (fetch16s).  A read on strand 1
// maps view positions past its end to nt before its offset, and positions before the view to
// nt past its end, so both directions must fit either side of the buffer.
PanelReach panel_reach(const HostPanel& hp, const DevPanel& dp) {
    int m_max = 0;
    bool band = true;
    for (int a = 0; a < hp.n; ++a) {
        m_max = std::max(m_max, (int)hp.ad[a].m);
        band &= hp.ad[a].kk <= 7;
    }
    PanelReach r;
    int pre = 63 + 16;   // ViewBlocks' floor to a block, fetch16's floor to a word
    if (hp.screen) pre = std::max(pre, m_max - dp.pre_len + dp.kf + 15 + 16);
    if (band) pre = std::max(pre, m_max + 7 + 16);
    r.pre_raw = pre;
    r.pre = std::min(pre, std::max(63 + 16, kViewReachPre + 16));
    r.post = 63 + 64 + 63;   // ViewBlocks: the block after the last stretch's two, in flight
    // strand 0: before the view -> before the offset; strand 1: before the view -> past the end
    r.need_pre = std::max(r.pre, r.post) - kMinOffset;
    r.need_post = std::max(r.pre, r.post) + 32 - kMinTail;   // (+ the 8-byte word pair)
    return r;
}

int reset_counts(Ctx* c) {
    CK(hipSetDevice(c->device));
    const size_t nc = counts_size(c);
    c->n_counts = 0;   // until there is room (ensure_pipeline)
    CK(c->d_counts.reserve(nc));
    c->n_counts = nc;
    CK(hipMemsetAsync(c->d_counts.p, 0, nc * sizeof(unsigned long long), c->stream));
    CK(hipStreamSynchronize(c->stream));
    c->counts_reduced = false;
    return DMX_OK;
}

int views_reserve(Ctx* c, size_t n) {
    CK(hipSetDevice(c->device));
    ++c->view_gen;   // the list is about to change: an earlier exec's items are no longer d_views
    CK(c->d_view_n.reserve(1));
    if (c->d_views.cap < std::max<size_t>(n, 1)) {
        // the last exec may still read the old list
        CK(hipStreamSynchronize(c->stream));
        CK(c->d_views.reserve(n));
    }
    return DMX_OK;
}

bool env_on(const char* name) {
    const char* e = std::getenv(name);
    return e && e[0] == '1';
}

PanelSwitches panel_switches_env() {
    PanelSwitches s;
    s.no_filter = env_on("DMX_NO_FILTER");
    s.no_verify = env_on("DMX_NO_VERIFY");
    s.no_pieces = env_on("DMX_NO_PIECES");
    s.near_all = env_on("DMX_NEAR_ALL");   // (DevPanel::near_shared = -1)
    return s;
}

}  // namespace dmx


extern "C" {

int dmx_abi_version(void) { return DMX_ABI_VERSION; }

int dmx_open(int device, dmx_ctx** out) {
    if (!out) return DMX_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return DMX_E_HIP;
    dmx_ctx* c = new dmx_ctx();
    c->device = device;
    c->sw = panel_switches_env();
    const char* rs = std::getenv("DMX_RESOLVE");
    c->force_ring = rs && std::strcmp(rs, "ring") == 0;
    c->no_screen = env_on("DMX_NO_SCREEN");   // A/B: no index screen before the window scan
    c->screen_v1 = env_on("DMX_SCREEN_V1");   // A/B: the unpacked index screen
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        dmx_close(c);
        return DMX_E_HIP;
    }
    hipError_t e = hipSuccess;
    bool nomem = false;   // which of the two failed: an event, or an allocation
    for (auto& ev : c->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    const auto room = [&](auto& buf, size_t n) {
        if (e == hipSuccess && (e = buf.reserve(n)) != hipSuccess) nomem = true;
    };
    for (int r = 0; r < 2; ++r) {
        room(c->d_panel[r], 1);
        room(c->d_pieces[r], 1);
    }
    room(c->d_counters, kCntCount);
    room(c->d_shard, (size_t)kShLists * kShards * kShardStride);
    if (e != hipSuccess) {
        dmx_close(c);   // what was made so far goes with the context
        return nomem ? DMX_E_NOMEM : DMX_E_HIP;
    }
    *out = c;
    return DMX_OK;
}

// What has an order: the device's work ends, the feature states and the communicator go, then
// the events and streams.  Every device buffer is freed with the context that owns it.
void dmx_close(dmx_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    chop_release(c);
    pd_release(c);
    lg_release(c);
    comm_release(c);
    for (auto& e : c->ev)
        if (e) hipEventDestroy(e);
    if (c->cstream) hipStreamDestroy(c->cstream);
    if (c->dstream) hipStreamDestroy(c->dstream);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

const char* dmx_last_error(dmx_ctx* c) {
    if (c) return c->err.c_str();
    // no context: the last context-free failure (thread-local copy: the pointer stays valid
    // until this thread's next call)
    thread_local std::string msg;
    msg = dmx::process_error();
    if (msg.empty()) msg = "null context";
    return msg.c_str();
}

int dmx_set_mode(dmx_ctx* c, int mode) {
    if (!c) return DMX_E_INVALID;
    if (mode != DMX_MODE_SINGLE && mode != DMX_MODE_TWO_ROUND && mode != DMX_MODE_LINKED) {
        c->err = "unknown mode";
        return DMX_E_INVALID;
    }
    c->mode = mode;
    ++c->panel_gen;
    return DMX_OK;
}

static int set_panel_impl(dmx_ctx* c, int round, const char* const* seqs, const int* lens,
                          const int* wheres, int n, double max_errors, int min_overlap,
                          int flags);

static int set_panel_ends(dmx_ctx* c, int round, const char* const* seqs, const int* lens,
                          const int* wheres, const int* min_overlaps, int n, double max_errors,
                          int min_overlap, int rc);

constexpr int kRestrictBits = DMX_ANCHORED | DMX_NONINTERNAL;

// A per-adapter `where`: one of DMX_FRONT / DMX_BACK, at most one of the restricted bits.
static bool where_valid(int w) {
    const int side = w & (DMX_FRONT | DMX_BACK);
    return (w & ~(DMX_FRONT | DMX_BACK | kRestrictBits)) == 0 &&
           (side == DMX_FRONT || side == DMX_BACK) && (w & kRestrictBits) != kRestrictBits;
}

int dmx_set_panel(dmx_ctx* c, int round, const char* const* seqs, const int* lens, int n,
                  double max_errors, int min_overlap, int flags) {
    if (!(flags & kRestrictBits))
        return set_panel_impl(c, round, seqs, lens, nullptr, n, max_errors, min_overlap, flags);
    if (!c || n <= 0 || n > kMaxAdapters) return DMX_E_INVALID;
    if (!where_valid(flags & ~DMX_RC)) {
        c->err = "panel flags: one of DMX_FRONT / DMX_BACK, at most one of DMX_ANCHORED / "
                 "DMX_NONINTERNAL";
        return DMX_E_INVALID;
    }
    int wheres[kMaxAdapters];
    for (int a = 0; a < n; ++a) wheres[a] = flags & ~DMX_RC;
    return set_panel_ends(c, round, seqs, lens, wheres, nullptr, n, max_errors, min_overlap,
                          (flags & DMX_RC) ? 1 : 0);
}

int dmx_set_panel_ex(dmx_ctx* c, int round, const char* const* seqs, const int* lens,
                     const int* wheres, const int* min_overlaps, int n, double max_errors,
                     int min_overlap, int rc) {
    if (!c || !wheres || !seqs || !lens) return DMX_E_INVALID;
    if (n <= 0 || n > kMaxAdapters) {
        c->err = "panel must hold 1..64 adapters";
        return DMX_E_INVALID;
    }
    bool plain = true;
    for (int a = 0; a < n; ++a) {
        if (!where_valid(wheres[a])) {
            c->err = "adapter " + std::to_string(a) + ": where must be DMX_FRONT or DMX_BACK, "
                     "alone or with one of DMX_ANCHORED / DMX_NONINTERNAL";
            return DMX_E_INVALID;
        }
        plain &= !(wheres[a] & kRestrictBits) && (!min_overlaps || min_overlaps[a] == min_overlap);
    }
    if (plain)   // nothing new asked for: dmx_set_panel_mixed itself
        return set_panel_impl(c, round, seqs, lens, wheres, n, max_errors, min_overlap,
                              DMX_FRONT | (rc ? DMX_RC : 0));
    return set_panel_ends(c, round, seqs, lens, wheres, min_overlaps, n, max_errors, min_overlap,
                          rc);
}

int dmx_set_panel_mixed(dmx_ctx* c, int round, const char* const* seqs, const int* lens,
                        const int* wheres, int n, double max_errors, int min_overlap, int rc) {
    if (!wheres) return DMX_E_INVALID;
    bool plain = true;
    for (int a = 0; a < n; ++a) plain &= wheres[a] == DMX_FRONT || wheres[a] == DMX_BACK;
    if (!plain) {
        for (int a = 0; a < n; ++a)
            if (!where_valid(wheres[a])) return DMX_E_INVALID;
        return dmx_set_panel_ex(c, round, seqs, lens, wheres, nullptr, n, max_errors, min_overlap,
                                rc);
    }
    return set_panel_impl(c, round, seqs, lens, wheres, n, max_errors, min_overlap,
                          DMX_FRONT | (rc ? DMX_RC : 0));
}

// Piece screen tables (dmx_device.h DevPieces).  Adapter a of an ACGT panel
// with K_a = acc[m_a] >= 0 (the largest accepted cost of an alignment covering all m_a rows) is
// cut into K_a + 1 disjoint row pieces of near-equal length (at most 16 nt each: a piece may be
// any sub-range of its rows).  An accepted full alignment has <= K_a edits, so some piece is
// aligned without one: an exact copy in the read, after which the alignment ends within
// (m_a - r1) +- K_a columns (r1 = the piece's end row).  Pieces are deduplicated per
// (codes, length, orientation) with the union of their end ranges; every piece contributes its
// 8-mers at offsets 0 .. s-1 (s = the sampling stride), so a copy starting anywhere has one of
// them at a sampled position.  Off (piece_step 0) for IUPAC panels, pieces shorter than 8 nt,
// tables that do not fit, or DMX_NO_PIECES=1.
static void build_pieces(const PanelSwitches& sw, const char* const* seqs, const int* lens, int n,
                         HostPanel& hp) {
    hp.piece_step = 0;
    DevPieces& Q = hp.pieces;
    memset(&Q, 0, sizeof(Q));
    if (!hp.filter || sw.no_pieces) return;
    struct Pc {
        uint32_t val;
        int len, o, dlo, dhi;
    };
    std::vector<Pc> pcs;
    auto code = [](char ch) -> int {
        switch (ch) {
            case 'A': return 0;
            case 'C': return 1;
            case 'G': return 2;
            case 'T': return 3;
            default: return -1;
        }
    };
    int minlen = 64;
    for (int a = 0; a < n; ++a) {
        const int m = lens[a];
        for (int i = 0; i < m; ++i)
            if (code(seqs[a][i]) < 0) return;   // IUPAC adapter: the full filter pass
        const int K = hp.ad[a].acc[m];
        if (K < 0) continue;                    // never accepted with every row aligned
        const int np = K + 1;
        if (m / np < kPieceK) return;
        for (int p = 0; p < np; ++p) {
            const int r0 = p * m / np, r1 = (p + 1) * m / np;
            const int len = std::min(16, r1 - r0), re = r0 + len;
            minlen = std::min(minlen, len);
            for (int o = 0; o < hp.n_orient; ++o) {
                uint32_t v = 0;
                for (int i = 0; i < len; ++i) {
                    // orientation 1: the reverse complement, as it appears in the view-0 codes
                    const int cd = o == 0 ? code(seqs[a][r0 + i]) : 3 - code(seqs[a][re - 1 - i]);
                    v |= (uint32_t)cd << (2 * i);
                }
                pcs.push_back({v, len, o, (m - re) - K, (m - re) + K});
            }
        }
    }
    // dedup by (codes, length, orientation), union of the end ranges
    std::sort(pcs.begin(), pcs.end(), [](const Pc& x, const Pc& y) {
        return std::make_tuple(x.val, x.len, x.o) < std::make_tuple(y.val, y.len, y.o);
    });
    std::vector<Pc> uq;
    for (const Pc& p : pcs) {
        if (!uq.empty() && uq.back().val == p.val && uq.back().len == p.len && uq.back().o == p.o) {
            uq.back().dlo = std::min(uq.back().dlo, p.dlo);
            uq.back().dhi = std::max(uq.back().dhi, p.dhi);
        } else {
            uq.push_back(p);
        }
    }
    if (uq.empty() || (int)uq.size() > kMaxPieceEntries) return;
    int step = minlen - kPieceK + 1 >= 4 ? 4 : (minlen - kPieceK + 1 >= 2 ? 2 : 1);
    if (const char* e = std::getenv("DMX_PIECE_STEP"))   // A/B: a denser sampling
        step = std::min(step, std::max(1, std::atoi(e)));
    while (step > 1 && (int)uq.size() * step > kMaxPieceEntries) step /= 2;
    if ((int)uq.size() * step > kMaxPieceEntries) return;
    // Sampled offsets: any `step` consecutive offsets j0 .. j0+step-1 of a piece cover every copy
    // (one of its 8-mers sits at a sampled position).  Per piece take the window whose 8-mers the
    // fewest other pieces share (pieces of different adapters that overlap a shared constant
    // block share 8-mers, and every entry of a key is checked on each sampled hit of it).  The
    // offset is a 2-bit field that both screens read the copy back with (the flat scan holds the
    // codes of nt [X - 3, X + 29) per sampled nt X), so the window ends at offset kPieceMaxOff.
    std::map<uint32_t, int> mult;
    for (const Pc& x : uq)
        for (int off = 0; off + kPieceK <= x.len; ++off) ++mult[(x.val >> (2 * off)) & 0xFFFFu];
    std::vector<std::pair<uint32_t, uint64_t>> ents;   // (8-mer, entry)
    int lo_off = 1 << 20, dlo_min = 0, len_max = 0, dhi_max = 0;
    bool any1 = false;
    for (const Pc& x : uq) {
        int best = 0, bcost = 1 << 30;
        for (int j0 = 0; j0 + step - 1 <= kPieceMaxOff && j0 + step - 1 + kPieceK <= x.len; ++j0) {
            int cost = 0;
            for (int off = j0; off < j0 + step; ++off) cost += mult[(x.val >> (2 * off)) & 0xFFFFu];
            if (cost < bcost) bcost = cost, best = j0;
        }
        for (int off = best; off < best + step; ++off)
            ents.push_back({(x.val >> (2 * off)) & 0xFFFFu,
                            piece_entry(x.val, x.len, x.o, off, x.dlo, x.dhi)});
        if (x.o == 0) {
            lo_off = std::min(lo_off, x.len + x.dlo - 1);
        } else {
            dlo_min = any1 ? std::min(dlo_min, x.dlo) : x.dlo;
            any1 = true;
        }
        len_max = std::max(len_max, x.len);
        dhi_max = std::max(dhi_max, x.dhi);
    }
    std::sort(ents.begin(), ents.end());
    int nk = 0;
    for (size_t e = 0; e < ents.size(); ++e) {
        if (e == 0 || ents[e].first != ents[e - 1].first) {
            Q.key[nk++] = (uint32_t)e;
            piece_pair_add(Q.pair, ents[e].first);
        }
        Q.key[nk - 1] += 1u << 16;
        Q.entry[e] = ents[e].second;
    }
    piece_rank_fill(Q);
    int reach = 0;   // FRONT: alignments entering at column 0 (rows skipped) end before it
    if (hp.ad[0].where == kFront)
        for (int a = 0; a < n; ++a)
            for (int L = 1; L <= (int)hp.ad[a].m; ++L)
                if (hp.ad[a].acc[L] >= 0) reach = std::max(reach, L + (int)hp.ad[a].acc[L]);
    // every cell a part can mark lies within 64 cells of its mask base (pscreen_kernel)
    int pmax = (992 - std::max(len_max + dhi_max, dhi_max - dlo_min)) / 16 * 16;
    pmax = std::min(pmax, 768);
    if (const char* e = std::getenv("DMX_PIECE_PART"))   // A/B: positions per screen lane
        pmax = std::min(pmax, std::max(64, std::atoi(e) / 16 * 16));
    if (pmax < 64) return;
    Q.on = 1;
    Q.step = step;
    Q.n_pieces = (int)uq.size();
    Q.n_keys = nk;
    Q.n_entries = (int)ents.size();
    Q.front_reach = reach;
    Q.part_max = pmax;
    Q.lo_off = std::max(0, lo_off == (1 << 20) ? 0 : lo_off);
    Q.dlo_min = dlo_min;
    hp.piece_step = step;
}

// The host and device forms of a panel (parser.py / adapters.py rules above), the filter /
// verification / screen blocks and the reach check.  It needs no context: the switches and where
// to leave the text of an error are all it takes (the dmx_panel_* information calls run it).
static int build_panel(const PanelSwitches& sw, std::string& err, const char* const* seqs,
                       const int* lens, const int* wheres, int n, double max_errors,
                       int min_overlap, int flags, HostPanel& hp, DevPanel& dp) {
    if (!seqs || !lens) return DMX_E_INVALID;
    if (n <= 0 || n > kMaxAdapters) {
        err = "panel must hold 1..64 adapters";
        return DMX_E_INVALID;
    }
    if (!(flags & (DMX_FRONT | DMX_BACK)) || ((flags & DMX_FRONT) && (flags & DMX_BACK))) {
        err = "panel flags need exactly one of DMX_FRONT / DMX_BACK";
        return DMX_E_INVALID;
    }
    if (!(max_errors >= 0.0)) {
        err = "max_errors must be >= 0";
        return DMX_E_INVALID;
    }
    hp = HostPanel();
    hp.n = n;
    hp.n_orient = (flags & DMX_RC) ? 2 : 1;
    for (int a = 0; a < n; ++a) {
        const int m = lens[a];
        if (m <= 0 || m > kMaxLen) {
            err = "adapter length must be 1..64 (one 64-bit Myers word)";
            return DMX_E_UNSUPPORTED;
        }
        DevAdapter& ad = hp.ad[a];
        memset(&ad, 0, sizeof(ad));
        bool wild = false;
        for (int i = 0; i < m; ++i) {
            const char ch = seqs[a][i];
            if (!iupac_mask(ch)) {
                err = std::string("adapter character not IUPAC uppercase: ") + ch;
                return DMX_E_INVALID;
            }
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') wild = true;
        }
        const double rate = max_errors >= 1.0 ? max_errors / (double)m : max_errors;
        const int k = (int)(rate * m);
        if (m + k + 2 + 4 > kRingSmall) hp.ring_small = false;
        if (m + k + 2 + 4 > kRingLarge) {
            err = "error rate too high for the resolve window (m + k + 6 > 128)";
            return DMX_E_UNSUPPORTED;
        }
        int ncount[kMaxLen + 1];
        int nc = 0;
        for (int i = 0; i < m; ++i) {
            ncount[i] = nc;
            if (seqs[a][i] == 'N') ++nc;
        }
        ncount[m] = nc;
        const int eff_len = wild ? m - nc : m;
        if (eff_len == 0) {
            err = "adapter consists only of N wildcards";
            return DMX_E_INVALID;
        }
        for (int i = 0; i < m; ++i) {
            // Adapter wildcards: IUPAC mask vs read base; otherwise ASCII equality. Read codes
            // 4..7 (any non-ACGT byte) match nothing in either mode.
            const uint8_t mask = wild ? iupac_mask(seqs[a][i]) : iupac_mask(seqs[a][i]);
            for (int code = 0; code < 4; ++code)
                if (mask & (1u << code)) ad.peq[code] |= 1ull << i;
        }
        int kk = -1;
        for (int L = 0; L < 72; ++L) {
            int allow = -1;
            if (L <= m && L >= min_overlap) {
                const int eff = wild ? (L < m ? L - ncount[L] : eff_len) : L;
                const double lim = (double)eff * rate;
                for (int cst = 0; cst <= 127 && (double)cst <= lim; ++cst) allow = cst;
            }
            ad.acc[L] = (int8_t)allow;
            kk = std::max(kk, allow);
            ad.pacc[L] = (int8_t)kk;
        }
        // score = aligned adapter length - 2 cost - (adapter chars facing a gap) >= L - 3 cost
        for (int L = 1; L < 72; ++L)
            if (ad.acc[L] >= 0 && L - 3 * (int)ad.acc[L] <= 0) hp.nonpos = true;
        ad.m = (uint8_t)m;
        ad.k = (uint8_t)k;
        ad.kk = (int8_t)std::min(kk, k);
        ad.where = wheres ? (wheres[a] == DMX_FRONT ? kFront : kBack)
                          : ((flags & DMX_FRONT) ? kFront : kBack);
    }
    hp.set = true;
    memset(&dp, 0, sizeof(dp));
    dp.n_adapters = hp.n;
    dp.n_orient = hp.n_orient;
    dp.where = hp.ad[0].where;
    for (int a = 1; a < n; ++a)
        if (hp.ad[a].where != hp.ad[0].where) dp.where = 0;
    dp.near_shared = -1;
    // Shared-suffix filter block: the longest suffix common to every adapter (<= 32 chars).
    int common = lens[0];
    for (int a = 1; a < n; ++a) {
        int l = 0;
        while (l < common && l < lens[a] &&
               seqs[a][lens[a] - 1 - l] == seqs[0][lens[0] - 1 - l])
            ++l;
        common = l;
    }
    int flen = std::min(common, 32);
    if (const char* fm = std::getenv("DMX_FILTER_MAXLEN"))   // A/B: a shorter suffix block
        flen = std::min(flen, std::max(1, std::atoi(fm)));
    bool uniform = true;
    for (int a = 1; a < n; ++a) uniform &= hp.ad[a].where == hp.ad[0].where;
    int kf_all = -1;
    for (int a = 0; a < n; ++a) kf_all = std::max(kf_all, (int)hp.ad[a].kk);
    // The filter's first 64 columns per segment carry per-column thresholds: the warm-up
    // W = flen + kf and the near-start acceptance pf[j + kf] < kf must both end within them.
    int8_t pf_all[72];
    for (int L = 0; L < 72; ++L) {
        pf_all[L] = -1;
        for (int a = 0; a < n; ++a) pf_all[L] = std::max(pf_all[L], hp.ad[a].pacc[L]);
    }
    const int kf_far = std::min(kf_all, (int)pf_all[71]);
    bool near_ok = true;
    for (int j = 65; j + kf_all < 71; ++j) near_ok &= pf_all[j + kf_all] >= kf_far;
    hp.filter = uniform && flen >= kMinFilterLen && flen + kf_all <= 64 && near_ok &&
                !sw.no_filter;
    if (hp.filter) {
        dp.filter_len = flen;
        int slen = flen;
        if (const char* fs = std::getenv("DMX_FILTER_SCANLEN"))   // A/B: scan a shorter suffix
            slen = std::min(flen, std::max(kMinFilterLen, std::atoi(fs)));
        dp.scan_len = slen;
        // the scanned rows in the top slen bits (last row = bit 31); the rows below match
        // every code, N included, so they stay at cost 0 like row 0 (filter_kernel)
        const int pad = 32 - slen;
        for (int code = 0; code < 8; ++code)
            dp.filter_peq[code] = pad > 0 ? (1u << pad) - 1u : 0u;
        const char* blk = seqs[0] + lens[0] - slen;
        for (int i = 0; i < slen; ++i) {
            const uint8_t mask = iupac_mask(blk[i]);
            for (int code = 0; code < 4; ++code)
                if (mask & (1u << code)) dp.filter_peq[code] |= 1u << (pad + i);
        }
        int kf = -1, mk = 0;
        for (int L = 0; L < 72; ++L) dp.pf[L] = -1;
        for (int a = 0; a < n; ++a) {
            kf = std::max(kf, (int)hp.ad[a].kk);
            mk = std::max(mk, (int)hp.ad[a].m + (int)hp.ad[a].k + 1);
            for (int L = 0; L < 72; ++L) dp.pf[L] = std::max(dp.pf[L], hp.ad[a].pacc[L]);
        }
        dp.kf = kf;
        dp.max_mk = mk;
        // clean flags: the exact stages read a window's view from j1 - (m + k
        // + 1) (window scan) and j1 - (m + 7) (band DP); off when that exceeds 128 positions
        int reach = 0;
        for (int a = 0; a < n; ++a)
            reach = std::max(reach, (int)hp.ad[a].m + std::max((int)hp.ad[a].k + 1, 7));
        reach = (reach + 15) / 16 * 16;
        dp.clean_reach = reach <= 128 && !std::getenv("DMX_NO_CLEAN") ? reach : 0;
        // Near-start cells inside the shared suffix.  A FRONT last-row cell
        // (m_a, j) of cost d <= kk_a with j + kf <= flen < m_a: every alignment of that cost ending
        // there starts at column 0 and covers at most j + d <= flen rows, the last rows of the
        // adapter, all of them rows of S (a start in row 0 needs j >= m_a - d).  D, the band's
        // score and its aligned length are then the same for every adapter, and the acceptance
        // lookups pacc[min(m, j + d)], acc[j - d], acc[rows] stay at indices <= flen.  Where the
        // tables agree there, every adapter accepts the cell alike and the lowest index wins the
        // slot (make_key_o): adapters > 0 skip the columns j <= near_shared of a near piece.
        {
            const int js = flen - kf;
            bool same = dp.where == kFront && js >= 1 && !sw.near_all;
            for (int a = 0; a < n && same; ++a) {
                same &= lens[a] > flen;
                for (int L = 0; L <= flen; ++L)
                    same &= hp.ad[a].acc[L] == hp.ad[0].acc[L] &&
                            hp.ad[a].pacc[L] == hp.ad[0].pacc[L];
            }
            if (same) dp.near_shared = js;
        }

        // shared prefix for the verification pass
        int pre = lens[0];
        int mmin = 1 << 30, mmax = 0;
        for (int a = 0; a < n; ++a) {
            int l = 0;
            while (l < pre && l < lens[a] && seqs[a][l] == seqs[0][l]) ++l;
            pre = l;
            mmin = std::min(mmin, lens[a]);
            mmax = std::max(mmax, lens[a]);
        }
        pre = std::min(pre, 32);
        if (pre >= kMinFilterLen && pre + flen <= mmin && !sw.no_verify) {
            hp.verify = true;
            dp.pre_len = pre;
            dp.off_min = mmin - pre;
            dp.off_max = mmax - pre;
            dp.m_max = mmax;
            // index screen: every adapter's middle block I_a = rows [pre, m - flen) fits a
            // 32-bit word
            int lmin = 64, lmx = 0, js = 0;
            for (int a = 0; a < n; ++a) {
                lmin = std::min(lmin, lens[a] - pre - flen);
                lmx = std::max(lmx, lens[a] - pre - flen);
                js = std::max(js, lens[a] - pre + (int)hp.ad[a].kk);
            }
            hp.screen = lmin >= 1 && lmx <= 32;
            dp.jsplit = js;
            bool shared = true;   // rows <= pre: identical acceptance for every adapter
            for (int a = 1; a < n; ++a)
                for (int L = 0; L <= pre; ++L) shared &= hp.ad[a].acc[L] == hp.ad[0].acc[L];
            dp.pshared = shared ? 1 : 0;
            for (int i = 0; i < pre; ++i) {
                const uint8_t mask = iupac_mask(seqs[0][i]);
                for (int code = 0; code < 4; ++code)
                    if (mask & (1u << code)) dp.pre_peq[code] |= 1u << i;
            }
        }
    }
    // Every gather of every kernel must stay inside the device guard words for every offset the
    // loaders accept (>= kMinOffset nt, >= kMinTail nt before the end): the deepest warm-up
    // before a view (index screen, edge bands), clamped at -kViewReachPre, and the block loads
    // past it.  Adapters of <= 64 nt always fit; the check keeps it explicit.
    build_pieces(sw, seqs, lens, n, hp);
    hp.reach = panel_reach(hp, dp);
    if (hp.reach.need_pre > kGuardNt || hp.reach.need_post > kGuardNt) {
        err = "panel: the kernels' reach around a view (" + std::to_string(hp.reach.pre) +
                 " nt before, " + std::to_string(hp.reach.post) +
                 " after) exceeds the device guard";
        return DMX_E_UNSUPPORTED;
    }
    for (int a = 0; a < n; ++a) dp.ad[a] = hp.ad[a];
    return DMX_OK;
}

static int set_panel_impl(dmx_ctx* c, int round, const char* const* seqs, const int* lens,
                          const int* wheres, int n, double max_errors, int min_overlap,
                          int flags) {
    if (!c || round < 0 || round > 1 || !seqs || !lens) return DMX_E_INVALID;
    HostPanel hp;
    DevPanel dp;
    const int brc = build_panel(c->sw, c->err, seqs, lens, wheres, n, max_errors, min_overlap,
                                flags, hp, dp);
    if (brc) return brc;
    c->panel[round] = hp;
    c->panel[round].n_all = n;
    c->ends_n[round] = 0;
    c->ends_remap[round] = false;
    ++c->panel_gen;
    c->ring_small[round] = hp.ring_small;
    c->band_ok[round] = true;
    int kkmax = 0;
    for (int a = 0; a < n; ++a) {
        c->band_ok[round] &= hp.ad[a].kk <= 7;
        kkmax = std::max(kkmax, (int)hp.ad[a].kk);
    }
    c->band_wide[round] = kkmax > 5;   // list 1 (costs 4..kk): 11 diagonals cover kk <= 5
    CK(hipSetDevice(c->device));
    CK(hipMemcpy(c->d_panel[round].p, &dp, sizeof(dp), hipMemcpyHostToDevice));
    if (hp.piece_step)
        CK(hipMemcpy(c->d_pieces[round].p, &hp.pieces, sizeof(DevPieces), hipMemcpyHostToDevice));
    return DMX_OK;
}

// A panel with restricted adapters or per-adapter minimum overlaps.  The
// unrestricted adapters form the sub-panel the internal pipeline runs (build_panel, as for any
// panel); every restricted adapter gets its tables from build_panel on itself alone, with its own
// minimum overlap; finalize decodes against the whole panel.
static int set_panel_ends(dmx_ctx* c, int round, const char* const* seqs, const int* lens,
                          const int* wheres, const int* min_overlaps, int n, double max_errors,
                          int min_overlap, int rc) {
    if (!c || round < 0 || round > 1 || !seqs || !lens || !wheres) return DMX_E_INVALID;
    if (n <= 0 || n > kMaxAdapters) {
        c->err = "panel must hold 1..64 adapters";
        return DMX_E_INVALID;
    }
    const int rcflag = rc ? DMX_RC : 0;
    std::vector<const char*> sseq;
    std::vector<int> slen, swhere, sidx;
    int sub_mo = -1;
    for (int a = 0; a < n; ++a) {
        if (!where_valid(wheres[a])) return DMX_E_INVALID;
        if (wheres[a] & kRestrictBits) continue;
        const int mo = min_overlaps ? min_overlaps[a] : min_overlap;
        if (sub_mo >= 0 && mo != sub_mo) {
            c->err = "the unrestricted adapters of a panel must share one minimum overlap";
            return DMX_E_UNSUPPORTED;
        }
        sub_mo = mo;
        sseq.push_back(seqs[a]);
        slen.push_back(lens[a]);
        swhere.push_back(wheres[a]);
        sidx.push_back(a);
    }
    HostPanel hp;
    std::unique_ptr<DevPanel> dp(new DevPanel()), all(new DevPanel());
    std::unique_ptr<DevEnds> de(new DevEnds());
    memset(dp.get(), 0, sizeof(DevPanel));
    memset(all.get(), 0, sizeof(DevPanel));
    memset(de.get(), 0, sizeof(DevEnds));
    if (!sseq.empty()) {
        const int brc = build_panel(c->sw, c->err, sseq.data(), slen.data(), swhere.data(),
                                    (int)sseq.size(), max_errors, sub_mo, DMX_FRONT | rcflag, hp,
                                    *dp);
        if (brc) return brc;
    } else {   // restricted adapters only: no screen, no scan
        hp = HostPanel();
        hp.set = true;
        hp.n_orient = rc ? 2 : 1;
        hp.reach = panel_reach(hp, *dp);
        dp->n_orient = hp.n_orient;
        dp->near_shared = -1;
    }
    bool band_ok = true;
    int kkmax = 0;
    for (int s = 0; s < hp.n; ++s) {
        band_ok &= hp.ad[s].kk <= 7;
        kkmax = std::max(kkmax, (int)hp.ad[s].kk);
        all->ad[sidx[s]] = hp.ad[s];
        de->remap[s] = (uint8_t)sidx[s];
        if (sidx[s] != s) de->remap_on = 1;
    }
    for (int a = 0; a < n; ++a) {
        if (!(wheres[a] & kRestrictBits)) continue;
        const bool front = (wheres[a] & DMX_FRONT) != 0;
        const bool anchored = (wheres[a] & DMX_ANCHORED) != 0;
        const int mo = anchored ? lens[a] : (min_overlaps ? min_overlaps[a] : min_overlap);
        if (mo < 1) {
            c->err = "adapter " + std::to_string(a) + ": minimum overlap must be >= 1";
            return DMX_E_INVALID;
        }
        PanelSwitches one;   // one adapter's tables, no filter blocks
        one.no_filter = one.no_verify = one.no_pieces = true;
        std::string err1;
        HostPanel h1;
        std::unique_ptr<DevPanel> d1(new DevPanel());
        const char* s1[1] = {seqs[a]};
        const int l1[1] = {lens[a]};
        const int brc = build_panel(one, err1, s1, l1, nullptr, 1, max_errors, mo,
                                    front ? DMX_FRONT : DMX_BACK, h1, *d1);
        if (brc) {
            c->err = "adapter " + std::to_string(a) + ": " + err1;
            return brc;
        }
        const DevAdapter& src = h1.ad[0];
        EndAdapter& e = de->ad[de->n++];
        for (int k = 0; k < 4; ++k) e.peq[k] = src.peq[k];
        memcpy(e.acc, src.acc, sizeof(e.acc));
        memcpy(e.pacc, src.pacc, sizeof(e.pacc));
        e.m = src.m;
        e.k = src.k;
        e.kk = src.kk;
        e.orig = (uint8_t)a;
        e.type = front ? (anchored ? kEndPrefix : kEndFrontX) : (anchored ? kEndSuffix : kEndBackX);
        all->ad[a] = src;
        hp.nonpos |= h1.nonpos;
        hp.ring_small &= h1.ring_small;
        band_ok &= src.kk <= 7;
    }
    hp.n_all = n;
    all->n_adapters = n;
    all->n_orient = hp.n_orient;
    all->near_shared = -1;
    de->n_orient = hp.n_orient;
    de->n_sub = hp.n;
    c->panel[round] = hp;
    c->ends_n[round] = de->n;
    c->ends_remap[round] = de->remap_on != 0;
    ++c->panel_gen;
    c->ring_small[round] = hp.ring_small;
    c->band_ok[round] = band_ok;
    c->band_wide[round] = kkmax > 5;
    CK(hipSetDevice(c->device));
    CK(hipMemcpy(c->d_panel[round].p, dp.get(), sizeof(DevPanel), hipMemcpyHostToDevice));
    if (hp.piece_step)
        CK(hipMemcpy(c->d_pieces[round].p, &hp.pieces, sizeof(DevPieces), hipMemcpyHostToDevice));
    if (de->n) {
        CK(c->d_ends[round].reserve(1));
        CK(c->d_panel_all[round].reserve(1));
        CK(hipMemcpy(c->d_ends[round].p, de.get(), sizeof(DevEnds), hipMemcpyHostToDevice));
        CK(hipMemcpy(c->d_panel_all[round].p, all.get(), sizeof(DevPanel), hipMemcpyHostToDevice));
    }
    return DMX_OK;
}

size_t dmx_pack_words(uint64_t total_nt, size_t n_reads) {
    const uint64_t nt = 2 * (uint64_t)DMX_PACK_PAD + total_nt + (uint64_t)kPackAlign * n_reads;
    return (size_t)((nt + 31) / 32 * 2 + 4);
}

int dmx_pack(const uint8_t* ascii, const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
             uint32_t* out_seq2b, uint32_t* out_nmask, uint64_t* out_offsets) {
    if ((n_reads && (!offsets || !lens)) || !out_seq2b || !out_nmask || !out_offsets)
        return DMX_E_INVALID;
    uint64_t g = DMX_PACK_PAD;
    uint64_t total = 0;
    for (size_t r = 0; r < n_reads; ++r) {
        out_offsets[r] = g;
        g += ((uint64_t)lens[r] + kPackAlign - 1) / kPackAlign * kPackAlign;
        total += lens[r];
    }
    if (!ascii && total) return DMX_E_INVALID;   // a batch of empty reads needs no text
    const size_t words = dmx_pack_words(total, n_reads);
    memset(out_seq2b, 0, words * sizeof(uint32_t));
    memset(out_nmask, 0, words * sizeof(uint32_t));
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t nth = n_reads < 4096 ? 1 : hw;
    if (nth == 1) {
        pack_range(ascii, offsets, lens, 0, n_reads, out_offsets, out_seq2b, out_nmask);
    } else {
        std::vector<std::thread> th;
        const size_t per = (n_reads + nth - 1) / nth;
        for (size_t t = 0; t < nth; ++t) {
            const size_t lo = t * per, hi = std::min(n_reads, lo + per);
            if (lo >= hi) break;
            th.emplace_back(pack_range, ascii, offsets, lens, lo, hi, out_offsets, out_seq2b,
                            out_nmask);
        }
        for (auto& t : th) t.join();
    }
    return DMX_OK;
}

}  // extern "C"

namespace {

// Room in `set` for a batch of `words` packed words between the guards.  New buffers are zeroed
// whole (the guards stay zero from then on) and start empty.
int reserve_words(Ctx* c, InputSet& set, size_t words) {
    const size_t total = words + 2 * kGuardWords;
    if (min_cap(set.seq, set.nmask) >= total) return DMX_OK;
    set.n_words = 0;
    const hipError_t e1 = set.seq.reserve(total), e2 = set.nmask.reserve(total);
    derive_inputs(c);
    CK(e1);
    CK(e2);
    CK(hipMemsetAsync(set.seq.p, 0, total * 4, c->stream));
    CK(hipMemsetAsync(set.nmask.p, 0, total * 4, c->stream));
    return DMX_OK;
}

// Mask words [mw0, mw0 + nmw) of the caller's batch into the resident set's d_nmask on stream s:
// a copy of the dense bitmap, or zero-fill + a scatter of the exceptions in that range (sorted
// by index, so the range is one binary search).  The exceptions are staged in the set's d_exc.
int upload_mask(Ctx* c, const MaskSrc& m, size_t mw0, size_t nmw, hipStream_t s) {
    if (m.dense) {
        CK(hipMemcpyAsync(c->d_nmask, m.dense + mw0, nmw * 4, hipMemcpyHostToDevice, s));
        return DMX_OK;
    }
    CK(hipMemsetAsync(c->d_nmask, 0, nmw * 4, s));
    const uint32_t* lo = std::lower_bound(m.idx, m.idx + m.n, (uint32_t)mw0);
    const uint32_t* hi = std::lower_bound(lo, m.idx + m.n, (uint32_t)(mw0 + nmw));
    const size_t n = (size_t)(hi - lo), first = (size_t)(lo - m.idx);
    if (!n) return DMX_OK;
    CK(c->in.exc.reserve(2 * n));
    CK(hipMemcpyAsync(c->in.exc.p, m.idx + first, n * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(c->in.exc.p + n, m.val + first, n * 4, hipMemcpyHostToDevice, s));
    return launch_mask_scatter(c->d_nmask, c->in.exc.p, (uint32_t)n, (uint32_t)mw0, s);
}

int load_impl(dmx_ctx* c, const uint32_t* seq2b, const MaskSrc& mask, const uint64_t* offsets,
              const uint32_t* lens, size_t n_words, size_t n_reads) {
    if (n_reads >= (1ull << 31)) {
        c->err = "too many reads in one batch";
        return DMX_E_UNSUPPORTED;
    }
    for (size_t r = 0; r < n_reads; ++r) {
        if (offsets[r] < 16 || (offsets[r] + lens[r] + 64) > (uint64_t)n_words * 16 ||
            lens[r] >= (1u << 30)) {
            c->err = "read offsets/lengths do not fit the packed buffer (use dmx_pack)";
            return DMX_E_INVALID;
        }
    }
    CK(hipSetDevice(c->device));
    int rc;
    if ((rc = reserve_words(c, c->in, n_words))) return rc;
    // the mask has 1 bit per nt: only its first half (of n_words words) carries data
    const size_t nmw = std::min(n_words, (n_words + 1) / 2 + 2);
    if (c->in.n_words > n_words)   // stale tail of a longer batch: guard zero
        CK(hipMemsetAsync(c->d_seq + n_words, 0, (c->in.n_words - n_words) * 4, c->stream));
    if (c->in.n_words > nmw)
        CK(hipMemsetAsync(c->d_nmask + nmw, 0, (std::min(c->in.n_words, c->in.cap_words()) - nmw) * 4,
                          c->stream));
    CK(c->in.offs.reserve(n_reads));
    CK(c->in.lens.reserve(n_reads));
    c->n_reads = n_reads;
    c->in.n_words = n_words;
    CK(hipMemcpyAsync(c->d_seq, seq2b, n_words * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = upload_mask(c, mask, 0, nmw, c->stream))) return rc;
    if (n_reads) {
        CK(hipMemcpyAsync(c->in.offs.p, offsets, n_reads * 8, hipMemcpyHostToDevice, c->stream));
        CK(hipMemcpyAsync(c->in.lens.p, lens, n_reads * 4, hipMemcpyHostToDevice, c->stream));
    }
    CK(hipStreamSynchronize(c->stream));
    c->executed = false;
    c->chunked = false;
    c->views_on = false;   // whole-read runs again (dmx_set_views / dmx_chop_views set a list)
    ++c->view_gen;
    ops_drop(c);           // ... and the sorting calls index reads again
    c->h_lens.assign(lens, lens + n_reads);   // view lists are checked and rendered against it
    chop_invalidate(c);
    lg_invalidate(c);
    return DMX_OK;
}

}  // namespace

extern "C" {

int dmx_load(dmx_ctx* c, const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
             const uint32_t* lens, size_t n_words, size_t n_reads) {
    if (!c || (n_reads && (!seq2b || !nmask || !offsets || !lens))) return DMX_E_INVALID;
    MaskSrc m;
    m.dense = nmask;
    return load_impl(c, seq2b, m, offsets, lens, n_words, n_reads);
}

int dmx_panel_pieces(const char* const* seqs, const int* lens, int n, double max_errors,
                     int min_overlap, int flags, int32_t* out, int n_out, uint64_t* entries,
                     int cap) {
    if (!out || n_out < 8) return DMX_E_INVALID;
    const PanelSwitches sw = panel_switches_env();   // the switches dmx_open would set
    std::string err;                                 // (no context to keep it in)
    HostPanel hp;
    DevPanel dp;
    const int rc = build_panel(sw, err, seqs, lens, nullptr, n, max_errors, min_overlap, flags,
                               hp, dp);
    for (int i = 0; i < n_out; ++i) out[i] = 0;
    if (rc != DMX_OK) return rc;
    const DevPieces& Q = hp.pieces;
    const int32_t v[8] = {hp.piece_step, Q.n_pieces, Q.n_keys, Q.n_entries, Q.front_reach,
                          Q.part_max, Q.lo_off, Q.dlo_min};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    if (entries)
        for (int e = 0; e < Q.n_entries && e < cap; ++e) entries[e] = Q.entry[e];
    return DMX_OK;
}

int dmx_panel_piece_pairs(const char* const* seqs, const int* lens, int n, double max_errors,
                          int min_overlap, int flags, uint32_t* pair, uint16_t* rank_base,
                          uint32_t* keys, int cap) {
    if (!pair || !rank_base) return DMX_E_INVALID;
    const PanelSwitches sw = panel_switches_env();   // the switches dmx_open would set
    std::string err;                                 // (no context to keep it in)
    HostPanel hp;
    DevPanel dp;
    const int rc = build_panel(sw, err, seqs, lens, nullptr, n, max_errors, min_overlap, flags,
                               hp, dp);
    if (rc != DMX_OK) return rc;
    const DevPieces& Q = hp.pieces;
    for (int r = 0; r < kPiecePairWords; ++r) pair[r] = Q.pair[r];
    for (int r = 0; r < kPieceRankWords; ++r) rank_base[r] = Q.rank_base[r];
    if (keys)
        for (int k = 0; k < Q.n_keys && k < cap; ++k) keys[k] = Q.key[k];
    return DMX_OK;
}

int dmx_panel_reach(const char* const* seqs, const int* lens, const int* wheres, int n,
                    double max_errors, int min_overlap, int flags, int32_t* out, int n_out) {
    if (!out || n_out < 6) return DMX_E_INVALID;
    // Restricted adapters (DMX_ANCHORED / DMX_NONINTERNAL in wheres or flags) take no part in the
    // internal pipeline: the reach is that of the sub-panel of the others.  The end-window stage
    // gathers view positions [0, len + 15] only, whatever the view's length: inside every
    // panel's reach.
    std::vector<const char*> sseq;
    std::vector<int> slen, swhere;
    if (wheres || (flags & kRestrictBits)) {
        if (!seqs || !lens || n <= 0 || n > kMaxAdapters) return DMX_E_INVALID;
        for (int a = 0; a < n; ++a) {
            const int w = wheres ? wheres[a] : (flags & ~DMX_RC);
            if (!where_valid(w)) return DMX_E_INVALID;
            if (w & kRestrictBits) continue;
            sseq.push_back(seqs[a]);
            slen.push_back(lens[a]);
            swhere.push_back(w);
        }
        if ((int)sseq.size() != n) {
            seqs = sseq.data();
            lens = slen.data();
            wheres = swhere.data();
            n = (int)sseq.size();
        }
        flags = DMX_FRONT | (flags & DMX_RC);
    }
    const PanelSwitches sw = panel_switches_env();   // the switches dmx_open would set
    std::string err;                                 // (no context to keep it in)
    HostPanel hp;
    DevPanel dp;
    PanelReach r;
    if (n == 0) {   // restricted adapters only
        memset(&dp, 0, sizeof(dp));
        r = panel_reach(hp, dp);
        const int32_t v0[6] = {r.pre_raw, r.pre, r.post, r.need_pre, r.need_post, kGuardNt};
        for (int i = 0; i < 6; ++i) out[i] = v0[i];
        return DMX_OK;
    }
    const int rc = build_panel(sw, err, seqs, lens, wheres, n, max_errors, min_overlap, flags, hp,
                               dp);
    if (rc == DMX_OK) r = hp.reach;
    else if (rc == DMX_E_UNSUPPORTED && hp.set) r = hp.reach;   // refused by the reach check
    else return rc;
    const int32_t v[6] = {r.pre_raw, r.pre, r.post, r.need_pre, r.need_post, kGuardNt};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
    return rc;
}

int dmx_panel_near_shared(const char* const* seqs, const int* lens, const int* wheres, int n,
                          double max_errors, int min_overlap, int flags, int32_t* out, int n_out) {
    if (!out || n_out < 4) return DMX_E_INVALID;
    if (wheres) {   // dmx_set_panel_mixed's form
        for (int a = 0; a < n; ++a)
            if (wheres[a] != DMX_FRONT && wheres[a] != DMX_BACK) return DMX_E_INVALID;
        flags = DMX_FRONT | (flags & DMX_RC);
    }
    const PanelSwitches sw = panel_switches_env();   // the switches dmx_open would set
    std::string err;                                 // (no context to keep it in)
    HostPanel hp;
    DevPanel dp;
    const int rc = build_panel(sw, err, seqs, lens, wheres, n, max_errors, min_overlap, flags, hp,
                               dp);
    if (rc != DMX_OK) return rc;
    int kk = -1;
    for (int a = 0; a < n; ++a) kk = std::max(kk, (int)hp.ad[a].kk);
    const int32_t v[4] = {dp.near_shared, dp.filter_len, dp.jsplit, kk};
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    return DMX_OK;
}

int dmx_debug_bounds_selftest(dmx_ctx* c, uint32_t* out3) {
    if (!c || !out3) return DMX_E_INVALID;
    CK(hipSetDevice(c->device));
    return bounds_selftest(c, out3);
}

// One round's matches into its winner slots: the internal pipeline for the unrestricted adapters
// (all of them, for every panel without restricted ones), then the end-window stage.
static int run_round(dmx_ctx* c, int round, hipStream_t st) {
    int rc;
    if (c->panel[round].n > 0) {
        if ((rc = launch_round(c, round, st))) return rc;
    } else {   // restricted adapters only: no screen, no scan; the stage times read as 0
        for (int k : {kEvRound, kEvScan, kEvResolve}) CK(hipEventRecord(c->ev[ev_of(k, round)], st));
    }
    return c->ends_n[round] ? launch_ends(c, round, st) : DMX_OK;
}

int dmx_exec(dmx_ctx* c) {
    if (!c) return DMX_E_INVALID;
    if (!c->panel[0].set || (c->mode != DMX_MODE_SINGLE && !c->panel[1].set)) {
        c->err = "panels not set for this mode";
        return DMX_E_STATE;
    }
    if (c->mode == DMX_MODE_LINKED && (c->ends_n[0] || c->ends_n[1])) {
        c->err = "linked mode does not take anchored / non-internal adapters";
        return DMX_E_UNSUPPORTED;
    }
    if (c->mode == DMX_MODE_LINKED && c->views_on) {
        c->err = "linked mode does not run on views (dmx_clear_views first)";
        return DMX_E_UNSUPPORTED;
    }
    CK(hipSetDevice(c->device));
    int rc = ensure_pipeline(c);
    if (rc) return rc;
    hipStream_t st = c->stream;
    CK(hipEventRecord(c->ev[kEvExec], st));
    CK(hipMemsetAsync(c->d_counters.p, 0, kCntCount * sizeof(uint32_t), st));
    CK(hipMemsetAsync(c->d_shard.p, 0, kShLists * kShards * kShardStride * sizeof(uint32_t), st));
    CK(hipMemsetAsync(c->d_counts.p, 0, c->n_counts * sizeof(unsigned long long), st));
    c->counts_reduced = false;
    // A panel whose accepted matches can score <= 0 keeps one winner per orientation:
    // ReverseComplementer compares the two orientations' best scores with "no match" = 0, so
    // a read whose only forward match scores -1 is taken reverse-complemented (and unmatched).
    for (int r = 0; r < 2; ++r)
        c->orient_slot[r] = c->mode != DMX_MODE_LINKED && c->panel[r].n_orient == 2 &&
                            c->panel[r].nonpos;
    const size_t slots0 = c->mode == DMX_MODE_LINKED ? c->n_reads * (size_t)c->panel[0].n
                                                     : round0_items(c) * (c->orient_slot[0] ? 2 : 1);
    CK(hipMemsetAsync(c->d_winner[0].p, 0xFF, slots0 * sizeof(unsigned long long), st));
    if ((rc = prepare_flat(c, st))) return rc;
    if ((rc = run_round(c, 0, st))) return rc;
    if ((rc = launch_finalize(c, 0, st))) return rc;
    if (c->mode != DMX_MODE_SINGLE) {
        CK(hipMemsetAsync(c->d_winner[1].p, 0xFF, c->item_cap * (c->orient_slot[1] ? 2 : 1) *
                                                     sizeof(unsigned long long), st));
        if ((rc = run_round(c, 1, st))) return rc;
        if ((rc = launch_finalize(c, 1, st))) return rc;
    }
    c->executed = true;
    c->exec_items = round0_items(c);
    c->exec_views = c->views_on;
    c->exec_view_gen = c->view_gen;
    c->exec_panel_gen = c->panel_gen;
    return bounds_check(c, "dmx_exec");   // DMX_DEBUG_BOUNDS builds only (else DMX_OK)
}

int dmx_sync(dmx_ctx* c) {
    if (!c) return DMX_E_INVALID;
    CK(hipStreamSynchronize(c->stream));
    return DMX_OK;
}

int dmx_fetch(dmx_ctx* c, dmx_result* out) {
    if (!c || (!out && (c->executed ? c->exec_items : c->n_reads))) return DMX_E_INVALID;
    if (!c->executed) {
        c->err = "dmx_fetch before dmx_exec";
        return DMX_E_STATE;
    }
    if (c->chunked) {
        c->err = "dmx_fetch after a chunked dmx_run (its results went to dmx_run's out)";
        return DMX_E_STATE;
    }
    CK(hipSetDevice(c->device));
    if (c->exec_items)   // one result per item of round 0: reads, or the views of a view run
        CK(hipMemcpyAsync(out, c->in.res.p, c->exec_items * sizeof(dmx_result),
                          hipMemcpyDeviceToHost, c->stream));
    CK(hipStreamSynchronize(c->stream));
    return DMX_OK;
}

int dmx_set_views(dmx_ctx* c, const uint32_t* read, const int32_t* start, const int32_t* stop,
                  const uint8_t* strand, size_t n_views) {
    if (!c || (n_views && (!read || !start || !stop || !strand))) return DMX_E_INVALID;
    if (!c->d_seq || !c->in.lens.p || c->chunked || c->h_lens.size() != c->n_reads) {
        c->err = "dmx_set_views: no resident batch (dmx_load first)";
        return DMX_E_STATE;
    }
    if (n_views >= (1ull << 31)) {
        c->err = "dmx_set_views: too many views in one list";
        return DMX_E_UNSUPPORTED;
    }
    CK(hipSetDevice(c->device));
    const std::vector<uint32_t>& lens = c->h_lens;   // dmx_load's copy: no device round trip
    // ItemView's start counts on the view's strand: strand 1 is the reverse complement of the read
    std::vector<ItemView> v(n_views);
    for (size_t k = 0; k < n_views; ++k) {
        const char* why = nullptr;
        if (read[k] >= c->n_reads) why = "names a read outside the batch";
        else if (start[k] < 0 || start[k] > stop[k]) why = "has start < 0 or start > stop";
        else if ((uint32_t)stop[k] > lens[read[k]]) why = "ends past its read";
        else if (strand[k] > 1) why = "has a strand other than 0 or 1";
        if (why) {
            c->err = "dmx_set_views: view " + std::to_string(k) + " " + why;
            return DMX_E_INVALID;
        }
        v[k].read = read[k];
        v[k].len = (uint32_t)(stop[k] - start[k]);
        v[k].start = strand[k] ? lens[read[k]] - (uint32_t)stop[k] : (uint32_t)start[k];
        v[k].strand = strand[k];
        v[k].pad = 0;
        v[k].only_adapter = -1;
    }
    int rc = views_reserve(c, n_views);
    if (rc) {
        c->views_on = false;
        return rc;
    }
    const uint32_t nv = (uint32_t)n_views;
    if (n_views)
        CK(hipMemcpyAsync(c->d_views.p, v.data(), n_views * sizeof(ItemView), hipMemcpyHostToDevice,
                          c->stream));
    CK(hipMemcpyAsync(c->d_view_n.p, &nv, sizeof nv, hipMemcpyHostToDevice, c->stream));
    CK(hipStreamSynchronize(c->stream));
    c->n_views = n_views;
    c->views_on = true;
    return DMX_OK;
}

int dmx_clear_views(dmx_ctx* c) {
    if (!c) return DMX_E_INVALID;
    c->views_on = false;
    ++c->view_gen;
    return DMX_OK;
}

int dmx_views_fetch(dmx_ctx* c, uint32_t* read, int32_t* start, int32_t* stop,
                    uint8_t* strand, size_t cap) {
    if (!c) return DMX_E_INVALID;
    if (!c->views_on) return 0;
    const size_t n = std::min(c->n_views, cap);
    if (n) {
        CK(hipSetDevice(c->device));
        std::vector<ItemView> v(n);
        const std::vector<uint32_t>& lens = c->h_lens;
        CK(hipMemcpyAsync(v.data(), c->d_views.p, n * sizeof(ItemView), hipMemcpyDeviceToHost,
                          c->stream));
        CK(hipStreamSynchronize(c->stream));
        for (size_t k = 0; k < n; ++k) {
            const uint32_t len = v[k].read < lens.size() ? lens[v[k].read] : 0u;
            const uint32_t a = v[k].strand ? len - v[k].start - v[k].len : v[k].start;
            if (read) read[k] = v[k].read;
            if (start) start[k] = (int32_t)a;
            if (stop) stop[k] = (int32_t)(a + v[k].len);
            if (strand) strand[k] = v[k].strand;
        }
    }
    return (int)c->n_views;
}

int dmx_counts(dmx_ctx* c, uint64_t* out, size_t n_out) {
    if (!c || !out) return DMX_E_INVALID;
    if (!c->executed) {
        c->err = "dmx_counts before dmx_exec";
        return DMX_E_STATE;
    }
    if (n_out < c->n_counts) {
        c->err = "counts buffer too small";
        return DMX_E_INVALID;
    }
    CK(hipSetDevice(c->device));
    CK(hipMemcpyAsync(out, c->d_counts.p, c->n_counts * 8, hipMemcpyDeviceToHost, c->stream));
    CK(hipStreamSynchronize(c->stream));
    return (int)c->n_counts;
}

int dmx_stats(dmx_ctx* c, float* stage_ms, int n_stage, uint64_t* counts, int n_counts,
              int* flags) {
    if (!c) return DMX_E_INVALID;
    if (!c->executed) {
        c->err = "dmx_stats before dmx_exec";
        return DMX_E_STATE;
    }
    CK(hipSetDevice(c->device));
    CK(hipStreamSynchronize(c->stream));
    const int rounds = c->mode == DMX_MODE_SINGLE ? 1 : 2;
    float t[kStCount] = {};
    const auto span = [&](int slot, int from, int to) {
        hipEventElapsedTime(&t[slot], c->ev[from], c->ev[to]);
    };
    for (int r = 0; r < rounds; ++r) {
        span(st_round(r, kStScan), ev_of(kEvRound, r), ev_of(kEvScan, r));
        span(st_round(r, kStResolve), ev_of(kEvScan, r), ev_of(kEvResolve, r));
        span(st_round(r, kStFinal), ev_of(kEvResolve, r), ev_of(kEvFinal, r));
        if (c->panel[r].filter && c->mode != DMX_MODE_LINKED) {
            span(st_filter(r), ev_of(kEvRound, r), ev_of(kEvFilter, r));
            span(st_verify(r), ev_of(kEvFilter, r), ev_of(kEvVerify, r));
            span(st_screen(r), ev_of(kEvVerify, r), ev_of(kEvScreen, r));
            span(st_wscan(r), ev_of(kEvScreen, r), ev_of(kEvScan, r));
            if (c->panel[r].piece_step)   // the piece screen's share of the filter stage
                span(st_pieces(r), ev_of(kEvRound, r), ev_of(kEvPieces, r));
        }
        if (c->ends_n[r]) span(st_ends(r), ev_of(kEvEndsIn, r), ev_of(kEvEndsOut, r));
    }
    span(kStTotal, kEvExec, ev_of(kEvFinal, rounds - 1));
    for (int i = 0; i < n_stage && i < kStCount; ++i) stage_ms[i] = t[i];
    uint32_t cnt[kCntCount];
    int list_ovf = 0;
    CK(read_counters(c, cnt, &list_ovf));
    if (getenv("DMX_DEBUG_STATS"))
        fprintf(stderr,
                "dmx stats: filter tasks %u %u windows raw %u %u verified %u %u screened tasks "
                "%u %u (by 3' cells only %u %u) cand %u %u %u %u\n",
                cnt[kCntFtasks], cnt[kCntFtasks + 1], cnt[kCntWindows], cnt[kCntWindows + 1],
                cnt[kCntVerified], cnt[kCntVerified + 1], cnt[kCntTasks], cnt[kCntTasks + 1],
                cnt[cnt_diag(0, kDiagEndOnly)], cnt[cnt_diag(1, kDiagEndOnly)], cnt[kCntCands],
                cnt[kCntCands + 1], cnt[kCntCands + 2], cnt[kCntCands + 3]);
    if (counts) {
        // per round: the pairs of include/dmx.h's list, in its order
        uint64_t v[18];
        for (int r = 0; r < 2; ++r) {
            v[0 + r] = cnt[kCntClusters + r];
            v[2 + r] = cnt[(c->panel[r].verify ? kCntVerified : kCntWindows) + r];
            v[4 + r] = band_round(c, r)
                           ? (uint64_t)cnt[kCntCands + 2 * r] + cnt[kCntCands + 2 * r + 1]
                           : cnt[cnt_diag(r, kDiagResolved)];
            v[6 + r] = cnt[cnt_diag(r, kDiagTraces)];
            v[8 + r] = cnt[kCntWindows + r];
            v[10 + r] = cnt[kCntTasks + r];
            v[12 + r] = cnt[kCntFtasks + r];
            v[14 + r] = cnt[kCntEndsDp + r];
            v[16 + r] = cnt[kCntEndsSeen + r];
        }
        for (int i = 0; i < n_counts && i < 18; ++i) counts[i] = v[i];
    }
    if (flags) {
        int f = (int)cnt[kCntFlags];
        if (cnt[kCntClusters] > cl_cap(c) || cnt[kCntClusters + 1] > cl_cap(c)) f |= kFlagClusters;
        f |= list_ovf;
        *flags = f;
    }
    return DMX_OK;
}

int dmx_debug_fetch(dmx_ctx* c, int what, int round, void* out, size_t cap_bytes) {
    if (!c || round < 0 || round > 1 || (!out && cap_bytes)) return DMX_E_INVALID;
    if (!c->executed) {
        c->err = "dmx_debug_fetch before dmx_exec";
        return DMX_E_STATE;
    }
    CK(hipSetDevice(c->device));
    CK(hipStreamSynchronize(c->stream));
    uint32_t cnt[kCntCount];
    CK(read_counters(c, cnt, nullptr));
    if (what == DMX_DBG_FLAGS) {
        if (cap_bytes >= 4) std::memcpy(out, &cnt[kCntFlags], 4);
        return 4;
    }
    // every list is sharded: gather its shards (windows and tasks of round 1 share buffers with
    // round 0: only the last executed round's are resident)
    int slot;
    const char* base;
    size_t cap, rec;
    switch (what) {
        case DMX_DBG_WINDOWS: slot = kShWin + round; base = (const char*)c->d_win.p; cap = win_cap(c); rec = sizeof(Window); break;
        case DMX_DBG_VERIFIED: slot = kShWin2 + round; base = (const char*)c->d_win2.p; cap = win_cap(c); rec = sizeof(Window); break;
        case DMX_DBG_TASKS: slot = kShTasks + round; base = (const char*)c->d_tasks.p; cap = task_cap(c); rec = sizeof(Window); break;
        case DMX_DBG_CANDS0: slot = kShCand + 2 * round; base = (const char*)c->d_cand[round][0].p; cap = cand_cap(c); rec = sizeof(Cand); break;
        case DMX_DBG_CANDS1: slot = kShCand + 2 * round + 1; base = (const char*)c->d_cand[round][1].p; cap = cand_cap(c); rec = sizeof(Cand); break;
        default: return DMX_E_INVALID;
    }
    uint32_t sh[kShards * kShardStride];
    CK(hipMemcpy(sh, c->d_shard.p + slot * kShards * kShardStride, sizeof(sh),
                 hipMemcpyDeviceToHost));
    const size_t scap = cap / kShards;
    size_t done = 0;
    for (int s = 0; s < kShards; ++s) {
        const size_t nb = std::min<size_t>(sh[s * kShardStride], scap) * rec;
        const size_t take = out ? std::min(nb, cap_bytes > done ? cap_bytes - done : 0) : 0;
        if (take) CK(hipMemcpy((char*)out + done, base + s * scap * rec, take, hipMemcpyDeviceToHost));
        done += nb;
    }
    return (int)std::min<size_t>(done, (size_t)1 << 30);
}

namespace {

// dmx_exec until every list held its records: an overflowed list is grown and the pipeline run
// again, never truncated (dmx_run, dmx_exec_checked).  `enqueued`, if any, runs once, after the
// first dmx_exec of the call has been enqueued and before the host waits for it.  Synchronises.
int exec_checked(dmx_ctx* c, const std::function<int()>& enqueued = nullptr) {
    int rc;
    for (int attempt = 0; attempt < 8; ++attempt) {
        if ((rc = dmx_exec(c))) return rc;
        if (attempt == 0 && enqueued && (rc = enqueued())) return rc;
        uint64_t cl[8];
        int flags = 0;
        float ms[7];
        if ((rc = dmx_stats(c, ms, 7, cl, 8, &flags))) return rc;
        if (flags & kFlagsInternal) {
            c->err = (flags & kFlagTraceback)
                         ? "internal: traceback left the exact window (please report)"
                         : "internal: filter task invariant violated (please report)";
            return DMX_E_STATE;
        }
        if (!(flags & kFlagsOverflow)) return DMX_OK;
        if (attempt == 7) break;
        if ((flags & kFlagClusters) && (rc = grow_clusters(c))) return rc;
        if ((flags & kFlagWindows) && (rc = grow_windows(c))) return rc;
        if ((flags & kFlagCands) && (rc = grow_cands(c))) return rc;
    }
    c->err = "candidate cluster buffer overflow";
    return DMX_E_NOMEM;
}

// One chunk of a chunked dmx_run: reads [lo, hi) of the caller's dmx_pack batch, rebased.
struct Chunk {
    size_t lo, hi, w0, words;
    uint64_t g0;      // the chunk's nt base: its offsets are rebased by -g0 on the device
    size_t exc_lo, exc_n;   // its range of the sparse mask's exceptions
};

// The resident set <-> the second set.
void swap_inputs(Ctx* c) {
    c->in.swap(c->alt);
    derive_inputs(c);
}

// Upload one chunk into the current set on the copy stream (asynchronous: the caller syncs
// cstream before the set is used), zeroing a longer previous chunk's tail.  Offsets go up as the
// caller gave them and are rebased on the device.
int upload_chunk(Ctx* c, const Chunk& k, const uint32_t* seq2b, const MaskSrc& mask,
                 const uint64_t* offsets, const uint32_t* lens) {
    hipStream_t s = c->cstream;
    // the nmask words of a range (1 bit per nt: half as many); the rest of the buffer stays
    // zero (the guard)
    const auto mask_words = [](size_t w) { return std::min(w, (w + 1) / 2 + 2); };
    const size_t nmw = mask_words(k.words), old_nmw = mask_words(c->in.n_words);
    if (c->in.n_words > k.words)
        CK(hipMemsetAsync(c->d_seq + k.words, 0, (c->in.n_words - k.words) * 4, s));
    if (old_nmw > nmw) CK(hipMemsetAsync(c->d_nmask + nmw, 0, (old_nmw - nmw) * 4, s));
    CK(hipMemcpyAsync(c->d_seq, seq2b + k.w0, k.words * 4, hipMemcpyHostToDevice, s));
    int rc;
    if ((rc = upload_mask(c, mask, k.w0 / 2, nmw, s))) return rc;
    const size_t n = k.hi - k.lo;
    CK(hipMemcpyAsync(c->in.offs.p, offsets + k.lo, n * 8, hipMemcpyHostToDevice, s));
    if ((rc = launch_rebase_offsets(c->in.offs.p, (uint32_t)n, k.g0, s))) return rc;
    CK(hipMemcpyAsync(c->in.lens.p, lens + k.lo, n * 4, hipMemcpyHostToDevice, s));
    c->in.n_words = k.words;
    return DMX_OK;
}

// fn(lo, hi) over [0, n) on up to 16 host threads
extern "C++" template <class F>
void parallel_ranges(size_t n, F fn) {
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t nth = n < (1u << 16) ? 1 : hw;
    if (nth == 1) {
        fn((size_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t per = (n + nth - 1) / nth;
    for (size_t t = 0; t < nth; ++t) {
        const size_t lo = t * per, hi = std::min(n, lo + per);
        if (lo < hi) th.emplace_back(fn, lo, hi);
    }
    for (auto& x : th) x.join();
}

// Room in `set` for chunks of up to `words` words and `reads` reads, and their results.
int alloc_set(Ctx* c, InputSet& set, size_t words, size_t reads) {
    if (set.cap_words() >= words && set.cap_reads() >= reads && set.res.cap >= reads)
        return DMX_OK;
    int rc;
    if ((rc = reserve_words(c, set, words))) return rc;
    CK(set.offs.reserve(reads));
    CK(set.lens.reserve(reads));
    CK(set.res.reserve(reads));
    CK(hipStreamSynchronize(c->stream));
    return DMX_OK;
}

// dmx_run of a batch larger than one chunk: chunks of `per` reads alternate between two input
// and result sets.  While chunk k's kernels run on the compute stream, the host uploads chunk
// k+1 and downloads chunk k-1's results on the copy stream; per-bin counts are summed on the
// host and left in d_counts for dmx_counts / dmx_allreduce_counts.  The batch must come from
// dmx_pack (offsets on kPackAlign boundaries after DMX_PACK_PAD).
int run_chunked(dmx_ctx* c, const uint32_t* seq2b, const MaskSrc& nmask,
                const uint64_t* offsets, const uint32_t* lens, size_t n_words, size_t n_reads,
                dmx_result* out, size_t per) {
    std::vector<Chunk> ch;
    size_t maxw = 0, maxn = 0, maxe = 0;
    for (size_t lo = 0; lo < n_reads; lo += per) {
        Chunk k;
        k.lo = lo;
        k.hi = std::min(n_reads, lo + per);
        if (offsets[lo] < (uint64_t)DMX_PACK_PAD || offsets[lo] % kPackAlign) {
            c->err = "dmx_run: offsets must come from dmx_pack";
            return DMX_E_INVALID;
        }
        k.g0 = offsets[lo] - DMX_PACK_PAD;   // a 32-nt (nmask word) boundary
        ch.push_back(k);
    }
    // each chunk's end (the largest rebased offset + length): one parallel pass over the reads
    std::vector<uint64_t> ends(ch.size(), 0);
    {
        std::vector<std::vector<uint64_t>> part;
        std::mutex mu;
        parallel_ranges(n_reads, [&](size_t lo, size_t hi) {
            std::vector<uint64_t> e(ch.size(), 0);
            for (size_t r = lo; r < hi; ++r) {
                const size_t k = r / per;
                e[k] = std::max<uint64_t>(e[k], offsets[r] + lens[r] - ch[k].g0);
            }
            std::lock_guard<std::mutex> g(mu);
            part.push_back(std::move(e));
        });
        for (const auto& e : part)
            for (size_t k = 0; k < ch.size(); ++k) ends[k] = std::max(ends[k], e[k]);
    }
    for (size_t k = 0; k < ch.size(); ++k) {
        Chunk& x = ch[k];
        x.w0 = (size_t)(x.g0 / 16);
        if (x.w0 >= n_words) {
            c->err = "dmx_run: offsets beyond the packed buffer";
            return DMX_E_INVALID;
        }
        x.words = std::min(n_words - x.w0, (size_t)((ends[k] + DMX_PACK_PAD + 31) / 32 * 2 + 4));
        maxw = std::max(maxw, x.words);
        maxn = std::max(maxn, x.hi - x.lo);
        if (!nmask.dense) {   // the chunk's exceptions: mask words [w0 / 2, w0 / 2 + nmw)
            const size_t mw0 = x.w0 / 2, nmw = std::min(x.words, (x.words + 1) / 2 + 2);
            const uint32_t* a = std::lower_bound(nmask.idx, nmask.idx + nmask.n, (uint32_t)mw0);
            const uint32_t* b = std::lower_bound(a, nmask.idx + nmask.n, (uint32_t)(mw0 + nmw));
            maxe = std::max(maxe, (size_t)(b - a));
        }
    }
    CK(hipSetDevice(c->device));
    if (!c->cstream) CK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
    if (!c->dstream) CK(hipStreamCreateWithFlags(&c->dstream, hipStreamNonBlocking));
    int rc;
    // both sets sized for the largest chunk (and its exception staging)
    for (InputSet* set : {&c->in, &c->alt}) {
        if ((rc = alloc_set(c, *set, maxw, maxn))) return rc;
        if (maxe) CK(set->exc.reserve(2 * maxe));
    }
    c->n_reads = maxn;
    c->views_on = false;
    ++c->view_gen;
    ops_drop(c);
    c->h_lens.clear();
    chop_invalidate(c);
    lg_invalidate(c);
    c->chunked = false;
    std::vector<uint64_t> total, part;
    if ((rc = upload_chunk(c, ch[0], seq2b, nmask, offsets, lens))) return rc;
    CK(hipStreamSynchronize(c->cstream));
    for (size_t i = 0; i < ch.size(); ++i) {
        const size_t n = ch[i].hi - ch[i].lo;
        c->n_reads = n;
        // meanwhile: the next chunk into the other set, the previous chunk's results out
        // (uploads on cstream and the download on dstream run in both directions at once;
        // the other set's inputs and its result array are disjoint buffers)
        const auto overlap = [&]() -> int {
            int rc = DMX_OK;
            swap_inputs(c);
            if (i + 1 < ch.size()) rc = upload_chunk(c, ch[i + 1], seq2b, nmask, offsets, lens);
            if (rc == DMX_OK && i > 0) {
                const size_t pn = ch[i - 1].hi - ch[i - 1].lo;
                const hipError_t e =
                    hipMemcpyAsync(out + ch[i - 1].lo, c->in.res.p, pn * sizeof(dmx_result),
                                   hipMemcpyDeviceToHost, c->dstream);
                if (e != hipSuccess) {
                    c->err = std::string("dmx_run: result download: ") + hipGetErrorString(e);
                    rc = DMX_E_HIP;
                }
            }
            swap_inputs(c);
            return rc;
        };
        if ((rc = exec_checked(c, overlap))) return rc;
        part.assign(c->n_counts, 0);
        CK(hipMemcpy(part.data(), c->d_counts.p, c->n_counts * 8, hipMemcpyDeviceToHost));
        if (total.size() != part.size()) total.assign(part.size(), 0);
        for (size_t x = 0; x < part.size(); ++x) total[x] += part[x];
        CK(hipStreamSynchronize(c->cstream));   // the next chunk is in, the previous one out
        CK(hipStreamSynchronize(c->dstream));
        swap_inputs(c);   // the next chunk (uploaded above) becomes the resident batch
    }
    // the last chunk's results sit in the other set now
    swap_inputs(c);
    {
        const Chunk& k = ch.back();
        CK(hipMemcpy(out + k.lo, c->in.res.p, (k.hi - k.lo) * sizeof(dmx_result),
                     hipMemcpyDeviceToHost));
    }
    CK(hipMemcpy(c->d_counts.p, total.data(), total.size() * 8, hipMemcpyHostToDevice));
    c->counts_reduced = false;
    c->chunked = true;
    return DMX_OK;
}

}  // namespace

namespace {

int run_impl(dmx_ctx* c, const uint32_t* seq2b, const MaskSrc& mask, const uint64_t* offsets,
             const uint32_t* lens, size_t n_words, size_t n_reads, dmx_result* out) {
    size_t per = (size_t)1 << 21;   // reads per chunk of an overlapped run
    if (const char* e = std::getenv("DMX_RUN_CHUNK")) per = (size_t)std::strtoull(e, nullptr, 10);
    // chunking rebases every chunk on a 32-nt boundary, which needs dmx_pack's layout at the
    // chunk starts; any other (caller-packed) batch runs in one shot, whatever its size
    bool chunkable = per > 0 && n_reads > per + per / 2;
    for (size_t lo = 0; chunkable && lo < n_reads; lo += per)
        chunkable = offsets[lo] >= (uint64_t)DMX_PACK_PAD && offsets[lo] % kPackAlign == 0;
    if (chunkable) {
        if (!c->panel[0].set || (c->mode != DMX_MODE_SINGLE && !c->panel[1].set)) {
            c->err = "panels not set for this mode";
            return DMX_E_STATE;
        }
        // Every read must also sit at or after its chunk's base g0 = offsets[chunk lo] -
        // DMX_PACK_PAD (+16, the guard any offset keeps): the device rebases offsets by g0, so
        // a read below it (a permuted batch) would wrap.  Such a batch runs in one shot.
        std::atomic<bool> bad{false}, permuted{false};
        parallel_ranges(n_reads, [&](size_t lo, size_t hi) {
            for (size_t r = lo; r < hi; ++r) {
                if (offsets[r] < 16 || (offsets[r] + lens[r] + 64) > (uint64_t)n_words * 16 ||
                    lens[r] >= (1u << 30)) {
                    bad = true;
                    return;
                }
                if (offsets[r] < offsets[r / per * per] - (uint64_t)DMX_PACK_PAD + 16u)
                    permuted = true;
            }
        });
        if (bad) {
            c->err = "read offsets/lengths do not fit the packed buffer (use dmx_pack)";
            return DMX_E_INVALID;
        }
        chunkable = !permuted;
    }
    if (chunkable)
        return run_chunked(c, seq2b, mask, offsets, lens, n_words, n_reads, out, per);
    int rc = load_impl(c, seq2b, mask, offsets, lens, n_words, n_reads);
    if (rc) return rc;
    if ((rc = exec_checked(c))) return rc;
    return dmx_fetch(c, out);
}

}  // namespace

int dmx_exec_checked(dmx_ctx* c) {
    if (!c) return DMX_E_INVALID;
    return exec_checked(c);
}

int dmx_run(dmx_ctx* c, const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
            const uint32_t* lens, size_t n_words, size_t n_reads, dmx_result* out) {
    if (!c || (n_reads && (!seq2b || !nmask || !offsets || !lens || !out))) return DMX_E_INVALID;
    MaskSrc m;
    m.dense = nmask;
    return run_impl(c, seq2b, m, offsets, lens, n_words, n_reads, out);
}

int dmx_run_sparse(dmx_ctx* c, const uint32_t* seq2b, const uint32_t* exc_idx,
                   const uint32_t* exc_val, size_t n_exc, const uint64_t* offsets,
                   const uint32_t* lens, size_t n_words, size_t n_reads, dmx_result* out) {
    if (!c || (n_reads && (!seq2b || !offsets || !lens || !out)) ||
        (n_exc && (!exc_idx || !exc_val)))
        return DMX_E_INVALID;
    const size_t nmw = std::min(n_words, (n_words + 1) / 2 + 2);
    std::atomic<bool> bad{false};
    parallel_ranges(n_exc, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i)
            if (exc_idx[i] >= nmw || (i && exc_idx[i] <= exc_idx[i - 1])) {
                bad = true;
                return;
            }
    });
    if (bad) {
        c->err = "dmx_run_sparse: exception indices must be strictly increasing mask words";
        return DMX_E_INVALID;
    }
    MaskSrc m;
    m.idx = exc_idx;
    m.val = exc_val;
    m.n = n_exc;
    return run_impl(c, seq2b, m, offsets, lens, n_words, n_reads, out);
}

size_t dmx_mask_exceptions(const uint32_t* nmask, size_t n_words, uint32_t* out_idx,
                           uint32_t* out_val, size_t cap) {
    if (!nmask) return 0;
    const size_t nmw = std::min(n_words, (n_words + 1) / 2 + 2);   // the words carrying data
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t nth = nmw < (1u << 20) ? 1 : hw;
    std::vector<size_t> cnt(nth + 1, 0);
    const size_t per = (nmw + nth - 1) / nth;
    auto count = [&](size_t t) {
        size_t n = 0;
        for (size_t w = t * per, e = std::min(nmw, w + per); w < e; ++w) n += nmask[w] != 0;
        cnt[t + 1] = n;
    };
    auto fill = [&](size_t t) {
        size_t o = cnt[t];
        for (size_t w = t * per, e = std::min(nmw, w + per); w < e; ++w)
            if (nmask[w]) {
                if (o < cap) {
                    out_idx[o] = (uint32_t)w;
                    out_val[o] = nmask[w];
                }
                ++o;
            }
    };
    auto par = [&](auto fn) {
        if (nth == 1) return fn((size_t)0);
        std::vector<std::thread> th;
        for (size_t t = 0; t < nth; ++t) th.emplace_back(fn, t);
        for (auto& x : th) x.join();
    };
    par(count);
    for (size_t t = 0; t < nth; ++t) cnt[t + 1] += cnt[t];
    if (out_idx && out_val && cap) par(fill);
    return cnt[nth];
}

int dmx_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return DMX_E_INVALID;
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? DMX_OK : DMX_E_HIP;
}

int dmx_host_unregister(void* p) {
    if (!p) return DMX_E_INVALID;
    return hipHostUnregister(p) == hipSuccess ? DMX_OK : DMX_E_HIP;
}

int dmx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dmx_run_multi(dmx_ctx* const* ctxs, int n_ctx, const uint32_t* seq2b, const uint32_t* nmask,
                  const uint64_t* offsets, const uint32_t* lens, size_t n_words, size_t n_reads,
                  dmx_result* out, uint64_t* out_counts, size_t n_counts) {
    if (!ctxs || n_ctx <= 0 || !ctxs[0]) return DMX_E_INVALID;
    dmx_ctx* c0 = ctxs[0];
    if (n_reads && (!seq2b || !nmask || !offsets || !lens || !out)) return DMX_E_INVALID;
    for (int k = 1; k < n_ctx; ++k) {
        if (!ctxs[k] || ctxs[k]->mode != c0->mode || ctxs[k]->panel[0].n_all != c0->panel[0].n_all ||
            ctxs[k]->panel[1].n_all != c0->panel[1].n_all) {
            c0->err = "dmx_run_multi: contexts must share mode and panels";
            return DMX_E_INVALID;
        }
    }
    // contiguous read ranges balanced by total length; outputs land in place,
    // so shard order = input order
    std::vector<size_t> cut(n_ctx + 1, n_reads);
    cut[0] = 0;
    {
        uint64_t total = 0;
        for (size_t r = 0; r < n_reads; ++r) total += lens[r];
        uint64_t acc = 0;
        int k = 1;
        for (size_t r = 0; r < n_reads && k < n_ctx; ++r) {
            acc += lens[r];
            while (k < n_ctx && acc * (uint64_t)n_ctx >= total * (uint64_t)k) cut[k++] = r + 1;
        }
        for (int j = 1; j <= n_ctx; ++j) cut[j] = std::max(cut[j], cut[j - 1]);
    }
    // one dmx_comm_init_all set over exactly these contexts: the counts are summed on the
    // devices by RCCL; otherwise (contexts sharing a device, no communicator) on the host
    bool rccl = out_counts && c0->comm_group != 0 && c0->comm_ranks == n_ctx;
    for (int k = 1; k < n_ctx && rccl; ++k)
        rccl = ctxs[k]->comm_group == c0->comm_group && ctxs[k]->comm_rank == k;
    if (rccl && c0->comm_rank != 0) rccl = false;
    std::vector<int> rcs(n_ctx, DMX_OK);
    std::vector<std::vector<uint64_t>> cnt(n_ctx);
    auto shard = [&](int k) {
        dmx_ctx* c = ctxs[k];
        const size_t lo = cut[k], hi = cut[k + 1];
        const size_t n = hi - lo;
        if (!n) {   // nothing to run; its counts are zero
            if (rccl) rcs[k] = reset_counts(c);
            return;
        }
        uint64_t g0 = 0;
        {
            if (offsets[lo] < (uint64_t)DMX_PACK_PAD || offsets[lo] % kPackAlign) {
                c->err = "dmx_run_multi: offsets must come from dmx_pack";
                rcs[k] = DMX_E_INVALID;
                return;
            }
            g0 = offsets[lo] - DMX_PACK_PAD;
        }
        std::vector<uint64_t> offs(n);
        uint64_t end = 0;
        for (size_t r = 0; r < n; ++r) {
            offs[r] = offsets[lo + r] - g0;
            end = std::max<uint64_t>(end, offs[r] + lens[lo + r]);
        }
        const size_t w0 = (size_t)(g0 / 16);
        if (w0 >= n_words) {
            c->err = "dmx_run_multi: offsets beyond the packed buffer";
            rcs[k] = DMX_E_INVALID;
            return;
        }
        const size_t words =
            std::min(n_words - w0, (size_t)((end + DMX_PACK_PAD + 31) / 32 * 2 + 4));
        int rc = dmx_run(c, seq2b + w0, nmask + g0 / 32, offs.data(), lens + lo, words, n, out + lo);
        if (rc == DMX_OK && out_counts && !rccl) {
            cnt[k].assign(c->n_counts, 0);
            rc = dmx_counts(c, cnt[k].data(), cnt[k].size());
            if (rc > 0) rc = DMX_OK;
        }
        rcs[k] = rc;
    };
    if (n_ctx == 1) {
        shard(0);
    } else {
        std::vector<std::thread> th;
        for (int k = 0; k < n_ctx; ++k) th.emplace_back(shard, k);
        for (auto& t : th) t.join();
    }
    for (int k = 0; k < n_ctx; ++k) {
        if (rcs[k] != DMX_OK) {
            if (k) c0->err = "device " + std::to_string(ctxs[k]->device) + ": " + ctxs[k]->err;
            return rcs[k];
        }
    }
    if (rccl) return allreduce_counts_group(ctxs, n_ctx, out_counts, n_counts);
    if (out_counts) {
        size_t nc = 0;
        for (int k = 0; k < n_ctx; ++k) nc = std::max(nc, cnt[k].size());
        if (n_counts < nc) {
            c0->err = "counts buffer too small";
            return DMX_E_INVALID;
        }
        for (size_t i = 0; i < n_counts; ++i) out_counts[i] = 0;
        for (int k = 0; k < n_ctx; ++k)
            for (size_t i = 0; i < cnt[k].size(); ++i) out_counts[i] += cnt[k][i];
        return (int)nc;
    }
    return DMX_OK;
}

}  // extern "C"
