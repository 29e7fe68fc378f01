// dmx_internal.h — host-side context of libdmx (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dmx.h"
#include "dmx_device.h"

struct ncclComm;   // RCCL (rccl/rccl.h: ncclComm_t = ncclComm*)

namespace dmx {

struct ChopState;   // read reorientation (dmx_chop.hip)
struct PdState;     // pairwise read distance (dmx_pairdist.hip)
struct PaState;     // pairwise alignment with edit path (dmx_pairdist.hip)
struct GaState;     // progressive alignment of read groups (dmx_pairdist.hip)
struct RdState;     // read distance against rows of masks (dmx_pairdist.hip)
struct RrState;     // distance between rows of masks, their hits (dmx_pairdist.hip)
struct RaState;     // reads assigned to rows of masks, best row per read (dmx_pairdist.hip)
struct LgState;     // hits of dmx_pairhits, link groups (dmx_groups.hip)

// A device buffer that grows on demand, never shrinks, and is freed with its owner.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) hipFree(p);
    }
    hipError_t reserve(size_t n) {   // room for n elements (one at least); the content is not kept
        if (p && cap >= n) return hipSuccess;
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
        n = std::max<size_t>(n, 1);
        const hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
};

// The capacity that buffers grown together share: the smallest of theirs, so a member whose
// allocation failed (capacity 0) makes the whole group read as too small.
template <typename T>
size_t min_cap(const DevBuf<T>& b) {
    return b.cap;
}
template <typename T, typename... R>
size_t min_cap(const DevBuf<T>& b, const R&... rest) {
    return std::min(b.cap, min_cap(rest...));
}

// One set of input buffers and the results computed from them.  A context has two: the resident
// batch and the set the chunks of a large dmx_run alternate with.
struct InputSet {
    DevBuf<uint32_t> seq, nmask;   // packed buffers with kGuardWords zeroed words on both sides
    DevBuf<uint64_t> offs;         // (the filter loads whole aligned 64-nt blocks)
    DevBuf<uint32_t> lens;
    DevBuf<dmx_result> res;
    DevBuf<uint32_t> exc;          // sparse no-match mask staging: [idx][val] (dmx_run_sparse)
    size_t n_words = 0;
    // words of a batch that fit between the guards; reads that fit offs / lens
    size_t cap_words() const {
        const size_t t = min_cap(seq, nmask);
        return t > 2 * (size_t)kGuardWords ? t - 2 * (size_t)kGuardWords : 0;
    }
    size_t cap_reads() const { return min_cap(offs, lens); }
    void swap(InputSet& o) {
        seq.swap(o.seq), nmask.swap(o.nmask), offs.swap(o.offs), lens.swap(o.lens);
        res.swap(o.res), exc.swap(o.exc);
        std::swap(n_words, o.n_words);
    }
};

// Indices of Ctx::ev: per round (ev_of) the start of the round, the end of its scan stage, of
// the resolve stage and of finalize; inside the scan stage the ends of the filter pass, the
// verification, the index screen and the piece screen (its filter tasks follow); before / after
// the end-window stage.  One more event marks the start of dmx_exec.
enum EvKind {
    kEvRound, kEvScan, kEvResolve, kEvFinal, kEvFilter, kEvVerify, kEvScreen, kEvPieces,
    kEvEndsIn, kEvEndsOut, kEvKinds
};
constexpr int ev_of(int kind, int round) { return 2 * kind + round; }
constexpr int kEvExec = 2 * kEvKinds;
constexpr int kEvCount = kEvExec + 1;

// Slots of dmx_stats' stage times (include/dmx.h): per round the scan, resolve and finalize
// stages; the whole exec; per round the filter pass, the verification, the index screen, the
// window scan after it, the piece screen's share of the filter pass and the end-window stage.
enum StageKind { kStScan, kStResolve, kStFinal };
constexpr int st_round(int round, int kind) { return 3 * round + kind; }
constexpr int kStTotal = 6;
constexpr int st_filter(int round) { return 7 + 2 * round; }
constexpr int st_verify(int round) { return 8 + 2 * round; }
constexpr int st_screen(int round) { return 11 + 2 * round; }
constexpr int st_wscan(int round) { return 12 + 2 * round; }
constexpr int st_pieces(int round) { return 15 + round; }
constexpr int st_ends(int round) { return 17 + round; }
constexpr int kStCount = st_ends(1) + 1;

// Reach of a panel's gathers around a view, in nt (panel_reach below).
struct PanelReach {
    int pre_raw = 0;     // before view position 0, as the kernels' formulas ask
    int pre = 0;         // ... after the fetch16s clamp at -kViewReachPre
    int post = 0;        // past the view end
    int need_pre = 0;    // guard nt needed below the buffer for a read at offset kMinOffset
    int need_post = 0;   // guard nt needed past n_words for reads keeping kMinTail nt of tail
};

struct PanelSwitches {        // the run-time switches a panel's tables depend on (build_panel)
    bool no_filter = false;   // DMX_NO_FILTER=1: always full scans (A/B testing)
    bool no_verify = false;   // DMX_NO_VERIFY=1: skip the shared-prefix window verification
    bool no_pieces = false;   // DMX_NO_PIECES=1: the full filter pass instead of the piece screen
    bool near_all = false;    // DMX_NEAR_ALL=1: near pieces keep every adapter's columns
};
bool env_on(const char* name);        // an on/off run-time switch: NAME=1 in the environment
PanelSwitches panel_switches_env();   // the four above, as the environment has them now

struct HostPanel {
    bool screen = false;      // index screen usable (filter + verify, index blocks 1..32)
    int n = 0;                // adapters of the internal pipeline (the unrestricted ones)
    int n_all = 0;            // adapters of the whole panel: bins, counts, finalize
    int n_orient = 1;
    bool set = false;
    bool ring_small = true;
    bool filter = false;
    bool verify = false;
    bool nonpos = false;      // an accepted match may score <= 0 (needs per-orientation winners)
    PanelReach reach;
    DevAdapter ad[kMaxAdapters];
    int piece_step = 0;       // piece screen sampling stride (0 = off: the full filter pass)
    DevPieces pieces;         // its tables
};

struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int mode = DMX_MODE_SINGLE;
    PanelSwitches sw;         // read by dmx_open
    HostPanel panel[2];
    DevBuf<DevPanel> d_panel[2];     // one record each, made by dmx_open
    DevBuf<DevPieces> d_pieces[2];
    // end-window stage: per round the number of restricted adapters (0: the
    // stage does not run and nothing below is read), whether the internal pipeline's keys need
    // their adapter index mapped back, the stage's tables and the whole panel for finalize
    int ends_n[2] = {0, 0};
    bool ends_remap[2] = {false, false};
    DevBuf<DevEnds> d_ends[2];
    DevBuf<DevPanel> d_panel_all[2];

    // resident batch.  dmx_run of a large batch alternates its chunks between `in` and `alt`
    // (inputs + results), so the next chunk's upload and the previous chunk's download overlap
    // the current chunk's kernels (dmx_api.cpp run_chunked).
    size_t n_reads = 0;
    InputSet in, alt;
    // the resident set's packed buffers past their leading guard words: the only pointers into
    // a buffer that are kept, re-derived by derive_inputs after every allocation or swap of `in`
    uint32_t* d_seq = nullptr;
    uint32_t* d_nmask = nullptr;
    hipStream_t cstream = nullptr;      // uploads of chunked runs
    hipStream_t dstream = nullptr;      // result downloads of chunked runs (the other direction)
    bool chunked = false;               // the last dmx_run was chunked: dmx_fetch is refused

    // pipeline state
    DevBuf<unsigned long long> d_winner[2];
    DevBuf<int32_t> d_origin[2];   // ring rounds only (band rounds: in the key)
    DevBuf<int32_t> d_lb[2];
    bool ring_small[2] = {true, true};
    bool band_ok[2] = {true, true};
    bool band_wide[2] = {true, true};      // some adapter has kk 6..7: list 1 needs 15 diagonals
    bool orient_slot[2] = {false, false};   // per round: one winner slot per (item, orientation)
    bool force_ring = false;          // DMX_RESOLVE=ring (A/B testing)
    bool resolve_attr_set = false;    // resolve_kernel's dynamic-LDS limit raised on this device
    DevBuf<Cluster> d_cl[2];
    DevBuf<Outcome> d_outc[2];
    DevBuf<Cand> d_cand[2][2];
    DevBuf<Window> d_win, d_win2;
    DevBuf<ItemView> d_items;            // sized by its own need (ensure_pipeline)
    size_t item_cap = 0;                 // round-2 items of the current mode and batch
    // view runs (dmx_set_views / dmx_chop_views): round 0's item list.  A buffer
    // of its own: finalize0 reads view k while it writes the round-1 list d_items.
    bool views_on = false;
    size_t n_views = 0;
    DevBuf<ItemView> d_views;
    std::vector<uint32_t> h_lens;        // the resident batch's read lengths (dmx_load's copy)
    DevBuf<uint32_t> d_view_n;           // the list's length on the device (round 0's n_items_dev)
    DevBuf<uint32_t> d_item_src;         // round-1 item -> the view it came from (its result)
    // operand table (dmx_set_operands / dmx_result_operands): with a table set the
    // amplicon-sorting calls index operands, not reads.  d_op_off / d_op_len stand in for d_offs /
    // d_lens in their launches (the sub-range as it lies in memory); d_op holds the table itself
    // (OperandRec) for dmx_operands_fetch.  The table lives on the device only.
    bool ops_on = false;
    size_t n_ops = 0;
    DevBuf<OperandRec> d_op;
    DevBuf<uint64_t> d_op_off;
    DevBuf<uint32_t> d_op_len;
    DevBuf<uint8_t> d_op_strand;
    // the host's mirror of d_op_len / d_op_strand for the calls' argument checks and the strand
    // folding: filled by dmx_set_operands, or on first need after dmx_result_operands (one copy per
    // table, not per call); h_op_any: some operand is on strand 1
    bool h_op_valid = false, h_op_any = false;
    std::vector<uint32_t> h_op_len;
    std::vector<uint8_t> h_op_strand;
    // dmx_result_operands' scratch: [block][bin] places, bin_first, the caller's keep flags
    DevBuf<uint32_t> d_op_hist;
    DevBuf<uint64_t> d_op_first;
    DevBuf<uint8_t> d_op_keep;
    DevBuf<uint32_t> d_shard;         // [kShLists][kShards] per-shard list counters (dmx_device.h)
    DevBuf<uint32_t> d_counters;      // kCntCount slots (dmx_device.h CounterSlot)
    DevBuf<unsigned long long> d_counts;   // n_counts of them are in use
    DevBuf<unsigned long long> d_linked;   // one key per read (linked mode)
    DevBuf<Window> d_tasks;           // index screen survivors (window piece of one adapter)
    DevBuf<FTask> d_ftask;            // piece screen -> filter tasks
    // flat piece scan (prepare_flat): one scan of the batch against the flat rounds' combined
    // table marks cells[2 r + strand] for every flat round r
    DevBuf<DevPieces> d_pieces_flat;
    int flat_rounds = 0;                 // bit r: round r's screen is the flat scan (this exec)
    int flat_want = 0;                   // the rounds the combined table was built for
    int flat_step = 0;                   // its sampling stride (0: no table)
    size_t flat_lds = 0;                 // its LDS image
    uint64_t panel_gen = 1;              // bumped by set_panel / set_mode
    uint64_t flat_gen = 0;               // panel_gen the combined table was built for
    DevBuf<uint32_t> d_cells[4];
    size_t cells_words = 0;
    bool no_screen = false;              // DMX_NO_SCREEN=1: every window runs every adapter
    bool screen_v1 = false;              // DMX_SCREEN_V1=1: one lane per (window, adapter) screen
    size_t n_counts = 0;
    hipEvent_t ev[kEvCount] = {};   // EvKind per round (ev_of), kEvExec
    bool executed = false;
    size_t exec_items = 0;       // results of the last dmx_exec (round 0's items)
    bool exec_views = false;     // ... which were the views of d_views as of exec_view_gen
    uint64_t view_gen = 0;       // bumped whenever the view list changes or goes
    uint64_t exec_view_gen = 0;
    uint64_t exec_panel_gen = 0; // panel_gen at that exec: its results were decoded by those panels
    ChopState* chop = nullptr;   // dmx_chop_* state, created by dmx_chop_set
    PdState* pd = nullptr;       // dmx_pairdist buffers, created by its first call
    PaState* pa = nullptr;       // dmx_pairalign buffers, created by its first call
    GaState* ga = nullptr;       // dmx_groupalign buffers, created by its first call
    RdState* rd = nullptr;       // dmx_rowdist buffers, created by its first call
    RrState* rr = nullptr;       // dmx_rowpairdist / dmx_rowhits buffers, created by the first call
    RaState* ra = nullptr;       // dmx_rowassign buffers, created by its first call
    LgState* lg = nullptr;       // dmx_pairhits' outcomes and the link-group buffers

    // RCCL communicator for the per-bin count exchange (dmx_comm.cpp)
    ncclComm* comm = nullptr;
    int comm_ranks = 0, comm_rank = 0;
    uint64_t comm_group = 0;     // nonzero: made by dmx_comm_init_all (one process, grouped calls)
    bool counts_reduced = false; // d_counts already summed over the ranks (cleared by dmx_exec)
};

// Capacities of the pipeline's buffer groups, as their buffers have them: the winner slots (with
// the slot lower bounds), the cluster, candidate and window lists.  The screen's task list holds
// 4 records per window record, the filter task list one.
inline size_t slot_cap(const Ctx* c) {
    return min_cap(c->d_winner[0], c->d_winner[1], c->d_lb[0], c->d_lb[1]);
}
inline size_t cl_cap(const Ctx* c) {
    return min_cap(c->d_cl[0], c->d_cl[1], c->d_outc[0], c->d_outc[1]);
}
inline size_t cand_cap(const Ctx* c) {
    return min_cap(c->d_cand[0][0], c->d_cand[0][1], c->d_cand[1][0], c->d_cand[1][1]);
}
inline size_t win_cap(const Ctx* c) {
    return std::min(min_cap(c->d_win, c->d_win2, c->d_ftask), c->d_tasks.cap / 4);
}
inline size_t task_cap(const Ctx* c) { return 4 * win_cap(c); }
// d_seq / d_nmask from the resident set's allocations.
inline void derive_inputs(Ctx* c) {
    c->d_seq = c->in.seq.p ? c->in.seq.p + kGuardWords : nullptr;
    c->d_nmask = c->in.nmask.p ? c->in.nmask.p + kGuardWords : nullptr;
}

void chop_release(Ctx* c);
void pd_release(Ctx* c);
void lg_release(Ctx* c);
void comm_release(Ctx* c);
int reset_counts(Ctx* c);      // size d_counts for the current panels/mode and zero it (sync)
// The last error of a call that has no context to keep it in (dmx_comm_unique_id's RCCL load),
// returned by dmx_last_error(NULL).
void set_process_error(const std::string& msg);
std::string process_error();
// Items of round 0: the views of a view run, else the resident reads.
inline size_t round0_items(const Ctx* c) { return c->views_on ? c->n_views : c->n_reads; }
// Room for a view list of n entries in d_views (content not kept) and its device count.
int views_reserve(Ctx* c, size_t n);
void chop_invalidate(Ctx* c);   // a new dmx_load makes the last dmx_chop_exec's results stale
void lg_invalidate(Ctx* c);     // ... and the last dmx_pairhits' outcomes
// No operand table: the sorting calls index reads again, and the outcomes of dmx_pairhits, which
// were made under the table, go with it (dmx_operands.hip).
void ops_drop(Ctx* c);
// The host mirror of the table's lengths and strands (h_op_*), copied down once per table.
int ops_mirror(Ctx* c, const char* who);
// dmx_pairhits (dmx_pairdist.hip) runs the distance form's launches; what becomes of a launch's
// distances stays on the device and is dmx_groups.hip's:
// lg_hits_begin uploads the call's pair list and caps and clears the outcomes;
// lg_hits_decide turns the distances `d_dist` of one launch (sorted pair k is input pair
// orig[k]) into outcomes: pass 0 the forward decisions, with bit i - lo of `need` set where input
// pair i has to be tried on the reverse complement, pass 1 the reverse decisions (synchronises);
// lg_hits_end brings down best[] and the number of hits and makes the state valid.
int lg_hits_begin(Ctx* c, const char* who, const uint32_t* q, const uint32_t* t,
                  const int32_t* cap_hit, const int32_t* cap_half, size_t n_pairs, size_t n_reads);
int lg_hits_decide(Ctx* c, const char* who, const uint32_t* d_dist, const uint32_t* orig, size_t np,
                   int pass, size_t lo, std::vector<uint32_t>* need);
int lg_hits_end(Ctx* c, const char* who, float forward_ms, uint32_t* best, uint64_t* n_hits);
// dmx_rowhits (dmx_pairdist.hip): the hit compaction (count, scan, scatter) over outcome words
// d_outc[0 .. n_pairs) that are the caller's, not the last dmx_pairhits': that call's outcomes,
// its pair list and the times of dmx_hitgroups_stats stay as they are (only the compaction's
// scratch buffers are shared).  *n_hits is always set; with hits_cap below it nothing is written
// and the call is DMX_E_INVALID.  *ms = the device time of the three kernels.  Synchronises.
int lg_compact_outcomes(Ctx* c, const char* who, const uint32_t* d_outc, size_t n_pairs,
                        size_t hits_cap, uint32_t* pair, uint32_t* d, uint8_t* rev, size_t* n_hits,
                        float* ms);
// Round `round` resolves its candidates with the band kernels (every adapter has kk <= 7 and
// DMX_RESOLVE=ring is not set): its winner keys carry their origin (make_key_o), and nothing
// reads or writes d_origin[round].
inline bool band_round(const Ctx* c, int round) { return c->band_ok[round] && !c->force_ring; }
int launch_round(Ctx* c, int round, hipStream_t st);
int prepare_flat(Ctx* c, hipStream_t st);   // the flat piece scan's index (dmx_kernels.hip)
int launch_finalize(Ctx* c, int round, hipStream_t st);
// The end-window stage of round `round` (dmx_ends.hip): maps the internal pipeline's adapter
// indices back to the whole panel's where they differ, then one atomicMin per accepted
// restricted-adapter match into the same winner slots (ring rounds: a second pass writes the
// winner's origin).  Called between launch_round and launch_finalize when ends_n[round] > 0.
int launch_ends(Ctx* c, int round, hipStream_t st);
// The panel finalize decodes with: the whole panel where the round has restricted adapters.
inline const DevPanel* final_panel(const Ctx* c, int round) {
    return c->ends_n[round] ? c->d_panel_all[round].p : c->d_panel[round].p;
}
// offs[i] -= g0 for a chunk's offsets uploaded as the caller gave them (stream st)
int launch_rebase_offsets(uint64_t* offs, uint32_t n, uint64_t g0, hipStream_t st);
// mask[idx[i] - base] = val[i] for the n staged exceptions at d_exc ([idx][val]); stream st
int launch_mask_scatter(uint32_t* mask, const uint32_t* d_exc, uint32_t n, uint32_t base,
                        hipStream_t st);

// DMX_DEBUG_BOUNDS builds (dmx_device.h Bounds): the extents of c's device buffers for a launch
// of kernel `kid`; a reset of the violation record (d_counters[24..27]); the check after a run
// (synchronises, and fails naming the kernel, buffer and index of the first violation).  In
// release builds make_bounds is empty, set_kid / bounds_reset do nothing and bounds_check
// returns DMX_OK without synchronising.
Bounds make_bounds(const Ctx* c, int kid);
inline void set_kid(Bounds& b, int kid) {
#ifdef DMX_DEBUG_BOUNDS
    b.kid = kid;
#else
    (void)b, (void)kid;
#endif
}
hipError_t bounds_reset(Ctx* c, hipStream_t st);
int bounds_check(Ctx* c, const char* where);

// Deepest reach of the kernels' gathers around a view for panel `hp` (nt before position 0,
// before and after the -kViewReachPre clamp, and past the view end), and the smallest guard
// that covers them for every offset dmx_load / dmx_run accept.
PanelReach panel_reach(const HostPanel& hp, const DevPanel& dp);
int bounds_selftest(Ctx* c, uint32_t* host_out);   // dmx_debug_bounds_selftest

// Where a batch's no-match mask comes from: the dense bitmap (1 bit per nt) of dmx_pack, or its
// nonzero words as sorted (index, value) exceptions (dmx_mask_exceptions, dmx_run_sparse).
struct MaskSrc {
    const uint32_t* dense = nullptr;
    const uint32_t* idx = nullptr;
    const uint32_t* val = nullptr;
    size_t n = 0;
};

}  // namespace dmx

// The public opaque handle (include/dmx.h) is the host context.
struct dmx_ctx : dmx::Ctx {};

namespace dmx {
// dmx_run_multi's grouped RCCL count all-reduce (dmx_comm.cpp)
int allreduce_counts_group(dmx_ctx* const* ctxs, int n_ctx, uint64_t* out, size_t n_out);
}  // namespace dmx
