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
// last-row score per column, and a second kernel that walks the edit path back through it
// (pairalign_traceback_kernel).
//
// dmx_groupalign (the loop of create_alignment, :324-356, as create_consensus
// runs it for every group) aligns member k of every group against the group's current row 0 in
// lock-step rounds.  Row 0 is not a read but a row of equality masks (one byte per column, bit c
// = the column equals query symbol c, 0 = a gap); the forward pass and the traceback are the
// trace form's, and a third kernel (groupalign_merge_kernel) lays the path over the row: the new
// row's masks and, per column, how many members showed each symbol and which member did first.
//
// dmx_rowdist (process_consensuslist / similarity_species, :1628-1716: every read
// not yet in a group against every group's consensus) is the distance form against such rows:
// NW, no trace, the rows given by the caller per call (rowdist_kernel).
//
// dmx_rowpairdist / dmx_rowhits (iden_consensus, :1140-1159, as the pair loops of
// comp_consensus_groups and compare_consensus run it: every consensus against every later one, HW,
// both strands) is the distance form with both sides rows of masks given per call
// (rowpair_kernel): two columns are equal iff their masks intersect; NW or HW; a reversed target
// is the row's reverse complement, which rowpair_rc_kernel writes beside the rows once per call.
// dmx_rowhits decides the hits on the device (rowhits_decide_kernel) and compacts them with
// dmx_groups.hip's kernels; only the hits come back.
//
// All forms share one forward pass (pd_forward: pairdist_kernel, pairalign_kernel,
// groupalign_kernel, groupalign_strands_kernel (members taken reverse-complemented,
// dmx_groupalign_strands), rowdist_kernel and rowpair_kernel are its instantiations, told apart at
// compile time by their argument struct), one traceback (pa_traceback) and one host path: the chunk planner (pd_plan: chunk
// limits, sort, wave packing, pair records), the staging of a launch (pd_stage: buffers, upload,
// the arguments every kernel takes; pa_stage_trace: the trace form's), the end of a launch group
// (pd_mark, pd_finish: error, events, wait, bounds check, times), the buffers themselves (PdBufs)
// and, for the forms whose rows come with the call, the rows on the device (PdRows,
// dmx_pd_rows.h; pd_rows_validate).  A change to the block step, the stripes, the planner, the
// launch protocol or the row layout is made once.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <type_traits>

#include "dmx_internal.h"
#include "dmx_pd_rows.h"

namespace dmx {

// The group sizes a wave may be cut into: every distinct floor(64 / k).  A pair runs in the
// smallest size that holds its query's words (64 for longer queries, which then run in stripes).
static const int kPdSizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21, 32, 64};
constexpr int kPdNSizes = (int)(sizeof kPdSizes / sizeof *kPdSizes);
constexpr uint32_t kPdWavesPerBlock = 4;
constexpr size_t kPdChunkDefault = 1u << 20;          // pairs per launch (DMX_PD_CHUNK)
constexpr size_t kPdScratchMax = 64u << 20;           // scratch bytes per launch

struct PdPair {
    uint32_t q, t, flags, cap;   // flags: DMX_PD_RC | 0x100 (cap given)
    uint64_t soff;               // the pair's scratch row (queries of more than one stripe)
};
static_assert(sizeof(PdPair) == 24, "the distance form uploads 24 bytes per pair");
// dmx_pairalign's record carries on where dmx_pairdist's ends (no cap: cap and its flag are 0)
struct PaPair : PdPair {
    uint64_t toff;               // its trace: word-step (wi, j) is entry toff + wi * n + j
    uint64_t roff;               // its (m + n)-byte op region
};
// dmx_groupalign's record: the target is a row of masks, `n` columns long now, at mask[row ..);
// the merge writes the group's next row at mask[dst ..).  PdPair::t is the group, PdPair::cap
// the most columns a row may have (a longer path is left unmerged and refused by the host).
// PdPair::flags & DMX_PD_RC: the member (the query) is taken reverse-complemented
// (dmx_groupalign_strands; pd_masks<true> and the merge read it backwards).
struct GaPair : PaPair {
    uint64_t row, dst;           // columns: an index into mask, times 5 into count / first
    uint32_t n;                  // the row's length in this round
    uint32_t ord;                // the member's 1-based place in its group
};
static_assert(sizeof(GaPair) == 64, "the group form uploads 64 bytes per pair");
// dmx_rowdist's record: the distance form's, with the target a row of `n` masks at mask[row ..).
// PdPair::t is the row's index among the call's rows, not a read.
struct RdPair : PdPair {
    uint64_t row;                // first column of the row in the device mask array
    uint32_t n;                  // the row's length
};
static_assert(sizeof(RdPair) == 40, "the row form uploads 40 bytes per pair");
// dmx_rowpairdist's record: query and target are both rows of the call's mask array.  PdPair::q
// and ::t are row indices; a pair flagged DMX_PD_RC has `row` in the reverse-complemented copy.
struct RrPair : PdPair {
    uint64_t row;                // first column of the target row in the device mask array
    uint64_t qrow;               // first column of the query row
    uint32_t n, m;               // their lengths
    uint32_t dst;                // the pair's place in the call's list: where its distance goes
    uint32_t pad;
};
static_assert(sizeof(RrPair) == 56, "the row-pair form uploads 56 bytes per pair");
// dmx_rowassign's record: dmx_rowdist's, and the place in the call's read list whose best line
// the pair may become (the decision kernel reads it; the forward pass does not).
struct RaPair : PdPair {
    uint64_t row;                // first column of the row in the device mask array
    uint32_t n;                  // the row's length
    uint32_t k;                  // the place of PdPair::q in the call's reads
};
static_assert(sizeof(RaPair) == 40, "the assign form uploads 40 bytes per pair");
struct PdWave {
    uint32_t first, count, G, steps;   // pairs[first .. first + count), one group of G lanes each
};

// What both forms' kernels are given (pd_stage fills it).  `out` is not here but at the end of
// both argument structs, and `flags` comes before `cap`: with this layout the trace form
// compiles to the same instructions as before it shared its body.  The forward pass of a short
// list (about one wave per SIMD) is sensitive to where its loop lies in the code.
template <class Pair>
struct PdHead {
    Packed pk;
    const uint64_t* offs;
    const uint32_t* lens;
    const Pair* pairs;
    const PdWave* waves;
    uint32_t n_waves;
    uint32_t n_pairs;
    uint8_t* scratch;
    uint64_t scratch_bytes;
};
struct PdArgs : PdHead<PdPair> {
    int mode;
    uint32_t* out;               // per pair: the distance
};
struct PaArgs : PdHead<PaPair> {
    ulonglong2* pm;              // trace: Pv, Mv of a word after a column
    uint16_t* sc;                // trace: D(word's last row, column)
    uint64_t trace_steps;        // entries of pm / sc
    uint8_t* ops;
    uint64_t ops_bytes;
    uint32_t* out;               // per pair: distance, path length
};

// dmx_groupalign: the trace form's arguments, and the column arrays of every group's row in both
// halves of the ping-pong (a round reads a group's row at P.row and writes the next at P.dst).
struct GaArgs : PdHead<GaPair> {
    ulonglong2* pm;
    uint16_t* sc;
    uint64_t trace_steps;
    uint8_t* ops;
    uint64_t ops_bytes;
    uint8_t* mask;               // per column: the equality mask (bit c: equals query symbol c)
    uint16_t* count;             // [column][5]: members that showed symbol c in the column
    uint16_t* first;             // [column][5]: the first such member's place, 0 = none
    uint64_t cols;               // columns of mask (count and first have 5 entries per column)
    uint32_t* out;               // per pair: distance, path length
};

// The same, for a launch in which some member is flagged DMX_PD_RC: a form of its own, so that
// groupalign_kernel (no flag in the launch, and every dmx_groupalign call) keeps the
// instructions it had before members had strands (groupalign_strands_kernel).
struct GaStrandArgs : GaArgs {};

// dmx_rowdist: the distance form's arguments (NW only, so no mode) and the call's rows.
struct RdArgs : PdHead<RdPair> {
    const uint8_t* mask;         // per column: the equality mask, every row padded to 16 columns
    uint64_t cols;               // columns of mask
    uint32_t* out;               // per pair: the distance
};

// dmx_rowassign: dmx_rowdist's arguments over its own record.  out is indexed by
// the pair's place in the launch, where the decision kernel finds it beside the record.
struct RaArgs : PdHead<RaPair> {
    const uint8_t* mask;         // the rows, then their reverse complements when a pair retries
    uint64_t cols;               // columns of mask
    uint32_t* out;               // per pair of the launch: the distance
};

// dmx_rowpairdist / dmx_rowhits: the distance form's arguments with the mode, and the call's rows
// (forward copies, then the reverse complements where some pair asks for one).  out is indexed by
// the pair's place in the call's list (RrPair::dst), not by its place in the launch: the
// distances of every chunk stay on the device for the hit decision.
struct RrArgs : PdHead<RrPair> {
    const uint8_t* mask;         // per column: the mask, every row padded to 16 columns
    uint64_t cols;               // columns of mask
    int mode;
    uint32_t out_n;              // entries of out
    uint32_t* out;               // per pair of the list: the distance
};

// The buffers and events of either form; they go with the context (pd_release).
template <class Pair>
struct PdBufs {
    DevBuf<Pair> pairs;
    DevBuf<PdWave> waves;
    DevBuf<uint32_t> out;
    DevBuf<uint8_t> scratch;
    hipEvent_t ev[4] = {};       // before the forward pass, after it, the traceback, the merge
    ~PdBufs() {
        for (auto& e : ev)
            if (e) hipEventDestroy(e);
    }
};
struct PdState : PdBufs<PdPair> {
    float ms = 0.f;
};
struct PaTrace {                    // what the trace form's two kernels share (pa_stage_trace)
    DevBuf<ulonglong2> pm;
    DevBuf<uint16_t> sc;
    DevBuf<uint8_t> ops;
};
struct PaState : PdBufs<PaPair>, PaTrace {
    float ms[2] = {0.f, 0.f};    // forward pass, traceback
    int launches = 0;            // chunks of the last call
};
struct GaState : PdBufs<GaPair>, PaTrace {
    DevBuf<uint8_t> mask;        // both halves of every group's row
    DevBuf<uint16_t> count, first;
    float ms[3] = {0.f, 0.f, 0.f};   // forward pass, traceback, merge
    int launches = 0, rounds = 0;
};

struct RdState : PdBufs<RdPair> {
    PdRows rows;                 // the call's rows (their copies: a query on strand 1)
    float ms = 0.f;
};

struct RrState : PdBufs<RrPair> {   // DESIGN.md §8j; PdBufs::out holds the whole list's distances
    PdRows rows;                 // the call's rows (their copies: a flagged pair)
    DevBuf<uint32_t> outc;       // dmx_rowhits: per pair d | DMX_LG_REV, or DMX_LG_NONE
    DevBuf<int32_t> cap;         // dmx_rowhits: the caller's caps
    float ms = 0.f;
};
struct RaState : PdBufs<RaPair> {   // DESIGN.md §8l; PdBufs::out holds one launch's distances
    PdRows rows;                 // the call's rows (their copies: a retry, a read on strand 1)
    DevBuf<int32_t> cap_hit, cap_half;   // the caller's tables, by the longer length
    DevBuf<uint32_t> bin_off;
    DevBuf<uint16_t> bins;
    DevBuf<unsigned long long> best;     // per place: the key of its best line, 0 = none
    DevBuf<unsigned long long> cnt;      // lines
    DevBuf<uint32_t> need;       // per launch: the retry bitmap
    DevBuf<uint32_t> o_row, o_d; // per place: what the finish kernel unpacks
    DevBuf<uint16_t> o_class;
    float ms = 0.f;
};

template <class State>
static void pd_drop(State*& s) {
    delete s;
    s = nullptr;
}
void pd_release(Ctx* c) {
    pd_drop(c->pd), pd_drop(c->pa), pd_drop(c->ga), pd_drop(c->rd), pd_drop(c->rr), pd_drop(c->ra);
}

// The five match masks (A, C, G, T, N) of query rows 64 wi .. 64 wi + 63, built in registers
// from the packed query.  A masked row is the fifth symbol whatever code it carries: it is kept
// out of the A/C/G/T masks.  Rows past the query's end match nothing.
// kStrand (GaStrandArgs: dmx_groupalign_strands' launches with a flagged member, DESIGN.md
// §8g): with rc set the query is the read taken
// reverse-complemented, row i = 3 - code[m - 1 - i].  The 64 positions of word wi then end at
// m - 1 - 64 wi and begin at m - 64 (wi + 1), which in the query's last word lies up to 63 nt
// before the read (before the packed buffer for a read at offset 16).  That word is loaded from
// the read's first nt instead and shifted up by the rows it lacks, so the positions below the
// read become zero bits and the ones loaded past the word's end fall off the top: nothing
// outside [qoff, qoff + m) reaches peq, and the loads stay where the forward form's are.
// kStrand = false holds no instruction of this.
template <bool kStrand>
__device__ __forceinline__ void pd_masks(const Packed& pk, uint64_t qoff, uint32_t m, uint32_t wi,
                                         uint32_t rc, uint64_t (&peq)[5]) {
    const uint32_t rows = min(64u, m - 64u * wi);
    int64_t g0 = (int64_t)qoff + 64ll * wi;
    if constexpr (kStrand) {
        if (rc) g0 = (int64_t)qoff + (int64_t)(m - 64u * wi - rows);   // m - 64 (wi + 1), or 0
    }
    uint32_t cw[4], nw[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) cw[k] = code32(pk, g0 + 16 * k);
#pragma unroll
    for (int k = 0; k < 2; ++k) nw[k] = mask32(pk, g0 + 32 * k);
    const uint64_t valid = rows >= 64u ? ~0ull : ((1ull << rows) - 1ull);
    uint64_t nb = (((uint64_t)nw[1] << 32) | nw[0]) & valid;
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
    if constexpr (kStrand) {
        if (rc) {   // bit k is position g0 + k: row 63 - (k + 64 - rows), complemented
            const uint32_t up = 64u - rows;   // 0..63
            lo = ~__brevll(lo << up);
            hi = ~__brevll(hi << up);
            nb = __brevll(nb << up);
        }
    }
    const uint64_t acgt = valid & ~nb;
    peq[0] = ~hi & ~lo & acgt;
    peq[1] = ~hi & lo & acgt;
    peq[2] = hi & ~lo & acgt;
    peq[3] = hi & lo & acgt;
    peq[4] = nb;
}

// pd_masks for a query that is itself a row of masks (RrArgs): peq[c] bit i = bit c of the mask
// of query row 64 wi + i, so that Eq = OR of peq[c] over the target mask's bits says "the masks
// intersect".  Four aligned 16-byte loads; a chunk is loaded only where it begins below the
// query's end, and then lies inside the row's padding to 16 columns (zeros: they match nothing,
// and `valid` clears them anyway).  Bit c of 4 mask bytes in a word is gathered into 4 adjacent
// bits by one multiply: bit 8 k moves to 24 + k (0x01020408 = 2^24 + 2^17 + 2^10 + 2^3; the other
// partial products land below bit 24 or leave the word, and no two meet, so nothing carries).
__device__ __forceinline__ void pd_masks_row(const Bounds& bd, const uint8_t* mask, uint64_t cols,
                                             uint64_t qrow, uint32_t m, uint32_t wi,
                                             uint64_t (&peq)[5]) {
    const uint32_t rows = min(64u, m - 64u * wi);
    const uint64_t g0 = qrow + 64ull * wi;
#pragma unroll
    for (int c = 0; c < 5; ++c) peq[c] = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        uint4 v = make_uint4(0, 0, 0, 0);
        const uint64_t ri = g0 + 16u * k;
        if (16u * k < rows && ri + 16u <= cols &&
            bchk(bd, (int64_t)ri + 15, 15, (int64_t)cols, kBufRrCols))
            v = *reinterpret_cast<const uint4*>(mask + ri);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
#pragma unroll
            for (uint32_t c = 0; c < 5u; ++c) {
                const uint32_t nib = (((w4[j] >> c) & 0x01010101u) * 0x01020408u) >> 24;
                peq[c] |= (uint64_t)(nib & 15u) << (16u * k + 4u * j);
            }
    }
    const uint64_t valid = rows >= 64u ? ~0ull : ((1ull << rows) - 1ull);
#pragma unroll
    for (int c = 0; c < 5; ++c) peq[c] &= valid;
}

// Where a pair's target lies: a read of the batch, or a row of masks (dmx_groupalign's group
// row, dmx_rowdist's and dmx_rowpairdist's given row).
template <class Pair>
constexpr bool kPdRowPair = std::is_same<Pair, GaPair>::value || std::is_same<Pair, RdPair>::value ||
                            std::is_same<Pair, RrPair>::value || std::is_same<Pair, RaPair>::value;
template <class Pair>
__device__ __forceinline__ bool pd_target_ok(const Bounds& bd, const Pair& P) {
    if constexpr (kPdRowPair<Pair>) return true;   // P.t is a group or a row, not a read
    else return DMX_BOUND(bd, reads, P.t, kBufRead);
}
template <class Pair>
__device__ __forceinline__ uint32_t pd_target_len(const uint32_t* lens, const Pair& P) {
    if constexpr (kPdRowPair<Pair>) return P.n;
    else return lens[P.t];
}
template <class Pair>
__device__ __forceinline__ uint64_t pd_target_off(const uint64_t* offs, const Pair& P) {
    if constexpr (kPdRowPair<Pair>) return P.row;
    else return offs[P.t];
}

// The forward pass of every form, told apart at compile time by the argument struct.
// PdArgs, the distance: NW or HW (A.mode); only the lane of the query's last word follows the
// score (and, for HW, its minimum over the columns); out[k] = the distance, clamped by the cap.
// PaArgs, the trace (dmx_pairalign's forward pass): NW; every live lane follows D(r, j) of its
// word's last row r = min(64 (wi + 1), m) and leaves Pv, Mv and that score of every column in
// the pair's trace at [wi][j] (a lane writes consecutive entries over time); out[2 k] = the
// distance.
// GaArgs, the trace against a row of masks (dmx_groupalign's forward pass): as PaArgs, but the
// target is P.n mask bytes at A.mask[P.row ..), the group's first lane loads 16 of them per 16
// columns, and the value that travels down the lanes carries the mask, not a symbol; Eq is the
// OR of the peq[c] whose bit is set (a gap column, mask 0, equals nothing).  Here the pair's RC
// flag turns the query, not the target: GaStrandArgs takes peq from pd_masks<true>, the only
// strand branch (GaArgs ignores the flag: the host launches it only where none is set).
// RdArgs, the distance against a row of masks (dmx_rowdist): the target and its fetch are
// GaArgs's, the score handling PdArgs's in NW (there is no mode and no reversed target: the
// caller gives a reversed row as a row of its own); out[k] = the distance, clamped by the cap.
// RrArgs, the distance between two rows of masks (dmx_rowpairdist, dmx_rowhits): the target and
// its fetch are RdArgs's, the query's peq comes from pd_masks_row, the mode and the score
// handling are PdArgs's (NW or HW); the record carries both lengths and both rows, so nothing of
// the resident batch is read, and a reversed target is a row of its own in the mask array;
// out[P.dst] = the distance, clamped by the cap.
// Every branch on the form is `if constexpr`: an instantiation holds no instruction of another.
// That is a constraint, not a style: pairdist_kernel and pairalign_kernel are sensitive to where
// their loop lands in the code, so a new form must leave their instructions as
// they are (compare the assembly of all of them before and after).
template <class Args>
__device__ __forceinline__ void pd_forward(const Args& A) {
    constexpr bool kRa = std::is_same<Args, RaArgs>::value;      // RdArgs over its own record
    constexpr bool kRd = std::is_same<Args, RdArgs>::value || kRa;
    constexpr bool kRr = std::is_same<Args, RrArgs>::value;
    constexpr bool kGa = std::is_base_of<GaArgs, Args>::value;   // GaArgs or GaStrandArgs
    constexpr bool kRow = kGa || kRd || kRr;
    constexpr bool kTrace = std::is_same<Args, PaArgs>::value || kGa;
    constexpr uint32_t kColsBuf = kRr ? kBufRrCols : kRa ? kBufRaCols : kRd ? kBufRdCols
                                                                          : kBufGaCols;
    const uint32_t wave = blockIdx.x * kPdWavesPerBlock + (threadIdx.x >> 6);
    if (wave >= A.n_waves) return;   // whole waves leave: the shift below sees full waves
    const uint32_t lane = threadIdx.x & 63u;
    const PdWave W = A.waves[wave];
    const uint32_t G = W.G;
    const uint32_t g = lane / G, w = lane - g * G;
    bool active = g < W.count && (uint64_t)W.first + g < A.n_pairs;
    bool nw = true;
    if constexpr (!kTrace && !kRd) nw = A.mode == DMX_PD_NW;

    uint32_t m = 1, n = 1, rc = 0, cap = 0, has_cap = 0, dst = 0;
    uint64_t qoff = 0, toff = 0, soff = 0, trace = 0;
    if (active) {
        const auto P = A.pairs[W.first + g];
        if constexpr (kRr) {   // both sides are rows: the record has all of it
            m = P.m;
            n = P.n;
            qoff = P.qrow;
            toff = P.row;
            soff = P.soff;
            has_cap = P.flags & 0x100u;
            cap = P.cap;
            dst = P.dst;
        } else if (DMX_BOUND(A.pk.bd, reads, P.q, kBufRead) && pd_target_ok(A.pk.bd, P)) {
            m = A.lens[P.q];
            n = pd_target_len(A.lens, P);
            qoff = A.offs[P.q];
            toff = pd_target_off(A.offs, P);
            rc = P.flags & DMX_PD_RC;
            soff = P.soff;
            if constexpr (kTrace) {
                trace = P.toff;
            } else {
                has_cap = P.flags & 0x100u;
                cap = P.cap;
            }
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
    uint32_t row2 = 0, row3 = 0;   // kRow: mask bytes 8..15 of the 16 in flight (codes, nbits: 0..7)
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
            if constexpr (kRr) {
                if (live) pd_masks_row(A.pk.bd, A.mask, A.cols, qoff, m, wi, peq);
            } else {
                if (live) pd_masks<std::is_same<Args, GaStrandArgs>::value>(A.pk, qoff, m, wi, rc, peq);
            }
            Pv = ~0ull;
            Mv = 0ull;
            // the word's last row: the query's in its last word, so no padded row is ever read
            const uint32_t r = min(m, 64u * (wi + 1u));
            hb = (r - 1u) & 63u;
            if (kTrace || last) score = best = (int)r;
            if constexpr (kTrace) tbase = trace + (uint64_t)wi * n;
        }
        if (w == 0) {   // the group's first lane feeds the array: row 0's delta or the stripe
                        // above's, and the target symbol
            uint32_t sym = 0, hin1 = 1;
            if (ts < n) {
                const uint32_t k = ts & 15u;
                if constexpr (kRow) {
                    if (k == 0u) {   // rows start at multiples of 16 columns and are padded to one
                        const uint64_t ri = toff + ts;
                        uint4 v = make_uint4(0, 0, 0, 0);
                        if (bchk(A.pk.bd, (int64_t)ri + 15, 15, (int64_t)A.cols, kColsBuf))
                            v = *reinterpret_cast<const uint4*>(A.mask + ri);
                        codes = v.x, nbits = v.y, row2 = v.z, row3 = v.w;
                    }
                    const uint32_t wd = k < 4u ? codes : k < 8u ? nbits : k < 12u ? row2 : row3;
                    sym = (wd >> (8u * (k & 3u))) & 31u;
                } else {
                    if (k == 0u) fetch16(A.pk, toff, n, rc, 0u, ts, codes, nbits);
                    sym = ((nbits >> k) & 1u) ? 4u : ((codes >> (2u * k)) & 3u);
                }
                if (s == 0) {
                    hin1 = nw ? 2u : 1u;   // D(0, j) = j, or 0 in HW
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
            uint64_t Eq;
            if constexpr (kRow) {
                Eq = ((sym & 1u) ? peq[0] : 0ull) | ((sym & 2u) ? peq[1] : 0ull) |
                     ((sym & 4u) ? peq[2] : 0ull) | ((sym & 8u) ? peq[3] : 0ull) |
                     ((sym & 16u) ? peq[4] : 0ull);
            } else {
                Eq = sym == 0 ? peq[0] : sym == 1 ? peq[1] : sym == 2 ? peq[2]
                   : sym == 3 ? peq[3] : peq[4];
            }
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
            if (kTrace || last) score += hout;
            if constexpr (kTrace) {
                const uint64_t ti = tbase + j;
                if (bchk(A.pk.bd, (int64_t)ti, 0, (int64_t)A.trace_steps, kBufPaTrace)) {
                    A.pm[ti] = make_ulonglong2(Pv, Mv);
                    A.sc[ti] = (uint16_t)score;
                }
            } else if (last) {
                best = min(best, score);
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
                if (last) {
                    if constexpr (kTrace) {
                        A.out[2u * (W.first + g)] = (uint32_t)score;
                    } else {
                        uint32_t d = (uint32_t)(nw ? score : best);
                        if (has_cap && d > cap) d = cap + 1u;
                        if constexpr (kRr) {
                            if (dst < A.out_n) A.out[dst] = d;
                        } else {
                            A.out[W.first + g] = d;
                        }
                    }
                }
            } else {
                __threadfence();   // the scratch row is read back by the group's first lane
            }
        }
    }
}

__global__ __launch_bounds__(64 * kPdWavesPerBlock) void pairdist_kernel(PdArgs A) { pd_forward(A); }
__global__ __launch_bounds__(64 * kPdWavesPerBlock) void pairalign_kernel(PaArgs A) { pd_forward(A); }
__global__ __launch_bounds__(64 * kPdWavesPerBlock) void groupalign_kernel(GaArgs A) { pd_forward(A); }
__global__ __launch_bounds__(64 * kPdWavesPerBlock) void rowdist_kernel(RdArgs A) { pd_forward(A); }
__global__ __launch_bounds__(64 * kPdWavesPerBlock) void groupalign_strands_kernel(GaStrandArgs A) {
    pd_forward(A);
}
__global__ __launch_bounds__(64 * kPdWavesPerBlock) void rowpair_kernel(RrArgs A) { pd_forward(A); }
__global__ __launch_bounds__(64 * kPdWavesPerBlock) void rowassign_kernel(RaArgs A) { pd_forward(A); }

// The reverse complement of every uploaded row, written `half` columns after the row itself (the
// second half of the mask array, padded as the first): column i of the copy is the complement
// (A <-> T, C <-> G; N and a gap column stay) of column n - 1 - i.  One block per row; the padding
// up to 16 columns is written as zeros.
constexpr uint32_t kRrRcBlock = 256;
struct RrRcArgs {
    Bounds bd;
    const RrRow* rows;
    uint32_t n_rows;
    uint8_t* mask;
    uint64_t half, cols;
};
__global__ __launch_bounds__(kRrRcBlock) void rowpair_rc_kernel(RrRcArgs A) {
    if (blockIdx.x >= A.n_rows) return;
    const RrRow R = A.rows[blockIdx.x];
    const uint32_t padded = (R.n + 15u) & ~15u;
    for (uint32_t i = threadIdx.x; i < padded; i += kRrRcBlock) {
        uint32_t v = 0;
        if (i < R.n) {
            const uint64_t src = R.off + (R.n - 1u - i);
            if (src < A.half && bchk(A.bd, (int64_t)src, 0, (int64_t)A.cols, kBufRrCols)) {
                const uint32_t x = A.mask[src];
                v = (x & 16u) | ((x & 1u) << 3) | ((x & 2u) << 1) | ((x & 4u) >> 1) | ((x & 8u) >> 3);
            }
        }
        const uint64_t dst = A.half + R.off + i;
        if (dst < A.cols && bchk(A.bd, (int64_t)dst, 0, (int64_t)A.cols, kBufRrCols))
            A.mask[dst] = (uint8_t)v;
    }
}

// dmx_rowhits' decision on the distances of the whole list: pair i's forward distance is
// dist[2 i], the one against the reversed target dist[2 i + 1] (both clamped at max(cap, 0) + 1,
// which keeps the minimum, the comparison with the cap and, among hits, the strand as the exact
// distances give them).  Ties are forward.  The outcome word is dmx_pairhits': d, d | DMX_LG_REV
// or DMX_LG_NONE, so the hit compaction of dmx_groups.hip takes it as it is.
struct RrDecide {
    const uint32_t* dist;
    const int32_t* cap;
    uint32_t n_pairs;
    uint32_t* outc;
};
__global__ __launch_bounds__(kRrRcBlock) void rowhits_decide_kernel(RrDecide A) {
    const uint32_t i = blockIdx.x * kRrRcBlock + threadIdx.x;
    if (i >= A.n_pairs) return;
    const uint32_t df = A.dist[2ull * i], dr = A.dist[2ull * i + 1ull];
    const bool rev = dr < df;
    const uint32_t d = rev ? dr : df;
    const int32_t cap = A.cap[i];
    A.outc[i] = (cap >= 0 && d <= (uint32_t)cap) ? (d | (rev ? DMX_LG_REV : 0u)) : DMX_LG_NONE;
}

// dmx_rowassign's decision on one launch's distances.  The key of a line orders
// the lines of a place as update_groups does in pair-generation order, the largest wins:
//   bit 63      set (0 is "no line": the places start there)
//   bits 47..62 the identity class of d at the pair's longer length L (the caller's table)
//   bits 16..46 the row
//   bit 15      the reverse bit
//   bits 0..14  d (<= DMX_PD_MAX_LEN = 2^14)
// A pair makes at most one line and a place meets a row once, so no two lines of a place agree
// in (class, row): the maximum does not depend on the order the atomics land in, nor on which
// launch a pair fell into.  Pass 0 (forward): d is clamped at max(cap_hit, cap_half, 0) + 1, so it
// compares against both caps as the exact distance would; d <= cap_hit is a line, otherwise
// cap_hit >= 0 and d > cap_half sets the pair's bit in `need`.  Pass 1 (the retries against the
// reversed rows, clamped at cap_hit + 1): d <= cap_hit is a line with the reverse bit.
constexpr int kRaClassShift = 47, kRaRowShift = 16;
constexpr uint64_t kRaRowMax = 1ull << 31;   // rows a key holds
constexpr uint64_t kRaValid = 1ull << 63;
constexpr uint32_t kRaRevBit = 1u << 15, kRaDistMask = kRaRevBit - 1u;
static_assert(DMX_PD_MAX_LEN <= kRaDistMask, "a distance must fit below the reverse bit");
struct RaDecide {
    Bounds bd;
    const RaPair* pairs;         // the launch's records, in the order they ran
    const uint32_t* dist;        // their distances
    const uint32_t* lens;        // the resident reads' lengths
    uint32_t np, pass;
    const int32_t* cap_hit;
    const int32_t* cap_half;
    const uint32_t* bin_off;
    const uint16_t* bins;
    uint32_t n_len, n_sel;
    uint64_t n_bins;
    unsigned long long* best;
    uint32_t* need;
    uint32_t need_words;
    unsigned long long* cnt;
};
__global__ __launch_bounds__(kRrRcBlock) void rowassign_decide_kernel(RaDecide A) {
    const uint32_t i = blockIdx.x * kRrRcBlock + threadIdx.x;
    bool line = false;
    if (i < A.np) {
        const RaPair P = A.pairs[i];
        if (DMX_BOUND(A.bd, reads, P.q, kBufRead)) {
            const uint32_t L = max(A.lens[P.q], P.n);
            if (L < A.n_len && bchk(A.bd, (int64_t)L, 0, (int64_t)A.n_len, kBufRaTable)) {
                const int64_t d = A.dist[i], ch = A.cap_hit[L], chalf = A.cap_half[L];
                const bool hit = d <= ch;
                if (A.pass == 0 && !hit && ch >= 0 && d > chalf) {
                    if ((i >> 5) < A.need_words) atomicOr(&A.need[i >> 5], 1u << (i & 31u));
                }
                const uint64_t at = (uint64_t)A.bin_off[L] + (uint64_t)d;
                if (hit && at < A.n_bins && P.k < A.n_sel &&
                    bchk(A.bd, (int64_t)at, 0, (int64_t)A.n_bins, kBufRaTable) &&
                    bchk(A.bd, (int64_t)P.k, 0, (int64_t)A.n_sel, kBufRaBest)) {
                    const uint64_t key = kRaValid | ((uint64_t)A.bins[at] << kRaClassShift) |
                                         ((uint64_t)P.t << kRaRowShift) |
                                         (A.pass ? kRaRevBit : 0u) | ((uint32_t)d & kRaDistMask);
                    atomicMax(&A.best[P.k], (unsigned long long)key);
                    line = true;
                }
            }
        }
    }
    const uint64_t bal = __ballot(line);   // every lane of the wave is here
    if ((threadIdx.x & 63u) == 0 && bal) atomicAdd(A.cnt, (unsigned long long)__popcll(bal));
}

// The keys unpacked into the call's three outputs, one place per lane.
struct RaFinish {
    Bounds bd;
    const unsigned long long* best;
    uint32_t n_sel;
    uint32_t* row;
    uint32_t* d;
    uint16_t* cls;
};
__global__ __launch_bounds__(kRrRcBlock) void rowassign_finish_kernel(RaFinish A) {
    const uint32_t k = blockIdx.x * kRrRcBlock + threadIdx.x;
    if (k >= A.n_sel || !bchk(A.bd, (int64_t)k, 0, (int64_t)A.n_sel, kBufRaBest)) return;
    const uint64_t key = A.best[k];
    const bool has = (key & kRaValid) != 0;
    const uint32_t lo = (uint32_t)key;
    A.row[k] = has ? (uint32_t)((key >> kRaRowShift) & (kRaRowMax - 1ull)) : DMX_LG_NONE;
    A.d[k] = has ? ((lo & kRaDistMask) | ((lo & kRaRevBit) ? DMX_LG_REV : 0u)) : DMX_LG_NONE;
    A.cls[k] = has ? (uint16_t)((key >> kRaClassShift) & 0xFFFFu) : (uint16_t)0;
}

// dmx_pairalign's traceback: one lane per pair walks back from (m, n), preferring up (INSERT),
// then left (DELETE), then the diagonal (include/dmx.h).  Bit b of a word's Pv / Mv at column j
// is D(64 wi + b + 1, j) - D(64 wi + b, j) = +1 / -1, so "up" is one bit test, and D(i, j - 1) is
// the word's score at column j - 1 minus the vertical deltas of the rows below i.  Column j of
// the matrix is trace column j - 1; D(i, 0) = i needs no trace.  Op k goes to
// region[m + n - 1 - k]: the path ends up in forward order at the region's tail.
// The walk reads no sequence: m, n, the trace and the distance are all it needs, so the group
// form (GaArgs) differs only in where n comes from (the record, not a read's length).
constexpr uint32_t kPaTbLanes = 64;
template <class Args>
__device__ __forceinline__ void pa_traceback(const Args& A) {
    const uint32_t k = blockIdx.x * kPaTbLanes + threadIdx.x;
    if (k >= A.n_pairs) return;
    const auto P = A.pairs[k];
    if (!(DMX_BOUND(A.pk.bd, reads, P.q, kBufRead) && pd_target_ok(A.pk.bd, P))) return;
    const uint32_t m = A.lens[P.q], n = pd_target_len(A.lens, P);
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
__global__ __launch_bounds__(kPaTbLanes) void pairalign_traceback_kernel(PaArgs A) { pa_traceback(A); }
__global__ __launch_bounds__(kPaTbLanes) void groupalign_traceback_kernel(GaArgs A) { pa_traceback(A); }

// dmx_groupalign's merge: one wave per pair lays the pair's forward path over the group's row.
// The path is taken 64 ops at a time, one op per lane; the column an op reads in the old row and
// the query symbol it shows are its ranks among the ops that consume the target / the query: a
// ballot, a popcount of the lanes below, and a base that runs over the chunks (the query symbol
// at rank r of a reversed member is the complement of the read's at m - 1 - r).  Column `col` of
// the new row is written by the lane of op `col` alone (plain stores, no atomics: the result
// does not depend on the order the lanes or the waves run in):
//   mask:  the old column's for M / X / D, 0 (a gap: equals nothing) for I
//   count: the old column's (0 for I), + 1 at the query's symbol for M / X / I
//   first: the old column's; the member's place where its symbol's count was 0
// A path longer than the row may become (P.cap) is left unmerged: the host refuses the call.
constexpr uint32_t kGaMergeWaves = 4;
__global__ __launch_bounds__(64 * kGaMergeWaves) void groupalign_merge_kernel(GaArgs A) {
    const uint32_t k = blockIdx.x * kGaMergeWaves + (threadIdx.x >> 6);
    if (k >= A.n_pairs) return;   // whole waves leave: the ballots below see full waves
    const uint32_t lane = threadIdx.x & 63u;
    const GaPair P = A.pairs[k];
    if (!DMX_BOUND(A.pk.bd, reads, P.q, kBufRead)) return;
    const uint32_t m = A.lens[P.q], n = P.n, len = A.out[2u * k + 1u];
    if (len > P.cap || len > m + n || len < max(m, n)) return;
    const uint64_t qoff = A.offs[P.q];
    const uint32_t rc = P.flags & DMX_PD_RC;
    const uint64_t start = P.roff + (m + n - len);
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t tbase = 0, qbase = 0;
    for (uint32_t c0 = 0; c0 < len; c0 += 64u) {
        const uint32_t col = c0 + lane;
        const bool in = col < len;
        uint32_t op = DMX_PA_DELETE;
        if (in && bchk(A.pk.bd, (int64_t)(start + col), 0, (int64_t)A.ops_bytes, kBufPaOps))
            op = A.ops[start + col];
        const bool takes_t = in && op != DMX_PA_INSERT, takes_q = in && op != DMX_PA_DELETE;
        const uint64_t bt = __ballot(takes_t), bq = __ballot(takes_q);
        if (in) {
            uint32_t mk = 0;
            uint16_t cnt[5] = {0, 0, 0, 0, 0}, fst[5] = {0, 0, 0, 0, 0};
            if (takes_t) {
                const uint64_t src = P.row + tbase + (uint32_t)__popcll(bt & below);
                if (bchk(A.pk.bd, (int64_t)src, 0, (int64_t)A.cols, kBufGaCols)) {
                    mk = A.mask[src];
#pragma unroll
                    for (int c = 0; c < 5; ++c) {
                        cnt[c] = A.count[5u * src + c];
                        fst[c] = A.first[5u * src + c];
                    }
                }
            }
            if (takes_q) {
                // rank r among the ops that consume the query; a reversed member shows
                // 3 - code of position m - 1 - r (a rank past the query reads position 0)
                const uint32_t r = qbase + (uint32_t)__popcll(bq & below);
                const uint32_t at = rc ? (r < m ? m - 1u - r : 0u) : r;
                const int64_t g = (int64_t)qoff + at;
                const uint32_t code = code32(A.pk, g) & 3u;
                const uint32_t sym = (mask32(A.pk, g) & 1u) ? 4u : rc ? 3u - code : code;
#pragma unroll
                for (int c = 0; c < 5; ++c)
                    if (sym == (uint32_t)c) {
                        if (cnt[c] == 0) fst[c] = (uint16_t)P.ord;
                        ++cnt[c];
                    }
            }
            const uint64_t dst = P.dst + col;
            if (bchk(A.pk.bd, (int64_t)dst, 0, (int64_t)A.cols, kBufGaCols)) {
                A.mask[dst] = (uint8_t)mk;
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    A.count[5u * dst + c] = cnt[c];
                    A.first[5u * dst + c] = fst[c];
                }
            }
        }
        tbase += (uint32_t)__popcll(bt);
        qbase += (uint32_t)__popcll(bq);
    }
}

}  // namespace dmx

using namespace dmx;

namespace {

// `who` is the entry point's name: it opens every message.
#define PD_CK(who, call)                                                                     \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            c->err = std::string(who) + ": " + #call + ": " + hipGetErrorString(e_);         \
            return DMX_E_HIP;                                                                \
        }                                                                                    \
    } while (0)

constexpr size_t kPaTraceEntry = sizeof(ulonglong2) + sizeof(uint16_t);   // bytes per word-step
constexpr size_t kPaTraceMbDefault = 1024;                                // DMX_PA_TRACE_MB
constexpr size_t kPdNoBudget = ~(size_t)0;                                // no trace: no budget

// A number from the environment: `dflt` when unset or 0, `most` at most.
size_t pd_env(const char* name, size_t dflt, size_t most) {
    const char* e = std::getenv(name);
    const size_t v = e ? (size_t)std::strtoull(e, nullptr, 10) : 0;
    return std::min(v ? v : dflt, most);
}
// Pairs per launch: the place in the chunk has 24 bits of the sort key.
size_t pd_chunk() { return pd_env("DMX_PD_CHUNK", kPdChunkDefault, 1u << 24); }
// Bytes of trace per launch.
size_t pa_trace_budget() { return pd_env("DMX_PA_TRACE_MB", kPaTraceMbDefault, (size_t)1 << 20) << 20; }

int pd_group_size(uint32_t m) {
    const uint32_t mw = std::min<uint32_t>((m + 63u) / 64u, 64u);
    for (int k = 0; k < kPdNSizes; ++k)
        if ((uint32_t)kPdSizes[k] >= mw) return kPdSizes[k];
    return 64;
}

// Arguments every form checks the same way.  0, or the code with *err set.
int pd_validate(const char* who, int mode, const uint32_t* lens, size_t n_reads, const uint32_t* q,
                const uint32_t* t, const uint8_t* flags, size_t n_pairs, std::string* err) {
    const std::string name = std::string(who) + ": ";
    if (mode != DMX_PD_NW && mode != DMX_PD_HW) {
        *err = name + "mode must be DMX_PD_NW or DMX_PD_HW";
        return DMX_E_INVALID;
    }
    for (size_t i = 0; i < n_pairs; ++i) {
        if (q[i] >= n_reads || t[i] >= n_reads) {
            *err = name + "pair " + std::to_string(i) + " names a read outside the batch";
            return DMX_E_INVALID;
        }
        if (flags && (flags[i] & ~DMX_PD_RC)) {
            *err = name + "pair " + std::to_string(i) + " has an unknown flag";
            return DMX_E_INVALID;
        }
    }
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t m = lens[q[i]], n = lens[t[i]];
        if (m < 1 || n < 1 || m > DMX_PD_MAX_LEN || n > DMX_PD_MAX_LEN) {
            *err = name + "pair " + std::to_string(i) + ": reads of 1.." +
                   std::to_string(DMX_PD_MAX_LEN) + " nt supported";
            return DMX_E_UNSUPPORTED;
        }
    }
    return DMX_OK;
}

// The rows a call gives (dmx_rowdist, dmx_rowpairdist / dmx_rowhits, dmx_rowassign): offsets and
// mask bits checked; rowlen[g] becomes the length of row g, clamped at DMX_PD_MAX_LEN + 1 (a
// length above the limit is refused by the caller, for the pairs that name the row).  `name`
// opens the message.
int pd_rows_validate(const std::string& name, size_t n_rows, const uint8_t* masks,
                     const uint64_t* row_off, std::vector<uint32_t>& rowlen, std::string* err) {
    rowlen.assign(n_rows, 0);
    for (size_t g = 0; g < n_rows; ++g) {
        if (row_off[g + 1] < row_off[g]) {
            *err = name + "row " + std::to_string(g) + ": offsets must not decrease";
            return DMX_E_INVALID;
        }
        for (uint64_t x = row_off[g]; x < row_off[g + 1]; ++x)
            if (masks[x] & 0xE0u) {
                *err = name + "row " + std::to_string(g) + ": column " +
                       std::to_string(x - row_off[g]) + " has a mask bit above the five symbols";
                return DMX_E_INVALID;
            }
        rowlen[g] = (uint32_t)std::min<uint64_t>(row_off[g + 1] - row_off[g], DMX_PD_MAX_LEN + 1u);
    }
    return DMX_OK;
}

// pd_validate for dmx_pairalign (NW), and the room the paths may need.
int pa_validate(const uint32_t* lens, size_t n_reads, const uint32_t* q, const uint32_t* t,
                const uint8_t* flags, size_t n_pairs, size_t ops_cap, std::string* err) {
    if (const int rc = pd_validate("dmx_pairalign", DMX_PD_NW, lens, n_reads, q, t, flags, n_pairs,
                                   err))
        return rc;
    size_t need = 0;
    for (size_t i = 0; i < n_pairs; ++i) need += (size_t)lens[q[i]] + lens[t[i]];
    if (ops_cap < need) {
        *err = "dmx_pairalign: ops_cap " + std::to_string(ops_cap) + " is below the " +
               std::to_string(need) + " bytes the paths may take (sum of both lengths)";
        return DMX_E_INVALID;
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

// The whole (m + 1) x (n + 1) matrix of query a against target b; returns D(m, n).
// eq(x, y): does query symbol x equal target entry y (a symbol, or a row's mask)?
// mode DMX_PD_HW (dmx_rowpairdist_host): row 0 is free and the result is the least of row m.
template <class Eq>
uint32_t pa_dp_matrix(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b,
                      std::vector<uint16_t>& D, Eq eq, int mode = DMX_PD_NW) {
    const size_t m = a.size(), n = b.size(), W = n + 1;
    D.resize((m + 1) * W);
    for (size_t j = 0; j <= n; ++j) D[j] = mode == DMX_PD_NW ? (uint16_t)j : (uint16_t)0;
    for (size_t i = 1; i <= m; ++i) {
        uint16_t* row = &D[i * W];
        const uint16_t* up = row - W;
        row[0] = (uint16_t)i;
        const uint8_t ai = a[i - 1];
        for (size_t j = 1; j <= n; ++j) {
            const uint32_t sub = up[j - 1] + (eq(ai, b[j - 1]) ? 0u : 1u);
            row[j] = (uint16_t)std::min<uint32_t>(sub, std::min<uint32_t>(up[j], row[j - 1]) + 1u);
        }
    }
    if (mode != DMX_PD_NW) return *std::min_element(D.begin() + m * W, D.begin() + (m + 1) * W);
    return D[m * W + n];
}

// That matrix, then the walk back from (m, n) by the contract's rule: up (INSERT) before left
// (DELETE) before the diagonal.  The ops come out last first in `rev`.
template <class Eq>
uint32_t pa_dp_path(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b,
                    std::vector<uint16_t>& D, std::vector<uint8_t>& rev, Eq eq) {
    const size_t m = a.size(), n = b.size(), W = n + 1;
    pa_dp_matrix(a, b, D, eq);
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
            rev.push_back(eq(a[i - 1], b[j - 1]) ? DMX_PA_MATCH : DMX_PA_MISMATCH), --i, --j;
        }
    }
    return D[m * W + n];
}

// work(k, nth) for k = 0 .. nth - 1 on nth <= n_threads threads; worker k takes pairs k, k + nth,
// ... (interleaved: similar work per thread).
template <class F>
void pd_parallel(size_t n_pairs, int n_threads, F work) {
    const size_t nth = std::min<size_t>((size_t)std::max(n_threads, 1), std::max<size_t>(n_pairs, 1));
    if (nth == 1) return work(0, 1);
    std::vector<std::thread> th;
    for (size_t k = 0; k < nth; ++k) th.emplace_back(work, k, nth);
    for (auto& x : th) x.join();
}

// The lengths of the resident batch, for the validation on the host before anything is
// launched (a copy, no kernel).  With an operand table the lengths are the
// operands', one entry each: every index of the call names an operand.
int pd_fetch_lens(Ctx* c, const char* who, size_t n_pairs, std::vector<uint32_t>& lens) {
    if (c->d_seq && c->ops_on) {   // the table's host mirror: one copy per table, not per call
        if (const int rc = ops_mirror(c, who)) return rc;
        lens = c->h_op_len;
        return DMX_OK;
    }
    lens.resize(c->d_seq ? c->n_reads : 0);
    if (!lens.empty() && n_pairs) {
        PD_CK(who, hipSetDevice(c->device));
        PD_CK(who, hipMemcpy(lens.data(), c->in.lens.p, lens.size() * 4, hipMemcpyDeviceToHost));
    }
    return DMX_OK;
}

// The operands' strands, one byte each; left empty without a table or when every operand is on
// strand 0 (the calls then run as they do on reads).  A strand is never seen by a kernel as such:
// the host folds it into the pair's DMX_PD_RC (read against read, a group's member) or into the
// copy of the row a pair is compared with (read against row).
int pd_fetch_strands(Ctx* c, const char* who, std::vector<uint8_t>& strands) {
    strands.clear();
    if (!c->d_seq || !c->ops_on || !c->n_ops) return DMX_OK;
    if (const int rc = ops_mirror(c, who)) return rc;
    if (c->h_op_any) strands = c->h_op_strand;
    return DMX_OK;
}

// Where the forms find their reads: the batch's offsets and lengths, or the operand table's.
inline const uint64_t* pd_offs(const Ctx* c) { return c->ops_on ? c->d_op_off.p : c->in.offs.p; }
inline const uint32_t* pd_lens(const Ctx* c) { return c->ops_on ? c->d_op_len.p : c->in.lens.p; }
// make_bounds for a kernel that indexes them (DMX_DEBUG_BOUNDS builds).
inline Bounds pd_bounds(const Ctx* c, int kid) {
    Bounds b = make_bounds(c, kid);
#ifdef DMX_DEBUG_BOUNDS
    if (c->ops_on) b.reads = c->n_ops;
#endif
    return b;
}

// The context's state of one form, made by the form's first call.
template <class State>
int pd_state(Ctx* c, const char* who, State*& s) {
    if (!s) {
        s = new State();
        for (auto& e : s->ev) PD_CK(who, hipEventCreate(&e));
    }
    return DMX_OK;
}

// One launch: the pairs of a chunk in the order they run, cut into waves.
template <class Pair>
struct PdPlan {
    std::vector<uint64_t> keys;   // sorted: (G, target length, place in the chunk), see place()
    std::vector<Pair> pairs;
    std::vector<PdWave> waves;
    size_t scratch = 0, trace = 0, ops = 0;   // totals: scratch bytes, trace entries, op bytes
    size_t place(size_t k) const { return (size_t)(keys[k] & 0xFFFFFFu); }   // of sorted pair k
};

// Plans the chunk that starts at pair `lo` and returns its end: up to max_pairs pairs, fewer
// when their scratch rows fill kPdScratchMax or their traces (kPaTraceEntry bytes per word and
// column) the budget; one pair at least.  The pairs are sorted by group size, then target
// length (similar step counts share a wave), longest first, and packed into waves of one group
// size, 64 / G groups at most.  tn (dmx_groupalign, dmx_rowdist): pair i's target is not read
// t[i] but a row of tn[i] columns (t[i] is then the pair's group or row, and the caller fills in
// where the row lies).
template <class Pair>
size_t pd_plan(PdPlan<Pair>& pl, const uint32_t* lens, const uint32_t* q, const uint32_t* t,
               const uint8_t* flags, const uint32_t* caps, size_t n_pairs, size_t lo,
               size_t max_pairs, size_t trace_budget, const uint32_t* tn = nullptr) {
    size_t hi = lo, scratch = 0, trace = 0;
    pl.keys.clear();
    while (hi < n_pairs && hi - lo < max_pairs) {
        const uint32_t m = lens[q[hi]], n = tn ? tn[hi] : lens[t[hi]];
        const size_t need = m > 64u * 64u ? n : 0;
        const size_t steps = (size_t)((m + 63u) / 64u) * n;
        if (hi > lo && (scratch + need > kPdScratchMax ||
                        (trace + steps) * kPaTraceEntry > trace_budget))
            break;
        scratch += need;
        trace += steps;
        pl.keys.push_back(((uint64_t)pd_group_size(m) << 48) | ((uint64_t)n << 24) |
                          (uint64_t)(hi - lo));
        ++hi;
    }
    const size_t np = hi - lo;
    std::sort(pl.keys.begin(), pl.keys.end(), std::greater<uint64_t>());
    pl.pairs.resize(np);
    pl.waves.clear();
    pl.scratch = pl.trace = pl.ops = 0;
    for (size_t k = 0; k < np;) {
        const uint32_t G = (uint32_t)(pl.keys[k] >> 48);
        const uint32_t per = 64u / G;
        PdWave W{(uint32_t)k, 0, G, 0};
        while (k < np && W.count < per && (uint32_t)(pl.keys[k] >> 48) == G) {
            const size_t i = lo + pl.place(k);
            const uint32_t m = lens[q[i]], n = tn ? tn[i] : lens[t[i]];
            const uint32_t mw = (m + 63u) / 64u, S = (mw + G - 1u) / G;
            Pair& P = pl.pairs[k];
            P.q = q[i];
            P.t = t[i];
            P.cap = caps ? caps[i] : 0u;
            P.flags = (flags ? (flags[i] & DMX_PD_RC) : 0u) | (caps ? 0x100u : 0u);
            P.soff = pl.scratch;
            if constexpr (std::is_base_of<PaPair, Pair>::value) {
                P.toff = pl.trace;
                P.roff = pl.ops;
            }
            if constexpr (kPdRowPair<Pair>) P.n = n;
            if (S > 1) pl.scratch += n;
            pl.trace += (size_t)mw * n;
            pl.ops += (size_t)m + n;
            W.steps = std::max(W.steps, S * (n + G));
            ++W.count;
            ++k;
        }
        pl.waves.push_back(W);
    }
    return hi;
}

// Stages a planned launch: room for its pairs, waves, scratch rows and out_words of output, the
// upload, the bounds record's reset, and the arguments every form's kernels take.
template <class Pair>
int pd_stage(Ctx* c, const char* who, PdBufs<Pair>& b, const PdPlan<Pair>& pl, size_t out_words,
             int kid, PdHead<Pair>& A) {
    const size_t np = pl.pairs.size(), nw = pl.waves.size();
    hipStream_t st = c->stream;
    PD_CK(who, b.pairs.reserve(np));
    PD_CK(who, b.out.reserve(out_words));
    PD_CK(who, b.waves.reserve(nw));
    PD_CK(who, b.scratch.reserve(pl.scratch));
    PD_CK(who, hipMemcpyAsync(b.pairs.p, pl.pairs.data(), np * sizeof(Pair), hipMemcpyHostToDevice,
                              st));
    PD_CK(who, hipMemcpyAsync(b.waves.p, pl.waves.data(), nw * sizeof(PdWave),
                              hipMemcpyHostToDevice, st));
    PD_CK(who, bounds_reset(c, st));
    A.pk.seq = c->d_seq;
    A.pk.nmask = c->d_nmask;
    A.pk.bd = pd_bounds(c, kid);
    A.offs = pd_offs(c);
    A.lens = pd_lens(c);
    A.pairs = b.pairs.p;
    A.waves = b.waves.p;
    A.n_waves = (uint32_t)nw;
    A.n_pairs = (uint32_t)np;
    A.scratch = b.scratch.p;
    A.scratch_bytes = b.scratch.cap;
    return DMX_OK;
}

template <class Args>
void pd_launch_forward(void (*kernel)(Args), const Args& A, hipStream_t st) {
    const uint32_t nb = (A.n_waves + kPdWavesPerBlock - 1u) / kPdWavesPerBlock;
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(64 * kPdWavesPerBlock), 0, st, A);
}

// After a launch: its error, if it made one, and the event that ends it.
int pd_mark(Ctx* c, const char* who, hipEvent_t ev) {
    PD_CK(who, hipGetLastError());
    PD_CK(who, hipEventRecord(ev, c->stream));
    return DMX_OK;
}

// The end of a launch group, after its launches and downloads are on the stream: waits for them
// (synced: the caller already has), checks the bounds record (DMX_DEBUG_BOUNDS builds) and adds
// the time between ev[k] and ev[k + 1] to ms[k] for the n events of the group.
int pd_finish(Ctx* c, const char* who, const hipEvent_t* ev, int n, float* ms, bool synced = false) {
    hipStream_t st = c->stream;
    if (!synced) PD_CK(who, hipStreamSynchronize(st));
    if (const int brc = bounds_check(c, who)) return brc;
    for (int k = 0; k + 1 < n; ++k) {
        float t = 0.f;
        hipEventElapsedTime(&t, ev[k], ev[k + 1]);
        ms[k] += t;
    }
    return DMX_OK;
}

// The trace form's share of a staged launch (PaArgs, GaArgs): room for `trace` word-steps and
// `ops` path bytes, and the fields both of its kernels read.
template <class Args>
int pa_stage_trace(Ctx* c, const char* who, PaTrace& b, size_t trace, size_t ops, uint32_t* out,
                   Args& A) {
    PD_CK(who, b.pm.reserve(trace));
    PD_CK(who, b.sc.reserve(trace));
    PD_CK(who, b.ops.reserve(ops));
    A.pm = b.pm.p;
    A.sc = b.sc.p;
    A.trace_steps = std::min(b.pm.cap, b.sc.cap);
    A.ops = b.ops.p;
    A.ops_bytes = b.ops.cap;
    A.out = out;
    return DMX_OK;
}
template <class Args>
void pa_launch_traceback(void (*kernel)(Args), Args& A, int kid, hipStream_t st) {
    set_kid(A.pk.bd, kid);
    hipLaunchKernelGGL(kernel, dim3((A.n_pairs + kPaTbLanes - 1u) / kPaTbLanes), dim3(kPaTbLanes), 0,
                       st, A);
}
// A path of `len` ops between m rows and n columns: what the traceback can have written.
inline bool pa_path_ok(uint32_t len, uint32_t m, uint32_t n) {
    return len <= m + n && len >= std::max(m, n);
}

// The pairs a launch's retry bitmap names, appended to `retry` as places in the list the chunk
// [lo, hi) was cut from.  Bit b is the pair at place b of the chunk, or (sorted) the pair the
// plan ran as its b-th.
template <class Pair>
void pd_retry_list(const std::vector<uint32_t>& need, const PdPlan<Pair>& pl, size_t lo, size_t hi,
                   bool sorted, std::vector<uint32_t>& retry) {
    for (size_t w = 0; w < need.size(); ++w)
        for (uint32_t bits = need[w]; bits; bits &= bits - 1u) {
            const size_t b = 32 * w + (size_t)__builtin_ctz(bits);
            if (b < hi - lo) retry.push_back((uint32_t)(lo + (sorted ? pl.place(b) : b)));
        }
}
// v[at[k]] for every k: a column of the second pass's list.
template <class T>
std::vector<uint32_t> pd_pick(const T* v, const std::vector<uint32_t>& at) {
    std::vector<uint32_t> out(at.size());
    for (size_t k = 0; k < at.size(); ++k) out[k] = (uint32_t)v[at[k]];
    return out;
}

}  // namespace

int dmx::PdRows::upload(Ctx* c, const char* who) {
    PD_CK(who, mask.reserve(2 * total));
    PD_CK(who, hipMemcpyAsync(mask.p, image.data(), total, hipMemcpyHostToDevice, c->stream));
    return DMX_OK;
}

int dmx::PdRows::write_rc(Ctx* c, const char* who, const hipEvent_t* ev, float* ms) {
    if (written) return DMX_OK;
    hipStream_t st = c->stream;
    PD_CK(who, rows.reserve(used.size()));
    PD_CK(who, hipMemcpyAsync(rows.p, used.data(), used.size() * sizeof(RrRow),
                              hipMemcpyHostToDevice, st));
    PD_CK(who, bounds_reset(c, st));
    RrRcArgs R;
    R.bd = make_bounds(c, kKerRowpairRc);
    R.rows = rows.p;
    R.n_rows = (uint32_t)used.size();
    R.mask = mask.p;
    R.half = total;
    R.cols = 2 * total;
    PD_CK(who, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(rowpair_rc_kernel, dim3(R.n_rows), dim3(kRrRcBlock), 0, st, R);
    if (const int rc = pd_mark(c, who, ev[1])) return rc;
    if (const int rc = pd_finish(c, who, ev, 2, ms)) return rc;   // `used` is pageable
    written = true;
    return DMX_OK;
}

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
    if (const int rc = pd_validate("dmx_pairdist", mode, lens, n_reads, q, t, flags, n_pairs, &err)) {
        set_process_error(err);
        return rc;
    }
    pd_parallel(n_pairs, n_threads, [&](size_t k, size_t nth) {
        std::vector<uint8_t> a, b;
        std::vector<uint32_t> row;
        for (size_t i = k; i < n_pairs; i += nth) {
            pd_decode(seq2b, nmask, offsets[q[i]], lens[q[i]], false, a);
            pd_decode(seq2b, nmask, offsets[t[i]], lens[t[i]], flags && (flags[i] & DMX_PD_RC), b);
            uint32_t d = pd_dp(mode, a, b, row);
            if (caps && d > caps[i]) d = caps[i] + 1u;
            out[i] = d;
        }
    });
    return DMX_OK;
}

extern "C" int dmx_pairdist(dmx_ctx* c, int mode, const uint32_t* q, const uint32_t* t,
                            const uint8_t* flags, const uint32_t* caps, size_t n_pairs,
                            uint32_t* out) {
    const char* const who = "dmx_pairdist";
    if (!c) return DMX_E_INVALID;
    if (n_pairs && (!q || !t || !out)) {
        c->err = "dmx_pairdist: null pair list or output";
        return DMX_E_INVALID;
    }
    if (c->pd) c->pd->ms = 0.f;
    std::vector<uint32_t> lens;
    if (const int rc = pd_fetch_lens(c, who, n_pairs, lens)) return rc;
    if (const int rc = pd_validate(who, mode, lens.data(), lens.size(), q, t, flags, n_pairs,
                                   &c->err))
        return rc;
    if (!n_pairs) return DMX_OK;
    PD_CK(who, hipSetDevice(c->device));
    // operands: the pair's flag with both strands folded in; the query is never turned
    std::vector<uint8_t> strands, eff;
    if (const int rc = pd_fetch_strands(c, who, strands)) return rc;
    if (!strands.empty()) {
        eff.resize(n_pairs);
        for (size_t i = 0; i < n_pairs; ++i)
            eff[i] = (uint8_t)(((flags ? flags[i] : 0u) ^ strands[q[i]] ^ strands[t[i]]) & DMX_PD_RC);
        flags = eff.data();
    }
    if (const int rc = pd_state(c, who, c->pd)) return rc;
    PdState* s = c->pd;
    hipStream_t st = c->stream;
    const size_t chunk = pd_chunk();

    PdPlan<PdPair> pl;
    std::vector<uint32_t> res;
    float total_ms = 0.f;
    for (size_t lo = 0; lo < n_pairs;) {
        const size_t hi = pd_plan(pl, lens.data(), q, t, flags, caps, n_pairs, lo, chunk,
                                  kPdNoBudget);
        const size_t np = hi - lo;
        PdArgs A;
        if (const int rc = pd_stage(c, who, *s, pl, np, kKerPairdist, A)) return rc;
        A.mode = mode;
        A.out = s->out.p;
        PD_CK(who, hipEventRecord(s->ev[0], st));
        pd_launch_forward(pairdist_kernel, A, st);
        if (const int rc = pd_mark(c, who, s->ev[1])) return rc;
        res.resize(np);
        PD_CK(who, hipMemcpyAsync(res.data(), A.out, np * 4, hipMemcpyDeviceToHost, st));
        if (const int rc = pd_finish(c, who, s->ev, 2, &total_ms)) return rc;
        for (size_t k = 0; k < np; ++k) out[lo + pl.place(k)] = res[k];
        lo = hi;
    }
    s->ms = total_ms;
    return DMX_OK;
}

// ---- dmx_pairhits: dmx_pairdist's launches, the hit decision on the device ------
// The distances of a launch stay in the distance form's output buffer; dmx_groups.hip turns them
// into outcomes there (lg_hits_decide) and only the bitmap of the pairs to retry on the reverse
// complement comes back.  The retries of all chunks are planned again as a list of their own.

extern "C" int dmx_pairhits(dmx_ctx* c, const uint32_t* q, const uint32_t* t,
                            const int32_t* cap_hit, const int32_t* cap_half, size_t n_pairs,
                            uint32_t* best, uint64_t* n_hits) {
    const char* const who = "dmx_pairhits";
    if (!c) return DMX_E_INVALID;
    lg_invalidate(c);
    // with an operand table the per-read arrays of this call and of those that read its outcomes
    // have one entry per operand
    const size_t n_reads = !c->d_seq ? 0 : c->ops_on ? c->n_ops : c->n_reads;
    if (!n_hits || (n_reads && !best) || (n_pairs && (!q || !t || !cap_hit || !cap_half))) {
        c->err = "dmx_pairhits: null pair list, caps or output";
        return DMX_E_INVALID;
    }
    if (n_pairs > DMX_LG_MAX_PAIRS) {
        c->err = "dmx_pairhits: at most " + std::to_string(DMX_LG_MAX_PAIRS) + " pairs supported";
        return DMX_E_UNSUPPORTED;
    }
    std::vector<uint32_t> lens;
    if (const int rc = pd_fetch_lens(c, who, n_pairs, lens)) return rc;
    if (const int rc = pd_validate(who, DMX_PD_NW, lens.data(), lens.size(), q, t, nullptr, n_pairs,
                                   &c->err))
        return rc;
    std::vector<uint32_t> fcap(n_pairs);
    for (size_t i = 0; i < n_pairs; ++i) {
        if (cap_hit[i] < -1 || cap_half[i] < -1) {
            c->err = "dmx_pairhits: pair " + std::to_string(i) +
                     ": a cap is a distance, or -1 for none";
            return DMX_E_INVALID;
        }
        fcap[i] = (uint32_t)std::max(std::max(cap_hit[i], cap_half[i]), 0);
    }
    PD_CK(who, hipSetDevice(c->device));
    // operands: the forward comparison's flag is the two strands', the retry's that flag toggled
    std::vector<uint8_t> strands, fwd;
    if (n_pairs)
        if (const int rc = pd_fetch_strands(c, who, strands)) return rc;
    if (!strands.empty()) {
        fwd.resize(n_pairs);
        for (size_t i = 0; i < n_pairs; ++i) fwd[i] = (uint8_t)((strands[q[i]] ^ strands[t[i]]) & 1u);
    }
    if (const int rc = lg_hits_begin(c, who, q, t, cap_hit, cap_half, n_pairs, n_reads)) return rc;
    float total_ms = 0.f;
    if (n_pairs) {
        if (const int rc = pd_state(c, who, c->pd)) return rc;
        PdState* s = c->pd;   // dmx_pairdist's buffers; its ms stays its own
        hipStream_t st = c->stream;
        const size_t chunk = pd_chunk();
        PdPlan<PdPair> pl;
        std::vector<uint32_t> orig, need, retry;
        // one launch of pairs[lo .. ) of a list; in[k]: the input pair of the list's pair k
        auto launch = [&](const uint32_t* lq, const uint32_t* lt, const uint8_t* lf,
                          const uint32_t* lcap, size_t n, size_t lo, const uint32_t* in, int pass,
                          size_t* end) -> int {
            const size_t hi = pd_plan(pl, lens.data(), lq, lt, lf, lcap, n, lo, chunk, kPdNoBudget);
            const size_t np = hi - lo;
            PdArgs A;
            if (const int rc = pd_stage(c, who, *s, pl, np, kKerPairdist, A)) return rc;
            A.mode = DMX_PD_NW;
            A.out = s->out.p;
            PD_CK(who, hipEventRecord(s->ev[0], st));
            pd_launch_forward(pairdist_kernel, A, st);
            if (const int rc = pd_mark(c, who, s->ev[1])) return rc;
            orig.resize(np);
            for (size_t k = 0; k < np; ++k)
                orig[k] = in ? in[lo + pl.place(k)] : (uint32_t)(lo + pl.place(k));
            if (const int rc = lg_hits_decide(c, who, A.out, orig.data(), np, pass, lo, &need))
                return rc;   // has synchronised
            *end = hi;
            return pd_finish(c, who, s->ev, 2, &total_ms, /*synced=*/true);
        };
        for (size_t lo = 0, hi = 0; lo < n_pairs; lo = hi) {
            if (const int rc = launch(q, t, fwd.empty() ? nullptr : fwd.data(), fcap.data(), n_pairs,
                                      lo, nullptr, 0, &hi))
                return rc;
            // the decision sets bit i - lo for input pair i: the place in the chunk
            pd_retry_list(need, pl, lo, hi, /*sorted=*/false, retry);
        }
        const size_t n2 = retry.size();
        // the second pass's list; a cap is >= 0 where a retry is asked for
        const std::vector<uint32_t> q2 = pd_pick(q, retry), t2 = pd_pick(t, retry),
                                    cap2 = pd_pick(cap_hit, retry);
        std::vector<uint8_t> rc2(n2, DMX_PD_RC);
        for (size_t k = 0; k < n2 && !fwd.empty(); ++k) rc2[k] = (uint8_t)(DMX_PD_RC ^ fwd[retry[k]]);
        for (size_t lo = 0, hi = 0; lo < n2; lo = hi)
            if (const int rc = launch(q2.data(), t2.data(), rc2.data(), cap2.data(), n2, lo,
                                      retry.data(), 1, &hi))
                return rc;
    }
    return lg_hits_end(c, who, total_ms, best, n_hits);
}

// ---- dmx_pairalign: the NW distance and the edit path (include/dmx.h) -----------

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
    pd_parallel(n_pairs, n_threads, [&](size_t k, size_t nth) {
        std::vector<uint8_t> a, b, rev;
        std::vector<uint16_t> D;
        for (size_t i = k; i < n_pairs; i += nth) {
            pd_decode(seq2b, nmask, offsets[q[i]], lens[q[i]], false, a);
            pd_decode(seq2b, nmask, offsets[t[i]], lens[t[i]], flags && (flags[i] & DMX_PD_RC), b);
            dist[i] = pa_dp_path(a, b, D, rev, [](uint8_t x, uint8_t y) { return x == y; });
            plen[i] = (uint32_t)rev.size();
            std::reverse_copy(rev.begin(), rev.end(), ops + roff[i + 1] - rev.size());
        }
    });
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
    const char* const who = "dmx_pairalign";
    if (!c) return DMX_E_INVALID;
    if (!op_off || (n_pairs && (!q || !t || !dist || !ops))) {
        c->err = "dmx_pairalign: null pair list or output";
        return DMX_E_INVALID;
    }
    if (c->ops_on) {
        c->err = "dmx_pairalign: not supported with an operand table (dmx_clear_operands first; "
                 "dmx_groupalign_strands aligns operands)";
        return DMX_E_UNSUPPORTED;
    }
    if (c->pa) {
        c->pa->ms[0] = c->pa->ms[1] = 0.f;
        c->pa->launches = 0;
    }
    std::vector<uint32_t> lens;
    if (const int rc = pd_fetch_lens(c, who, n_pairs, lens)) return rc;
    if (const int rc = pa_validate(lens.data(), lens.size(), q, t, flags, n_pairs, ops_cap, &c->err))
        return rc;
    op_off[0] = 0;
    if (!n_pairs) return DMX_OK;
    PD_CK(who, hipSetDevice(c->device));
    if (const int rc = pd_state(c, who, c->pa)) return rc;
    PaState* s = c->pa;
    hipStream_t st = c->stream;
    const size_t budget = pa_trace_budget();

    PdPlan<PaPair> pl;
    std::vector<uint32_t> res, place;
    std::vector<uint8_t> region;
    float ms2[2] = {0.f, 0.f};   // forward pass, traceback
    uint64_t at = 0;   // bytes of `ops` filled
    for (size_t lo = 0; lo < n_pairs;) {
        const size_t hi = pd_plan(pl, lens.data(), q, t, flags, nullptr, n_pairs, lo,
                                  kPdChunkDefault, budget);
        const size_t np = hi - lo;
        PaArgs A;
        if (const int rc = pd_stage(c, who, *s, pl, 2 * np, kKerPairalign, A)) return rc;
        if (const int rc = pa_stage_trace(c, who, *s, pl.trace, pl.ops, s->out.p, A)) return rc;
        PD_CK(who, hipEventRecord(s->ev[0], st));
        pd_launch_forward(pairalign_kernel, A, st);
        if (const int rc = pd_mark(c, who, s->ev[1])) return rc;
        pa_launch_traceback(pairalign_traceback_kernel, A, kKerPairalignTb, st);
        if (const int rc = pd_mark(c, who, s->ev[2])) return rc;
        res.resize(2 * np);
        region.resize(pl.ops);
        PD_CK(who, hipMemcpyAsync(res.data(), A.out, 2 * np * 4, hipMemcpyDeviceToHost, st));
        PD_CK(who, hipMemcpyAsync(region.data(), A.ops, pl.ops, hipMemcpyDeviceToHost, st));
        if (const int rc = pd_finish(c, who, s->ev, 3, ms2)) return rc;
        ++s->launches;
        // the chunk's paths in the caller's pair order: pair lo + x ran at sorted place[x]
        place.resize(np);
        for (size_t k = 0; k < np; ++k) place[pl.place(k)] = (uint32_t)k;
        for (size_t x = 0; x < np; ++x) {
            const size_t k = place[x];
            const uint32_t m = lens[q[lo + x]], n = lens[t[lo + x]];
            const uint32_t len = res[2 * k + 1];
            if (!pa_path_ok(len, m, n)) {
                c->err = "dmx_pairalign: pair " + std::to_string(lo + x) + ": path of " +
                         std::to_string(len) + " ops for reads of " + std::to_string(m) + " and " +
                         std::to_string(n) + " nt";
                return DMX_E_STATE;
            }
            dist[lo + x] = res[2 * k];
            op_off[lo + x] = at;
            std::memcpy(ops + at, region.data() + pl.pairs[k].roff + (m + n - len), len);
            at += len;
        }
        lo = hi;
    }
    op_off[n_pairs] = at;
    s->ms[0] = ms2[0], s->ms[1] = ms2[1];
    return DMX_OK;
}

// ---- dmx_groupalign: progressive alignment of read groups (include/dmx.h) --------

namespace {

constexpr size_t kGaMaxMembers = 65535;   // count and first are 16 bits wide

// What the checked arguments come to: the cap on a row, the columns a group's row may grow to
// (its seed and every member inserted whole, the cap at most) and the sums the outputs must hold.
struct GaShape {
    uint32_t max_cols = 0;
    std::vector<uint32_t> bound;   // per group
    size_t cols = 0;               // sum of the bounds
    size_t ops = 0;                // sum over the members of the bound of the row they leave
    size_t members = 0, rounds = 0;
};

// Every argument check of both entry points, naming the group.  0, or the code with *err set.
int ga_validate(const char* who, const uint32_t* lens, size_t n_reads, size_t n_groups,
                const uint8_t* seed_masks, const uint64_t* seed_off, const uint32_t* members,
                const uint8_t* member_flags, const uint64_t* member_off, uint32_t max_cols,
                size_t cols_cap, bool want_ops, size_t ops_cap, GaShape& sh, std::string* err) {
    const std::string name = std::string(who) + ": ";
    if (max_cols > DMX_PD_MAX_LEN) {
        *err = name + "max_cols " + std::to_string(max_cols) + " is above " +
               std::to_string(DMX_PD_MAX_LEN);
        return DMX_E_UNSUPPORTED;
    }
    sh.max_cols = max_cols ? max_cols : DMX_PD_MAX_LEN;
    sh.bound.assign(n_groups, 0);
    for (size_t g = 0; g < n_groups; ++g) {
        const std::string grp = name + "group " + std::to_string(g) + ": ";
        if (seed_off[g + 1] < seed_off[g] || member_off[g + 1] < member_off[g]) {
            *err = grp + "offsets must not decrease";
            return DMX_E_INVALID;
        }
        const uint64_t sl = seed_off[g + 1] - seed_off[g], nm = member_off[g + 1] - member_off[g];
        if (sl < 1 || sl > sh.max_cols) {
            *err = grp + "a seed row of " + std::to_string(sl) + " columns (1.." +
                   std::to_string(sh.max_cols) + " supported)";
            return DMX_E_UNSUPPORTED;
        }
        if (nm > kGaMaxMembers) {
            *err = grp + std::to_string(nm) + " members (" + std::to_string(kGaMaxMembers) +
                   " at most)";
            return DMX_E_UNSUPPORTED;
        }
        for (uint64_t x = seed_off[g]; x < seed_off[g + 1]; ++x)
            if (seed_masks[x] & 0xE0u) {
                *err = grp + "seed column " + std::to_string(x - seed_off[g]) +
                       " has a mask bit above the five symbols";
                return DMX_E_INVALID;
            }
        uint64_t grow = sl;
        for (uint64_t x = member_off[g]; x < member_off[g + 1]; ++x) {
            if (members[x] >= n_reads) {
                *err = grp + "member " + std::to_string(x - member_off[g]) +
                       " names a read outside the batch";
                return DMX_E_INVALID;
            }
            if (member_flags && (member_flags[x] & ~DMX_PD_RC)) {
                *err = grp + "member " + std::to_string(x - member_off[g]) +
                       " has an unknown flag";
                return DMX_E_INVALID;
            }
            const uint32_t m = lens[members[x]];
            if (m < 1 || m > DMX_PD_MAX_LEN) {
                *err = grp + "member " + std::to_string(x - member_off[g]) + ": reads of 1.." +
                       std::to_string(DMX_PD_MAX_LEN) + " nt supported";
                return DMX_E_UNSUPPORTED;
            }
            grow = std::min<uint64_t>(grow + m, sh.max_cols);
            sh.ops += grow;
        }
        sh.bound[g] = (uint32_t)grow;
        sh.cols += grow;
        sh.members += nm;
        sh.rounds = std::max<size_t>(sh.rounds, nm);
    }
    if (cols_cap < sh.cols) {
        *err = name + "cols_cap " + std::to_string(cols_cap) + " is below the " +
               std::to_string(sh.cols) + " columns the rows may take (per group: seed and " +
               "member lengths, max_cols at most)";
        return DMX_E_INVALID;
    }
    if (want_ops && ops_cap < sh.ops) {
        *err = name + "ops_cap " + std::to_string(ops_cap) + " is below the " +
               std::to_string(sh.ops) + " bytes the paths may take";
        return DMX_E_INVALID;
    }
    return DMX_OK;
}

std::string ga_overflow(const char* who, size_t g, size_t round, uint32_t len, uint32_t max_cols) {
    return std::string(who) + ": group " + std::to_string(g) + ", round " + std::to_string(round) +
           ": the row would grow to " + std::to_string(len) + " columns, above max_cols " +
           std::to_string(max_cols);
}

// The members' paths in the caller's order, closed up.
void ga_emit_paths(const std::vector<std::vector<uint8_t>>& paths, uint64_t* op_off, uint8_t* ops) {
    uint64_t at = 0;
    for (size_t x = 0; x < paths.size(); ++x) {
        op_off[x] = at;
        if (!paths[x].empty()) std::memcpy(ops + at, paths[x].data(), paths[x].size());
        at += paths[x].size();
    }
    op_off[paths.size()] = at;
}

}  // namespace

extern "C" int dmx_groupalign_stats(dmx_ctx* c, float* ms, int n_ms, int* rounds) {
    if (!c) return DMX_E_INVALID;
    for (int k = 0; k < n_ms && k < 3 && ms; ++k) ms[k] = c->ga ? c->ga->ms[k] : 0.f;
    if (rounds) *rounds = c->ga ? c->ga->rounds : 0;
    return c->ga ? c->ga->launches : 0;
}

// Both host entry points: member_flags == NULL is dmx_groupalign_host (`who` opens the messages).
static int ga_host(const char* who, const uint32_t* seq2b, const uint32_t* nmask,
                   const uint64_t* offsets, const uint32_t* lens, size_t n_reads, size_t n_groups,
                   const uint8_t* seed_masks, const uint64_t* seed_off, const uint32_t* members,
                   const uint8_t* member_flags, const uint64_t* member_off, uint32_t max_cols,
                   uint64_t* col_off, uint8_t* mask, uint16_t* count, uint16_t* first,
                   size_t cols_cap, uint32_t* dist, uint64_t* op_off, uint8_t* ops, size_t ops_cap,
                   int n_threads) {
    const bool some = n_groups && member_off && member_off[n_groups] > member_off[0];
    if (!seed_off || !member_off || !col_off || (ops && !op_off) ||
        (n_groups && (!seed_masks || !mask || !count || !first)) ||
        (some && (!members || !dist || !seq2b || !nmask || !offsets || !lens))) {
        set_process_error(std::string(who) + ": null argument");
        return DMX_E_INVALID;
    }
    GaShape sh;
    std::string err;
    if (const int rc = ga_validate(who, lens, n_reads, n_groups, seed_masks, seed_off, members,
                                   member_flags, member_off, max_cols, cols_cap, ops != nullptr,
                                   ops_cap, sh, &err)) {
        set_process_error(err);
        return rc;
    }
    struct Cols {
        std::vector<uint8_t> mask;
        std::vector<uint16_t> count, first;
    };
    std::vector<Cols> rows(n_groups);
    std::vector<std::vector<uint8_t>> paths(ops ? sh.members : 0);
    std::vector<std::string> errs(n_groups);
    const uint64_t m0 = n_groups ? member_off[0] : 0;
    pd_parallel(n_groups, n_threads, [&](size_t k, size_t nth) {
        std::vector<uint8_t> a, rev;
        std::vector<uint16_t> D;
        for (size_t g = k; g < n_groups; g += nth) {
            Cols cur, nxt;
            cur.mask.assign(seed_masks + seed_off[g], seed_masks + seed_off[g + 1]);
            cur.count.assign(5 * cur.mask.size(), 0);
            cur.first.assign(5 * cur.mask.size(), 0);
            for (uint64_t x = member_off[g]; x < member_off[g + 1]; ++x) {
                const size_t r = (size_t)(x - member_off[g]);
                pd_decode(seq2b, nmask, offsets[members[x]], lens[members[x]],
                          member_flags && (member_flags[x] & DMX_PD_RC), a);
                const uint32_t d = pa_dp_path(a, cur.mask, D, rev, [](uint8_t sym, uint8_t mk) {
                    return ((mk >> sym) & 1u) != 0;
                });
                const size_t len = rev.size();
                if (len > sh.max_cols) {
                    errs[g] = ga_overflow(who, g, r, (uint32_t)len, sh.max_cols);
                    break;
                }
                dist[x - m0] = d;
                nxt.mask.assign(len, 0);
                nxt.count.assign(5 * len, 0);
                nxt.first.assign(5 * len, 0);
                size_t tj = 0, qi = 0;
                for (size_t col = 0; col < len; ++col) {
                    const uint8_t op = rev[len - 1 - col];
                    if (op != DMX_PA_INSERT) {   // the old column moves here
                        nxt.mask[col] = cur.mask[tj];
                        for (int s = 0; s < 5; ++s) {
                            nxt.count[5 * col + s] = cur.count[5 * tj + s];
                            nxt.first[5 * col + s] = cur.first[5 * tj + s];
                        }
                        ++tj;
                    }
                    if (op != DMX_PA_DELETE) {   // the member shows a symbol here
                        const uint8_t sym = a[qi++];
                        if (nxt.count[5 * col + sym]++ == 0) nxt.first[5 * col + sym] = (uint16_t)(r + 1);
                    }
                }
                if (ops) paths[x - m0].assign(rev.rbegin(), rev.rend());
                std::swap(cur, nxt);
            }
            rows[g] = std::move(cur);
        }
    });
    for (size_t g = 0; g < n_groups; ++g)
        if (!errs[g].empty()) {
            set_process_error(errs[g]);
            return DMX_E_UNSUPPORTED;
        }
    uint64_t at = 0;
    for (size_t g = 0; g < n_groups; ++g) {
        const size_t len = rows[g].mask.size();
        col_off[g] = at;
        std::memcpy(mask + at, rows[g].mask.data(), len);
        std::memcpy(count + 5 * at, rows[g].count.data(), 10 * len);
        std::memcpy(first + 5 * at, rows[g].first.data(), 10 * len);
        at += len;
    }
    col_off[n_groups] = at;
    if (ops) ga_emit_paths(paths, op_off, ops);
    return DMX_OK;
}

extern "C" int dmx_groupalign_host(const uint32_t* seq2b, const uint32_t* nmask,
                                   const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
                                   size_t n_groups, const uint8_t* seed_masks,
                                   const uint64_t* seed_off, const uint32_t* members,
                                   const uint64_t* member_off, uint32_t max_cols, uint64_t* col_off,
                                   uint8_t* mask, uint16_t* count, uint16_t* first, size_t cols_cap,
                                   uint32_t* dist, uint64_t* op_off, uint8_t* ops, size_t ops_cap,
                                   int n_threads) {
    return ga_host("dmx_groupalign_host", seq2b, nmask, offsets, lens, n_reads, n_groups,
                   seed_masks, seed_off, members, nullptr, member_off, max_cols, col_off, mask,
                   count, first, cols_cap, dist, op_off, ops, ops_cap, n_threads);
}

extern "C" int dmx_groupalign_strands_host(
    const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets, const uint32_t* lens,
    size_t n_reads, size_t n_groups, const uint8_t* seed_masks, const uint64_t* seed_off,
    const uint32_t* members, const uint8_t* member_flags, const uint64_t* member_off,
    uint32_t max_cols, uint64_t* col_off, uint8_t* mask, uint16_t* count, uint16_t* first,
    size_t cols_cap, uint32_t* dist, uint64_t* op_off, uint8_t* ops, size_t ops_cap,
    int n_threads) {
    return ga_host("dmx_groupalign_strands_host", seq2b, nmask, offsets, lens, n_reads, n_groups,
                   seed_masks, seed_off, members, member_flags, member_off, max_cols, col_off,
                   mask, count, first, cols_cap, dist, op_off, ops, ops_cap, n_threads);
}

// Both device entry points: member_flags == NULL is dmx_groupalign (`who` opens the messages).
static int ga_device(const char* who, dmx_ctx* c, size_t n_groups, const uint8_t* seed_masks,
                     const uint64_t* seed_off, const uint32_t* members,
                     const uint8_t* member_flags, const uint64_t* member_off, uint32_t max_cols,
                     uint64_t* col_off, uint8_t* mask, uint16_t* count, uint16_t* first,
                     size_t cols_cap, uint32_t* dist, uint64_t* op_off, uint8_t* ops,
                     size_t ops_cap) {
    if (!c) return DMX_E_INVALID;
    if (c->ga) {
        c->ga->ms[0] = c->ga->ms[1] = c->ga->ms[2] = 0.f;
        c->ga->launches = c->ga->rounds = 0;
    }
    const bool some = n_groups && member_off && member_off[n_groups] > member_off[0];
    if (!seed_off || !member_off || !col_off || (ops && !op_off) ||
        (n_groups && (!seed_masks || !mask || !count || !first)) || (some && (!members || !dist))) {
        c->err = std::string(who) + ": null argument";
        return DMX_E_INVALID;
    }
    std::vector<uint32_t> lens;
    if (const int rc = pd_fetch_lens(c, who, some ? 1 : 0, lens)) return rc;
    GaShape sh;
    if (const int rc = ga_validate(who, lens.data(), lens.size(), n_groups, seed_masks, seed_off,
                                   members, member_flags, member_off, max_cols, cols_cap,
                                   ops != nullptr, ops_cap, sh, &c->err))
        return rc;
    col_off[0] = 0;
    if (ops) op_off[0] = 0;
    if (!n_groups) return DMX_OK;
    PD_CK(who, hipSetDevice(c->device));
    // operands: a member's flag with its strand folded in (a launch with a turned member runs
    // the strands form, dmx_groupalign's included)
    std::vector<uint8_t> strands, mflags;
    if (some)
        if (const int rc = pd_fetch_strands(c, who, strands)) return rc;
    if (!strands.empty()) {
        const uint64_t m0 = member_off[0], m1 = member_off[n_groups];
        mflags.resize(m1);   // indexed as member_flags is: by the member's place in `members`
        for (uint64_t x = m0; x < m1; ++x)
            mflags[x] = (uint8_t)(((member_flags ? member_flags[x] : 0u) ^ strands[members[x]]) &
                                  DMX_PD_RC);
        member_flags = mflags.data();
    }
    if (const int rc = pd_state(c, who, c->ga)) return rc;
    GaState* s = c->ga;
    hipStream_t st = c->stream;
    const size_t budget = pa_trace_budget();
    const uint64_t m0 = member_off[0];

    // every group's row has a region of its bound, padded to 16 columns (the forward pass loads
    // 16 mask bytes at a time), at the same place in both halves of the column arrays
    std::vector<uint64_t> goff(n_groups);
    uint64_t total = 0;
    for (size_t g = 0; g < n_groups; ++g) {
        goff[g] = total;
        total += ((uint64_t)sh.bound[g] + 15u) & ~(uint64_t)15u;
    }
    PD_CK(who, s->mask.reserve(2 * total));
    PD_CK(who, s->count.reserve(10 * total));
    PD_CK(who, s->first.reserve(10 * total));
    std::vector<uint8_t> seed(total, 0);
    std::vector<uint32_t> cur(n_groups), half(n_groups, 0);
    for (size_t g = 0; g < n_groups; ++g) {
        cur[g] = (uint32_t)(seed_off[g + 1] - seed_off[g]);
        std::memcpy(seed.data() + goff[g], seed_masks + seed_off[g], cur[g]);
    }
    PD_CK(who, hipMemcpyAsync(s->mask.p, seed.data(), total, hipMemcpyHostToDevice, st));
    PD_CK(who, hipMemsetAsync(s->count.p, 0, 5 * total * sizeof(uint16_t), st));
    PD_CK(who, hipMemsetAsync(s->first.p, 0, 5 * total * sizeof(uint16_t), st));
    PD_CK(who, hipStreamSynchronize(st));   // `seed` is pageable

    PdPlan<GaPair> pl;
    std::vector<uint32_t> rq, rg, rn, res;
    std::vector<uint8_t> rf, region;   // rf: the round's member flags (empty without any)
    std::vector<std::vector<uint8_t>> paths(ops ? sh.members : 0);
    float ms3[3] = {0.f, 0.f, 0.f};
    for (size_t round = 0; round < sh.rounds; ++round) {
        // member `round` of every group that has one, against the group's row as it stands
        rq.clear(), rg.clear(), rn.clear(), rf.clear();
        for (size_t g = 0; g < n_groups; ++g)
            if (member_off[g + 1] - member_off[g] > round) {
                rq.push_back(members[member_off[g] + round]);
                rg.push_back((uint32_t)g);
                rn.push_back(cur[g]);
                if (member_flags) rf.push_back(member_flags[member_off[g] + round]);
            }
        const size_t n_pairs = rq.size();
        for (size_t lo = 0; lo < n_pairs;) {
            const size_t hi = pd_plan(pl, lens.data(), rq.data(), rg.data(),
                                      member_flags ? rf.data() : nullptr, nullptr, n_pairs, lo,
                                      kPdChunkDefault, budget, rn.data());
            const size_t np = hi - lo;
            for (GaPair& P : pl.pairs) {
                const size_t g = P.t;
                P.row = half[g] * total + goff[g];
                P.dst = (1u - half[g]) * total + goff[g];
                P.ord = (uint32_t)round + 1u;
                P.cap = sh.max_cols;
            }
            GaArgs A;
            if (const int rc = pd_stage(c, who, *s, pl, 2 * np, kKerGroupalign, A)) return rc;
            if (const int rc = pa_stage_trace(c, who, *s, pl.trace, pl.ops, s->out.p, A)) return rc;
            A.mask = s->mask.p;
            A.count = s->count.p;
            A.first = s->first.p;
            A.cols = std::min(s->mask.cap, std::min(s->count.cap, s->first.cap) / 5);
            // a pair the kernels skip must not leave a stale length behind
            PD_CK(who, hipMemsetAsync(A.out, 0, 2 * np * 4, st));
            PD_CK(who, hipEventRecord(s->ev[0], st));
            bool any_rc = false;   // a launch without a flagged member runs the plain form
            for (const GaPair& P : pl.pairs) any_rc = any_rc || (P.flags & DMX_PD_RC);
            if (any_rc) {
                GaStrandArgs S;
                static_cast<GaArgs&>(S) = A;
                pd_launch_forward(groupalign_strands_kernel, S, st);
            } else {
                pd_launch_forward(groupalign_kernel, A, st);
            }
            if (const int rc = pd_mark(c, who, s->ev[1])) return rc;
            pa_launch_traceback(groupalign_traceback_kernel, A, kKerGroupalignTb, st);
            if (const int rc = pd_mark(c, who, s->ev[2])) return rc;
            set_kid(A.pk.bd, kKerGroupalignMerge);
            hipLaunchKernelGGL(groupalign_merge_kernel,
                               dim3((A.n_pairs + kGaMergeWaves - 1u) / kGaMergeWaves),
                               dim3(64 * kGaMergeWaves), 0, st, A);
            if (const int rc = pd_mark(c, who, s->ev[3])) return rc;
            res.resize(2 * np);
            PD_CK(who, hipMemcpyAsync(res.data(), A.out, 2 * np * 4, hipMemcpyDeviceToHost, st));
            if (ops) {
                region.resize(pl.ops);
                PD_CK(who, hipMemcpyAsync(region.data(), A.ops, pl.ops, hipMemcpyDeviceToHost, st));
            }
            if (const int rc = pd_finish(c, who, s->ev, 4, ms3)) return rc;
            ++s->launches;
            for (size_t k = 0; k < np; ++k) {
                const GaPair& P = pl.pairs[k];
                const size_t g = P.t;
                const uint32_t m = lens[P.q], n = P.n, len = res[2 * k + 1];
                if (!pa_path_ok(len, m, n)) {
                    c->err = std::string(who) + ": group " + std::to_string(g) + ", round " +
                             std::to_string(round) + ": path of " + std::to_string(len) +
                             " ops for a read of " + std::to_string(m) + " nt and a row of " +
                             std::to_string(n) + " columns";
                    return DMX_E_STATE;
                }
                if (len > sh.max_cols) {
                    c->err = ga_overflow(who, g, round, len, sh.max_cols);
                    return DMX_E_UNSUPPORTED;
                }
                const uint64_t x = member_off[g] + round - m0;
                dist[x] = res[2 * k];
                if (ops)
                    paths[x].assign(region.begin() + P.roff + (m + n - len),
                                    region.begin() + P.roff + (m + n));
                cur[g] = len;      // the group's row of the next round: the other half
                half[g] ^= 1u;
            }
            lo = hi;
        }
    }
    s->rounds = (int)sh.rounds;
    s->ms[0] = ms3[0], s->ms[1] = ms3[1], s->ms[2] = ms3[2];

    uint64_t at = 0;
    for (size_t g = 0; g < n_groups; ++g) {
        const uint64_t src = half[g] * total + goff[g];
        const size_t len = cur[g];
        col_off[g] = at;
        PD_CK(who, hipMemcpyAsync(mask + at, s->mask.p + src, len, hipMemcpyDeviceToHost, st));
        PD_CK(who, hipMemcpyAsync(count + 5 * at, s->count.p + 5 * src, 10 * len,
                                  hipMemcpyDeviceToHost, st));
        PD_CK(who, hipMemcpyAsync(first + 5 * at, s->first.p + 5 * src, 10 * len,
                                  hipMemcpyDeviceToHost, st));
        at += len;
    }
    col_off[n_groups] = at;
    PD_CK(who, hipStreamSynchronize(st));
    if (ops) ga_emit_paths(paths, op_off, ops);
    return DMX_OK;
}

extern "C" int dmx_groupalign(dmx_ctx* c, size_t n_groups, const uint8_t* seed_masks,
                              const uint64_t* seed_off, const uint32_t* members,
                              const uint64_t* member_off, uint32_t max_cols, uint64_t* col_off,
                              uint8_t* mask, uint16_t* count, uint16_t* first, size_t cols_cap,
                              uint32_t* dist, uint64_t* op_off, uint8_t* ops, size_t ops_cap) {
    return ga_device("dmx_groupalign", c, n_groups, seed_masks, seed_off, members, nullptr,
                     member_off, max_cols, col_off, mask, count, first, cols_cap, dist, op_off,
                     ops, ops_cap);
}

extern "C" int dmx_groupalign_strands(dmx_ctx* c, size_t n_groups, const uint8_t* seed_masks,
                                      const uint64_t* seed_off, const uint32_t* members,
                                      const uint8_t* member_flags, const uint64_t* member_off,
                                      uint32_t max_cols, uint64_t* col_off, uint8_t* mask,
                                      uint16_t* count, uint16_t* first, size_t cols_cap,
                                      uint32_t* dist, uint64_t* op_off, uint8_t* ops,
                                      size_t ops_cap) {
    return ga_device("dmx_groupalign_strands", c, n_groups, seed_masks, seed_off, members,
                     member_flags, member_off, max_cols, col_off, mask, count, first, cols_cap,
                     dist, op_off, ops, ops_cap);
}

// ---- dmx_rowdist: resident reads against rows of masks (include/dmx.h) -----------

namespace {

// Every argument check of both entry points, naming the pair or the row; rowlen[g] becomes the
// length of row g, rn[i] that of pair i's row.  0, or the code with *err set.
int rd_validate(const char* who, const uint32_t* lens, size_t n_reads, size_t n_rows,
                const uint8_t* masks, const uint64_t* row_off, const uint32_t* q, const uint32_t* r,
                size_t n_pairs, std::vector<uint32_t>& rowlen, std::vector<uint32_t>& rn,
                std::string* err) {
    const std::string name = std::string(who) + ": ";
    if (const int rc = pd_rows_validate(name, n_rows, masks, row_off, rowlen, err)) return rc;
    rn.resize(n_pairs);
    for (size_t i = 0; i < n_pairs; ++i) {
        if (q[i] >= n_reads) {
            *err = name + "pair " + std::to_string(i) + " names a read outside the batch";
            return DMX_E_INVALID;
        }
        if (r[i] >= n_rows) {
            *err = name + "pair " + std::to_string(i) + " names a row outside the " +
                   std::to_string(n_rows) + " given";
            return DMX_E_INVALID;
        }
    }
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t m = lens[q[i]];
        const uint64_t n = row_off[r[i] + 1] - row_off[r[i]];
        if (m < 1 || m > DMX_PD_MAX_LEN) {
            *err = name + "pair " + std::to_string(i) + ": reads of 1.." +
                   std::to_string(DMX_PD_MAX_LEN) + " nt supported";
            return DMX_E_UNSUPPORTED;
        }
        if (n < 1 || n > DMX_PD_MAX_LEN) {
            *err = name + "pair " + std::to_string(i) + ": row " + std::to_string(r[i]) + " has " +
                   std::to_string(n) + " columns (1.." + std::to_string(DMX_PD_MAX_LEN) +
                   " supported)";
            return DMX_E_UNSUPPORTED;
        }
        rn[i] = (uint32_t)n;
    }
    return DMX_OK;
}

}  // namespace

extern "C" float dmx_rowdist_ms(dmx_ctx* c) { return c && c->rd ? c->rd->ms : 0.f; }

extern "C" int dmx_rowdist_host(const uint32_t* seq2b, const uint32_t* nmask,
                                const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
                                size_t n_rows, const uint8_t* masks, const uint64_t* row_off,
                                const uint32_t* q, const uint32_t* r, const uint32_t* caps,
                                size_t n_pairs, uint32_t* out, int n_threads) {
    const char* const who = "dmx_rowdist_host";
    if (!n_pairs) return DMX_OK;
    if (!q || !r || !out || !masks || !row_off || !seq2b || !nmask || !offsets || !lens) {
        set_process_error(std::string(who) + ": null argument");
        return DMX_E_INVALID;
    }
    std::string err;
    std::vector<uint32_t> rowlen, rn;
    if (const int rc = rd_validate(who, lens, n_reads, n_rows, masks, row_off, q, r, n_pairs, rowlen,
                                   rn, &err)) {
        set_process_error(err);
        return rc;
    }
    pd_parallel(n_pairs, n_threads, [&](size_t k, size_t nth) {
        std::vector<uint8_t> a, b;
        std::vector<uint16_t> D;
        for (size_t i = k; i < n_pairs; i += nth) {
            pd_decode(seq2b, nmask, offsets[q[i]], lens[q[i]], false, a);
            b.assign(masks + row_off[r[i]], masks + row_off[r[i] + 1]);
            uint32_t d = pa_dp_matrix(a, b, D, [](uint8_t sym, uint8_t mk) {
                return ((mk >> sym) & 1u) != 0;
            });
            if (caps && d > caps[i]) d = caps[i] + 1u;
            out[i] = d;
        }
    });
    return DMX_OK;
}

extern "C" int dmx_rowdist(dmx_ctx* c, size_t n_rows, const uint8_t* masks, const uint64_t* row_off,
                           const uint32_t* q, const uint32_t* r, const uint32_t* caps,
                           size_t n_pairs, uint32_t* out) {
    const char* const who = "dmx_rowdist";
    if (!c) return DMX_E_INVALID;
    if (c->rd) c->rd->ms = 0.f;
    if (!n_pairs) return DMX_OK;
    if (!q || !r || !out || !masks || !row_off) {
        c->err = "dmx_rowdist: null rows, pair list or output";
        return DMX_E_INVALID;
    }
    std::vector<uint32_t> lens, rowlen, rn;
    if (const int rc = pd_fetch_lens(c, who, n_pairs, lens)) return rc;
    if (const int rc = rd_validate(who, lens.data(), lens.size(), n_rows, masks, row_off, q, r,
                                   n_pairs, rowlen, rn, &c->err))
        return rc;
    PD_CK(who, hipSetDevice(c->device));
    if (const int rc = pd_state(c, who, c->rd)) return rc;
    RdState* s = c->rd;
    PdRows& rows = s->rows;
    hipStream_t st = c->stream;
    const size_t chunk = pd_chunk();

    // operands: a query on strand 1 against a row is the sub-range as it lies in memory against
    // the row's reverse complement
    std::vector<uint8_t> strands;
    if (const int rc = pd_fetch_strands(c, who, strands)) return rc;
    bool turned = false;
    for (size_t i = 0; i < n_pairs && !strands.empty() && !turned; ++i) turned = strands[q[i]] != 0;
    rows.place(masks, row_off, rowlen, r, nullptr, n_pairs);
    if (const int rc = rows.upload(c, who)) return rc;
    float rc_ms = 0.f;   // not part of dmx_rowdist_ms
    if (turned) {
        if (const int rc = rows.write_rc(c, who, s->ev, &rc_ms)) return rc;
    } else {
        PD_CK(who, hipStreamSynchronize(st));   // one wait for the upload either way
    }

    PdPlan<RdPair> pl;
    std::vector<uint32_t> res;
    float total_ms = 0.f;
    for (size_t lo = 0; lo < n_pairs;) {
        const size_t hi = pd_plan(pl, lens.data(), q, r, nullptr, caps, n_pairs, lo, chunk,
                                  kPdNoBudget, rn.data());
        const size_t np = hi - lo;
        for (RdPair& P : pl.pairs) P.row = rows.off(P.t, turned && strands[P.q]);
        RdArgs A;
        if (const int rc = pd_stage(c, who, *s, pl, np, kKerRowdist, A)) return rc;
        A.mask = rows.mask.p;
        A.cols = rows.cols();
        A.out = s->out.p;
        PD_CK(who, hipEventRecord(s->ev[0], st));
        pd_launch_forward(rowdist_kernel, A, st);
        if (const int rc = pd_mark(c, who, s->ev[1])) return rc;
        res.resize(np);
        PD_CK(who, hipMemcpyAsync(res.data(), A.out, np * 4, hipMemcpyDeviceToHost, st));
        if (const int rc = pd_finish(c, who, s->ev, 2, &total_ms)) return rc;
        for (size_t k = 0; k < np; ++k) out[lo + pl.place(k)] = res[k];
        lo = hi;
    }
    s->ms = total_ms;
    return DMX_OK;
}

// ---- dmx_rowpairdist, dmx_rowhits: rows of masks against rows of masks ----------

namespace {

// Every argument check of the four entry points, naming the pair or the row; rowlen[g] becomes
// the length of row g.  0, or the code with *err set.
int rr_validate(const char* who, int mode, size_t n_rows, const uint8_t* masks,
                const uint64_t* row_off, const uint32_t* q, const uint32_t* t, const uint8_t* flags,
                size_t n_pairs, std::vector<uint32_t>& rowlen, std::string* err) {
    const std::string name = std::string(who) + ": ";
    if (mode != DMX_PD_NW && mode != DMX_PD_HW) {
        *err = name + "mode must be DMX_PD_NW or DMX_PD_HW";
        return DMX_E_INVALID;
    }
    if (!n_pairs) return DMX_OK;
    if (n_pairs > DMX_LG_MAX_PAIRS) {
        *err = name + "at most " + std::to_string(DMX_LG_MAX_PAIRS) + " pairs supported";
        return DMX_E_UNSUPPORTED;
    }
    if (const int rc = pd_rows_validate(name, n_rows, masks, row_off, rowlen, err)) return rc;
    for (size_t i = 0; i < n_pairs; ++i) {
        if (q[i] >= n_rows || t[i] >= n_rows) {
            *err = name + "pair " + std::to_string(i) + " names a row outside the " +
                   std::to_string(n_rows) + " given";
            return DMX_E_INVALID;
        }
        if (flags && (flags[i] & ~DMX_PD_RC)) {
            *err = name + "pair " + std::to_string(i) + " has an unknown flag";
            return DMX_E_INVALID;
        }
    }
    for (size_t i = 0; i < n_pairs; ++i)
        for (const uint32_t g : {q[i], t[i]})
            if (rowlen[g] < 1 || rowlen[g] > DMX_PD_MAX_LEN) {
                *err = name + "pair " + std::to_string(i) + ": row " + std::to_string(g) + " has " +
                       std::to_string(row_off[g + 1] - row_off[g]) + " columns (1.." +
                       std::to_string(DMX_PD_MAX_LEN) + " supported)";
                return DMX_E_UNSUPPORTED;
            }
    return DMX_OK;
}

// dmx_rowhits' caps: -1 = never a hit, below that refused.
int rr_validate_caps(const char* who, const int32_t* cap, size_t n_pairs, std::string* err) {
    for (size_t i = 0; i < n_pairs; ++i)
        if (cap[i] < -1) {
            *err = std::string(who) + ": pair " + std::to_string(i) +
                   ": a cap is a distance, or -1 for none";
            return DMX_E_INVALID;
        }
    return DMX_OK;
}

// A row's reverse complement (lib.mask_rc; rowpair_rc_kernel on the device).
void rr_mask_rc(const uint8_t* row, size_t n, std::vector<uint8_t>& out) {
    out.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t x = row[n - 1 - i];
        out[i] = (uint8_t)((x & 16u) | ((x & 1u) << 3) | ((x & 2u) << 1) | ((x & 4u) >> 1) |
                           ((x & 8u) >> 3));
    }
}

// The distances of a validated list on the device, into the state's `out` in list order:
// the rows some pair names closed up, padded to 16 columns and uploaded once; their reverse
// complements written beside them when a pair is flagged; then dmx_pairdist's chunked launches.
// *ms = the device time of the kernels.
int rr_run(Ctx* c, const char* who, int mode, size_t n_rows, const uint8_t* masks,
           const uint64_t* row_off, const std::vector<uint32_t>& rowlen, const uint32_t* q,
           const uint32_t* t, const uint8_t* flags, const uint32_t* caps, size_t n_pairs,
           float* ms_total) {
    PD_CK(who, hipSetDevice(c->device));
    if (const int rc = pd_state(c, who, c->rr)) return rc;
    RrState* s = c->rr;
    PdRows& rows = s->rows;
    hipStream_t st = c->stream;
    const size_t chunk = pd_chunk();

    std::vector<uint32_t> tn(n_pairs);
    bool any_rc = false;
    for (size_t i = 0; i < n_pairs; ++i) {
        tn[i] = rowlen[t[i]];
        any_rc = any_rc || (flags && (flags[i] & DMX_PD_RC));
    }
    rows.place(masks, row_off, rowlen, q, t, n_pairs);
    PD_CK(who, s->out.reserve(n_pairs));
    if (const int rc = rows.upload(c, who)) return rc;
    float ms_sum = 0.f;
    if (any_rc) {
        if (const int rc = rows.write_rc(c, who, s->ev, &ms_sum)) return rc;
    } else {
        PD_CK(who, hipStreamSynchronize(st));   // one wait for the upload either way
    }

    PdPlan<RrPair> pl;
    for (size_t lo = 0; lo < n_pairs;) {
        const size_t hi = pd_plan(pl, rowlen.data(), q, t, flags, caps, n_pairs, lo, chunk,
                                  kPdNoBudget, tn.data());
        for (size_t k = 0; k < pl.pairs.size(); ++k) {
            RrPair& P = pl.pairs[k];
            P.row = rows.off(P.t, (P.flags & DMX_PD_RC) != 0);
            P.qrow = rows.off(P.q, false);
            P.m = rowlen[P.q];
            P.dst = (uint32_t)(lo + pl.place(k));
            P.pad = 0;
        }
        RrArgs A;
        // out_words = the whole list: the buffer is not reallocated between the chunks
        if (const int rc = pd_stage(c, who, *s, pl, n_pairs, kKerRowpair, A)) return rc;
        A.mask = rows.mask.p;
        A.cols = rows.cols();
        A.mode = mode;
        A.out_n = (uint32_t)n_pairs;
        A.out = s->out.p;
        PD_CK(who, hipEventRecord(s->ev[0], st));
        pd_launch_forward(rowpair_kernel, A, st);
        if (const int rc = pd_mark(c, who, s->ev[1])) return rc;
        // waits: the plan's pair records are pageable
        if (const int rc = pd_finish(c, who, s->ev, 2, &ms_sum)) return rc;
        lo = hi;
    }
    *ms_total = ms_sum;
    return DMX_OK;
}

}  // namespace

extern "C" float dmx_rowhits_ms(dmx_ctx* c) { return c && c->rr ? c->rr->ms : 0.f; }

extern "C" int dmx_rowpairdist_host(int mode, size_t n_rows, const uint8_t* masks,
                                    const uint64_t* row_off, const uint32_t* q, const uint32_t* t,
                                    const uint8_t* flags, const uint32_t* caps, size_t n_pairs,
                                    uint32_t* out, int n_threads) {
    const char* const who = "dmx_rowpairdist_host";
    if (n_pairs && (!q || !t || !out || !masks || !row_off)) {
        set_process_error(std::string(who) + ": null argument");
        return DMX_E_INVALID;
    }
    std::string err;
    std::vector<uint32_t> rowlen;
    if (const int rc = rr_validate(who, mode, n_rows, masks, row_off, q, t, flags, n_pairs, rowlen,
                                   &err)) {
        set_process_error(err);
        return rc;
    }
    pd_parallel(n_pairs, n_threads, [&](size_t k, size_t nth) {
        std::vector<uint8_t> a, b;
        std::vector<uint16_t> D;
        for (size_t i = k; i < n_pairs; i += nth) {
            a.assign(masks + row_off[q[i]], masks + row_off[q[i] + 1]);
            if (flags && (flags[i] & DMX_PD_RC))
                rr_mask_rc(masks + row_off[t[i]], rowlen[t[i]], b);
            else
                b.assign(masks + row_off[t[i]], masks + row_off[t[i] + 1]);
            uint32_t d = pa_dp_matrix(a, b, D, [](uint8_t x, uint8_t y) { return (x & y) != 0; },
                                      mode);
            if (caps && d > caps[i]) d = caps[i] + 1u;
            out[i] = d;
        }
    });
    return DMX_OK;
}

extern "C" int dmx_rowhits_host(int mode, size_t n_rows, const uint8_t* masks,
                                const uint64_t* row_off, const uint32_t* q, const uint32_t* t,
                                const int32_t* cap, size_t n_pairs, uint32_t* pair, uint32_t* d,
                                uint8_t* rev, size_t hits_cap, size_t* n_hits, int n_threads) {
    const char* const who = "dmx_rowhits_host";
    if (!n_hits || (n_pairs && (!q || !t || !cap || !masks || !row_off))) {
        set_process_error(std::string(who) + ": null argument");
        return DMX_E_INVALID;
    }
    *n_hits = 0;
    std::string err;
    std::vector<uint32_t> rowlen;
    int rc = rr_validate(who, mode, n_rows, masks, row_off, q, t, nullptr, n_pairs, rowlen, &err);
    if (!rc) rc = rr_validate_caps(who, cap, n_pairs, &err);
    if (rc) {
        set_process_error(err);
        return rc;
    }
    std::vector<uint32_t> df(n_pairs), dr(n_pairs);
    const std::vector<uint8_t> rflags(n_pairs, DMX_PD_RC);
    if ((rc = dmx_rowpairdist_host(mode, n_rows, masks, row_off, q, t, nullptr, nullptr, n_pairs,
                                   df.data(), n_threads)))
        return rc;
    if ((rc = dmx_rowpairdist_host(mode, n_rows, masks, row_off, q, t, rflags.data(), nullptr,
                                   n_pairs, dr.data(), n_threads)))
        return rc;
    size_t hits = 0;
    for (size_t i = 0; i < n_pairs; ++i)
        hits += cap[i] >= 0 && std::min(df[i], dr[i]) <= (uint32_t)cap[i];
    *n_hits = hits;
    if (!hits) return DMX_OK;
    if (hits_cap < hits || !pair || !d || !rev) {
        set_process_error(std::string(who) + ": room for " + std::to_string(hits_cap) + " hits, " +
                          std::to_string(hits) + " to return");
        return DMX_E_INVALID;
    }
    size_t k = 0;
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t best = std::min(df[i], dr[i]);
        if (cap[i] < 0 || best > (uint32_t)cap[i]) continue;
        pair[k] = (uint32_t)i;
        d[k] = best;
        rev[k] = dr[i] < df[i] ? 1 : 0;   // ties are forward
        ++k;
    }
    return DMX_OK;
}

extern "C" int dmx_rowpairdist(dmx_ctx* c, int mode, size_t n_rows, const uint8_t* masks,
                               const uint64_t* row_off, const uint32_t* q, const uint32_t* t,
                               const uint8_t* flags, const uint32_t* caps, size_t n_pairs,
                               uint32_t* out) {
    const char* const who = "dmx_rowpairdist";
    if (!c) return DMX_E_INVALID;
    if (c->rr) c->rr->ms = 0.f;
    if (n_pairs && (!q || !t || !out || !masks || !row_off)) {
        c->err = "dmx_rowpairdist: null rows, pair list or output";
        return DMX_E_INVALID;
    }
    std::vector<uint32_t> rowlen;
    if (const int rc = rr_validate(who, mode, n_rows, masks, row_off, q, t, flags, n_pairs, rowlen,
                                   &c->err))
        return rc;
    if (!n_pairs) return DMX_OK;
    float ms = 0.f;
    if (const int rc = rr_run(c, who, mode, n_rows, masks, row_off, rowlen, q, t, flags, caps,
                              n_pairs, &ms))
        return rc;
    PD_CK(who, hipMemcpy(out, c->rr->out.p, n_pairs * 4, hipMemcpyDeviceToHost));
    c->rr->ms = ms;
    return DMX_OK;
}

extern "C" int dmx_rowhits(dmx_ctx* c, int mode, size_t n_rows, const uint8_t* masks,
                           const uint64_t* row_off, const uint32_t* q, const uint32_t* t,
                           const int32_t* cap, size_t n_pairs, uint32_t* pair, uint32_t* d,
                           uint8_t* rev, size_t hits_cap, size_t* n_hits) {
    const char* const who = "dmx_rowhits";
    if (!c) return DMX_E_INVALID;
    if (c->rr) c->rr->ms = 0.f;
    if (!n_hits || (n_pairs && (!q || !t || !cap || !masks || !row_off))) {
        c->err = "dmx_rowhits: null rows, pair list, caps or count";
        return DMX_E_INVALID;
    }
    *n_hits = 0;
    std::vector<uint32_t> rowlen;
    if (const int rc = rr_validate(who, mode, n_rows, masks, row_off, q, t, nullptr, n_pairs,
                                   rowlen, &c->err))
        return rc;
    if (const int rc = rr_validate_caps(who, cap, n_pairs, &c->err)) return rc;
    if (!n_pairs) return DMX_OK;
    // the list the launches run: pair i forward at 2 i, against the reversed target at 2 i + 1
    std::vector<uint32_t> q2(2 * n_pairs), t2(2 * n_pairs), cap2(2 * n_pairs);
    std::vector<uint8_t> f2(2 * n_pairs);
    for (size_t i = 0; i < n_pairs; ++i) {
        q2[2 * i] = q2[2 * i + 1] = q[i];
        t2[2 * i] = t2[2 * i + 1] = t[i];
        cap2[2 * i] = cap2[2 * i + 1] = (uint32_t)std::max(cap[i], 0);
        f2[2 * i] = 0;
        f2[2 * i + 1] = DMX_PD_RC;
    }
    float ms = 0.f, ms_decide = 0.f, ms_compact = 0.f;
    if (const int rc = rr_run(c, who, mode, n_rows, masks, row_off, rowlen, q2.data(), t2.data(),
                              f2.data(), cap2.data(), 2 * n_pairs, &ms))
        return rc;
    RrState* s = c->rr;
    hipStream_t st = c->stream;
    PD_CK(who, s->outc.reserve(n_pairs));
    PD_CK(who, s->cap.reserve(n_pairs));
    PD_CK(who, hipMemcpyAsync(s->cap.p, cap, n_pairs * 4, hipMemcpyHostToDevice, st));
    RrDecide D;
    D.dist = s->out.p;
    D.cap = s->cap.p;
    D.n_pairs = (uint32_t)n_pairs;
    D.outc = s->outc.p;
    PD_CK(who, hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(rowhits_decide_kernel,
                       dim3((uint32_t)((n_pairs + kRrRcBlock - 1) / kRrRcBlock)), dim3(kRrRcBlock),
                       0, st, D);
    if (const int rc = pd_mark(c, who, s->ev[1])) return rc;
    // waits: `cap` is pageable.  The decision takes no bounds record, so the check reads the
    // record as rr_run's last launch left it: clean, or rr_run had failed.
    if (const int rc = pd_finish(c, who, s->ev, 2, &ms_decide)) return rc;
    const int rc = lg_compact_outcomes(c, who, s->outc.p, n_pairs, hits_cap, pair, d, rev, n_hits,
                                       &ms_compact);
    if (rc == DMX_OK || rc == DMX_E_INVALID) s->ms = ms + ms_decide + ms_compact;
    return rc;
}

// ---- dmx_rowassign: the best row per read, decided on the device ----------------

namespace {

// The call's pairs in generation order: place[i] in the read list, row[i], and the pair's longer
// length.  Filled by ra_prepare after every check has passed.
struct RaPairs {
    std::vector<uint32_t> place, row, q, tn, L;
    std::vector<uint32_t> rowlen;   // per row of the call, clamped at DMX_PD_MAX_LEN + 1
};

// Every argument check of both entry points, then the pair generation: the 5 % rule with the
// reference's double products (:1664) and the stop after the place at whose end max_chunks full
// chunks have been made (:1669-1676; equality, tested once per place).  Names the place, row or
// length.  0, or the code with *err set.
int ra_prepare(const char* who, const uint32_t* lens, size_t n_reads, size_t n_rows,
               const uint8_t* masks, const uint64_t* row_off, const uint32_t* reads, size_t n_sel,
               const int32_t* cap_hit, const int32_t* cap_half, const uint32_t* bin_off,
               size_t n_len, size_t n_bins, uint64_t chunk, uint64_t max_chunks, RaPairs& ps,
               std::string* err) {
    const std::string name = std::string(who) + ": ";
    if (!chunk) {
        *err = name + "chunk must be at least 1";
        return DMX_E_INVALID;
    }
    if (n_rows > kRaRowMax) {
        *err = name + "at most " + std::to_string(kRaRowMax) + " rows supported";
        return DMX_E_UNSUPPORTED;
    }
    if (const int rc = pd_rows_validate(name, n_rows, masks, row_off, ps.rowlen, err)) return rc;
    for (size_t k = 0; k < n_sel; ++k)
        if (reads[k] >= n_reads) {
            *err = name + "place " + std::to_string(k) + " names a read outside the batch";
            return DMX_E_INVALID;
        }
    for (size_t L = 0; L < n_len; ++L)
        if (cap_hit[L] < -1 || cap_half[L] < -1) {
            *err = name + "length " + std::to_string(L) + ": a cap is a distance, or -1 for none";
            return DMX_E_INVALID;
        }
    ps.place.clear(), ps.row.clear(), ps.q.clear(), ps.tn.clear(), ps.L.clear();
    uint64_t made = 0;
    for (size_t k = 0; k < n_sel; ++k) {
        const uint32_t m = lens[reads[k]];
        const double la = (double)m;
        for (size_t g = 0; g < n_rows; ++g) {
            const uint64_t n64 = row_off[g + 1] - row_off[g];
            const double lb = (double)n64;
            if (la * 1.05 < lb || lb * 1.05 < la) continue;
            if (m < 1 || m > DMX_PD_MAX_LEN) {
                *err = name + "place " + std::to_string(k) + ": reads of 1.." +
                       std::to_string(DMX_PD_MAX_LEN) + " nt supported";
                return DMX_E_UNSUPPORTED;
            }
            if (n64 < 1 || n64 > DMX_PD_MAX_LEN) {
                *err = name + "place " + std::to_string(k) + ": row " + std::to_string(g) +
                       " has " + std::to_string(n64) + " columns (1.." +
                       std::to_string(DMX_PD_MAX_LEN) + " supported)";
                return DMX_E_UNSUPPORTED;
            }
            const uint32_t n = (uint32_t)n64, L = std::max(m, n);
            if (L >= n_len) {
                *err = name + "place " + std::to_string(k) + ", row " + std::to_string(g) +
                       ": length " + std::to_string(L) + " is outside the " +
                       std::to_string(n_len) + " entries of the tables";
                return DMX_E_INVALID;
            }
            if ((uint64_t)bin_off[L] + (uint64_t)std::max(cap_hit[L], 0) >= n_bins) {
                *err = name + "length " + std::to_string(L) + ": its classes end outside the " +
                       std::to_string(n_bins) + " entries of bins";
                return DMX_E_INVALID;
            }
            if (made >= DMX_LG_MAX_PAIRS) {
                *err = name + "at most " + std::to_string(DMX_LG_MAX_PAIRS) + " pairs supported";
                return DMX_E_UNSUPPORTED;
            }
            ps.place.push_back((uint32_t)k);
            ps.row.push_back((uint32_t)g);
            ps.q.push_back(reads[k]);
            ps.tn.push_back(n);
            ps.L.push_back(L);
            ++made;
        }
        if (made / chunk == max_chunks) break;
    }
    return DMX_OK;
}

void ra_fill_none(size_t n_sel, uint32_t* best_row, uint32_t* best_d, uint16_t* best_class) {
    for (size_t k = 0; k < n_sel; ++k) {
        best_row[k] = DMX_LG_NONE;
        best_d[k] = DMX_LG_NONE;
        best_class[k] = 0;
    }
}

}  // namespace

extern "C" float dmx_rowassign_ms(dmx_ctx* c) { return c && c->ra ? c->ra->ms : 0.f; }

extern "C" int dmx_rowassign_host(const uint32_t* seq2b, const uint32_t* nmask,
                                  const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
                                  size_t n_rows, const uint8_t* masks, const uint64_t* row_off,
                                  const uint32_t* reads, size_t n_sel, const int32_t* cap_hit,
                                  const int32_t* cap_half, const uint32_t* bin_off, size_t n_len,
                                  const uint16_t* bins, size_t n_bins, uint64_t chunk,
                                  uint64_t max_chunks, uint32_t* best_row, uint32_t* best_d,
                                  uint16_t* best_class, uint64_t* n_pairs, uint64_t* n_lines,
                                  int n_threads) {
    const char* const who = "dmx_rowassign_host";
    if (!n_pairs || !n_lines || (n_sel && (!reads || !best_row || !best_d || !best_class)) ||
        (n_sel && n_rows &&
         (!masks || !row_off || !cap_hit || !cap_half || !bin_off || !bins || !seq2b || !nmask ||
          !offsets || !lens))) {
        set_process_error(std::string(who) + ": null argument");
        return DMX_E_INVALID;
    }
    RaPairs ps;
    if (n_sel && n_rows) {
        std::string err;
        if (const int rc = ra_prepare(who, lens, n_reads, n_rows, masks, row_off, reads, n_sel,
                                      cap_hit, cap_half, bin_off, n_len, n_bins, chunk, max_chunks,
                                      ps, &err)) {
            set_process_error(err);
            return rc;
        }
    }
    *n_pairs = ps.place.size();
    *n_lines = 0;
    ra_fill_none(n_sel, best_row, best_d, best_class);
    const size_t n = ps.place.size();
    if (!n) return DMX_OK;
    std::vector<uint32_t> fcap(n), df(n);
    for (size_t i = 0; i < n; ++i)
        fcap[i] = (uint32_t)std::max(std::max(cap_hit[ps.L[i]], cap_half[ps.L[i]]), 0);
    if (const int rc = dmx_rowdist_host(seq2b, nmask, offsets, lens, n_reads, n_rows, masks, row_off,
                                        ps.q.data(), ps.row.data(), fcap.data(), n, df.data(),
                                        n_threads))
        return rc;
    // the retries, against the reverse complements as rows of their own
    std::vector<uint32_t> again, q2, r2, cap2, dr;
    for (size_t i = 0; i < n; ++i) {
        const int64_t d = df[i], ch = cap_hit[ps.L[i]], chalf = cap_half[ps.L[i]];
        if (!(d <= ch) && ch >= 0 && d > chalf) {
            again.push_back((uint32_t)i);
            q2.push_back(ps.q[i]);
            r2.push_back(ps.row[i]);
            cap2.push_back((uint32_t)ch);
        }
    }
    if (!again.empty()) {
        std::vector<uint8_t> rmasks(row_off[n_rows] ? row_off[n_rows] : 1), one;
        for (size_t g = 0; g < n_rows; ++g) {
            rr_mask_rc(masks + row_off[g], (size_t)(row_off[g + 1] - row_off[g]), one);
            std::copy(one.begin(), one.end(), rmasks.begin() + row_off[g]);
        }
        dr.resize(again.size());
        if (const int rc = dmx_rowdist_host(seq2b, nmask, offsets, lens, n_reads, n_rows,
                                            rmasks.data(), row_off, q2.data(), r2.data(),
                                            cap2.data(), again.size(), dr.data(), n_threads))
            return rc;
    }
    // the lines in pair-generation order; a later line replaces the kept one iff its class is
    // at least the kept one's (update_groups)
    uint64_t lines = 0;
    size_t a = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t L = ps.L[i];
        const int64_t ch = cap_hit[L];
        uint32_t d = df[i], rev = 0;
        bool line = (int64_t)d <= ch;
        if (a < again.size() && again[a] == i) {
            d = dr[a++];
            rev = DMX_LG_REV;
            line = (int64_t)d <= ch;
        }
        if (!line) continue;
        ++lines;
        const uint16_t cls = bins[(size_t)bin_off[L] + d];
        const uint32_t k = ps.place[i];
        if (best_row[k] == DMX_LG_NONE || cls >= best_class[k]) {
            best_row[k] = ps.row[i];
            best_d[k] = d | rev;
            best_class[k] = cls;
        }
    }
    *n_lines = lines;
    return DMX_OK;
}

extern "C" int dmx_rowassign(dmx_ctx* c, size_t n_rows, const uint8_t* masks,
                             const uint64_t* row_off, const uint32_t* reads, size_t n_sel,
                             const int32_t* cap_hit, const int32_t* cap_half,
                             const uint32_t* bin_off, size_t n_len, const uint16_t* bins,
                             size_t n_bins, uint64_t chunk, uint64_t max_chunks,
                             uint32_t* best_row, uint32_t* best_d, uint16_t* best_class,
                             uint64_t* n_pairs, uint64_t* n_lines) {
    const char* const who = "dmx_rowassign";
    if (!c) return DMX_E_INVALID;
    if (c->ra) c->ra->ms = 0.f;
    if (!n_pairs || !n_lines || (n_sel && (!reads || !best_row || !best_d || !best_class)) ||
        (n_sel && n_rows && (!masks || !row_off || !cap_hit || !cap_half || !bin_off || !bins))) {
        c->err = "dmx_rowassign: null rows, reads, tables or output";
        return DMX_E_INVALID;
    }
    RaPairs ps;
    std::vector<uint32_t> lens;
    if (n_sel && n_rows) {
        if (const int rc = pd_fetch_lens(c, who, 1, lens)) return rc;
        if (const int rc = ra_prepare(who, lens.data(), lens.size(), n_rows, masks, row_off, reads,
                                      n_sel, cap_hit, cap_half, bin_off, n_len, n_bins, chunk,
                                      max_chunks, ps, &c->err))
            return rc;
    }
    const size_t n = ps.place.size();
    *n_pairs = n;
    *n_lines = 0;
    if (!n) {
        ra_fill_none(n_sel, best_row, best_d, best_class);
        return DMX_OK;
    }
    PD_CK(who, hipSetDevice(c->device));
    if (const int rc = pd_state(c, who, c->ra)) return rc;
    RaState* s = c->ra;
    PdRows& rows = s->rows;
    hipStream_t st = c->stream;
    const size_t chunk_pairs = pd_chunk();

    // the reverse complements are written only when a pair retries or a read is on strand 1
    rows.place(masks, row_off, ps.rowlen, ps.row.data(), nullptr, n);
    PD_CK(who, s->cap_hit.reserve(n_len));
    PD_CK(who, s->cap_half.reserve(n_len));
    PD_CK(who, s->bin_off.reserve(n_len));
    PD_CK(who, s->bins.reserve(n_bins));
    PD_CK(who, s->best.reserve(n_sel));
    PD_CK(who, s->cnt.reserve(1));
    PD_CK(who, s->o_row.reserve(n_sel));
    PD_CK(who, s->o_d.reserve(n_sel));
    PD_CK(who, s->o_class.reserve(n_sel));
    if (const int rc = rows.upload(c, who)) return rc;
    PD_CK(who, hipMemcpyAsync(s->cap_hit.p, cap_hit, n_len * 4, hipMemcpyHostToDevice, st));
    PD_CK(who, hipMemcpyAsync(s->cap_half.p, cap_half, n_len * 4, hipMemcpyHostToDevice, st));
    PD_CK(who, hipMemcpyAsync(s->bin_off.p, bin_off, n_len * 4, hipMemcpyHostToDevice, st));
    PD_CK(who, hipMemcpyAsync(s->bins.p, bins, n_bins * 2, hipMemcpyHostToDevice, st));
    PD_CK(who, hipMemsetAsync(s->best.p, 0, n_sel * sizeof(unsigned long long), st));
    PD_CK(who, hipMemsetAsync(s->cnt.p, 0, sizeof(unsigned long long), st));
    PD_CK(who, hipStreamSynchronize(st));   // `rows` and the caller's tables are pageable

    // operands: for a read on strand 1 the two comparisons swap copies (the forward line is the
    // sub-range as it lies in memory against the row's reverse complement, the reverse line the
    // same against the row), so the copies are written before the first pass
    std::vector<uint8_t> strands;
    if (const int rc = pd_fetch_strands(c, who, strands)) return rc;
    bool turned = false;
    for (size_t i = 0; i < n && !strands.empty() && !turned; ++i) turned = strands[ps.q[i]] != 0;

    PdPlan<RaPair> pl;
    std::vector<uint32_t> need;
    float total_ms = 0.f;
    if (turned)
        if (const int rc = rows.write_rc(c, who, s->ev, &total_ms)) return rc;
    // one launch of pairs[lo .. ) of a list and its decision; in[i]: the list's pair i among the
    // call's pairs; pass 0 brings the launch's retry bitmap back (bit b: sorted pair b)
    auto launch = [&](const uint32_t* lq, const uint32_t* lr, const uint32_t* lcap,
                      const uint32_t* ltn, size_t cnt, size_t lo, const uint32_t* in, int pass,
                      size_t* end) -> int {
        const size_t hi = pd_plan(pl, lens.data(), lq, lr, nullptr, lcap, cnt, lo, chunk_pairs,
                                  kPdNoBudget, ltn);
        const size_t np = hi - lo, words = (np + 31) / 32;
        for (size_t k = 0; k < np; ++k) {
            RaPair& P = pl.pairs[k];
            const size_t i = lo + pl.place(k);
            const bool rev = (pass != 0) != (turned && strands[P.q] != 0);
            P.row = rows.off(P.t, rev);
            P.k = ps.place[in ? in[i] : i];
        }
        RaArgs A;
        if (const int rc = pd_stage(c, who, *s, pl, np, kKerRowassign, A)) return rc;
        A.mask = rows.mask.p;
        A.cols = rows.cols();
        A.out = s->out.p;
        PD_CK(who, s->need.reserve(words));
        if (pass == 0) PD_CK(who, hipMemsetAsync(s->need.p, 0, words * 4, st));
        RaDecide D;
        D.bd = pd_bounds(c, kKerRowassignDecide);
        D.pairs = s->pairs.p, D.dist = s->out.p, D.lens = pd_lens(c);
        D.np = (uint32_t)np, D.pass = (uint32_t)pass;
        D.cap_hit = s->cap_hit.p, D.cap_half = s->cap_half.p;
        D.bin_off = s->bin_off.p, D.bins = s->bins.p;
        D.n_len = (uint32_t)n_len, D.n_sel = (uint32_t)n_sel, D.n_bins = n_bins;
        D.best = s->best.p, D.need = s->need.p;
        D.need_words = pass == 0 ? (uint32_t)words : 0u;
        D.cnt = s->cnt.p;
        PD_CK(who, hipEventRecord(s->ev[0], st));
        pd_launch_forward(rowassign_kernel, A, st);
        hipLaunchKernelGGL(rowassign_decide_kernel,
                           dim3((uint32_t)((np + kRrRcBlock - 1) / kRrRcBlock)), dim3(kRrRcBlock),
                           0, st, D);
        if (const int rc = pd_mark(c, who, s->ev[1])) return rc;
        if (pass == 0) {
            need.resize(words);
            PD_CK(who, hipMemcpyAsync(need.data(), s->need.p, words * 4, hipMemcpyDeviceToHost, st));
        }
        *end = hi;
        return pd_finish(c, who, s->ev, 2, &total_ms);   // waits: the pair records are pageable
    };

    std::vector<uint32_t> fcap(n), retry;
    for (size_t i = 0; i < n; ++i)
        fcap[i] = (uint32_t)std::max(std::max(cap_hit[ps.L[i]], cap_half[ps.L[i]]), 0);
    for (size_t lo = 0, hi = 0; lo < n; lo = hi) {
        if (const int rc = launch(ps.q.data(), ps.row.data(), fcap.data(), ps.tn.data(), n, lo,
                                  nullptr, 0, &hi))
            return rc;
        // the decision sets bit b for the b-th pair the launch ran
        pd_retry_list(need, pl, lo, hi, /*sorted=*/true, retry);
    }
    const size_t n2 = retry.size();
    if (n2) {
        if (const int rc = rows.write_rc(c, who, s->ev, &total_ms)) return rc;
        std::sort(retry.begin(), retry.end());   // pair-generation order again
        // the second pass's list; a cap is >= 0 where a retry is asked for
        const std::vector<uint32_t> q2 = pd_pick(ps.q.data(), retry), r2 = pd_pick(ps.row.data(), retry),
                                    tn2 = pd_pick(ps.tn.data(), retry),
                                    cap2 = pd_pick(cap_hit, pd_pick(ps.L.data(), retry));
        for (size_t lo = 0, hi = 0; lo < n2; lo = hi)
            if (const int rc = launch(q2.data(), r2.data(), cap2.data(), tn2.data(), n2, lo,
                                      retry.data(), 1, &hi))
                return rc;
    }
    RaFinish F;
    F.bd = make_bounds(c, kKerRowassignFinish);
    F.best = s->best.p;
    F.n_sel = (uint32_t)n_sel;
    F.row = s->o_row.p, F.d = s->o_d.p, F.cls = s->o_class.p;
    PD_CK(who, bounds_reset(c, st));
    PD_CK(who, hipEventRecord(s->ev[0], st));
    hipLaunchKernelGGL(rowassign_finish_kernel,
                       dim3((uint32_t)((n_sel + kRrRcBlock - 1) / kRrRcBlock)), dim3(kRrRcBlock), 0,
                       st, F);
    if (const int rc = pd_mark(c, who, s->ev[1])) return rc;
    unsigned long long lines = 0;
    PD_CK(who, hipMemcpyAsync(best_row, s->o_row.p, n_sel * 4, hipMemcpyDeviceToHost, st));
    PD_CK(who, hipMemcpyAsync(best_d, s->o_d.p, n_sel * 4, hipMemcpyDeviceToHost, st));
    PD_CK(who, hipMemcpyAsync(best_class, s->o_class.p, n_sel * 2, hipMemcpyDeviceToHost, st));
    PD_CK(who, hipMemcpyAsync(&lines, s->cnt.p, sizeof lines, hipMemcpyDeviceToHost, st));
    if (const int rc = pd_finish(c, who, s->ev, 2, &total_ms)) return rc;
    s->ms = total_ms;
    *n_lines = lines;
    return DMX_OK;
}
