// dmx_operands.hip — operand tables of the amplicon-sorting calls (include/dmx.h).
//
// With a table set, every index the sorting calls document as "a read of the resident batch"
// names an operand: read[start:stop] of the resident batch, taken reverse-complemented when its
// strand is 1.  The kernels of dmx_pairdist.hip find an operand through an offset and a length
// array, so a table is those two arrays for the sub-range as it lies in memory (operand_locate)
// and a strand per operand that the host folds into the pair flags.
//
// dmx_set_operands takes a table from the caller.  dmx_result_operands makes the table of a
// demultiplexer run on the device: one operand per kept item of round 0, the final trimmed and
// oriented record the fused loop writes for it, grouped by bin in item order.  Three passes:
//   operands_hist_kernel     per block, how many of its items go to each bin
//   operands_scan_kernel     one scan over bins x blocks: bin_first and every block's first place
//   operands_scatter_kernel  every block writes its items from its places on, in item order
// A block owns a contiguous span of items and walks it in tiles of kOpBlock, so "the blocks in
// order, the tiles of a block in order, the threads of a tile in order" is item order and the
// scatter is stable.  Only bin_first comes back.
#include <cstring>

#include "dmx_internal.h"

namespace dmx {

constexpr uint32_t kOpBlock = 256;     // items per tile, threads per block
constexpr uint32_t kOpGrid = 256;      // blocks at most
constexpr uint32_t kOpMaxBins = (kMaxAdapters + 1) * (kMaxAdapters + 1);

struct OpBuildArgs {
    Bounds bd;
    const dmx_result* res;
    const ItemView* views;       // round 0's items, nullptr: item k is read k
    const uint32_t* lens;
    const uint64_t* offs;
    const DevPanel* p0;
    const DevPanel* p1;
    const uint8_t* keep;         // per bin, nullptr: the items matched in every round
    uint32_t n_items, n_reads;
    uint32_t span;               // items per block, a multiple of kOpBlock
    uint32_t n_bins;             // (A0 + 1) * (A1 + 1), A1 = 0 in single mode
    int32_t A0, A1, two_round;
    int32_t min_len;
    uint32_t* hist;              // [block][bin]: counts, then first places
    uint64_t* bin_first;         // n_bins + 1
    OperandRec* op;              // the table
    uint64_t* op_off;
    uint32_t* op_len;
    uint8_t* op_strand;
    uint32_t cap;                // entries of the four above
};

// The operand of item k, and its bin; false where the item gives none.
__device__ __forceinline__ bool operand_of(const OpBuildArgs& A, uint32_t k, OperandRec& R,
                                           uint32_t& bin) {
    if (k >= A.n_items || !DMX_BOUND(A.bd, res, k, kBufRes)) return false;
    const dmx_result r = A.res[k];
    ItemView v;
    if (A.views) {
        if (!DMX_BOUND(A.bd, views, k, kBufItem)) return false;
        v = A.views[k];
    } else {
        v.read = k;
        v.strand = 0;
        v.start = 0;
        v.len = k < A.n_reads ? A.lens[k] : 0u;
    }
    if (v.read >= A.n_reads) return false;
    const int b1 = r.bin1, b2 = A.two_round ? r.bin2 : -1;
    if (b1 < -1 || b1 >= A.A0 || (A.two_round && (b2 < -1 || b2 >= A.A1))) return false;
    bin = (uint32_t)((b1 + 1) * (A.A1 + 1) + (b2 + 1));
    if (bin >= A.n_bins) return false;
    if (A.keep ? A.keep[bin] == 0 : (b1 < 0 || (A.two_round && b2 < 0))) return false;
    const uint32_t rl = A.lens[v.read];
    // an unmatched round keeps the whole view in the orientation it was taken: [0:] of it
    const bool f0 = b1 < 0 || A.p0->ad[b1].where == kFront;
    v = trimmed_view(v, rl, r.rc1, f0, v.len, r.m1.rstart, b1 < 0 ? 0 : r.m1.rstop);
    if (A.two_round && b1 >= 0) {
        const bool f1 = b2 < 0 || A.p1->ad[b2].where == kFront;
        v = trimmed_view(v, rl, r.rc2, f1, v.len, r.m2.rstart, b2 < 0 ? 0 : r.m2.rstop);
    }
    if ((uint64_t)v.start + v.len > rl || (int64_t)v.len < (int64_t)A.min_len) return false;
    const uint32_t a = v.strand ? rl - v.start - v.len : v.start;   // on the read as given
    R.read = v.read;
    R.start = (int32_t)a;
    R.stop = (int32_t)(a + v.len);
    R.strand = v.strand;
    return true;
}

__global__ __launch_bounds__(kOpBlock) void operands_hist_kernel(OpBuildArgs A) {
    extern __shared__ uint32_t s_bins[];
    for (uint32_t b = threadIdx.x; b < A.n_bins; b += kOpBlock) s_bins[b] = 0;
    __syncthreads();
    const uint32_t lo = blockIdx.x * A.span, hi = min(A.n_items, lo + A.span);
    for (uint32_t base = lo; base < hi; base += kOpBlock) {
        OperandRec R;
        uint32_t bin;
        if (operand_of(A, base + threadIdx.x, R, bin)) atomicAdd(&s_bins[bin], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < A.n_bins; b += kOpBlock)
        A.hist[(size_t)blockIdx.x * A.n_bins + b] = s_bins[b];
}

// One block.  Column sums over the blocks, an exclusive scan over the bins, then every (block,
// bin) count becomes the first place of that block's items in that bin.
__global__ __launch_bounds__(kOpBlock) void operands_scan_kernel(OpBuildArgs A, uint32_t n_blocks) {
    extern __shared__ uint32_t s_bins[];
    for (uint32_t b = threadIdx.x; b < A.n_bins; b += kOpBlock) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < n_blocks; ++k) sum += A.hist[(size_t)k * A.n_bins + b];
        s_bins[b] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // a few thousand bins at most
        uint32_t at = 0;
        for (uint32_t b = 0; b < A.n_bins; ++b) {
            const uint32_t n = s_bins[b];
            s_bins[b] = at;
            A.bin_first[b] = at;
            at += n;
        }
        A.bin_first[A.n_bins] = at;
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < A.n_bins; b += kOpBlock) {
        uint32_t at = s_bins[b];
        for (uint32_t k = 0; k < n_blocks; ++k) {
            const size_t x = (size_t)k * A.n_bins + b;
            const uint32_t n = A.hist[x];
            A.hist[x] = at;
            at += n;
        }
    }
}

// Where operand R lies in memory: the kernels of dmx_pairdist.hip read [off, off + len) forwards
// (strand 0) or backwards (a reversed target or member); the strand itself is the host's to fold.
__device__ __forceinline__ void operand_locate(const uint64_t* offs, const OperandRec& R,
                                               uint64_t& off, uint32_t& len) {
    off = offs[R.read] + (uint32_t)R.start;
    len = (uint32_t)(R.stop - R.start);
}

__global__ __launch_bounds__(kOpBlock) void operands_scatter_kernel(OpBuildArgs A) {
    extern __shared__ uint32_t s_bins[];   // per bin: the next place of this block's items
    for (uint32_t b = threadIdx.x; b < A.n_bins; b += kOpBlock)
        s_bins[b] = A.hist[(size_t)blockIdx.x * A.n_bins + b];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t lo = blockIdx.x * A.span, hi = min(A.n_items, lo + A.span);
    for (uint32_t base = lo; base < hi; base += kOpBlock) {   // uniform: every thread walks every tile
        OperandRec R;
        uint32_t bin = 0;
        const bool has = operand_of(A, base + threadIdx.x, R, bin);
        // the lane's rank among the wave's lanes of its bin, and how many they are
        uint32_t rank = 0, cnt = 0;
        uint64_t todo = __ballot(has);
        while (todo) {
            const int lead = __ffsll((unsigned long long)todo) - 1;
            const uint32_t lb = (uint32_t)__shfl((int)bin, lead);
            const uint64_t same = __ballot(has && bin == lb);
            if (has && bin == lb) {
                rank = (uint32_t)__popcll(same & below);
                cnt = (uint32_t)__popcll(same);
            }
            todo &= ~same;
        }
        // the waves of the tile take their places one after the other
        uint32_t at = 0;
        for (uint32_t w = 0; w < kOpBlock / 64u; ++w) {
            if (w == wave && has) at = s_bins[bin];
            __syncthreads();
            if (w == wave && has && rank == 0) s_bins[bin] = at + cnt;
            __syncthreads();
        }
        if (has) {
            const uint32_t dst = at + rank;
            if (dst < A.cap) {
                uint64_t off;
                uint32_t len;
                operand_locate(A.offs, R, off, len);
                A.op[dst] = R;
                A.op_off[dst] = off;
                A.op_len[dst] = len;
                A.op_strand[dst] = (uint8_t)R.strand;
            }
        }
    }
}

// dmx_set_operands: the offset and length arrays of an uploaded table.
__global__ __launch_bounds__(kOpBlock) void operands_locate_kernel(const OperandRec* op, uint32_t n,
                                                                  const uint64_t* offs,
                                                                  uint32_t n_reads, uint64_t* op_off,
                                                                  uint32_t* op_len,
                                                                  uint8_t* op_strand) {
    const uint32_t k = blockIdx.x * kOpBlock + threadIdx.x;
    if (k >= n) return;
    const OperandRec R = op[k];
    if (R.read >= n_reads) return;   // refused on the host before the upload
    uint64_t off;
    uint32_t len;
    operand_locate(offs, R, off, len);
    op_off[k] = off;
    op_len[k] = len;
    op_strand[k] = (uint8_t)R.strand;
}

#define OP_CK(call)                                                                   \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            c->err = std::string(who) + ": " + #call + ": " + hipGetErrorString(e_);  \
            ops_drop(c);                                                              \
            return DMX_E_HIP;                                                         \
        }                                                                             \
    } while (0)

// The same for the calls that only read the table, and for what dmx_set_operands does before the
// old table goes: the error is reported and the table stays as it was.
#define OP_CK_KEEP(call)                                                              \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            c->err = std::string(who) + ": " + #call + ": " + hipGetErrorString(e_);  \
            return DMX_E_HIP;                                                         \
        }                                                                             \
    } while (0)

void ops_drop(Ctx* c) {
    if (c->ops_on) lg_invalidate(c);   // outcomes made under the table name its operands
    c->ops_on = false;
    c->n_ops = 0;
    c->h_op_valid = false;
}

int ops_mirror(Ctx* c, const char* who) {
    if (!c->ops_on || c->h_op_valid) return DMX_OK;
    c->h_op_len.resize(c->n_ops);
    c->h_op_strand.resize(c->n_ops);
    if (c->n_ops) {
        OP_CK_KEEP(hipSetDevice(c->device));
        OP_CK_KEEP(hipMemcpy(c->h_op_len.data(), c->d_op_len.p, c->n_ops * 4, hipMemcpyDeviceToHost));
        OP_CK_KEEP(hipMemcpy(c->h_op_strand.data(), c->d_op_strand.p, c->n_ops, hipMemcpyDeviceToHost));
    }
    c->h_op_any = std::any_of(c->h_op_strand.begin(), c->h_op_strand.end(),
                              [](uint8_t x) { return x != 0; });
    c->h_op_valid = true;
    return DMX_OK;
}

namespace {

int ops_reserve(Ctx* c, const char* who, size_t n) {
    OP_CK(c->d_op.reserve(n));
    OP_CK(c->d_op_off.reserve(n));
    OP_CK(c->d_op_len.reserve(n));
    OP_CK(c->d_op_strand.reserve(n));
    return DMX_OK;
}

// The argument checks of dmx_set_operands; 0, or the code with *err set.
int ops_validate(const uint32_t* lens, size_t n_reads, const uint32_t* read, const int32_t* start,
                 const int32_t* stop, const uint8_t* strand, size_t n, std::string* err) {
    if (n >= (1ull << 31)) {
        *err = "dmx_set_operands: too many operands in one table";
        return DMX_E_UNSUPPORTED;
    }
    for (size_t k = 0; k < n; ++k) {
        const char* why = nullptr;
        if (read[k] >= n_reads) why = "names a read outside the batch";
        else if (start[k] < 0 || start[k] > stop[k]) why = "has start < 0 or start > stop";
        else if ((uint32_t)stop[k] > lens[read[k]]) why = "ends past its read";
        else if (strand[k] > 1) why = "has a strand other than 0 or 1";
        if (why) {
            *err = "dmx_set_operands: operand " + std::to_string(k) + " " + why;
            return DMX_E_INVALID;
        }
    }
    return DMX_OK;
}

}  // namespace
}  // namespace dmx

using namespace dmx;

extern "C" {

int dmx_set_operands(dmx_ctx* c, const uint32_t* read, const int32_t* start, const int32_t* stop,
                     const uint8_t* strand, size_t n) {
    const char* const who = "dmx_set_operands";
    if (!c) return DMX_E_INVALID;
    if (n && (!read || !start || !stop || !strand)) {
        c->err = "dmx_set_operands: null table";
        return DMX_E_INVALID;
    }
    if (!c->d_seq || !c->in.lens.p || c->chunked || c->h_lens.size() != c->n_reads) {
        c->err = "dmx_set_operands: no resident batch (dmx_load first)";
        return DMX_E_STATE;
    }
    if (const int rc = ops_validate(c->h_lens.data(), c->n_reads, read, start, stop, strand, n,
                                    &c->err))
        return rc;
    std::vector<OperandRec> v(n);
    for (size_t k = 0; k < n; ++k) v[k] = OperandRec{read[k], start[k], stop[k], strand[k]};
    OP_CK_KEEP(hipSetDevice(c->device));
    OP_CK_KEEP(hipStreamSynchronize(c->stream));
    ops_drop(c);
    lg_invalidate(c);   // outcomes made on whole reads name reads, not these operands
    if (const int rc = ops_reserve(c, who, n)) return rc;
    if (n) {
        OP_CK(hipMemcpyAsync(c->d_op.p, v.data(), n * sizeof(OperandRec), hipMemcpyHostToDevice,
                             c->stream));
        hipLaunchKernelGGL(operands_locate_kernel, dim3((uint32_t)((n + kOpBlock - 1) / kOpBlock)),
                           dim3(kOpBlock), 0, c->stream, (const OperandRec*)c->d_op.p, (uint32_t)n,
                           (const uint64_t*)c->in.offs.p, (uint32_t)c->n_reads, c->d_op_off.p,
                           c->d_op_len.p, c->d_op_strand.p);
        OP_CK(hipGetLastError());
    }
    OP_CK(hipStreamSynchronize(c->stream));   // `v` is pageable
    c->n_ops = n;
    c->ops_on = true;
    c->h_op_len.resize(n);   // the mirror, from the caller's own arrays
    c->h_op_strand.assign(strand, strand + n);
    for (size_t k = 0; k < n; ++k) c->h_op_len[k] = (uint32_t)(stop[k] - start[k]);
    c->h_op_any = std::any_of(c->h_op_strand.begin(), c->h_op_strand.end(),
                              [](uint8_t x) { return x != 0; });
    c->h_op_valid = true;
    return DMX_OK;
}

int dmx_clear_operands(dmx_ctx* c) {
    if (!c) return DMX_E_INVALID;
    ops_drop(c);
    return DMX_OK;
}

int dmx_operands_fetch(dmx_ctx* c, uint32_t* read, int32_t* start, int32_t* stop, uint8_t* strand,
                       size_t cap) {
    const char* const who = "dmx_operands_fetch";
    if (!c) return DMX_E_INVALID;
    if (!c->ops_on) return 0;
    const size_t n = std::min(c->n_ops, cap);
    if (n) {
        std::vector<OperandRec> v(n);
        OP_CK_KEEP(hipSetDevice(c->device));
        OP_CK_KEEP(hipMemcpyAsync(v.data(), c->d_op.p, n * sizeof(OperandRec), hipMemcpyDeviceToHost,
                             c->stream));
        OP_CK_KEEP(hipStreamSynchronize(c->stream));
        for (size_t k = 0; k < n; ++k) {
            if (read) read[k] = v[k].read;
            if (start) start[k] = v[k].start;
            if (stop) stop[k] = v[k].stop;
            if (strand) strand[k] = (uint8_t)v[k].strand;
        }
    }
    return (int)c->n_ops;
}

int dmx_result_operands(dmx_ctx* c, const uint8_t* keep, size_t n_keep, int32_t min_len,
                        uint64_t* bin_first, size_t n_first, uint64_t* n_operands) {
    const char* const who = "dmx_result_operands";
    if (!c) return DMX_E_INVALID;
    if (!bin_first) {
        c->err = "dmx_result_operands: null bin_first";
        return DMX_E_INVALID;
    }
    if (c->mode == DMX_MODE_LINKED) {
        c->err = "dmx_result_operands: linked mode has no operand table";
        return DMX_E_UNSUPPORTED;
    }
    if (!c->executed || c->chunked || !c->in.res.p || c->h_lens.size() != c->n_reads ||
        (c->exec_views && c->exec_view_gen != c->view_gen)) {
        c->err = "dmx_result_operands: no dmx_exec on the current batch and view list";
        return DMX_E_STATE;
    }
    if (c->n_counts < 3) {
        c->err = "dmx_result_operands: no bins";
        return DMX_E_STATE;
    }
    const size_t n_bins = c->n_counts - 2;
    const int A0 = c->panel[0].n_all;
    const int A1 = c->mode == DMX_MODE_TWO_ROUND ? c->panel[1].n_all : 0;
    if (c->exec_panel_gen != c->panel_gen || n_bins != (size_t)(A0 + 1) * (size_t)(A1 + 1) ||
        n_bins > kOpMaxBins) {
        c->err = "dmx_result_operands: the panels or the mode changed since the dmx_exec";
        return DMX_E_STATE;
    }
    if (min_len < 1) {
        c->err = "dmx_result_operands: min_len must be at least 1";
        return DMX_E_INVALID;
    }
    if (keep && n_keep != n_bins) {
        c->err = "dmx_result_operands: keep has " + std::to_string(n_keep) + " entries for " +
                 std::to_string(n_bins) + " bins (dmx_counts' indices)";
        return DMX_E_INVALID;
    }
    if (n_first != n_bins + 1) {
        c->err = "dmx_result_operands: bin_first has " + std::to_string(n_first) +
                 " entries, one more than the " + std::to_string(n_bins) + " bins are needed";
        return DMX_E_INVALID;
    }
    const size_t n = c->exec_items;
    OP_CK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    ops_drop(c);
    lg_invalidate(c);   // outcomes made on whole reads name reads, not these operands
    if (const int rc = ops_reserve(c, who, n)) return rc;
    const uint32_t tiles = (uint32_t)((n + kOpBlock - 1) / kOpBlock);
    const uint32_t n_blocks = std::max(1u, std::min(tiles, kOpGrid));
    const uint32_t span = std::max(1u, (tiles + n_blocks - 1) / n_blocks) * kOpBlock;
    DevBuf<uint32_t>& hist = c->d_op_hist;   // kept with the context: no allocation per call
    DevBuf<uint64_t>& first = c->d_op_first;
    DevBuf<uint8_t>& d_keep = c->d_op_keep;
    OP_CK(hist.reserve((size_t)n_blocks * n_bins));
    OP_CK(first.reserve(n_bins + 1));
    if (keep) {
        OP_CK(d_keep.reserve(n_bins));
        OP_CK(hipMemcpyAsync(d_keep.p, keep, n_bins, hipMemcpyHostToDevice, st));
    }
    OpBuildArgs A;
    A.bd = make_bounds(c, kKerOperands);
    A.res = c->in.res.p;
    A.views = c->exec_views ? c->d_views.p : nullptr;
    A.lens = c->in.lens.p;
    A.offs = c->in.offs.p;
    A.p0 = final_panel(c, 0);
    A.p1 = final_panel(c, 1);
    A.keep = keep ? d_keep.p : nullptr;
    A.n_items = (uint32_t)n;
    A.n_reads = (uint32_t)c->n_reads;
    A.span = span;
    A.n_bins = (uint32_t)n_bins;
    A.A0 = A0, A.A1 = A1, A.two_round = c->mode == DMX_MODE_TWO_ROUND;
    A.min_len = min_len;
    A.hist = hist.p;
    A.bin_first = first.p;
    A.op = c->d_op.p;
    A.op_off = c->d_op_off.p;
    A.op_len = c->d_op_len.p;
    A.op_strand = c->d_op_strand.p;
    A.cap = (uint32_t)std::min<size_t>(c->d_op.cap, 0xFFFFFFFFu);
    const size_t lds = n_bins * sizeof(uint32_t);
    OP_CK(bounds_reset(c, st));
    hipLaunchKernelGGL(operands_hist_kernel, dim3(n_blocks), dim3(kOpBlock), lds, st, A);
    hipLaunchKernelGGL(operands_scan_kernel, dim3(1), dim3(kOpBlock), lds, st, A, n_blocks);
    hipLaunchKernelGGL(operands_scatter_kernel, dim3(n_blocks), dim3(kOpBlock), lds, st, A);
    OP_CK(hipGetLastError());
    OP_CK(hipMemcpyAsync(bin_first, first.p, (n_bins + 1) * 8, hipMemcpyDeviceToHost, st));
    OP_CK(hipStreamSynchronize(st));
    if (const int brc = bounds_check(c, who)) return brc;
    c->n_ops = (size_t)bin_first[n_bins];
    c->ops_on = true;
    c->h_op_valid = false;   // the mirror comes down when a sorting call first needs it
    if (n_operands) *n_operands = c->n_ops;
    return DMX_OK;
}

// Plain sequential C++ on dmx_fetch's results.  The coordinates are composed as intervals of the
// read in the orientation each round took it (dmx/loop.py's plan_rounds and view_coords), not with
// the kernels' item records.
int dmx_result_operands_host(const dmx_result* res, size_t n_items, const uint32_t* v_read,
                             const int32_t* v_start, const int32_t* v_stop,
                             const uint8_t* v_strand, const uint32_t* lens, size_t n_reads,
                             int mode, const int* wheres0, int n0, const int* wheres1, int n1,
                             const uint8_t* keep, size_t n_keep, int32_t min_len, uint32_t* read,
                             int32_t* start, int32_t* stop, uint8_t* strand, size_t cap,
                             uint64_t* bin_first, size_t n_first, uint64_t* n_operands) {
    const std::string name = "dmx_result_operands_host: ";
    auto fail = [&](int code, const std::string& why) {
        set_process_error(name + why);
        return code;
    };
    if (mode == DMX_MODE_LINKED) return fail(DMX_E_UNSUPPORTED, "linked mode has no operand table");
    if (mode != DMX_MODE_SINGLE && mode != DMX_MODE_TWO_ROUND) return fail(DMX_E_INVALID, "unknown mode");
    const bool two = mode == DMX_MODE_TWO_ROUND, views = v_read != nullptr;
    if (n0 < 1 || !wheres0 || (two && (n1 < 1 || !wheres1)) || !bin_first || (n_items && !res) ||
        (n_reads && !lens) || (views && (!v_start || !v_stop || !v_strand)))
        return fail(DMX_E_INVALID, "null argument or empty panel");
    const int A1 = two ? n1 : 0;
    const size_t n_bins = (size_t)(n0 + 1) * (size_t)(A1 + 1);
    if (min_len < 1) return fail(DMX_E_INVALID, "min_len must be at least 1");
    if (keep && n_keep != n_bins) return fail(DMX_E_INVALID, "keep must have one entry per bin");
    if (n_first != n_bins + 1) return fail(DMX_E_INVALID, "bin_first must have one entry more than there are bins");
    struct Rec {
        uint32_t read, bin;
        int64_t a, b;
        uint8_t t;
    };
    std::vector<Rec> recs;
    std::vector<uint64_t> count(n_bins, 0);
    for (size_t k = 0; k < n_items; ++k) {
        const dmx_result& r = res[k];
        const int b1 = r.bin1, b2 = two ? r.bin2 : -1;
        if (b1 < -1 || b1 >= n0 || (two && (b2 < -1 || b2 >= n1)))
            return fail(DMX_E_INVALID, "item " + std::to_string(k) + " has a bin outside the panels");
        const size_t bin = (size_t)(b1 + 1) * (size_t)(A1 + 1) + (size_t)(b2 + 1);
        if (keep ? keep[bin] == 0 : (b1 < 0 || (two && b2 < 0))) continue;
        const uint32_t rd = views ? v_read[k] : (uint32_t)k;
        if (rd >= n_reads) return fail(DMX_E_INVALID, "item " + std::to_string(k) + " names a read outside the batch");
        // the item P = orient(read[vs:ve], vst); positions below count on orient(P, o)
        const int64_t vs = views ? v_start[k] : 0, ve = views ? v_stop[k] : (int64_t)lens[rd];
        const int vst = views ? v_strand[k] : 0;
        if (vs < 0 || vs > ve || ve > (int64_t)lens[rd] || vst > 1)
            return fail(DMX_E_INVALID, "item " + std::to_string(k) + " is no sub-range of its read");
        const int64_t n = ve - vs;
        // round 0 keeps orient(P, rc1)[x1:y1]
        int64_t x1 = 0, y1 = n;
        if (b1 >= 0) {
            if (wheres0[b1] & DMX_FRONT) x1 = r.m1.rstop;
            else y1 = r.m1.rstart;
        }
        int o = r.rc1 ? 1 : 0;
        int64_t x = x1, y = y1;
        if (two && b1 >= 0) {
            // round 1 ran on T1 = orient(P, rc1)[x1:y1] and keeps orient(T1, rc2)[x2:y2], which
            // is orient(P, rc1 ^ rc2)[..]: on the reversed strand T1 is [n - y1 : n - x1]
            const int64_t n1len = y1 - x1;
            int64_t x2 = 0, y2 = n1len;
            if (b2 >= 0) {
                if (wheres1[b2] & DMX_FRONT) x2 = r.m2.rstop;
                else y2 = r.m2.rstart;
            }
            const int64_t base = r.rc2 ? n - y1 : x1;
            o ^= r.rc2 ? 1 : 0;
            x = base + x2;
            y = base + y2;
        }
        if (x < 0 || x > y || y > n)
            return fail(DMX_E_INVALID, "item " + std::to_string(k) + " has a match outside its view");
        if (y - x < min_len) continue;
        // orient(read[vs:ve], t)[x:y], t = vst ^ o, on the read as given
        const int t = vst ^ o;
        Rec R;
        R.read = rd;
        R.bin = (uint32_t)bin;
        R.a = t ? ve - y : vs + x;
        R.b = t ? ve - x : vs + y;
        R.t = (uint8_t)t;
        recs.push_back(R);
        ++count[bin];
    }
    uint64_t at = 0;
    for (size_t b = 0; b < n_bins; ++b) {
        bin_first[b] = at;
        at += count[b];
    }
    bin_first[n_bins] = at;
    std::vector<uint64_t> next(bin_first, bin_first + n_bins);
    for (const Rec& R : recs) {   // in item order: stable inside a bin
        const uint64_t dst = next[R.bin]++;
        if (dst >= cap) continue;
        if (read) read[dst] = R.read;
        if (start) start[dst] = (int32_t)R.a;
        if (stop) stop[dst] = (int32_t)R.b;
        if (strand) strand[dst] = R.t;
    }
    if (n_operands) *n_operands = at;
    return DMX_OK;
}

// Host only: dmx_set_operands' argument checks on read lengths, without a context.
int dmx_operands_check_host(const uint32_t* lens, size_t n_reads, const uint32_t* read,
                            const int32_t* start, const int32_t* stop, const uint8_t* strand,
                            size_t n) {
    if ((n_reads && !lens) || (n && (!read || !start || !stop || !strand))) {
        set_process_error("dmx_set_operands: null table");
        return DMX_E_INVALID;
    }
    std::string err;
    const int rc = ops_validate(lens, n_reads, read, start, stop, strand, n, &err);
    if (rc) set_process_error(err);
    return rc;
}

}  // extern "C"
