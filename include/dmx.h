/*
 * dmx.h — C-ABI of the MI355X-native two-round barcode demultiplexer (libdmx.so).
 *
 * Drop-in boundary.  In the reference the hot path is a PROCESS boundary: bash calls the
 * `cutadapt` executable (scripts/02_cutadapt_loop.sh:64-72 round 1, :91-103 round 2;
 * scripts/04_cleaning_primers.sh:371-388 linked primers).  Our drop-in `cutadapt` CLI
 * (nanopore-barcoding-orc_amd/bin/cutadapt, Python) keeps that surface and calls this library
 * through ctypes.  Each entry point below names the cutadapt-side interface whose work it
 * replaces (upstream cutadapt 4.9 is not vendored in /root/reference).
 *
 * Conventions: plain pointers and sizes, no torch types.  Host buffers are caller-owned, device
 * buffers library-owned.  Status 0 = OK, negative = error (message via dmx_last_error).
 * One context per device; a context is not thread-safe (one host thread per context).
 */
#ifndef DMX_H
#define DMX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 also covers the calls added since without a bump, all additive (no existing signature or
 * behaviour changed): the amplicon-sorting entry points below, and dmx_set_panel_ex,
 * dmx_ends_host, DMX_ANCHORED, DMX_NONINTERNAL and the operand-table calls.  A caller that needs
 * one of them checks for the symbol. */
#define DMX_ABI_VERSION 4

/* Panel flags (dmx_set_panel.flags). */
#define DMX_FRONT 0x01  /* -g ADAPTER: 5' adapter, Where.FRONT (prefix of adapter may be skipped at read start) */
#define DMX_BACK 0x02   /* -a ADAPTER: 3' adapter, Where.BACK  (suffix may be skipped at read end)          */
/* Restricted adapter types, each combined with DMX_FRONT or DMX_BACK; both
 * together is DMX_E_INVALID.  Their matches touch the start (FRONT) or the end (BACK) of the view. */
#define DMX_ANCHORED 0x04    /* -g ^ADAPTER / -a ADAPTER$: the whole adapter (min_overlap = its length)      */
#define DMX_NONINTERNAL 0x08 /* -g XADAPTER / -a ADAPTERX: may be cut off at the read end it touches only     */
#define DMX_RC 0x10     /* --rc: also try the reverse complement; use it iff its score is strictly greater  */

/* Run modes (dmx_set_mode). */
#define DMX_MODE_SINGLE 0    /* one cutadapt invocation: round 0 panel only                                   */
#define DMX_MODE_TWO_ROUND 1 /* 02_cutadapt_loop.sh fused: round 0 on the read, round 1 on the round-0-trimmed */
#define DMX_MODE_LINKED 2    /* -g F...R linked pairs: round 0 = fronts, round 1 = backs (pair i <-> i)        */

/* Error codes. */
#define DMX_OK 0
#define DMX_E_INVALID -1
#define DMX_E_HIP -2
#define DMX_E_NOMEM -3
#define DMX_E_UNSUPPORTED -4
#define DMX_E_STATE -5

/* One adapter match (cutadapt Match: astart/astop on the adapter, rstart/rstop on the read view
 * that round was run on, i.e. already reverse-complemented when rc == 1). */
typedef struct dmx_match {
    int32_t rstart, rstop;
    int16_t astart, astop;
    int16_t score, errors;
} dmx_match;

/* Per-read result (caller-owned array, one entry per read).
 * bin = adapter index in the panel (file order), -1 = no match ("unknown").
 * TWO_ROUND: m2 coordinates are on the round-1 output (trimmed, oriented) sequence.
 * LINKED: bin1 = bin2 = pair index; m1 = front part on the read, m2 = back part on
 *         read[m1.rstop:]. */
typedef struct dmx_result {
    int16_t bin1, bin2;
    uint8_t rc1, rc2;
    uint8_t flags, _pad;
    dmx_match m1, m2;
} dmx_result;

typedef struct dmx_ctx dmx_ctx;

/* Replaces: process start-up of `cutadapt -j N` (cli.main).  Opens HIP device `device`. */
int dmx_open(int device, dmx_ctx** out);
/* Replaces: cutadapt's exit. */
void dmx_close(dmx_ctx* ctx);
/* ctx = NULL: the last failure of a call that takes no context (dmx_comm_unique_id: why RCCL
 * could not be loaded), or "null context". */
const char* dmx_last_error(dmx_ctx* ctx);
int dmx_abi_version(void);

/* Replaces: parser.py adapter parsing of `-g file:` / `-a file:` / `-g F...R` (one call per panel).
 * seqs: uppercase IUPAC (U already mapped to T), lens <= 64.  max_errors: -e value (< 1 rate,
 * >= 1 absolute count).  min_overlap: -O (cutadapt default 3).  Adapter wildcards are enabled for
 * an adapter iff it has a non-ACGT character (cutadapt default). */
int dmx_set_panel(dmx_ctx* ctx, int round, const char* const* seqs, const int* lens,
                  int n_adapters, double max_errors, int min_overlap, int flags);
/* As dmx_set_panel, with a per-adapter DMX_FRONT / DMX_BACK (one cutadapt call mixing -g and -a,
 * scripts/04_cleaning_primers.sh:476-507); rc: 1 for --rc. */
int dmx_set_panel_mixed(dmx_ctx* ctx, int round, const char* const* seqs, const int* lens,
                        const int* wheres, int n_adapters, double max_errors, int min_overlap,
                        int rc);
/* As dmx_set_panel_mixed, with a minimum overlap per adapter: min_overlaps[a] replaces
 * min_overlap for adapter a (NULL: min_overlap for all).  wheres[a] is DMX_FRONT or DMX_BACK,
 * alone or with DMX_ANCHORED or DMX_NONINTERNAL (dmx_set_panel's flags and dmx_set_panel_mixed's
 * wheres take the two bits too).  An anchored adapter's minimum overlap is its length, whatever
 * is passed.  The unrestricted adapters of a panel share one minimum overlap (DMX_E_UNSUPPORTED
 * otherwise) and run through the internal-adapter pipeline; the restricted ones run through the
 * end-window stage, and both meet in the read's winner slot with their panel indices.
 * DMX_MODE_LINKED refuses a panel with restricted adapters at dmx_exec (DMX_E_UNSUPPORTED). */
int dmx_set_panel_ex(dmx_ctx* ctx, int round, const char* const* seqs, const int* lens,
                     const int* wheres, const int* min_overlaps, int n_adapters,
                     double max_errors, int min_overlap, int rc);
int dmx_set_mode(dmx_ctx* ctx, int mode);
/* Host only (no GPU; tests, the sanitizer program): one DMX_MODE_SINGLE round of the panel
 * dmx_set_panel_ex would build, on a dmx_pack layout, by a plain full-matrix DP per (read,
 * orientation, adapter) over cutadapt's column range with its boundary conditions (a different
 * algorithm from the kernels' on purpose: no bit-vectors, no windows lists, no keys).  Every
 * adapter type, restricted or not.  out[i] is what dmx_run writes for read i.  Errors:
 * dmx_last_error(NULL). */
int dmx_ends_host(const char* const* seqs, const int* lens, const int* wheres,
                  const int* min_overlaps, int n_adapters, double max_errors, int min_overlap,
                  int rc, const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
                  const uint32_t* read_lens, size_t n_reads, dmx_result* out);
/* Host only (no GPU; tests): the piece screen dmx_set_panel would build for
 * these arguments: out[0..7] = {sampling stride (0 = off: the full filter pass), pieces, sampled
 * 8-mer keys, entries, FRONT partial-alignment reach, positions per screen lane, min len + dlo - 1
 * of orientation-0 pieces, min dlo of orientation-1 pieces}; entries (up to cap, may be NULL):
 * the packed (piece, offset) entries, grouped by 8-mer (dmx_device.h piece_entry). */
int dmx_panel_pieces(const char* const* seqs, const int* lens, int n_adapters, double max_errors,
                     int min_overlap, int flags, int32_t* out, int n_out, uint64_t* entries,
                     int cap);
/* Host only (no GPU; tests): the lookup tables of that piece screen as the kernels hold them.
 * pair[4096]: row r (a 6-nt core, 12 bits) has bit a set iff the 8-mer r << 4 | a is sampled and
 * bit 16 + b iff the 8-mer b << 12 | r is, so 20 bits K of codes answer the 8-mers at nt 0 and
 * nt 2 from row K[4:16].  rank_base[1024]: low-half bits set in the rows before row 4 i; the key
 * index of a sampled 8-mer k is rank_base[k >> 6] + the low-half bits of rows (k >> 4 & ~3) ..
 * (k >> 4) - 1 + the bits below k & 15 of row k >> 4.  keys (up to cap, may be NULL): key i =
 * first entry | count << 16 into dmx_panel_pieces' entries, by increasing 8-mer (out[2] keys).
 * All zero when the screen is off. */
int dmx_panel_piece_pairs(const char* const* seqs, const int* lens, int n_adapters,
                          double max_errors, int min_overlap, int flags, uint32_t* pair,
                          uint16_t* rank_base, uint32_t* keys, int cap);
/* Host only (no GPU; tests): how far the kernels' gathers reach around a read view for the
 * panel dmx_set_panel (wheres == NULL) or dmx_set_panel_mixed (wheres, flags & DMX_RC) would
 * build from these arguments, in nt: out[0] before view position 0 as the kernels' warm-up
 * formulas ask, out[1] after the clamp at -64 (positions before it are read at -64: warm-up
 * columns, where any codes are safe), out[2] past the view end, out[3] / out[4] the guard
 * needed below / above the packed words for the smallest offset and tail dmx_run accepts, out[5]
 * the guard the device buffers carry.  Returns what dmx_set_panel would return: it refuses a
 * panel with out[3] or out[4] > out[5] (DMX_E_UNSUPPORTED, out still filled). */
int dmx_panel_reach(const char* const* seqs, const int* lens, const int* wheres, int n_adapters,
                    double max_errors, int min_overlap, int flags, int32_t* out, int n_out);
/* Host only (no GPU; tests): the near-start columns of that panel that only its first adapter
 * scans.  A 5' panel whose adapters share a suffix S keeps, at the read start, partial matches
 * that lie wholly inside S; they are the same match for every adapter, and the first adapter
 * wins ties.  out[0] = the last such column (|S| - out[3]), or -1 where every adapter scans
 * every column: a 3' or mixed panel, no shared suffix block, |S| <= out[3], acceptance limits
 * that differ among the adapters for overlaps <= |S|, or DMX_NEAR_ALL=1 in the environment (A/B
 * and tests).  out[1] = |S| as the filter uses it (0 = off), out[2] = the first column whose
 * matches contain a whole index block (0 without the index screen), out[3] = the largest
 * number of errors any match of the panel may have.  n_out >= 4. */
int dmx_panel_near_shared(const char* const* seqs, const int* lens, const int* wheres,
                          int n_adapters, double max_errors, int min_overlap, int flags,
                          int32_t* out, int n_out);

/* Host-side packer (no GPU needed): ASCII reads -> 2-bit codes (A=0,C=1,G=2,T=3, 16 nt per
 * little-endian u32 word) + 1-bit "no-match" mask (any non-ACGT byte, e.g. N).  Reads are laid
 * out back to back starting at nt offset DMX_PACK_PAD; out_offsets[i] is read i's first nt.
 * Required words for both outputs: dmx_pack_words(total_nt). */
#define DMX_PACK_PAD 64
size_t dmx_pack_words(uint64_t total_nt, size_t n_reads);
int dmx_pack(const uint8_t* ascii, const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
             uint32_t* out_seq2b, uint32_t* out_nmask, uint64_t* out_offsets);

/* Replaces: the per-read hot loop of one or more cutadapt runs (ReverseComplementer ->
 * AdapterCutter.best_match -> Adapter.match_to -> Aligner.locate, for every read) for the whole
 * input.  Synchronous: uploads, runs both rounds on the GPU, downloads `out`.  Layout contract
 * (checked; DMX_E_INVALID otherwise): every read has offsets[i] >= 16 and offsets[i] + lens[i]
 * + 64 <= 16 * n_words, lens[i] < 2^30.  Reads may overlap or come in any order.  The device
 * copies carry 1024 nt of zeroed guard on both sides, and every panel is checked to keep the
 * kernels' gathers around a view inside it for such offsets (dmx_panel_reach).  Batches in
 * dmx_pack's layout above 1.5 chunks (DMX_RUN_CHUNK reads, default 2^21) run as overlapped
 * chunks, others in one shot (same results). */
int dmx_run(dmx_ctx* ctx, const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
            const uint32_t* lens, size_t n_words, size_t n_reads, dmx_result* out);

/* As dmx_run, with the no-match mask given sparsely: its nonzero 32-bit words (mask word index
 * = nt / 32, as in dmx_pack's nmask) as strictly increasing exc_idx[] with their values
 * exc_val[].  Almost every nt of a read is A/C/G/T, so this uploads ~1% of the dense bitmap's
 * bytes; the device zero-fills the mask and scatters the exceptions.  Same results as dmx_run. */
int dmx_run_sparse(dmx_ctx* ctx, const uint32_t* seq2b, const uint32_t* exc_idx,
                   const uint32_t* exc_val, size_t n_exc, const uint64_t* offsets,
                   const uint32_t* lens, size_t n_words, size_t n_reads, dmx_result* out);
/* Host helper (no GPU): the nonzero words of a dmx_pack no-match mask of n_words words, in
 * increasing index order (first `cap` written); returns their total number. */
size_t dmx_mask_exceptions(const uint32_t* nmask, size_t n_words, uint32_t* out_idx,
                           uint32_t* out_val, size_t cap);
/* Page-lock (pin) / release caller host memory that batches are uploaded from (reused batch
 * buffers): pinned uploads run at the DMA rate instead of through pageable staging. */
int dmx_host_register(void* ptr, size_t bytes);
int dmx_host_unregister(void* ptr);

/* Number of visible HIP devices (0 if none). */
int dmx_device_count(void);

/* Multi-GPU form of dmx_run: the batch (dmx_pack layout) is split into
 * n_ctx contiguous read ranges balanced by total length, each range runs on its own context
 * (one device each) from its own host thread, and results land in `out` in input order.
 * out_counts (optional, n_counts entries) receives the per-bin counts summed over the shards:
 * when the contexts are one dmx_comm_init_all set (in that order), by an RCCL all-reduce of the
 * devices' count arrays over xGMI; otherwise (e.g. several contexts sharing one device) on the
 * host.  Returns the number of count entries (or DMX_OK without out_counts), negative on error
 * (message via dmx_last_error(ctxs[0])).  Contexts must share mode and panels. */
int dmx_run_multi(dmx_ctx* const* ctxs, int n_ctx, const uint32_t* seq2b, const uint32_t* nmask,
                  const uint64_t* offsets, const uint32_t* lens, size_t n_words, size_t n_reads,
                  dmx_result* out, uint64_t* out_counts, size_t n_counts);

/* ---- Multi-GPU count exchange (RCCL over xGMI) -------------------------------
 * Replaces: the per-adapter totals of the reference's single cutadapt process per panel
 * (scripts/02_cutadapt_loop.sh:64-72,91-103, `-j 24` workers on one node, report.py); sharded
 * over GPUs, each shard's (A0+1)(A1+1)+2 counts are summed in HBM by one ncclAllReduce.
 * One process, several GPUs: dmx_comm_init_all over contexts on distinct devices (ncclCommInitAll;
 * rank k = ctxs[k]); dmx_run_multi then reduces its counts with RCCL.
 * One process per GPU: rank 0 calls dmx_comm_unique_id and hands the DMX_COMM_ID_BYTES bytes to
 * every rank (any control plane), each rank calls dmx_comm_init_rank (ncclCommInitRank; blocks
 * until all ranks joined), then after each dmx_exec dmx_allreduce_counts (collective: every rank
 * calls it) sums the ranks' counts in place on the context's stream and copies them to
 * out_counts (optional); dmx_counts then returns the summed counts until the next dmx_exec.
 * dmx_close releases the communicator. */
#define DMX_COMM_ID_BYTES 128
int dmx_comm_unique_id(uint8_t* id);
int dmx_comm_init_rank(dmx_ctx* ctx, const uint8_t* id, int n_ranks, int rank);
int dmx_comm_init_all(dmx_ctx* const* ctxs, int n_ctx);
/* Number of ranks of the context's communicator (0 = none). */
int dmx_comm_size(dmx_ctx* ctx);
/* Returns the number of count entries, negative on error. */
int dmx_allreduce_counts(dmx_ctx* ctx, uint64_t* out_counts, size_t n_out);

/* Device-resident form (benchmarks / pipelined hosts): dmx_load copies a packed batch to HBM
 * once; dmx_exec enqueues the full pipeline on the context's stream (asynchronous); dmx_sync
 * waits; dmx_fetch copies results of the last exec to the host. */
int dmx_load(dmx_ctx* ctx, const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
             const uint32_t* lens, size_t n_words, size_t n_reads);
int dmx_exec(dmx_ctx* ctx);
/* dmx_exec as dmx_run runs it: waits for the pipeline, and when an intermediate list overflowed
 * grows it and runs again (never a truncated result); DMX_E_STATE on an exactness flag.  For
 * hosts that keep the batch resident (the view runs below) and want dmx_run's guarantees. */
int dmx_exec_checked(dmx_ctx* ctx);
int dmx_sync(dmx_ctx* ctx);
int dmx_fetch(dmx_ctx* ctx, dmx_result* out);

/* Replaces: cutadapt's per-adapter match statistics (report.py).  counts has
 * (A0+1)*(A1+1) entries: index (bin1+1)*(A1+1) + (bin2+1) (A1 = 0 in SINGLE mode), then
 * two more entries: number of reads that used the reverse complement in round 0 / round 1. */
int dmx_counts(dmx_ctx* ctx, uint64_t* out_counts, size_t n_out);

/* Diagnostics of the last dmx_exec: per-stage device time in ms measured with HIP events on the
 * context's stream (order: scan0, resolve0, finalize0, scan1, resolve1, finalize1, total, then
 * the parts of scan0/scan1 spent in the shared-suffix filter and the prefix verification:
 * filter0, verify0, filter1, verify1, then the index screen and the window scan:
 * screen0, wscan0, screen1, wscan1, then the piece screen's part of filter0 / filter1:
 * pieces0, pieces1, then the end-window stage: ends0, ends1 — pass n_stage = 19 to receive them
 * all), and
 * counts[n_counts <= 18] = {candidate clusters r0, r1, filter windows kept for the window scan
 * r0, r1, candidate cells (band mode) or clusters resolved after pruning (ring mode) r0, r1,
 * band DPs / tracebacks r0, r1, filter windows before prefix verification r0, r1, (window
 * piece, adapter) tasks passed by the index screen r0, r1, filter tasks of the piece screen
 * r0, r1, (view, orientation, restricted adapter) triples the end-window stage ran its exact DP
 * for r0, r1, triples it looked at (views of at least min_overlap columns) r0, r1}, and flags
 * (bit0 cluster overflow, bit1 exactness-check violation, bit2 filter-window / task overflow,
 * bit3 candidate-cell overflow, bit4 a filter invariant (step bucket or piece-screen cell range)
 * violated, bit5 a bounds violation (DMX_DEBUG_BOUNDS builds); must be 0). */
int dmx_stats(dmx_ctx* ctx, float* stage_ms, int n_stage, uint64_t* counts, int n_counts,
              int* flags);

/* Diagnostics (tests and tools only): copy an intermediate list of the last dmx_exec to the host
 * (up to cap_bytes; returns the list's size in bytes, negative on error).  The window and task
 * lists are shared by both rounds, so after a two-round exec only round 1's are resident; the
 * candidate lists are per round.  Records are the library's internal layouts (40-byte windows /
 * tasks / candidates; DMX_DBG_FLAGS: the 4-byte pipeline flags word). */
#define DMX_DBG_WINDOWS 0
#define DMX_DBG_VERIFIED 1
#define DMX_DBG_TASKS 2
#define DMX_DBG_CANDS0 3
#define DMX_DBG_CANDS1 4
#define DMX_DBG_FLAGS 5
int dmx_debug_fetch(dmx_ctx* ctx, int what, int round, void* out, size_t cap_bytes);
/* DMX_DEBUG_BOUNDS builds only (dmx/libdmx_bounds.so; DMX_E_UNSUPPORTED otherwise): every gather
 * of the packed batch and every winner-slot / item / result / count access of every kernel is
 * checked against its buffer; a violation is skipped, and dmx_exec / dmx_run / dmx_chop_exec fail
 * with DMX_E_STATE naming the kernel, buffer and index (dmx_last_error).  This self test launches
 * one gather below the guard, one winner slot past its array and one valid gather; out3 receives
 * {codes read below the guard (0), slot check result (0), a valid gather}; returns DMX_E_STATE
 * with the first violation's message when the checks work. */
int dmx_debug_bounds_selftest(dmx_ctx* ctx, uint32_t* out3);

/* ---- Residual-primer failsafe: exact degenerate-motif location (`seqkit locate -d`) ---------
 * Replaces: `seqkit locate -d --pattern-file PRIMERS ENDS` in the failsafe of
 * scripts/04_cleaning_primers.sh:397-460 (`:422`; seqkit v2, not vendored).  Every occurrence
 * (overlapping ones included) of every IUPAC pattern (1..64 nt, at most 128 patterns) in every
 * record, on the positive strand and — unless DMX_LOC_ONLY_POSITIVE — on the negative strand
 * (the pattern matched against the reverse complement; reported in positive-strand
 * coordinates).  Case-sensitive unless DMX_LOC_IGNORE_CASE (seqkit -i).  Pattern codes admit
 * A/C/G/T(U) as IUPAC says (N = any of them); any other record byte matches nothing.
 * Records are ASCII (caller-owned blob + offsets/lengths).  Writes min(total, cap) hits in
 * unspecified order, *n_hits = total (call again with a larger buffer if total > cap). */
#define DMX_LOC_IGNORE_CASE 0x1
#define DMX_LOC_ONLY_POSITIVE 0x2
typedef struct dmx_hit {
    uint64_t seq;      /* record index                                    */
    int32_t pattern;   /* pattern index                                   */
    int32_t strand;    /* 0 = '+', 1 = '-'                                */
    int32_t start;     /* 1-based first position on the positive strand   */
    int32_t end;       /* 1-based last position (inclusive)               */
} dmx_hit;
int dmx_locate(dmx_ctx* ctx, const char* const* patterns, const int* plens, int n_patterns,
               int flags, const uint8_t* ascii, const uint64_t* offsets, const uint32_t* lens,
               size_t n_seqs, dmx_hit* out, size_t cap, uint64_t* n_hits);

/* ---- Read reorientation, pychopper style (the producer of the demultiplexer's input) ---------
 * Replaces: the primer search and read segmentation of
 *   `pychopper -b M13_seqs_for_pychopper.fa -c M13_config_for_pychopper.txt -p -m edlib`
 * (scripts/01_pychopper.sh:45-57; pychopper 2.7.10 / edlib are not vendored — the semantics are
 * restated in DESIGN.md §8d, parity unpinned).  Runs on the batch made resident by dmx_load.
 * Labels: primer p (file order) is label 2p, its reverse complement label 2p+1 (pychopper's
 * "-NAME").  IUPAC codes in primers (N = any base); a read N matches anything.
 * Hits: per label, as one edlib HW / EDLIB_TASK_LOC call with k = (int)(cutoff * m): when the
 * least infix edit distance over the read, best, is <= k, every read column whose least
 * distance equals best is a hit (stop), with the start of the longest optimal alignment
 * ending there (edlib's reverse SHW alignment, last position).
 * Segments: in a read's hits sorted by (start, stop, label), consecutive hits (a, b) with a
 * rule (rule_left[r], rule_right[r]) are a candidate segment on strand rule_strand[r] (0 '+',
 * 1 '-'; the first rule of a pair wins) spanning [a.start, b.stop) with keep_primers
 * (pychopper -p), else [a.stop, b.start) (empty if the hits overlap).  The read's segments are
 * the best path over its candidates: no two share a hit, greatest summed length (pychopper's
 * usable length), ties -> the earlier candidate. */
#define DMX_CHOP_MAX_PRIMERS 8
#define DMX_CHOP_MAX_RULES 32
typedef struct dmx_chop_hit {
    uint32_t read;
    int16_t label;
    int16_t dist;          /* edit distance                                        */
    int32_t start, stop;   /* [start, stop) on the read as given                   */
} dmx_chop_hit;
typedef struct dmx_chop_seg {
    uint32_t read;
    int32_t start, stop;   /* [start, stop) on the read as given, stop >= start     */
    int16_t strand;        /* 0 = '+', 1 = '-' (the segment is written reverse-complemented) */
    int16_t rule;
} dmx_chop_seg;
/* primers: uppercase IUPAC (U -> T), 1..64 nt each; cutoff in [0, 1). */
int dmx_chop_set(dmx_ctx* ctx, const char* const* primers, const int* plens, int n_primers,
                 const int* rule_left, const int* rule_right, const int* rule_strand, int n_rules,
                 double cutoff, int keep_primers);
/* Hits and segments of every resident read (synchronous); totals in *n_hits / *n_segs. */
int dmx_chop_exec(dmx_ctx* ctx, uint64_t* n_hits, uint64_t* n_segs);
/* Results of the last dmx_chop_exec (any pointer may be NULL): per-read segment and hit counts
 * (n_reads entries each) and the first seg_cap / hit_cap records in read order (within a read:
 * segments left to right, hits by (start, stop, label)). */
int dmx_chop_fetch(dmx_ctx* ctx, uint32_t* n_seg, uint32_t* n_hit, dmx_chop_seg* segs,
                   size_t seg_cap, dmx_chop_hit* hits, size_t hit_cap);
/* Device time (ms) of the last dmx_chop_exec: [0] chop_kernel (and chop_big_kernel when blocks
 * overflowed), [1] the read-order compaction.  Returns the number of 64-read blocks redone with
 * global hit lists (more primer hits than the 512-entry LDS list holds). */
int dmx_chop_stats(dmx_ctx* ctx, float* ms, int n_ms);

/* ---- Views of the resident reads ----------------------------------------------
 * Run the demultiplexer on oriented sub-ranges of the resident reads instead of on the reads:
 * rescued segments, caller-chosen windows, or pychopper's PASS segments without repacking them
 * (the fused 01 -> 02 loop).  View k is read[k][start[k]:stop[k]] of the batch made resident by
 * dmx_load, on the read as given, taken reverse-complemented when strand[k] == 1 (the
 * conventions of dmx_batch_pack_views and dmx_chop_seg).  With a view list set, round 0 of
 * dmx_exec runs on the views: item k is view k, dmx_fetch writes one result per view (m1 in view
 * coordinates, m2 on the round-1 output of view k: what dmx_run returns for the batch
 * dmx_batch_pack_views makes of the same list), dmx_counts counts views.  Views may repeat,
 * overlap, come in any order, be empty or shorter than min_overlap, and outnumber the reads.
 * DMX_MODE_SINGLE and DMX_MODE_TWO_ROUND, every adapter type; DMX_MODE_LINKED with views set is
 * refused by dmx_exec (DMX_E_UNSUPPORTED).  dmx_load, dmx_run, dmx_run_sparse and dmx_run_multi
 * drop the list (whole-read runs again); dmx_run_multi and the chunked dmx_run are whole-read only.
 * Everything is checked on the host before anything is uploaded or launched, and a refused call
 * leaves the context and its current list as they were: no resident batch is DMX_E_STATE; a read
 * index outside the batch, start < 0, start > stop, stop past the read's end or strand > 1 is
 * DMX_E_INVALID naming the view; more than 2^31 views is DMX_E_UNSUPPORTED.  (A failed device
 * allocation, DMX_E_HIP, leaves no list: whole-read runs.)
 * dmx_fetch copies as many results as the last dmx_exec's round 0 had items, whatever list was
 * set or cleared since that exec: size its buffer by the list the exec ran on. */
int dmx_set_views(dmx_ctx* ctx, const uint32_t* read, const int32_t* start, const int32_t* stop,
                  const uint8_t* strand, size_t n_views);
/* Back to whole-read runs (no-op without a list). */
int dmx_clear_views(dmx_ctx* ctx);
/* The view list made on the device from the last dmx_chop_exec, in read order: read r gives its
 * segment as a view iff it has exactly one segment, qc_ok == NULL or qc_ok[r] != 0 (one byte per
 * read) and stop - start >= min_len: pychopper's PASS records.  The segments are not fetched; the
 * list and its length stay on the device for dmx_exec, *n_views (optional) receives the length.
 * DMX_E_STATE without a dmx_chop_exec on the current batch. */
int dmx_chop_views(dmx_ctx* ctx, const uint8_t* qc_ok, int32_t min_len, uint64_t* n_views);
/* The current list in dmx_set_views' convention, first `cap` views written (any pointer may be
 * NULL); returns its length (0 without a list), negative on error. */
int dmx_views_fetch(dmx_ctx* ctx, uint32_t* read, int32_t* start, int32_t* stop,
                    uint8_t* strand, size_t cap);
/* Host only (no GPU; tests): dmx_chop_views' rule in plain sequential C++ on dmx_chop_fetch's
 * arrays (n_seg: per-read segment counts, segs: the records in read order).  First `cap` views
 * written (any out pointer may be NULL); returns the list's length, negative on error
 * (dmx_last_error(NULL)). */
int dmx_chop_views_host(const uint32_t* n_seg, const dmx_chop_seg* segs, const uint8_t* qc_ok,
                        int32_t min_len, size_t n_reads, uint32_t* read, int32_t* start,
                        int32_t* stop, uint8_t* strand, size_t cap);

/* ---- Operand tables: the sorting calls on sub-ranges of the resident reads ----
 * The demultiplexer leaves every base of every well in HBM, as a sub-range of a resident read in
 * a known orientation.  With an operand table set, the amplicon-sorting calls below run on such
 * sub-ranges without a second pack and dmx_load.  Operand k is read[k][start[k]:stop[k]] of the
 * batch made resident by dmx_load, on the read as given, taken reverse-complemented when
 * strand[k] == 1 (the conventions of dmx_set_views).
 * Contract with a table set: every index that dmx_pairdist, dmx_pairhits (and dmx_pairhits_fetch,
 * dmx_hitgroups, dmx_hithist, dmx_pairhits_cross, dmx_hitgroups_within on its outcomes),
 * dmx_groupalign, dmx_groupalign_strands, dmx_rowdist and dmx_rowassign document as "a read of
 * the resident batch" names an operand, every per-read array (best, tie, label, cap2, bin_off,
 * labels, n_nodes >= n_reads and the like) has one entry per operand, and the results are those
 * the same call returns on a batch whose reads are the operands' sequences, packed by dmx_pack.
 * dmx_pairhits' rev bit is the caller's view: 1 = the retry against the reverse-complemented
 * target hit.  dmx_pairalign with a table set is DMX_E_UNSUPPORTED; dmx_rowpairdist and
 * dmx_rowhits read no batch and are unchanged.
 * Everything is checked on the host before anything is uploaded, and a refused call leaves the
 * context and its current table as they were: no resident batch is DMX_E_STATE; a read index
 * outside the batch, start < 0, start > stop, stop past the read's end or strand > 1 is
 * DMX_E_INVALID naming the operand; more than 2^31 operands is DMX_E_UNSUPPORTED.  (A device
 * failure, DMX_E_HIP, while a table is being set or built leaves no table; one in a call that
 * only reads the table, dmx_operands_fetch or a sorting call, leaves it as it was.)  Operands may repeat, overlap, outnumber the
 * reads and be empty; an empty operand is refused only by a call that names it, as a 0-nt read is.
 * dmx_load, dmx_run, dmx_run_sparse, dmx_run_multi and dmx_clear_operands drop the table.  Setting,
 * replacing or dropping a table drops the outcomes of dmx_pairhits, which name its operands.  The
 * table is independent of the demultiplexer's view list (dmx_set_views); both may be set. */
int dmx_set_operands(dmx_ctx* ctx, const uint32_t* read, const int32_t* start, const int32_t* stop,
                     const uint8_t* strand, size_t n_operands);
/* Back to whole reads (no-op without a table). */
int dmx_clear_operands(dmx_ctx* ctx);
/* The current table in dmx_set_operands' convention, first `cap` operands written (any pointer
 * may be NULL); returns its length (0 without a table), negative on error. */
int dmx_operands_fetch(dmx_ctx* ctx, uint32_t* read, int32_t* start, int32_t* stop,
                       uint8_t* strand, size_t cap);
/* Test-only (host, no GPU; not for callers, who get the same answers from dmx_set_operands):
 * dmx_set_operands' argument checks against the read lengths of a batch, so that the CPU suite
 * reaches them.  DMX_OK, or the code dmx_set_operands returns, with the message in dmx_last_error(NULL). */
int dmx_operands_check_host(const uint32_t* lens, size_t n_reads, const uint32_t* read,
                            const int32_t* start, const int32_t* stop, const uint8_t* strand,
                            size_t n_operands);
/* The table of a demultiplexer run, made on the device.  After a dmx_exec / dmx_exec_checked in
 * DMX_MODE_SINGLE or DMX_MODE_TWO_ROUND on the current batch and view list (DMX_E_STATE
 * otherwise; DMX_MODE_LINKED is DMX_E_UNSUPPORTED): one operand per item of round 0 (a read, or
 * view k of a view run) whose bin is kept, the bin index being dmx_counts' index.  An item is kept
 * when keep == NULL and it is matched in every round, or when keep[index] != 0; n_keep must equal
 * the number of bins (dmx_counts' length less its two trailing entries).  The operand is the
 * final trimmed, oriented record the fused loop writes for the item: rc1, m1's trim, rc2 and m2's
 * trim composed ([rstop:] for a 5' adapter, [:rstart] for a 3' adapter; a round without a match
 * keeps its whole input in the orientation it was taken), on the read as given.  Items whose
 * final length is below min_len (>= 1) are dropped.  Operands are ordered by bin and, inside a
 * bin, by item.  bin_first[b] is the first operand of bin b; it has one more entry than there are
 * bins (n_first is checked), the last being the table's length, which *n_operands (optional)
 * receives too.  Only bin_first leaves the device; dmx_operands_fetch brings the table down. */
int dmx_result_operands(dmx_ctx* ctx, const uint8_t* keep, size_t n_keep, int32_t min_len,
                        uint64_t* bin_first, size_t n_first, uint64_t* n_operands);
/* Host only (no GPU; tests): the same table in plain sequential C++ from dmx_fetch's results
 * (n_items of them), round 0's item list in dmx_set_views' convention (v_read == NULL: item k is
 * read k), the batch's read lengths, the mode and both panels' adapter types (wheres as
 * dmx_set_panel_ex takes them; wheres1 / n1 are not read in DMX_MODE_SINGLE).  First `cap`
 * operands written (any of read, start, stop, strand may be NULL).  Errors:
 * dmx_last_error(NULL). */
int dmx_result_operands_host(const dmx_result* res, size_t n_items, const uint32_t* v_read,
                             const int32_t* v_start, const int32_t* v_stop,
                             const uint8_t* v_strand, const uint32_t* lens, size_t n_reads,
                             int mode, const int* wheres0, int n0, const int* wheres1, int n1,
                             const uint8_t* keep, size_t n_keep, int32_t min_len, uint32_t* read,
                             int32_t* start, int32_t* stop, uint8_t* strand, size_t cap,
                             uint64_t* bin_first, size_t n_first, uint64_t* n_operands);

/* ---- Pairwise read distance: the amplicon-sorting stage's similarity pass --------------------
 * Replaces: the edlib.align(A1, A2, task='distance', mode=...) calls of
 * scripts/auxiliary_code/amplicon_sorter.py: distance() (:225-235) as similarity() (:777-808)
 * calls it for every pair process_list() makes (mode 'NW', repeated on the reverse complement
 * when the forward identity is below 0.5), and the 'HW' comparisons of finetune() (:840-852).
 * edlib is not vendored; edit distance has one right answer, so parity is pinned by a
 * full-matrix DP (dmx_pairdist_host).  The best-hit filter and the gene groups that read these
 * identities are dmx_pairhits / dmx_hitgroups, the alignments of consensus building
 * dmx_groupalign's, both below.
 * Runs on the batch made resident by dmx_load.  Symbols: A, C, G, T and the no-match mask as a
 * fifth symbol (edlib compares bytes, so N equals N and nothing else).
 * DMX_PD_NW: Levenshtein distance of the two whole reads.  DMX_PD_HW: the least edit distance
 * between the query and any substring of the target, the empty one included (edlib's infix
 * mode).  Pair flag DMX_PD_RC: the target is taken reverse-complemented (read backwards in
 * place, masked positions stay masked).  Reads of 1..DMX_PD_MAX_LEN nt (DMX_E_UNSUPPORTED
 * otherwise); a pair index >= the batch's reads, an unknown flag or mode is DMX_E_INVALID.
 * Everything is checked on the host before anything is launched.  Pairs may repeat and come in
 * any order.  Lists above DMX_PD_CHUNK pairs (environment, default 2^20) run as several
 * launches with bounded device memory (same results). */
#define DMX_PD_NW 0
#define DMX_PD_HW 1
#define DMX_PD_RC 0x1            /* pair flag: target reverse-complemented */
#define DMX_PD_MAX_LEN 16384
/* Edit distance of read q[i] (query) against read t[i] (target) of the resident batch.
 * flags, caps may be NULL (0 / no cap).  out[i] = min(d, caps[i] + 1).  Synchronous. */
int dmx_pairdist(dmx_ctx* ctx, int mode, const uint32_t* q, const uint32_t* t,
                 const uint8_t* flags, const uint32_t* caps, size_t n_pairs, uint32_t* out);
/* Host only (no GPU; tests, CPU baseline): the same contract on a dmx_pack layout, by a plain
 * full-matrix DP (a different algorithm from the kernel's on purpose).  Errors: the message is
 * dmx_last_error(NULL). */
int dmx_pairdist_host(int mode, const uint32_t* seq2b, const uint32_t* nmask,
                      const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
                      const uint32_t* q, const uint32_t* t, const uint8_t* flags,
                      const uint32_t* caps, size_t n_pairs, uint32_t* out, int n_threads);
float dmx_pairdist_ms(dmx_ctx* ctx);  /* device time of the last dmx_pairdist (HIP events) */
/* Host only: the lane-group sizes G the kernel cuts a wave into (first `cap` written, ascending;
 * returns their number).  A query of w = ceil(len / 64) words runs in the smallest G >= w, one
 * word per lane; above 64 words it runs in stripes of 64 G rows with G = 64. */
int dmx_pairdist_group_sizes(int* out, int cap);

/* ---- Global alignment with the edit path ----------------------------------------
 * The GPU counterpart of edlib.align(q, t, mode='NW', task='path'), which create_alignment()
 * of amplicon_sorter.py (:333-339) runs for every read of every group it builds a consensus
 * of.  This entry point aligns resident reads against resident reads; the loop itself, whose
 * alignments are sequential within a group and whose targets carry gaps, is dmx_groupalign
 * below.  Alphabet, equality, DMX_PD_RC, the length limits and the argument checks are
 * dmx_pairdist's; additionalEqualities is not supported here (dmx_groupalign's masks carry it).
 * The query is the rows, the target the columns (edlib's orientation); ops carry edlib's
 * numbering.  An INSERT is a step up (a gap in the target), a DELETE a step left (a gap in
 * the query).  The distance has one right answer, a path has not, so the tie rule is part of
 * the contract: walking back from (m, n), at (i, j) with i, j > 0
 *   1. D(i-1, j) + 1 == D(i, j): INSERT;  2. else D(i, j-1) + 1 == D(i, j): DELETE;
 *   3. else the diagonal, MATCH on equal symbols and MISMATCH otherwise;
 * on row 0 only DELETE, on column 0 only INSERT.  Ops are reported in forward order.  Whether
 * edlib breaks ties the same way is not pinned (edlib is not vendored); the host version below
 * applies the rule literally on a full matrix and the kernel equals it op for op. */
#define DMX_PA_MATCH 0           /* consumes query and target */
#define DMX_PA_INSERT 1          /* consumes query only */
#define DMX_PA_DELETE 2          /* consumes target only */
#define DMX_PA_MISMATCH 3        /* consumes query and target */
/* dist[i] and the path of read q[i] against read t[i] of the resident batch: pair i's ops are
 * ops[op_off[i] .. op_off[i + 1]) (op_off has n_pairs + 1 entries).  ops_cap must be at least
 * the sum over the pairs of both reads' lengths (DMX_E_INVALID otherwise).  flags may be NULL.
 * The forward pass keeps a trace of about 18 bytes per (64-row word, column); the pair list
 * runs in as many launches as keep one launch's trace under DMX_PA_TRACE_MB MiB (environment,
 * default 1024; one pair at least per launch), with the same results.  Synchronous. */
int dmx_pairalign(dmx_ctx* ctx, const uint32_t* q, const uint32_t* t, const uint8_t* flags,
                  size_t n_pairs, uint32_t* dist, uint64_t* op_off, uint8_t* ops, size_t ops_cap);
/* Host only (no GPU; tests, CPU baseline): the same contract on a dmx_pack layout, by a plain
 * full-matrix DP and the tie rule applied literally (2 bytes per cell and thread).  Errors: the
 * message is dmx_last_error(NULL). */
int dmx_pairalign_host(const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
                       const uint32_t* lens, size_t n_reads, const uint32_t* q, const uint32_t* t,
                       const uint8_t* flags, size_t n_pairs, uint32_t* dist, uint64_t* op_off,
                       uint8_t* ops, size_t ops_cap, int n_threads);
float dmx_pairalign_ms(dmx_ctx* ctx);  /* device time of both kernels, last dmx_pairalign */
/* ms[0] = the forward pass, ms[1] = the traceback of the last dmx_pairalign (first n_ms
 * written); returns the number of launches the pair list was cut into. */
int dmx_pairalign_stats(dmx_ctx* ctx, float* ms, int n_ms);

/* ---- Progressive alignment of read groups ---------------------------------------
 * The loop of create_alignment() (amplicon_sorter.py:324-356) as create_consensus() (:358-441)
 * runs it: row 0 of a group is a consensus, member k is aligned (NW, path, the tie rule above)
 * against row 0 as it stands, and every column the member inserts becomes a '-' column of row 0
 * and of every earlier row.  The caller only ever reads per-column symbol counts (:372-384), so
 * no rows are kept: per column of the final row 0, the result is its mask, how many members
 * showed each symbol there, and which member did first.
 * A row is one mask byte per column: bit c (0..4 = A, C, G, T, masked/N) is set iff the column
 * equals query symbol c; bits 5..7 must be 0.  '-' is 0 (it equals nothing, and stepping over
 * it costs 1 like any edit), A/C/G/T/N are single bits, and the additionalEqualities of
 * :334-339 are R = A|G, Y = C|T, M = A|C, K = G|T, S = G|C, W = A|T.
 * Group g: its seed row is seed_masks[seed_off[g] .. seed_off[g + 1]), its members the resident
 * reads members[member_off[g] .. member_off[g + 1]) in alignment order (a read may be a member
 * of several groups; a group may have none, its seed row then comes back with zero counts).
 * max_cols caps any row's length (0 = DMX_PD_MAX_LEN).  Out, per group g, columns
 * col_off[g] .. col_off[g + 1) of the final row: mask[col], count[5 col + c] (members showing
 * symbol c; row 0's own symbol is not counted) and first[5 col + c] (the 1-based place in the
 * group of the first member that showed c, 0 = none).  cols_cap (entries of mask; count and
 * first hold 5 per column) must be at least the sum over the groups of
 * min(max_cols, seed length + member lengths).  dist[member_off[g] + k - member_off[0]] is the
 * distance of member k's alignment.  ops may be NULL; otherwise member x's path against the
 * row it met is ops[op_off[x] .. op_off[x + 1]) in member order, and ops_cap must be at least
 * the sum over the members of the bound of the row they leave behind (DMX_E_INVALID otherwise).
 * Runs in lock-step rounds: round k aligns member k of every group that has one (forward pass,
 * traceback, merge into the group's next row), as many launches per round as keep the trace
 * under DMX_PA_TRACE_MB; the results do not depend on the split.  Everything is checked on the
 * host before anything is launched, naming the group: DMX_E_INVALID for a null argument, a
 * member outside the batch, a mask byte with bits 5..7 set or too small an output;
 * DMX_E_UNSUPPORTED for a member of 0 or more than DMX_PD_MAX_LEN nt, a seed outside
 * 1..max_cols columns, max_cols above DMX_PD_MAX_LEN, more than 65535 members, and, during
 * the run, a row that would grow past max_cols (naming group and round; the outputs are then
 * undefined and the context stays usable).  Synchronous. */
int dmx_groupalign(dmx_ctx* ctx, size_t n_groups, const uint8_t* seed_masks,
                   const uint64_t* seed_off, const uint32_t* members, const uint64_t* member_off,
                   uint32_t max_cols, uint64_t* col_off, uint8_t* mask, uint16_t* count,
                   uint16_t* first, size_t cols_cap, uint32_t* dist, uint64_t* op_off,
                   uint8_t* ops, size_t ops_cap);
/* Host only (no GPU; tests, CPU baseline): the same contract on a dmx_pack layout, group after
 * group and member after member: a full-matrix DP with the equality (mask[j] >> symbol) & 1,
 * the tie rule applied literally, the merge in plain loops.  Errors: dmx_last_error(NULL). */
int dmx_groupalign_host(const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
                        const uint32_t* lens, size_t n_reads, size_t n_groups,
                        const uint8_t* seed_masks, const uint64_t* seed_off,
                        const uint32_t* members, const uint64_t* member_off, uint32_t max_cols,
                        uint64_t* col_off, uint8_t* mask, uint16_t* count, uint16_t* first,
                        size_t cols_cap, uint32_t* dist, uint64_t* op_off, uint8_t* ops,
                        size_t ops_cap, int n_threads);
/* dmx_groupalign with a strand per member (consensus_direction's outcome, :1826-1838, applied in
 * place): member_flags is parallel to members; bit DMX_PD_RC takes the member
 * reverse-complemented (read backwards, codes complemented, masked positions stay masked: what
 * DMX_PD_RC means for dmx_pairdist's target).  dist, ops, count and first are then those of the
 * reverse-complemented read against the row; everything else (tie rule, rounds, the
 * DMX_PA_TRACE_MB split, max_cols, the refusals) is dmx_groupalign's.  Any other bit is
 * DMX_E_INVALID, naming group and member, checked on the host before anything is launched.
 * member_flags == NULL is dmx_groupalign itself (the two entry points above are these with
 * NULL). */
int dmx_groupalign_strands(dmx_ctx* ctx, size_t n_groups, const uint8_t* seed_masks,
                           const uint64_t* seed_off, const uint32_t* members,
                           const uint8_t* member_flags, const uint64_t* member_off,
                           uint32_t max_cols, uint64_t* col_off, uint8_t* mask, uint16_t* count,
                           uint16_t* first, size_t cols_cap, uint32_t* dist, uint64_t* op_off,
                           uint8_t* ops, size_t ops_cap);
int dmx_groupalign_strands_host(const uint32_t* seq2b, const uint32_t* nmask,
                                const uint64_t* offsets, const uint32_t* lens, size_t n_reads,
                                size_t n_groups, const uint8_t* seed_masks,
                                const uint64_t* seed_off, const uint32_t* members,
                                const uint8_t* member_flags, const uint64_t* member_off,
                                uint32_t max_cols, uint64_t* col_off, uint8_t* mask,
                                uint16_t* count, uint16_t* first, size_t cols_cap, uint32_t* dist,
                                uint64_t* op_off, uint8_t* ops, size_t ops_cap, int n_threads);
/* ms[0] = the forward passes, ms[1] = the tracebacks, ms[2] = the merges of the last
 * dmx_groupalign (first n_ms written); *rounds (may be NULL) = its lock-step rounds; returns
 * the number of launches of each kernel. */
int dmx_groupalign_stats(dmx_ctx* ctx, float* ms, int n_ms, int* rounds);

/* ---- Read distance against rows of masks ----------------------------------------
 * The comparisons of process_consensuslist() / similarity_species() (amplicon_sorter.py
 * :1628-1716): every read not yet in a group against the consensus of every group, which
 * rest_reads() (:1962-2023) repeats pass after pass.  A consensus is not a read of the resident
 * batch, so the targets are given per call, as rows of dmx_groupalign's masks: row g is
 * masks[row_off[g] .. row_off[g + 1]) (row_off has n_rows + 1 entries), one byte per column,
 * bit c (0..4 = A, C, G, T, masked/N) set iff the column equals query symbol c, 0 = a gap column
 * that equals nothing, bits 5..7 must be 0.
 * out[i] = the NW (whole read, whole row) edit distance of resident read q[i] against row r[i],
 * min(d, caps[i] + 1) when caps is given (caps may be NULL).  There is no HW mode and no
 * DMX_PD_RC here: a reversed target is a second row that the caller builds.  Pairs may repeat
 * and come in any order; a row may serve any number of pairs.  The rows are uploaded with the
 * call; lists above DMX_PD_CHUNK pairs run as several launches, as dmx_pairdist's do.
 * Everything is checked on the host before anything is launched, naming the pair or the row:
 * DMX_E_INVALID for a null pointer with n_pairs > 0, a read index outside the batch, a row
 * index outside n_rows, decreasing offsets or a mask byte with bits 5..7 set;
 * DMX_E_UNSUPPORTED for a read or a row of 0 or more than DMX_PD_MAX_LEN entries.  A refused
 * call launches nothing and leaves the context usable.  Synchronous. */
int dmx_rowdist(dmx_ctx* ctx, size_t n_rows, const uint8_t* masks, const uint64_t* row_off,
                const uint32_t* q, const uint32_t* r, const uint32_t* caps, size_t n_pairs,
                uint32_t* out);
/* Host only (no GPU; tests, CPU baseline): the same contract on a dmx_pack layout, by a plain
 * full-matrix DP with the equality (mask[j] >> symbol) & 1 (dmx_groupalign_host's; a different
 * algorithm from the kernel's on purpose).  Errors: dmx_last_error(NULL). */
int dmx_rowdist_host(const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
                     const uint32_t* lens, size_t n_reads, size_t n_rows, const uint8_t* masks,
                     const uint64_t* row_off, const uint32_t* q, const uint32_t* r,
                     const uint32_t* caps, size_t n_pairs, uint32_t* out, int n_threads);
float dmx_rowdist_ms(dmx_ctx* ctx);  /* device time of the last dmx_rowdist (HIP events) */

/* ---- Reads assigned to rows of masks: the best row per read ---------------------
 * One pass of process_consensuslist() / similarity_species() and the best-hit filter of
 * update_groups() (amplicon_sorter.py:1628-1755) with the pair generation, the decision and the
 * reduction inside the call: one record per read leaves it, not a distance per pair.
 * Rows: dmx_rowdist's (n_rows, masks, row_off; the same equality; bits 5..7 refused).
 * Reads: reads[0 .. n_sel), resident read indices in the caller's order.  A read may be named
 * twice; each place k is an entry of its own.
 * Tables indexed by the longer length L = max(length of the read, length of the row), n_len
 * entries each: cap_hit[L], cap_half[L] (-1 = none; below -1 is refused) and bin_off[L]; the
 * identity class of distance d at length L is bins[bin_off[L] + d] (n_bins entries), as
 * dmx_hithist takes them.
 * Pairs: for k ascending and row g ascending, pair (k, g) is compared unless
 * (double)la * 1.05 < (double)lb || (double)lb * 1.05 < (double)la, with la the read's and lb
 * the row's length (:1664; the same IEEE products as Python's).  After the last row of place k,
 * if floor(pairs so far / chunk) == max_chunks, no later place is compared (:1669-1676).  The
 * test is for equality: a place that takes the quotient past max_chunks does not stop anything,
 * as in the reference.
 * Per pair: df = the NW distance of the read against the row, capped at
 * max(cap_hit[L], cap_half[L], 0).  df <= cap_hit[L] is a forward line with d = df.  Otherwise,
 * when cap_hit[L] >= 0 and df > cap_half[L], dr = the distance against the row's reverse
 * complement (the row backwards, bits A <-> T and C <-> G swapped, N and gap columns fixed:
 * dmx_rowpairdist's definition), capped at cap_hit[L]; dr <= cap_hit[L] is a reverse line with
 * d = dr.  Otherwise the pair has no line.
 * Best per place: among the lines of place k the one with the largest (class, g): the largest
 * identity class, and among equal classes the largest row index (update_groups' "the last of
 * equal identities wins", in pair-generation order).
 * Out: best_row[k] (DMX_LG_NONE where place k has no line; best_d and best_class are then
 * DMX_LG_NONE and 0), best_d[k] (d, or d | DMX_LG_REV), best_class[k]; *n_pairs = the pairs
 * compared (the reference's "comparisons to calculate"), *n_lines = the lines.
 * Everything is checked on the host before anything is launched, naming the place, row or
 * length: DMX_E_INVALID for a null argument, chunk == 0, a read outside the batch, decreasing
 * offsets, a mask byte with bits 5..7 set, a cap below -1, L >= n_len for a pair that occurs,
 * bin_off[L] + max(cap_hit[L], 0) >= n_bins for a length that occurs; DMX_E_UNSUPPORTED for a
 * compared read or row of 0 or more than DMX_PD_MAX_LEN entries, more than 2^31 rows (the key
 * below holds 31 bits of row) and more than DMX_LG_MAX_PAIRS pairs.  A refused call launches
 * nothing, leaves the outputs untouched, dmx_rowassign_ms at 0 and the context usable.
 * n_sel == 0 or n_rows == 0 is a valid call that launches nothing (*n_pairs = *n_lines = 0).
 * Device: the rows are uploaded once per call and their reverse complements written beside them
 * on the device when some pair asks for one; the distances are dmx_rowdist's launches (chunks of
 * DMX_PD_CHUNK pairs) and stay on the device; per chunk a decision kernel does one 64-bit
 * atomicMax per line on the place's key (class, g, reverse bit, d) and only a bitmap of the pairs
 * to retry comes back; the retries run as launches of their own.  The result depends neither on
 * the order the atomics land in nor on DMX_PD_CHUNK.  The call leaves the resident batch and the
 * outcomes of dmx_pairhits as they are.  Synchronous. */
int dmx_rowassign(dmx_ctx* ctx, size_t n_rows, const uint8_t* masks, const uint64_t* row_off,
                  const uint32_t* reads, size_t n_sel, const int32_t* cap_hit,
                  const int32_t* cap_half, const uint32_t* bin_off, size_t n_len,
                  const uint16_t* bins, size_t n_bins, uint64_t chunk, uint64_t max_chunks,
                  uint32_t* best_row, uint32_t* best_d, uint16_t* best_class, uint64_t* n_pairs,
                  uint64_t* n_lines);
/* Host only (no GPU; tests, ctx=None of dmx.sorter.assign_best): the same contract on a dmx_pack
 * layout, on dmx_rowdist_host (full-matrix DP, n_threads) with the decision and the reduction in
 * plain sequential C++.  Errors: dmx_last_error(NULL). */
int dmx_rowassign_host(const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
                       const uint32_t* lens, size_t n_reads, size_t n_rows, const uint8_t* masks,
                       const uint64_t* row_off, const uint32_t* reads, size_t n_sel,
                       const int32_t* cap_hit, const int32_t* cap_half, const uint32_t* bin_off,
                       size_t n_len, const uint16_t* bins, size_t n_bins, uint64_t chunk,
                       uint64_t max_chunks, uint32_t* best_row, uint32_t* best_d,
                       uint16_t* best_class, uint64_t* n_pairs, uint64_t* n_lines, int n_threads);
float dmx_rowassign_ms(dmx_ctx* ctx);  /* device time of the last dmx_rowassign (HIP events) */

/* ---- Gene groups: best-hit links and their connected components -----------------
 * Replaces: what update_list() of amplicon_sorter.py does with the similarity lines (:983-1034:
 * per longer read j the lines of the largest identity, ties kept; then greedy groups) and
 * merge_groups() (:1058-1087: merged until nothing moves).  Every kept line i:j is an edge
 * {i, j}, and the groups are the connected components of the edges.  Only a label per read
 * leaves the device.  The species groups (SSG / Estimate, read_indexes) are the section after
 * this one.  Not replaced: the random sampling of comp_consensus_groups (:1206) onward, finetune,
 * and the .group and results files. */
#define DMX_LG_NONE 0xFFFFFFFFu  /* a node on no edge; a read with no hit; a pair with no outcome */
#define DMX_LG_REV 0x80000000u   /* an outcome's reverse bit (the host twins' outcome words)      */
#define DMX_LG_MAX_PAIRS 0x7FFFFFFFu /* pairs per dmx_pairhits, edges per dmx_edgegroups: places
                                      * and counts are 32-bit on the device */
/* Connected components of the undirected edges {a[e], b[e]} over nodes 0 .. n_nodes - 1:
 * labels[v] = the smallest node of v's component, DMX_LG_NONE for a node on no edge (a node
 * with only a self-loop is its own component).  Self-loops and repeated edges are allowed.  An
 * endpoint >= n_nodes is DMX_E_INVALID (checked on the host before anything is launched), more
 * than DMX_LG_MAX_PAIRS edges DMX_E_UNSUPPORTED.  Needs no resident batch.  Hooking by atomicMin
 * on a parent array and pointer jumping, repeated until a round changes nothing; the result does
 * not depend on the order the atomics land in.  Synchronous. */
int dmx_edgegroups(dmx_ctx* ctx, const uint32_t* a, const uint32_t* b, size_t n_edges,
                   uint32_t n_nodes, uint32_t* labels);
/* Host only (no GPU; tests): the same contract by a sequential union-find.  Errors:
 * dmx_last_error(NULL). */
int dmx_edgegroups_host(const uint32_t* a, const uint32_t* b, size_t n_edges, uint32_t n_nodes,
                        uint32_t* labels);
/* The similarity pass over pairs of the resident batch with the hit decision on the device.
 * cap_hit[i] / cap_half[i]: the largest distance whose identity is still >= the hit threshold /
 * >= 0.5 for pair i's target length, -1 where there is none (a value below -1 is DMX_E_INVALID).
 * Per pair: the forward NW distance df, capped at max(cap_hit, cap_half, 0); df <= cap_hit is a
 * forward hit with d = df; otherwise, when cap_hit >= 0 and df > cap_half, the distance dr
 * against the reverse-complemented target (DMX_PD_RC), capped at cap_hit, and dr <= cap_hit is a
 * reverse hit with d = dr; otherwise the pair has no hit.  The outcomes stay on the device, in
 * the context, until the next dmx_load, dmx_run, dmx_pairhits or dmx_close.  best[r] (one entry
 * per read of the batch) = the least d over the hits whose target is r, DMX_LG_NONE where there
 * is none; *n_hits = the number of hits.  The distances are dmx_pairdist's launches (the same
 * kernel, chunks of DMX_PD_CHUNK pairs, same results whatever the chunk); per chunk only a
 * bitmap of the pairs to retry comes back, and the retries run as launches of their own.
 * Validation and the length limits are dmx_pairdist's; more than DMX_LG_MAX_PAIRS pairs is
 * DMX_E_UNSUPPORTED.  Device memory: 20 bytes per pair beside dmx_pairdist's.  Synchronous. */
int dmx_pairhits(dmx_ctx* ctx, const uint32_t* q, const uint32_t* t, const int32_t* cap_hit,
                 const int32_t* cap_half, size_t n_pairs, uint32_t* best, uint64_t* n_hits);
/* The hits of the last dmx_pairhits in ascending place in its pair list, compacted on the device
 * (flag, prefix sum, scatter): pair[k] the place, d[k] the distance, rev[k] 1 for a reverse hit.
 * *n = the number of hits, always; with cap below it nothing is written and the call is
 * DMX_E_INVALID, as it is without valid dmx_pairhits outcomes. */
int dmx_pairhits_fetch(dmx_ctx* ctx, uint32_t* pair, uint32_t* d, uint8_t* rev, size_t cap,
                       size_t* n);
/* The groups: the edges are the hits {q, t} of the last dmx_pairhits with d <= tie[t] (tie has
 * one entry per read of the batch: the largest distance that still rounds to the identity of
 * best[t], which the caller computes with the reference's own rounding; entries of reads
 * without a hit are not read).  They are filtered by the compaction above and fed to
 * dmx_edgegroups' kernels without leaving the device; labels as dmx_edgegroups', one per read.
 * DMX_E_INVALID without valid dmx_pairhits outcomes. */
int dmx_hitgroups(dmx_ctx* ctx, const uint32_t* tie, uint32_t* labels);
/* Host only (no GPU; tests, ctx=None of dmx.sorter.gene_groups): dmx_pairhits on a dmx_pack
 * layout, on dmx_pairdist_host; the state is the caller's: outcome[i] = d, d | DMX_LG_REV or
 * DMX_LG_NONE for pair i.  Errors: dmx_last_error(NULL). */
int dmx_pairhits_host(const uint32_t* seq2b, const uint32_t* nmask, const uint64_t* offsets,
                      const uint32_t* lens, size_t n_reads, const uint32_t* q, const uint32_t* t,
                      const int32_t* cap_hit, const int32_t* cap_half, size_t n_pairs,
                      uint32_t* outcome, uint32_t* best, uint64_t* n_hits, int n_threads);
/* Host only: dmx_hitgroups on the outcomes of dmx_pairhits_host and its pair list, by the
 * sequential union-find. */
int dmx_hitgroups_host(const uint32_t* q, const uint32_t* t, const uint32_t* outcome,
                       size_t n_pairs, const uint32_t* tie, size_t n_reads, uint32_t* labels);
/* Device time (ms, HIP events; first n_ms written): ms[0] the distance launches of the last
 * dmx_pairhits, ms[1] the last compaction (dmx_pairhits_fetch, dmx_hitgroups), ms[2] the last
 * components run (dmx_edgegroups, dmx_hitgroups; first kernel to last, the flag's trips to the
 * host between the rounds included), ms[3] the last dmx_hithist.  Returns that run's hooking
 * rounds. */
int dmx_hitgroups_stats(dmx_ctx* ctx, float* ms, int n_ms);

/* ---- Species groups: identity histogram, cross hits, per-group components ------
 * Replaces: SSG() of amplicon_sorter.py (:810-836, the histogram of all similarity lines behind
 * the estimated species threshold) and the first half of read_indexes() (:1363-1411: per gene
 * group the lines at that threshold with a read in the group, the best per longer read, greedy
 * groups, merge_groups).  All three work on the outcomes of the last dmx_pairhits and leave
 * them, best[] and dmx_pairhits_fetch as they are; all are DMX_E_INVALID without valid outcomes.
 * Not replaced: finetune, the random sampling, the .group and results files.
 *
 * dmx_hithist: for every hit (forward or reverse) with distance d and target t,
 * hist[bins[bin_off[t] + d]] += 1: the caller's table maps a distance to a class (the sorter:
 * thousandths of identity by the reference's own rounding, a row per distinct target length).
 * bin_off has one entry per resident read, bins n_bins entries, hist n_classes <= 1024 counters
 * that the call adds to.  A target outside the reads, bin_off[t] + d >= n_bins or a class >=
 * n_classes is detected on the device in every build and not followed: the call is
 * DMX_E_INVALID naming the kind, and hist is left untouched.  A block counts in LDS and adds its
 * counters to the global ones once. */
int dmx_hithist(dmx_ctx* ctx, const uint32_t* bin_off, const uint16_t* bins, size_t n_bins,
                uint32_t n_classes, uint64_t* hist);
/* label[r] (one per resident read) = the read's gene group, or DMX_LG_NONE; cap2[r] = the largest
 * distance whose identity is still >= the species threshold at r's length, -1 for none.
 * The cross hits: the hits with cap2[t] >= 0, d <= cap2[t] and label[q] != label[t] (so at least
 * one of the two is in a group), in ascending place, by dmx_pairhits_fetch's compaction with
 * this predicate.  pair, d, rev, cap and *n as dmx_pairhits_fetch's: *n is always the count; with
 * cap below it nothing is written and the call is DMX_E_INVALID. */
int dmx_pairhits_cross(dmx_ctx* ctx, const uint32_t* label, const int32_t* cap2, uint32_t* pair,
                       uint32_t* d, uint8_t* rev, size_t cap, size_t* n);
/* Components over n_nodes >= n_reads nodes (the resident reads first, then the caller's own).
 * Edges: the hits {q, t} with label[q] == label[t] != DMX_LG_NONE and d <= tie2[t], where
 * tie2[t] == DMX_LG_NONE means no edge for t; and the n_extra edges {xa[e], xb[e]}, which are
 * written behind the compacted hits, so that one components run sees both.  labels_out (n_nodes)
 * as dmx_edgegroups'.  An endpoint >= n_nodes or n_nodes < n_reads is DMX_E_INVALID before
 * anything is launched. */
int dmx_hitgroups_within(dmx_ctx* ctx, const uint32_t* tie2, const uint32_t* label,
                         const uint32_t* xa, const uint32_t* xb, size_t n_extra, uint32_t n_nodes,
                         uint32_t* labels_out);
/* Host only (no GPU; tests, ctx=None of dmx.sorter): the three on the state of dmx_pairhits_host
 * (its pair list and outcome words).  Errors: dmx_last_error(NULL). */
int dmx_hithist_host(const uint32_t* t, const uint32_t* outcome, size_t n_pairs, size_t n_reads,
                     const uint32_t* bin_off, const uint16_t* bins, size_t n_bins,
                     uint32_t n_classes, uint64_t* hist);
int dmx_pairhits_cross_host(const uint32_t* q, const uint32_t* t, const uint32_t* outcome,
                            size_t n_pairs, size_t n_reads, const uint32_t* label,
                            const int32_t* cap2, uint32_t* pair, uint32_t* d, uint8_t* rev,
                            size_t cap, size_t* n);
int dmx_hitgroups_within_host(const uint32_t* q, const uint32_t* t, const uint32_t* outcome,
                              size_t n_pairs, size_t n_reads, const uint32_t* tie2,
                              const uint32_t* label, const uint32_t* xa, const uint32_t* xb,
                              size_t n_extra, uint32_t n_nodes, uint32_t* labels_out);

/* ---- Rows of masks against rows of masks ----------------------------------------
 * The comparisons of iden_consensus() (amplicon_sorter.py:1140-1159) as the pair loops of
 * comp_consensus_groups (:1276-1296) and compare_consensus (:1869-1889) run them: every consensus
 * against every later one, edlib's HW mode, both strands.  Query and target are both rows of the
 * call, laid out as dmx_rowdist's (row g is masks[row_off[g] .. row_off[g + 1]), n_rows + 1
 * offsets, bits 5..7 refused); q[i] and t[i] are row indices.  Two columns are equal iff their
 * masks intersect: literal equality for A/C/G/T/N, a gap column (0) equals nothing on either
 * side, an IUPAC column equals each of its letters.
 * dmx_rowpairdist: out[i] = the distance of row q[i] (query, rows of the matrix) against row
 * t[i] (target, columns), mode DMX_PD_NW or DMX_PD_HW, against the target's reverse complement
 * (the row backwards, bits A <-> T and C <-> G swapped, N and gap columns fixed) where flags[i]
 * has DMX_PD_RC; min(d, caps[i] + 1) with caps.  flags and caps may be NULL.
 * dmx_rowhits: per pair df = the forward distance and dr = the distance against the reversed
 * target, both always computed; d = min(df, dr), rev = dr < df (ties are forward); a hit iff
 * cap[i] >= 0 and d <= cap[i] (cap[i] = -1: never a hit; below -1 is DMX_E_INVALID).  The
 * decision and the compaction (flag, prefix sum, scatter) run on the device and only the hits
 * come back, ascending in their place in the pair list: pair[k], d[k], rev[k].  *n_hits is always
 * set; with hits_cap below it nothing is written and the call is DMX_E_INVALID.
 * Neither call needs or disturbs a resident batch: they work on a context that never saw
 * dmx_load, and the outcomes of a previous dmx_load and dmx_pairhits stay valid.  Pairs may
 * repeat and come in any order.  The rows some pair names are uploaded once per call; lists
 * above DMX_PD_CHUNK pairs run as several launches with the same results.
 * Everything is checked on the host before anything is launched, naming the pair or the row:
 * DMX_E_INVALID for a null pointer with n_pairs > 0, a row index outside n_rows, decreasing
 * offsets, a mask byte with bits 5..7 set, an unknown mode or flag; DMX_E_UNSUPPORTED for a named
 * row of 0 or more than DMX_PD_MAX_LEN columns and for more than DMX_LG_MAX_PAIRS pairs.  A
 * refused call launches nothing, leaves dmx_rowhits_ms at 0 and the context usable.
 * Synchronous. */
int dmx_rowpairdist(dmx_ctx* ctx, int mode, size_t n_rows, const uint8_t* masks,
                    const uint64_t* row_off, const uint32_t* q, const uint32_t* t,
                    const uint8_t* flags, const uint32_t* caps, size_t n_pairs, uint32_t* out);
int dmx_rowhits(dmx_ctx* ctx, int mode, size_t n_rows, const uint8_t* masks,
                const uint64_t* row_off, const uint32_t* q, const uint32_t* t, const int32_t* cap,
                size_t n_pairs, uint32_t* pair, uint32_t* d, uint8_t* rev, size_t hits_cap,
                size_t* n_hits);
/* Host only (no GPU; tests, ctx=None of dmx.sorter.compare_consensuses): the same contracts by
 * a plain full-matrix DP with the intersect equality (HW: row 0 is free, the result is the
 * least of the last row); dmx_rowhits_host sits on dmx_rowpairdist_host.  Errors:
 * dmx_last_error(NULL). */
int dmx_rowpairdist_host(int mode, size_t n_rows, const uint8_t* masks, const uint64_t* row_off,
                         const uint32_t* q, const uint32_t* t, const uint8_t* flags,
                         const uint32_t* caps, size_t n_pairs, uint32_t* out, int n_threads);
int dmx_rowhits_host(int mode, size_t n_rows, const uint8_t* masks, const uint64_t* row_off,
                     const uint32_t* q, const uint32_t* t, const int32_t* cap, size_t n_pairs,
                     uint32_t* pair, uint32_t* d, uint8_t* rev, size_t hits_cap, size_t* n_hits,
                     int n_threads);
float dmx_rowhits_ms(dmx_ctx* ctx);  /* device time of the last dmx_rowpairdist or dmx_rowhits */

#ifdef __cplusplus
}
#endif
#endif /* DMX_H */
