/*
 * groot_hip.h -- C ABI of libgroot_hip.so: the MI355X (gfx950) device path of `groot align`.
 *
 * The reference has no FFI seam; the drop-in boundary is the body of
 *     func (b *theBoss) mapReads() error                      src/pipeline/boss.go:108-242
 * i.e. everything between "reads arrive on a channel" and "sam.Records + weighted graphs":
 *     Sequence.RunMinHash          src/seqio/seqio.go:40-68  (+ src/minhash/khf.go:35-55, nthash)
 *     ContainmentIndex.Query       src/lshe/lshe.go:153-175  (+ lshensemble Query/Containment)
 *     graphMinion loop             src/pipeline/graphminion.go:46-102
 *     GrootGraph.IncrementSubPath  src/graph/graph.go:401-451   (as exact integer call counts)
 *     GrootGraph.AlignRead         src/graph/alignment.go:13-317
 * The reference streams reads continuously through that loop (boss.go:145-203).  Here a host drains its read channel
 * into batches and keeps SEVERAL of them in flight in one ctx: groot_hip_submit* enqueues a batch (copy to pinned
 * staging -> H2D -> kernels -> D2H, each on its own HIP stream), groot_hip_collect blocks for the OLDEST batch and
 * hands back its traversal records, which the host turns into sam.Records (it keeps ID/Seq/Qual).  After the last batch
 * the host pulls the IncrementSubPath call counts (summed over GPUs by groot_hip_attempts_allreduce when there are
 * several) and replays the float formula (groot_host_weights_rows).  cgo/ has the Go binding, INTEGRATION.md the patch.
 *
 * Plain C: pointers and sizes only.  One ctx per GPU; a ctx is used from one host thread at a time, different ctxs
 * may be used concurrently.  No call retains a caller pointer after it returns (cgo rule), except buffers the ctx itself
 * handed out (groot_hip_acquire) and the caller-owned table of groot_hip_attempts_layout.  Every call returns 0 or a
 * negative GROOT_E_* (include/groot_host.h); groot_hip_last_error(ctx) has the text.  There is no CPU fallback: without
 * a usable HIP device groot_hip_open fails with GROOT_E_DEVICE.
 */
#ifndef GROOT_HIP_H
#define GROOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "groot_host.h"
#include "groot_index.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct groot_ctx groot_ctx;

typedef struct groot_params {
    double   containment_threshold; /* -t / --contThresh (cmd/align.go:47), default 0.99            */
    uint32_t no_exact_align;        /* --noAlign (cmd/align.go:46)                                   */
    uint32_t max_read_len;          /* longest read accepted (sizes LDS staging + DFS stacks); 0=256 */
    uint32_t max_batch_reads;       /* capacity of one submit; 0 = 1<<20                             */
    uint32_t max_seeds_per_read;    /* initial per-read seed slots (grown automatically); 0 = 8      */
    uint64_t max_batch_bases;       /* 0 = max_batch_reads * max_read_len                            */
    uint32_t keep_sketches;         /* 1: keep every read's KHF sketch on the device (tests)         */
    uint32_t pipeline_depth;        /* batches that may be in flight (submitted, not yet released); 0 = 3 */
    uint32_t results_on_device;     /* 1: traversal records stay in HBM (groot_batch_result.d_*), no D2H unless
                                       groot_hip_read_travs asks; 0 (default): D2H into pinned host memory, overlapped
                                       with the next batch's kernels                                 */
    uint32_t memo_budget_mb;        /* the memo of groot_hip_open (every WindowSize-mer of every indexed path run through the ctx's
                                       own pipeline once; reads that equal one are answered from it): 0 = default budget
                                       (GROOT_MEMO_DEFAULT_MB of HBM, and about as much host memory while it is built),
                                       GROOT_MEMO_OFF = no memo, else the budget in MiB.  An index whose strings need more than
                                       the budget is opened without the memo (groot_open_stats.memo_strings == 0); a caller
                                       with little input should switch it off: it costs ~0.3 s per GB of path bases at open
                                       and pays for itself only after some hundred million reads       */
} groot_params;
#define GROOT_MEMO_OFF 0xFFFFFFFFu
#define GROOT_MEMO_DEFAULT_MB 8192u

void groot_params_default(groot_params *p);

/* one seed = one lshe.Key returned by ContainmentIndex.Query for a read (lshe.go:165-171) */
typedef struct groot_seed {
    uint32_t read_id;   /* first_read_id + position in the batch */
    uint32_t window_id; /* window index in the groot_index_view  */
} groot_seed;

/* groot_trav (one traversal + its path set) is declared in groot_host.h: the host expands it to records */

typedef struct groot_counts {
    uint64_t received;       /* theBoss.receivedReadCount */
    uint64_t mapped;         /* theBoss.mappedCount       */
    uint64_t multimapped;    /* theBoss.multimappedCount  */
    uint64_t alignments;     /* theBoss.alignmentCount (= number of sam.Records)                     */
    uint64_t seeds;          /* total lshe.Keys returned by Query                                    */
    uint64_t travs;          /* groot_trav records of the batch                                      */
    uint64_t revcomp_panics; /* reads on which the reference panics in RevComplement (seqio.go:126)  */
    uint64_t short_reads;    /* reads shorter than k (reference panics, boss.go:164-166)             */
    uint64_t full_sketch_reads; /* reads whose seeds the full-width sketch kernel decided: all of them, or -- when the text
                                 * lookup / the signature kernel runs in front of it -- those it could not decide (diagnostic) */
    uint64_t walked_reads;      /* reads that went through the align stage's graph walk (the others: no seed window, or their
                                 * whole outcome came from the memo of groot_hip_open) (diagnostic) */
    uint64_t lean_reads;        /* ... of them, reads the align stage's first pass finished (one seed window, a walk that never
                                 * has two neighbours to choose from); the others took the state-machine kernel (diagnostic) */
} groot_counts;

/* per-stage device time of a batch, HIP events (ms); 0 if profiling off.
 * h2d = input copy on the copy-in stream; sketch_seed = the sketch+seed kernel alone; schedule = radix sort of the
 * processing order (or its stream compaction); align = the align kernel; sort = ordering of the traversal records into
 * (read, ord) order -- for reads answered from the outcome table this is where their records are written; total = first kernel .. last kernel; d2h = result copy on the copy-out stream */
typedef struct groot_stage_ms {
    float h2d, sketch_seed, align, sort, total, schedule, d2h, unpack;
    /* single kernels inside the stages above (for roofline figures): first_seed_kernel = the kernel that sees every read of the
     * batch first (text lookup / signature kernel / full-width kernel), inside sketch_seed; order_kernel = order_first_kernel,
     * inside sort */
    float first_seed_kernel, order_kernel;
    /* list_pass = what runs behind the first seed kernel inside sketch_seed: the full-width hashing kernel on the reads the first
     * kernel could not decide (LIST instance) + the wavefront-per-read LSH-Forest walk; 0 when the full-width kernel ran alone.
     * wall = first kernel of the batch .. last kernel of the batch on the wall clock of the device: the seed stage of the next
     * batch runs beside this batch's align stage, so wall < sketch_seed + schedule + align + sort of two neighbouring batches */
    float list_pass, wall;
    /* lean_pass = the first pass of the align stage (align_lean_kernel + the stream compaction of what it leaves), inside align; 0 when it did not run */
    float lean_pass;
} groot_stage_ms;

int groot_hip_device_count(int *n);
const char *groot_hip_last_error(const groot_ctx *ctx); /* ctx may be NULL: error of a failed open */

/* Uploads (replicates) the index into this GPU's HBM and builds the device lookup structures
 * (what ContainmentIndex.Load / BootstrapLshEnsembleEquiDepth do, lshe.go:95-147).  The view is checked first
 * (groot_index_view_check's pass): GROOT_E_FORMAT for one whose indices or offsets do not resolve. */
int groot_hip_open(groot_ctx **out, int device_id, const groot_index_view *idx, const groot_params *p);
/* The same with flags.  GROOT_OPEN_BACKGROUND: return as soon as the ctx can take batches (graphs, window arrays, exact and
 * LSH-Forest tables in HBM) and build the rest -- per-window prefix tables, the signature index: 0.6 of the 0.75 s an open without
 * memo takes on arg-annot.90 -- on a thread of the ctx while the first batches run through the full-width kernels; results are the
 * same whichever kernels a batch met.  The one exception to "no call retains a caller pointer": `idx` must stay valid until
 * groot_hip_open_wait (or groot_hip_close) has returned.  Ignored when the memo is wanted (it needs everything at once).
 * groot_hip_open_wait blocks until the background part is in place (0 at once if there is none); its failure is reported there
 * or by the next submit.  Replaces nothing in the reference: `groot align` rebuilds its LSH forests before the first read
 * (cmd/align.go:93-111). */
#define GROOT_OPEN_BACKGROUND 1u
int groot_hip_open_flags(groot_ctx **out, int device_id, const groot_index_view *idx, const groot_params *p, uint32_t flags);
int groot_hip_open_wait(groot_ctx *ctx);
/* Tell a background open to stop at its next checkpoint (a tenth of a second at most): for a caller whose input has ended before
 * the tables were there -- they would only be built to be freed (groot_hip_close asks the same before it joins the thread).  The ctx
 * keeps working, through the full-width kernels.  No-op without a background build in progress. */
int groot_hip_open_abandon(groot_ctx *ctx);
void groot_hip_close(groot_ctx *ctx);

/* What groot_hip_open built besides the uploaded index (diagnostic; times in ms, host wall clock).  The memo: every
 * WindowSize-mer of every indexed path went through the ctx's own pipeline once; reads that equal one of those strings are answered
 * from it (DESIGN.md "memo"). */
typedef struct groot_open_stats {
    double open_ms;            /* the whole of groot_hip_open                                            */
    double memo_ms;            /* of which: enumerating the strings, running the pipeline on them, tables */
    uint64_t memo_strings;     /* distinct path strings                                                  */
    uint64_t memo_tabulated;   /* of them with a stored outcome                                          */
    uint64_t memo_entries;     /* outcome-table entries (one per traversal, at least one per string)      */
    uint64_t text_entries;     /* strings in the text table (0: the text lookup is not used)              */
    uint64_t memo_hbm_bytes;   /* HBM held by outcome table + text table + sig_info                       */
} groot_open_stats;
int groot_hip_open_stats(const groot_ctx *ctx, groot_open_stats *out);

/* The SEED stage of every batch (decode, hashing, containment look-up, processing order) is enqueued on a caller-owned
 * hipStream_t (e.g. torch's current stream), so that it starts behind whatever the caller enqueued there (the kernels that
 * produced an IN_DEVICE batch); NULL = the ctx's own.  Only while nothing is in flight.
 * The align and order stages, and everything behind them, run on a stream PRIVATE to the ctx beside the next batch's seed
 * stage (boss.go:134-203: the reference's sketching and graph minions work side by side too).  Work the caller enqueues on
 * its stream after a submit is therefore NOT ordered behind the batch's results, and the inputs of groot_hip_submit_device
 * are still being read when the caller's stream has drained.  Three ways to order against a batch: groot_hip_wait /
 * groot_hip_collect (host side), or groot_hip_stream_join (device side, no host wait). */
int groot_hip_set_stream(groot_ctx *ctx, void *hip_stream);
/* Make `hip_stream` (NULL = the stream given to groot_hip_set_stream) wait -- on the device, the call returns at once --
 * until every batch submitted so far is through its kernels: records, path sets, counters and call counts of its FIRST PASS
 * are in place and that pass no longer reads the batch's inputs.  For callers that consume results_on_device buffers or
 * recycle groot_hip_submit_device inputs from kernels of their own.
 * The first pass is the only one unless a growable buffer of the ctx was too small for the batch (more seeds per read,
 * traversals, overflow records or kmerCount rows than it had room for): then groot_hip_wait / groot_hip_collect grow the
 * buffer on the HOST and run the batch again -- reading its inputs again, rewriting (possibly reallocating) its results.  A
 * consumer that is ordered by the join alone must therefore look at the batch's status word first (groot_hip_redo_status):
 * non-zero = this batch will be redone at collect, its device results are not final and its inputs are still needed. */
int groot_hip_stream_join(groot_ctx *ctx, void *hip_stream);
/* *d_status = device address of the newest submitted batch's status word (valid until that batch is released), *redo_mask = the bits of it
 * that mean "a buffer overflowed: collect will redo the batch".  A kernel (or a 4-byte copy) ordered behind groot_hip_stream_join reads
 * `*d_status & redo_mask`: zero = the results the join made visible are final.  GROOT_E_STATE when nothing has been submitted. */
int groot_hip_redo_status(groot_ctx *ctx, const uint32_t **d_status, uint32_t *redo_mask);
int groot_hip_set_profiling(groot_ctx *ctx, int enable);

/* ---- submitting batches ------------------------------------------------------------------------------------------
 * Every submit takes a free pipeline slot (GROOT_E_STATE "pipeline full" when pipeline_depth batches are submitted and
 * not yet released: collect + release first), copies the caller's buffers into the slot's pinned staging, enqueues
 * H2D -> kernels -> D2H on the ctx's three streams and returns at once.  Batches complete in submission order.
 * first_read_id only labels the records (groot_trav.read_id = first_read_id + position in the batch); a host that
 * streams more than 2^32 reads passes 0 and keeps its own 64-bit base.                                              */

/* read.Seq bytes back to back, seq_off[i]..seq_off[i+1] = read i (n_reads+1 entries). */
int groot_hip_submit(groot_ctx *ctx, const uint8_t *seq_concat, const uint64_t *seq_off, uint32_t n_reads,
                     uint32_t first_read_id);
/* Same batch, bases packed 2 bits each: base b of seq_concat sits in bits 2*(b%4).. of packed[b/4] as
 * (byte >> 1) & 3 (A=0 C=1 T=2 G=3); every byte that is not one of ACGT is listed in exc_pos (its index in
 * seq_concat) / exc_byte and may carry any code in `packed`.  A quarter of the PCIe traffic of groot_hip_submit for
 * the same result (the device unpacks to the byte layout first); groot_host_pack_reads builds the arguments. */
int groot_hip_submit_packed(groot_ctx *ctx, const uint8_t *packed, const uint64_t *seq_off, uint32_t n_reads,
                            uint32_t first_read_id, const uint64_t *exc_pos, const uint8_t *exc_byte, uint64_t n_exc);
/* The wire format proper: packed bases + one u16 LENGTH per read (the device scans them into offsets) + exceptions:
 * 27 bytes per 100 bp read over PCIe instead of 108. */
int groot_hip_submit_packed16(groot_ctx *ctx, const uint8_t *packed, const uint16_t *seq_len, uint32_t n_reads,
                              uint32_t first_read_id, const uint64_t *exc_pos, const uint8_t *exc_byte, uint64_t n_exc);
/* Zero-copy producer side of the same format: acquire hands out the pinned staging of a free slot, the caller (a FASTQ
 * parser) packs straight into it, submit_acquired enqueues it.  Capacities: packed (max_batch_bases+3)/4 bytes,
 * seq_len max_batch_reads entries, exceptions exc_cap entries (a batch with more goes through
 * groot_hip_submit_packed16, which grows the staging). */
typedef struct groot_batch_buffers {
    uint64_t ticket;       /* pass back to groot_hip_submit_acquired / groot_hip_release */
    uint8_t *packed;
    uint16_t *seq_len;
    uint64_t *exc_pos;
    uint8_t *exc_byte;
    uint64_t packed_cap, exc_cap;
    uint32_t reads_cap, reserved;
} groot_batch_buffers;
int groot_hip_acquire(groot_ctx *ctx, groot_batch_buffers *out);
int groot_hip_submit_acquired(groot_ctx *ctx, uint64_t ticket, uint32_t n_reads, uint64_t n_exc, uint32_t first_read_id);
/* Inputs already resident in HBM (no staging, no H2D).  d_seq must be 16-byte aligned and readable for 16 bytes past
 * the last base (the kernels load 16-byte / 8-byte words); max_len = longest read of the batch
 * (0 = params.max_read_len), taken as THE read length of the batch unless GROOT_MAXLEN_MIXED is set.  The buffers must stay valid until the batch is collected. */
#define GROOT_MAXLEN_MIXED 0x80000000u /* OR into max_len: the reads of the batch differ in length (scheduling hint only) */
int groot_hip_submit_device(groot_ctx *ctx, const void *d_seq, const void *d_seq_off, uint32_t n_reads,
                            uint32_t first_read_id, uint32_t max_len);

/* ---- collecting results -------------------------------------------------------------------------------------------
 * groot_hip_collect blocks until the OLDEST submitted batch is finished (its D2H included) and describes it; the
 * pointers stay valid until groot_hip_release(ticket), which frees the slot for another submit.  Several collected
 * batches may be held at once (e.g. while BAM writer threads work on them).  status = what the reference does with
 * the batch: GROOT_E_SHORT_READ / GROOT_E_REVCOMP where it panics (results remain readable), GROOT_E_NOSPACE for a
 * read longer than max_read_len; collect itself returns that status. */
typedef struct groot_batch_result {
    uint64_t ticket;
    uint32_t first_read_id, n_reads;
    groot_counts counts;
    const groot_trav *travs;   /* [n_travs] in (read, ord) order; pinned host memory (NULL with results_on_device) */
    /* Path sets, COMPACT: traversal i owns max(1, ceil(paths of graph travs[i].graph_id / 8)) consecutive BYTES (path p = bit
     * p % 8 of byte p / 8), traversal after traversal; mask_ckpt[j] = offset of the first byte of traversal 256*j.  (1 to 2
     * instead of 24 bytes per traversal over PCIe on arg-annot.90.)  groot_host_unpack_masks widens them to path_words words each. */
    const uint8_t *masks;
    const uint32_t *mask_ckpt;
    uint64_t n_mask_bytes;
    uint64_t n_travs;
    const void *d_travs;       /* in HBM: the records and their path sets at path_words words per traversal */
    const void *d_masks;
    uint32_t path_words;
    int32_t status;
    groot_stage_ms ms;
} groot_batch_result;
int groot_hip_collect(groot_ctx *ctx, groot_batch_result *out);
int groot_hip_release(groot_ctx *ctx, uint64_t ticket);
int groot_hip_in_flight(groot_ctx *ctx, uint32_t *submitted_not_collected, uint32_t *free_slots);

/* One-batch-at-a-time convenience over the same machinery (tests, simple hosts): wait = collect, the batch is released
 * by the next submit / wait; read_* copy out of it. */
int groot_hip_wait(groot_ctx *ctx, groot_counts *counts);
int groot_hip_read_travs(groot_ctx *ctx, groot_trav *out, uint64_t *masks /* [cap*path_words] */, uint64_t cap,
                         uint64_t *n);
/* seeds / sketches live in one of the ctx's two work sets (batches take them in turn): readable until the second batch
 * submitted after the waited one has started, i.e. always for the newest batch and the one before it (GROOT_E_STATE otherwise) */
int groot_hip_read_seeds(groot_ctx *ctx, groot_seed *out, uint64_t cap, uint64_t *n);
int groot_hip_read_sketches(groot_ctx *ctx, uint64_t *out /* [cap_reads*sketch_size] */, uint64_t cap_reads,
                            uint64_t *n_reads);
int groot_hip_stage_ms(groot_ctx *ctx, groot_stage_ms *out);
/* the waited batch's first pass against path text (align_path_kernel, the default first pass of the align stage): ran = 1 when it ran,
 * reads = the reads it finished (the rest of the walked reads went to align_kernel), ms = its time with the stream compaction behind
 * it (profiling on, else 0).  groot_counts.lean_reads stays 0 on this path. */
int groot_hip_path_pass_stats(groot_ctx *ctx, uint32_t *ran, uint64_t *reads, float *ms);

/* ---- IncrementSubPath call counts ---------------------------------------------------------------------------------
 * Accumulated over every batch since open/reset in a table [rows][n_windows] of uint32, one row per kmerCount
 * (len-k+1, graphminion.go:60) that occurred among seeded reads -- 1.3 MB per distinct read length on arg-annot.90,
 * not (max_read_len-k+2) rows.  Rows are created on the device as kmerCounts show up.                               */
/* rows in ascending kmerCount order: q_values[i] and counts[i*n_windows ..]; *n_rows = rows available, at most
 * cap_rows are written.  Waits for everything in flight. */
int groot_hip_attempts_export(groot_ctx *ctx, uint32_t *q_values, uint32_t *counts, uint32_t cap_rows, uint32_t *n_rows,
                              uint32_t *n_windows);
/* Fixes the row layout: row i holds kmerCount q_values[i] (strictly ascending; must include every kmerCount that has
 * counts).  d_table NULL: ctx-owned storage (still grows if a new kmerCount appears).  d_table != NULL: the table
 * lives in that caller-owned device buffer of n_q*n_windows uint32 (e.g. a torch tensor that is all-reduced over RCCL
 * afterwards); existing counts are copied into it; a kmerCount outside the layout then fails the batch with
 * GROOT_E_NOSPACE.  Only while nothing is in flight. */
int groot_hip_attempts_layout(groot_ctx *ctx, const uint32_t *q_values, uint32_t n_q, void *d_table);
/* Adds exported rows back (same shapes as groot_hip_attempts_export): a host that re-opens its ctx, e.g. for longer
 * reads, carries the counts over.  kmerCounts the table lacks get rows.  Only while nothing is in flight. */
int groot_hip_attempts_import(groot_ctx *ctx, const uint32_t *q_values, const uint32_t *counts, uint32_t n_rows);
int groot_hip_attempts_device(groot_ctx *ctx, void **d_table, uint32_t *n_rows, uint32_t *n_windows);
int groot_hip_attempts_reset(groot_ctx *ctx);
/* SURVEY 8e / north_star: the one exchange of a multi-GPU run.  Brings every ctx to the union row layout and sums the
 * tables in place over RCCL (ncclAllReduce, one communicator over the ctxs' devices, xGMI on an MI355X node); ctxs that
 * share a device are summed by a kernel instead.  Afterwards every ctx holds the totals.  All ctxs must be idle. */
int groot_hip_attempts_allreduce(groot_ctx *const *ctxs, int n_ctx);
/* dense compatibility view: counts[q * n_windows + w], q in [0, max_read_len-k+2) */
int groot_hip_attempts_shape(groot_ctx *ctx, uint32_t *n_q, uint32_t *n_windows);
int groot_hip_attempts_read(groot_ctx *ctx, uint32_t *out, uint64_t n_elems);

/* ---- report coverage ------------------------------------------------------------------------------------------------
 * What `groot report` reads back from the BAM of `groot align` (src/reporting/reporting.go:100-127), accumulated on the device
 * batch by batch behind the order stage, so that `align | report` needs no BAM.  Per global path p (BAM header order):
 * records[p] = the records AlignRead emits on p (alignment.go:113-156: one per path of a traversal's path set, secondary ones
 * included) and the pileup depth[i] = the records covering base i, a record at Pos with the M op of M = read length - clips
 * covering [Pos, min(Pos + M, path_len - 1)] -- both ends included, reporting.go:104-127.  groot_host_report_coverage turns
 * them into the report.  Off by default: then nothing is launched and no device memory is taken.
 * A batch is counted once: a pass the ctx redoes at collect (groot_hip_redo_status) counts in its redo only, and a batch that
 * fails with GROOT_E_NOSPACE (a read longer than max_read_len, more than 65535 traversals for one read) is not counted.  A batch
 * that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP is counted whole: the records of its other reads, which remain readable. */
/* Switch on (zeroed counters; 16 bytes per path base of HBM) or off (freed).  Only while nothing is in flight. */
int groot_hip_coverage_enable(groot_ctx *ctx, int on);
/* records[n_paths], depth[sum of path_len] with path p at sum_{q<p} path_len[q].  Waits for everything in flight (redoing what
 * needs a redo); counts every batch submitted so far.  GROOT_E_STATE when coverage is off. */
int groot_hip_coverage_export(groot_ctx *ctx, uint64_t *records, uint64_t *depth);
/* Zeroes the counters (after waiting for everything in flight).  No-op when coverage is off. */
int groot_hip_coverage_reset(groot_ctx *ctx);

/* ---- shared reads ---------------------------------------------------------------------------------------------------
 * Which reads two references share (the multimapper check of the reference tutorial, without a BAM).  For a read r let S(r) be
 * the set of global paths (BAM references) that carry at least one record of r -- the records groot_host_expand_alns emits and
 * `report` counts: every traversal, both strands, primary and secondary.  For paths a <= b in BAM header order,
 * shared[a][b] = |{r : a in S(r) and b in S(r)}|; shared[a][a] is the number of distinct reads on a.  A read is one input read of
 * the batch (one FASTQ record); groot_host_report_shared, which works from a BAM, groups records by QNAME instead, so the two
 * agree whenever read names are unique.  Accumulated on the device batch by batch behind the order stage (kernels_shared.hpp);
 * counted once exactly as coverage is (a redone pass counts in its redo only, a batch that fails with GROOT_E_NOSPACE not at all, one
 * that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP whole: the records of its other reads).
 * Off by default: then nothing is launched and no device memory is taken. */
#define GROOT_SHARED_MAX_BYTES (1ull << 30)   /* bound of the pair table: n_paths (n_paths + 1) / 2 u64 counters */
/* Switch on (zeroed counters: the pair table, plus ~(36 + 32 path_words) bytes per read of max_batch_reads) or off (freed).  Only
 * while nothing is in flight.  GROOT_E_UNSUPPORTED when the pair table would exceed GROOT_SHARED_MAX_BYTES (16 383 paths). */
int groot_hip_shared_enable(groot_ctx *ctx, int on);
/* The nonzero pairs, ascending by (a, b): *n_pairs = their number; the first min(cap, *n_pairs) are written to pa / pb / count (call
 * with cap = 0 to size the arrays).  Waits for everything in flight (redoing what needs a redo).  GROOT_E_STATE when off. */
int groot_hip_shared_export(groot_ctx *ctx, uint32_t *pa, uint32_t *pb, uint64_t *count, uint64_t cap, uint64_t *n_pairs);
/* Zeroes the counters (after waiting for everything in flight).  No-op when off. */
int groot_hip_shared_reset(groot_ctx *ctx);
/* Diagnostics since enable / reset: reads with at least one record, distinct path sets summed over batches (one table slot each),
 * reads whose records lie in more than 4 graphs (counted by the slower wave-per-read kernel).  GROOT_E_STATE when off. */
int groot_hip_shared_stats(groot_ctx *ctx, uint64_t *reads, uint64_t *distinct_sets, uint64_t *slow_reads);

/* ---- equivalence classes -------------------------------------------------------------------------------------------
 * The input of an abundance estimate by EM (groot_host_em).  S(r) is exactly the S(r) of shared reads above: the set of global paths
 * (BAM header order) that carry at least one record of input read r -- every traversal, both strands, primary and secondary.  Reads
 * with no record are in no class.  An equivalence class (EC) is a distinct non-empty S(r), written as its global path IDs in
 * ascending order; count(EC) is the number of reads r with that S(r).  Canonical EC order: lexicographic on the ascending ID lists.
 * Accumulated over the run (kernels_ec.hpp): each batch's distinct sets are folded into a run-wide table in HBM that grows as needed;
 * reads in more than 4 graphs are folded in exactly on the host when their batch is collected.  Counted once exactly as coverage is:
 * a batch that fails with GROOT_E_NOSPACE not at all, one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP whole.
 * Off by default: then nothing is launched and no device memory is taken. */
/* Switch on (an empty table; the per-read buffers of shared reads, shared with it when both are on) or off (freed).  Only while
 * nothing is in flight. */
int groot_hip_ec_enable(groot_ctx *ctx, int on);
/* The ECs since enable / reset in canonical order, as CSR: EC i is ids[off[i] .. off[i+1]), count[i] its reads.  *n_ec / *n_ids =
 * their sizes; call with cap_ec = cap_ids = 0 to get them, then with off[cap_ec + 1], ids[cap_ids], count[cap_ec] (GROOT_E_NOSPACE
 * when they are too small).  Waits for everything in flight (redoing what needs a redo).  GROOT_E_STATE when off. */
int groot_hip_ec_export(groot_ctx *ctx, uint64_t *off, uint32_t *ids, uint64_t *count, uint64_t cap_ec, uint64_t cap_ids, uint64_t *n_ec,
                        uint64_t *n_ids);
/* Empties the table (after waiting for everything in flight).  No-op when off. */
int groot_hip_ec_reset(groot_ctx *ctx);
/* Since enable / reset: reads in an EC (the sum of the counts), distinct ECs, reads folded in on the host (in more than 4 graphs, or
 * in more than one under GROOT_TEST_SHARED_SLOW), times the table grew.  Waits for everything in flight.  GROOT_E_STATE when off. */
int groot_hip_ec_stats(groot_ctx *ctx, uint64_t *reads, uint64_t *distinct, uint64_t *slow_reads, uint64_t *grows);

/* ---- assigned coverage ---------------------------------------------------------------------------------------------
 * The pileup of the reads the abundance EM assigns to each path: every record of read r on path p gets the weight of r's posterior
 * on p.  The definition (README.md, DESIGN.md 13, groot_host.h and the tests quote it):
 *
 *   S(r), equivalence classes (ECs), their canonical order and alpha = groot_host_em over the run's ECs: exactly as for --abundance.
 *   For an EC e (ascending path IDs) and p in e:   w(e,p) = alpha[p] / denom(e),  denom(e) = sum of alpha[q], q in e, in ID order;
 *                                                  w(e,p) = 0.0 where the EM skips e (denom < 2^-52).  Double, no FMA contraction.
 *   A record of read r on path p with an M op of M bases at Pos covers [Pos, last], last = min(Pos + M, path_len(p) - 1), both ends
 *   included: the interval `report` piles up.  EVERY record counts (both strands, primary and secondary), as in the report.
 *   The assigned-coverage table of a run is the multiset of records grouped by (e = EC of S(r), p, Pos, last):  n(e,p,Pos,last), integers.
 *   Per path p, per EC e holding p:  d_e[x] = number of records of (e,p,.,.) covering base x   (integers).
 *   Assigned depth:  D_p[x] = sum over the ECs holding p, in canonical EC order, of (double)d_e[x] * w(e,p).
 *   A base is covered when D_p[x] >= callDepth (default 1.0).  breadth = covered / path_len;  depth = (sum of D_p[x] in x order) / path_len.
 *
 * Only the integer table is computed on the device (kernels_acov.hpp); everything in floating point happens once, on the host, in a
 * fixed order (groot_host_calls_from_table), so the result depends on neither the batch size, the pipeline depth, the first-pass
 * variant nor the number of ctxs or GPUs.  The table is a run-wide open-addressing table in HBM keyed by (serial of the EC's slot in
 * the EC table, path, Pos, last), 16 bytes a key and a u64 count, that grows as it fills (a batch whose keys found no room adds
 * nothing and is counted again at collect, after the growth: no count is lost or doubled).  Reads in more than 4 graphs are grouped
 * on the host at collect, as their ECs are.  Counted once exactly as the other counters are.  Not with pairing (GROOT_E_UNSUPPORTED,
 * from whichever of the two enables comes second) but through groot_hip_acov_pairs_enable, below.  Off by default: then nothing is launched and no device memory is taken. */
/* Switch on (an empty table of 2^20 slots, 24 MB; equivalence classes are switched on if they are off, and stay on) or off (freed;
 * groot_hip_ec_enable(ctx, 0) switches it off too).  Only while nothing is in flight. */
int groot_hip_acov_enable(groot_ctx *ctx, int on);
/* The ctx's ECs since enable / reset exactly as groot_hip_ec_export gives them (canonical order, CSR: ec_off[cap_ec + 1],
 * ec_ids[cap_ids], ec_count[cap_ec]) and the table: tuple i = tuples[4 i .. 4 i + 4) = (EC index into that list, path, Pos, last),
 * n[i] its records; the tuples ascend.  *n_ec / *n_ids / *n_tuples = the sizes; call with all three caps 0 to get them
 * (GROOT_E_NOSPACE when an array is too small).  Waits for everything in flight.  GROOT_E_STATE when off.  (Tuples count from
 * groot_hip_acov_enable / _reset, ECs from groot_hip_ec_enable / _reset: enable both before the first batch for a consistent pair.) */
int groot_hip_acov_export(groot_ctx *ctx, uint64_t *ec_off, uint32_t *ec_ids, uint64_t *ec_count, uint32_t *tuples, uint64_t *n,
                          uint64_t cap_ec, uint64_t cap_ids, uint64_t cap_tuples, uint64_t *n_ec, uint64_t *n_ids, uint64_t *n_tuples);
/* Empties the table (after waiting for everything in flight); groot_hip_ec_reset does this too.  No-op when off. */
int groot_hip_acov_reset(groot_ctx *ctx);
/* Since enable / reset: records in the table (the sum of n), distinct tuples, slots of the device table, times it grew, records
 * grouped on the host (slow-path reads); all zero while off.  launches: kernels launched for assigned coverage since the ctx was
 * opened -- it does not move while the feature is off.  Waits for everything in flight. */
int groot_hip_acov_stats(groot_ctx *ctx, uint64_t *records, uint64_t *tuples, uint64_t *slots, uint64_t *grows, uint64_t *slow_records,
                         uint64_t *launches);

/* ---- assignment: each read to its best allele by EM posterior --------------------------------------------------------------
 * `align --assignFrom`: with the alpha of an earlier run's abundance estimate in hand, a batch keeps, per read, only the records on the
 * path with the largest posterior, decided on the device before anything is copied out.  The definition (groot_host.h, README.md,
 * DESIGN.md 14 and the tests quote it):
 *
 *   Input: alpha[n_paths] (global path = BAM reference order), every value finite and 0 <= alpha[p] <= 1e300; min_post in [0, 1].
 *   S(r) exactly as for --sharedReads: the global paths carrying at least one record of read r.
 *   For a read r with records, double precision, no FMA contraction, p running over S(r) in ASCENDING global ID:
 *       denom = 0.0;  denom = denom + alpha[p]
 *       best  = the p of S(r) with the largest alpha[p]; among equal values the lowest ID
 *     unassigned:  denom == 0.0.                                   No record of r is kept.
 *     below:       not (alpha[best] >= min_post * denom)           (one product, one comparison, no division).  No record of r is kept.
 *     assigned:    otherwise.  Every record of r on `best` is kept (every traversal whose path set holds best; both strands), nothing else.
 *       rest = denom - alpha[best]                                 (>= 0: a sum of non-negative terms is never below one of them)
 *       j    = the number of k in 1..20 with ldexp(rest, k) <= denom   (a product by 2^k is exact; rest == 0 gives 20)
 *       mapq = 3 * j                                               (0, 3, .., 60: one step per halving of the posterior mass elsewhere)
 *   What happens to the batch's traversal records, in place, BEFORE anything else reads them:
 *     the number of traversals, their order, read_id, graph_id, node, offset, ord and the RC / clip flags do not change;
 *     a kept traversal's path set becomes {best} (every other bit of all its words cleared); a traversal that is not kept gets the EMPTY
 *     path set (it expands to no record), loses GROOT_TRAV_FIRST and has reserved = 0;
 *     GROOT_TRAV_FIRST is cleared on all of r's traversals and set on the first kept one in (read, ord) order: an assigned read has exactly
 *     one primary record, its further records on `best` are secondary;
 *     kept traversals get GROOT_TRAV_MAPQ (16u, new) and reserved = mapq.
 *   Per read (batch position): best[r] = the global path, 0xFFFFFFFF when r keeps no record; mapq[r], 0 then.
 *   groot_counts (mapped, multimapped, alignments, travs, ...), call counts, weights and the GFA are those of the unfiltered run.
 *
 * assign_kernel (kernels_assign.hpp) runs on the tail stream right behind the order stage's last scatter, one thread per read, so the
 * compact copy-out, the packed records, report coverage and groot_hip_read_travs all see the filtered records; the result depends on
 * alpha and the read's records alone, not on the batch size, the pipeline depth, the first-pass variant or the number of ctxs.  A batch
 * is filtered, and counted in the stats, once: a pass that collect redoes by its redo, a batch that fails with GROOT_E_NOSPACE not at all
 * (its records stay unfiltered, best = 0xFFFFFFFF).  Off by default: then no allocation, no launch, no sync. */
/* Switch on with a copy of alpha[n_paths] (a second call replaces it), or off with alpha == NULL.  Only while nothing is in flight
 * (GROOT_E_STATE).  GROOT_E_INVALID when n_paths is not the index's or a value or min_posterior is out of range.  GROOT_E_UNSUPPORTED
 * while shared reads, equivalence classes, assigned coverage or pairing is on -- they count S(r), which assignment collapses --, and from
 * their enable calls while assignment is on.  Report coverage is allowed and counts the kept records. */
int groot_hip_assign_enable(groot_ctx *ctx, const double *alpha, uint32_t n_paths, double min_posterior);
/* best[n_reads] / mapq[n_reads] of a collected, unreleased batch (ticket 0: the batch groot_hip_wait collected), in pinned host memory
 * that stays valid until the batch is released; either pointer may be NULL.  GROOT_E_STATE when assignment is off or was off when the
 * batch was submitted. */
int groot_hip_assign_batch(groot_ctx *ctx, uint64_t ticket, const uint32_t **best, const uint8_t **mapq);
/* The eight counters since enable / reset (replacing alpha keeps them) plus launches: kernels launched for assignment since the ctx was
 * opened -- it does not move while the feature is off.  Zeros (but for launches) while off.  Waits for everything in flight. */
int groot_hip_assign_stats(groot_ctx *ctx, groot_assign_stats *out);
/* Zeroes the eight counters (after waiting for everything in flight).  No-op when off. */
int groot_hip_assign_reset(groot_ctx *ctx);

/* ---- paired-end reads -------------------------------------------------------------------------------------------------
 * With pairing on, reads 2i and 2i+1 of a batch are the mates of fragment i.  The index is batch-relative: read_id - first_read_id;
 * first_read_id may be odd.  Let A = S(r_2i) and B = S(r_2i+1), S(r) exactly as above.
 *   joined:  A and B intersect.  The fragment is one unit with the set A n B.
 *   split:   A and B are non-empty and do not intersect.  The fragment is two units, A and B, exactly as without pairing (mates on
 *            different genes are evidence for both).
 *   single:  exactly one of A, B is non-empty.  The fragment is one unit with that set.
 *   none:    both are empty.  There is no unit.
 * Everywhere shared reads and equivalence classes say "read", paired mode says "unit": shared[a][b] is the number of units whose set
 * holds both a and b (the diagonal: the units on a); an EC is a distinct unit set and its count the units with that set; the `reads`
 * fields of the shared and EC stats count units; bootstrap replicates draw units.  Coverage, records, call counts, weights, the BAM and
 * every groot_counts field do not depend on pairing.
 * The units are made on the device by a gather of their own (kernels_shared.hpp, shared_gather_paired_kernel): one thread per fragment
 * intersects the two mates' per-graph path sets; the result does not depend on which path a unit takes (in at most 4 graphs or in
 * more, GROOT_TEST_SHARED_SLOW, a redone batch, the pipeline depth, the first-pass variant).  Fragments whose mates lie in different
 * batches are not supported.  Off by default: then every launch and every count is what it is without this section. */
/* Switch on or off; takes effect on whichever of shared reads and equivalence classes are on, whichever is enabled first, and costs
 * nothing (no launch, no memory) while both are off.  Zeroes the fragment counts.  Only while nothing is in flight (GROOT_E_STATE).
 * While it is on, every submit call (groot_hip_submit, _packed, _packed16, _acquired, _device) of a batch with an odd number of
 * reads fails with GROOT_E_INVALID before anything is enqueued; the ctx stays usable, and a batch of 0 reads is fine. */
int groot_hip_pairs_enable(groot_ctx *ctx, int on);
/* Fragments per class since groot_hip_pairs_enable, groot_hip_shared_reset or groot_hip_ec_reset (each zeroes them), counted once
 * exactly as the counters are.  joined + 2 split + single = the `reads` of groot_hip_shared_stats = the `reads` of groot_hip_ec_stats.
 * Waits for everything in flight.  GROOT_E_STATE when pairing is off. */
int groot_hip_pairs_stats(groot_ctx *ctx, uint64_t *joined, uint64_t *split, uint64_t *single);

/* ---- assigned coverage over fragments ------------------------------------------------------------------------------------
 * `align --calls --callsPaired`: the pileup of --calls with paired-end units.  The rule (README.md, DESIGN.md 24 and the tests quote it):
 *
 *   S(r), fragments, A = S(r_2i), B = S(r_2i+1), joined / split / single / none, units, ECs over units, canonical order, alpha, w(e,p):
 *   exactly as in "paired-end reads"  and "assigned coverage" (DESIGN 13).
 *   U(r), the UNIT SET of a read r with records:   A n B  when r's fragment is joined (both mates get the same set);
 *                                                  S(r)   when it is split or single.
 *   A record of read r on path p COUNTS when p is in U(r); it is then a record of the pileup under e = EC of U(r), covering [Pos, last],
 *   last = min(Pos + M, path_len(p) - 1), M the record's own M op (its own mate's length less its clips): the interval of DESIGN 13, unchanged.
 *   A record of a joined fragment on a path outside A n B is LEFT OUT: the unit the EM counted has no posterior there (w(e,p) is defined for
 *   p in e only), so its weight is zero.  Both mates' records count, each as one record; every strand, primary and secondary, as in DESIGN 13.
 *   The assigned-coverage table of a run with the feature on is the multiset of counting records grouped by (e, p, Pos, last).
 *   d_e[x], D_p[x], depth, breadth, cigar, called, --callSupport's and --rarefy's columns: the existing host and device functions on that
 *   table and those ECs, unchanged.  A pass that collect redoes counts once; a batch under kCovSkipFlags counts nothing.
 *   The table depends on the reads, their pairing and the index alone: not on batch size, pipeline depth, align stage, --ctxPerGpu or --gpus.
 *
 * So with split and single fragments only the table is the unpaired run's, and fragments (r, r) give the unpaired run's ECs with every n
 * doubled.  On the device (kernels_acov.hpp): ec_merge_kernel<true> leaves the units' serials, acov_serial_paired_kernel (a thread per
 * fragment) hands both mates of a joined fragment the unit's serial and each the span of the other's records, 8 bytes per read in a
 * buffer of the batch's slot, and acov_count_kernel<.., true> counts a record on p only when a record of the mate in the same graph
 * holds p too.  Joined fragments whose set spans more than 4 graphs are folded on the host at collect, as their ECs are. */
typedef struct groot_acov_pairs_stats {
    uint64_t records;         /* records that counted since enable / groot_hip_acov_reset, device and host: the sum of n of the table */
    uint64_t left_out;        /* records left out under the rule (a joined fragment's, on a path outside A n B), device and host */
    uint64_t joined_reads;    /* reads of joined fragments (two per fragment), whichever path their unit took */
    uint64_t slow_fragments;  /* joined fragments folded on the host (their set in more than 4 graphs, or in more than one under GROOT_TEST_SHARED_SLOW) */
} groot_acov_pairs_stats;
/* on != 0: puts the ctx into "assigned coverage over fragments" -- switches on whichever of equivalence classes, assigned coverage and
 * pairing is off, and the rule above; the one way in which assigned coverage and pairing run together (groot_hip_acov_enable with
 * pairing on, and groot_hip_pairs_enable(1) with assigned coverage on and the rule off, keep refusing).  GROOT_E_UNSUPPORTED while
 * assignment or the rescued reads in the classes (groot_hip_rescue_ec_enable and everything built on it) are on.  on == 0: the rule and
 * assigned coverage go, equivalence classes and pairing stay; groot_hip_acov_enable(ctx, 0) and groot_hip_pairs_enable(ctx, 0) while the
 * rule is on do the same (the latter switches pairing off too).  Only while nothing is in flight (GROOT_E_STATE).
 * groot_hip_acov_export / _reset / _stats keep their meaning; groot_hip_acov_reset zeroes the stats below. */
int groot_hip_acov_pairs_enable(groot_ctx *ctx, int on);
/* The four counts; zeros while the rule is off.  Waits for everything in flight. */
int groot_hip_acov_pairs_stats(groot_ctx *ctx, groot_acov_pairs_stats *out);

/* ---- mismatch rescue of unaligned reads ---------------------------------------------------------------------------------
 * The aligner is exact-match (AlignRead): a read with one sequencing error, or across the one SNP by which a sample's allele differs
 * from every indexed one, leaves no record, so no counter above sees it.  With rescue on, two kernels behind every batch's order stage
 * (kernels_rescue.hpp) lay the reads WITHOUT a record ungapped on the paths' linear texts with up to M substitutions and pile up where
 * they lie and what differs.  Records, BAM, weights and every other counter stay what they are.  The definition, all of it integers:
 *
 *   M = max mismatches, 1 <= M <= 3.   A = 16 (anchor length in bases).
 *   Text of path p: the concatenation of its nodes' sequences in Position order, for the paths build_path_tables gives a text
 *   (non-empty nodes, no gap or overlap, joined by OutEdges); path coordinate x = Position of the path's first node + offset in the text.
 *   A read r of a batch is a CANDIDATE when: the batch pass is counted (the kCovSkipFlags rule of the other counters), r has NO traversal
 *   record, every base of r is A/C/G/T (nothing of it on the exception list), and len(r) >= A * (M + 1).
 *   A PLACEMENT of r is (p, strand, x): the oriented read (r, or its reverse complement for strand = 1) laid ungapped on
 *   text_p[x .. x + len), entirely inside the text (0 <= x, x + len <= path_len(p)), with no 'N' of the path in the window, and
 *   Hamming distance d <= M.   (len >= A(M+1) leaves at least one of the disjoint blocks [0,16), [16,32), .. of the oriented read error-free, so
 *   every placement holds an exact 16-mer anchor: the anchor search loses none.)
 *   d*(r) = the smallest d over r's placements.  r is RESCUED when it has a placement; its KEPT placements are all those with d = d*
 *   (every path, both strands, every x: as the aligner keeps every multimapper).  A placement is counted once, however many blocks anchor it.
 *   Per kept placement:   rdepth[p][x .. x + len - 1] += 1;   for every mismatching base at path coordinate y:  alt[p][y][b] += 1, b = the
 *   base the oriented read has there (path strand: a strand-1 read contributes the complement of what the FASTQ says).
 *   Stats: candidates, rescued, rescued with d* = 0, kept placements, reads left out as too short / non-ACGT.
 *
 * Read closely: 'N' stands for any byte of the graph other than A, C, G, T; a read without a record that is both non-ACGT and too short
 * counts as non-ACGT; b is indexed A, C, G, T = 0..3.  The tables depend on the reads and the index alone: not on batch size, pipeline
 * depth, first-pass variant, results_on_device, or how the reads are spread over ctxs (the merge of several ctxs is a sum).  A batch
 * is counted once, by the rule of report coverage.  With pairing on, mates are rescued one by one.  Independent of coverage, shared
 * reads, equivalence classes and assigned coverage; refused with assignment, whichever is enabled second (GROOT_E_UNSUPPORTED):
 * assignment rewrites the records that tell which reads are unaligned.  Off by default: then no allocation, launch or sync. */
typedef struct groot_rescue_stats {
    uint64_t candidates, rescued, exact /* rescued with d* = 0 */, placements /* kept */, too_short, non_acgt;
    uint64_t text_paths; /* paths with a text (0 while off) */
    uint64_t launches;   /* kernels launched for rescue since open, whether it is on now or not */
} groot_rescue_stats;
/* max_mismatch 1..3: on (0: off, everything freed; above 3: GROOT_E_INVALID).  The first time it comes on, the path texts and an exact
 * table of their 16-mers are built from `idx` on the host and uploaded -- `idx` must be the view the ctx was opened with (GROOT_E_INVALID);
 * it is only read during the call (no call retains a caller pointer), and may be NULL to switch off or to change M.  Counters start at
 * zero; another M while on zeroes them.  Device memory: 48 bytes per path base, the texts and the table (about 20 bytes per path base),
 * max_batch_bases / 2 + 20 max_batch_reads bytes of work space.  Only while nothing is in flight (GROOT_E_STATE).  GROOT_E_UNSUPPORTED
 * when the texts are beyond 32-bit bit offsets. */
int groot_hip_rescue_enable(groot_ctx *ctx, const groot_index_view *idx, uint32_t max_mismatch);
/* depth[sum of path_len] = rdepth, alt[4 * sum of path_len] with path p at sum_{q<p} path_len[q], global path order; paths without a
 * text stay zero.  Waits for everything in flight (redoing what needs a redo).  GROOT_E_STATE when rescue is off. */
int groot_hip_rescue_export(groot_ctx *ctx, uint64_t *depth, uint64_t *alt);
/* Since enable / reset, counted once exactly as the tables are; zeros while off, but for launches.  Waits for everything in flight. */
int groot_hip_rescue_stats(groot_ctx *ctx, groot_rescue_stats *out);
/* Zeroes tables and stats (after waiting for everything in flight).  No-op when off. */
int groot_hip_rescue_reset(groot_ctx *ctx);

/* ---- gapped rescue of the reads mismatch rescue leaves ------------------------------------------------------------------
 * Mismatch rescue places reads that differ from a path's text by substitutions only.  A read across a frameshift, or across a codon
 * deletion or insertion, stays unplaced.  With gapped rescue on (it needs mismatch rescue on), a third kernel behind the two of rescue
 * (kernels_gap.hpp) lays those reads on the texts with ONE gap of up to G bases and up to M substitutions, and piles up where they lie
 * and which gaps they show.  Everything else, mismatch rescue's tables included, stays what it is.  The definition, all of it integers:
 *
 *   M, A = 16, texts, path coordinates, 'N', CANDIDATE, oriented read, strand: exactly mismatch rescue's.   G = max gap length, 1 <= G <= 8.
 *   A GAP CANDIDATE is a candidate of mismatch rescue that is NOT rescued (no ungapped placement with d <= M) and has len >= A * (M + 3).
 *      (A candidate that is rescued ungapped is never looked at here, even if a gapped placement would cost less.)
 *   A GAPPED PLACEMENT of r is (p, strand, x, type, g, k), 1 <= g <= G, with the oriented read R (len bases) and T = text_p:
 *      type DEL (g text bases missing from the read):   R[0,k) on T[x, x+k),  R[k,len) on T[x+k+g, x+len+g);   A <= k <= len - A
 *                                                       occupied window W = T[x, x+len+g)
 *      type INS (g read bases missing from the text):   R[0,k) on T[x, x+k),  R[k+g,len) on T[x+k, x+len-g);   A <= k <= len - g - A
 *                                                       occupied window W = T[x, x+len-g);  R[k,k+g) is the inserted sequence
 *      W lies entirely inside the text's bases inside path_len (mismatch rescue's bound) and holds no 'N' (the deleted bases included).
 *      d(k) = the number of mismatching bases of the two aligned parts.   (Both flanks are at least A bases: a gap nearer to an end
 *      than that is not told apart from substitutions at the end, and is left out.)
 *   For fixed (p, strand, x, type, g):  d = min over the allowed k of d(k);  k* = the SMALLEST k with d(k) = d (the gap is left-aligned);
 *      the gapped placement of (p, strand, x, type, g) is the one at k*, and it exists when d <= M.    Its cost is e = d + g.
 *   e*(r) = the smallest e over r's gapped placements.  r is GAP-RESCUED when it has one; its KEPT gapped placements are all those with
 *      e = e* (every path, both strands, every x, both types, every g).  Each (p, strand, x, type, g) counts once, however it was found.
 *   Per kept gapped placement, in path coordinates (X = first Position of the path + x):
 *      gdepth[p][y] += 1 for every text base y an aligned read base lies on:  DEL: [X, X+k*) and [X+k*+g, X+len+g);  INS: [X, X+len-g).
 *      event (p, pos = X + k* - 1, type, g, seq) += 1.   pos is the last text base before the gap.  seq = the g inserted read bases
 *      R[k*, k*+g) in path strand for INS (2 bits per base, base i in bits 2i..2i+1, A C G T = 0 1 2 3), 0 for DEL.
 *      Substitutions of gapped placements are not piled up anywhere.
 *   Stats: gap candidates, gap-rescued, kept gapped placements, kept DEL placements, kept INS placements, candidates left out as too short
 *      for a gap (len < A (M + 3)), distinct events, events dropped (table full).
 *
 * Why the anchor search loses nothing: len >= A(M+3) gives at least M+3 disjoint 16-base blocks [0,16), [16,32), .. of the oriented read.
 * Substitutions spoil at most M of them, a DEL cut spoils at most one, the inserted bases of an INS (at most 8) touch at most two.  So at
 * least one block lies wholly in the part in front of the gap or wholly in the part behind it, error-free, inside a window without 'N':
 * that block is in the 16-mer table, and the kernel tries every occurrence of every block under both hypotheses.
 * The tables depend on the reads and the index alone: not on batch size, pipeline depth, first-pass variant, results_on_device, or how the
 * reads are spread over ctxs; merging several ctxs is a sum (gdepth elementwise, events by key).  A batch is counted once, by the rule
 * of report coverage.  Off by default: then no allocation, launch or sync, and rescue_count_kernel is the one without the hand-over. */
/* groot_gap_event, GROOT_GAP_DEL and GROOT_GAP_INS: groot_host.h ("Indels"), whose writer reads them */
typedef struct groot_gap_stats {
    uint64_t candidates, rescued, placements /* kept */, del_placements, ins_placements, too_short, events /* distinct */, dropped;
    uint64_t event_slots; /* slots of the event table (0 while off) */
    uint64_t launches;    /* rescue_gap_kernel launches since open, whether it is on now or not (not part of groot_rescue_stats.launches) */
} groot_gap_stats;
/* max_gap 1..8: on (0: off, everything freed, nothing launched afterwards; above 8: GROOT_E_INVALID).  GROOT_E_STATE when mismatch rescue is
 * off, or when something is in flight.  event_slots: the slots of the event table, a power of two (0: 2^22 = 64 MB; anything else:
 * GROOT_E_INVALID); the table does not grow.  Tables start at zero; another G or another event_slots while on zeroes them, and so do
 * groot_hip_rescue_enable with another M and groot_hip_rescue_reset (they are derived from the same reads); groot_hip_rescue_enable(.., 0)
 * switches gapped rescue off as well.  Device memory: 16 bytes per path base, 16 bytes per event slot, 4 bytes per read of a batch. */
int groot_hip_gap_enable(groot_ctx *ctx, uint32_t max_gap, uint64_t event_slots);
/* gdepth[sum of path_len] laid out as groot_hip_rescue_export's depth; events[0 .. *n_events) ascending by (path, pos, type, len, seq).
 * *n_events is always set to the number of distinct events; cap below it: GROOT_E_INVALID.  Events were dropped because the table was
 * full: GROOT_E_NOSPACE, and the message names event_slots.  Waits for everything in flight (redoing what needs a redo).
 * GROOT_E_STATE when gapped rescue is off. */
int groot_hip_gap_export(groot_ctx *ctx, uint64_t *gdepth, groot_gap_event *events, uint64_t cap, uint64_t *n_events);
/* Since enable / reset, counted once exactly as the tables are; zeros while off, but for launches.  Waits for everything in flight. */
int groot_hip_gap_stats(groot_ctx *ctx, groot_gap_stats *out);
/* Zeroes the gap tables and stats (after waiting for everything in flight).  No-op when off. */
int groot_hip_gap_reset(groot_ctx *ctx);

/* ---- rescued reads in the equivalence classes ---------------------------------------------------------------------------
 * The equivalence classes count S(r), and the aligner is exact-match: a read with one sequencing error has no record and is in no
 * class, though mismatch rescue knows where it lies.  With this on, a rescued read is a unit of the classes with the set of paths it
 * was placed on.  The definition:
 *
 *   S(r)   as in "equivalence classes": the global paths with a record of r.
 *   R(r)   for a read r that is RESCUED under "mismatch rescue" (a candidate with d*(r) <= M): the set of global paths p for which r has
 *          a KEPT placement (p, strand, x) -- any strand, any x, each p once.  Not defined for any other read.
 *   S+(r)  = S(r) when r has a record;  R(r) when r is rescued;  empty otherwise.   (The two cases exclude each other: a candidate has
 *          no record.)
 *
 * With the feature on, the run's ECs are the distinct non-empty S+(r) with their read counts; a rescued read and an exact read with
 * the same set are one EC.  Nothing else changes: records, BAM, GFA, weights, coverage, shared reads, the rescue tables, the gap tables
 * (a read placed with a gap is in no class, unless the gap-placed reads in the classes are on: below), and every stat that exists today.  The ECs depend on the reads and the index alone: not on
 * batch size, pipeline depth, align-stage variant, results_on_device, or how the reads are spread over ctxs; the merge of several ctxs
 * is a sum by set.  A pass that collect redoes counts once, a batch under the skip flags of report coverage counts nothing.
 * Off by default: then no allocation, launch or sync, and rescue_count_kernel is the one of mismatch rescue alone. */
#define GROOT_RESCUE_EC_BYTES (8ull << 20)   /* per pipeline slot: the bitmaps (n_paths bits each) of a batch's rescued reads in more than 4 graphs */
typedef struct groot_rescue_ec_stats {
    uint64_t reads;       /* rescued reads added to the classes since enable / groot_hip_ec_reset */
    uint64_t slow_reads;  /* those among them whose set lies in more than 4 graphs (1 under GROOT_TEST_SHARED_SLOW): folded on the host from bitmaps */
    uint64_t rows;        /* bitmaps per batch: min(max_batch_reads, GROOT_RESCUE_EC_BYTES / (8 ceil(n_paths / 64))), or GROOT_TEST_RESCUE_EC_ROWS; 0 while off */
    uint64_t launches;    /* kernels launched for it since open, whether it is on now or not (rescue_count_ec_kernel counts in groot_rescue_stats.launches) */
} groot_rescue_ec_stats;
/* While the rule of "rescued mates in paired-end units" (below) is on, the reads are mates of fragments: `reads` is the rescued mates in a unit
 * (groot_rescue_pairs_stats.rescued_mates), `slow_reads` those of them in a unit that took a bitmap, and `launches` stays put -- the kernels
 * that run in its place count in groot_rescue_pairs_stats.launches. */
/* on != 0: on.  Needs mismatch rescue and equivalence classes on (GROOT_E_STATE otherwise), and nothing in flight (GROOT_E_STATE).
 * GROOT_E_UNSUPPORTED beside pairing (the two run together through groot_hip_rescue_pairs_enable alone: below) or assigned coverage, whichever is enabled second.  Switching mismatch rescue or the equivalence
 * classes off switches it off too.  groot_hip_rescue_enable with another M and groot_hip_rescue_reset leave the classes alone;
 * groot_hip_ec_reset zeroes them, the rescued reads in them and these stats.  A batch with more rescued reads in more than 4 graphs than
 * `rows` fails at collect with GROOT_E_NOSPACE (the message names GROOT_TEST_RESCUE_EC_ROWS): no read is dropped silently.
 * groot_hip_ec_export and groot_hip_ec_stats then count the rescued reads too (reads, distinct); slow_reads there stays the reads with
 * a record.  Device memory: 8 bytes per path, 1 byte per read of a batch, `rows` bitmaps per pipeline slot. */
int groot_hip_rescue_ec_enable(groot_ctx *ctx, int on);
/* Waits for everything in flight; zeros while off, but for launches. */
int groot_hip_rescue_ec_stats(groot_ctx *ctx, groot_rescue_ec_stats *out);

/* ---- rescued mates in paired-end units -------------------------------------------------------------------------------------
 * Pairing makes the classes count fragments, and the rescued reads in the classes put the reads with a sequencing error back; the two
 * enables refuse each other, because a rescued mate's set exists only behind the kernels that make the fragments' units.  With this rule
 * on they run together (kernels_rescue_pairs.hpp).  The rule:
 *
 *   S(r), R(r), S+(r), candidate, rescued, d*, kept placement: exactly as in "mismatch rescue" and "rescued reads in the equivalence classes".
 *   Fragments, joined / split / single / none, units, ECs over units: exactly as in "paired-end reads" (DESIGN §12), with
 *       A = S+(r_2i),  B = S+(r_2i+1)
 *   in place of S(.).  So a mate counts with its records' paths when it has records, with R(r) when mismatch rescue places it, and as
 *   empty otherwise (no record and: no candidate, or a candidate left unplaced, or placed only with a gap).
 *     joined:  A n B not empty: one unit, A n B.     split: both non-empty, disjoint: two units, A and B.
 *     single:  one non-empty: one unit.              none: no unit.
 *   R(r) is the set at d*(r) and nothing else: a rescued mate whose kept placements miss every path of its partner is SPLIT from it, even where
 *   a placement at a larger distance would have met one.  Mates are still rescued one by one; no insert size, no orientation.
 *   The run's ECs are the distinct unit sets with their unit counts; a unit made of exact mates, of rescued mates or of one of each, with the
 *   same set, is one EC.  joined + 2 split + single = ec_stats.reads.
 *
 * A fragment whose mates both have records is what it is under pairing alone; with no rescued mate in the run the classes are those of
 * pairing and the classes alone; fragments (r, r) give the classes of the unpaired run with the rescued reads in the classes.  Nothing else
 * changes: records, BAM, coverage, the rescue and gap tables, the rescued and gapped records, and every stat that exists.  A pass that
 * collect redoes counts once, a batch under the skip flags of report coverage counts nothing.  The classes depend on the reads, their
 * pairing and the index alone: not on batch size, pipeline depth, align-stage variant, results_on_device, or how the fragments are spread
 * over ctxs (the merge of several ctxs is a sum by set). */
typedef struct groot_rescue_pairs_stats {
    uint64_t exact_rescued_joined, exact_rescued_split;         /* fragments of one mate with records and one rescued mate */
    uint64_t rescued_rescued_joined, rescued_rescued_split;     /* fragments of two rescued mates */
    uint64_t single_exact, single_rescued;                      /* fragments with one non-empty mate: it has records / it is rescued */
    uint64_t rescued_mates;   /* rescued mates in a unit (a joined fragment of two rescued mates has two) */
    uint64_t bitmap_units;    /* units among the above folded on the host from a bitmap: a mate in more than 4 graphs (1 under GROOT_TEST_SHARED_SLOW) */
    uint64_t launches;        /* the three kernels of kernels_rescue_pairs.hpp since open, whether the rule is on now or not */
} groot_rescue_pairs_stats;
/* on != 0: puts the ctx into "rescued mates in paired-end units" -- switches on whichever of equivalence classes, pairing and the rescued
 * reads in the classes is off, and the rule above; the one way in which pairing and the rescued classes run together
 * (groot_hip_rescue_ec_enable with pairing on, and groot_hip_pairs_enable(1) with the rescued classes on and the rule off, keep refusing).
 * Needs mismatch rescue on (GROOT_E_STATE) and nothing in flight (GROOT_E_STATE).  GROOT_E_UNSUPPORTED, whichever is enabled second, beside
 * shared reads, assigned coverage in any form, assigned coverage over fragments, the gap-placed reads in the classes, and assignment.
 * on == 0: the rule and the rescued classes go, equivalence classes and pairing stay; groot_hip_rescue_ec_enable(ctx, 0),
 * groot_hip_rescue_enable(ctx, .., 0) and groot_hip_ec_enable(ctx, 0) while the rule is on do the same, and so does
 * groot_hip_pairs_enable(ctx, 0), which switches pairing off too.  groot_hip_ec_reset zeroes the classes and these stats and leaves the
 * rule on.  While the rule is on, groot_hip_pairs_stats and groot_hip_ec_stats cover the fragments with a rescued mate,
 * groot_rescue_ec_stats.reads is rescued_mates and .slow_reads those of them in a unit that took a bitmap.  A fragment with a mate that
 * fits no row takes one bitmap of groot_rescue_ec_stats.rows per non-empty mate; a batch that needs more fails at collect with
 * GROOT_E_NOSPACE (the message names GROOT_TEST_RESCUE_EC_ROWS) and counts NOTHING: the classes, groot_hip_ec_stats, groot_hip_pairs_stats and
 * these stats are what they were before it, the fragments whose mates both have records included.  Device memory: 1 byte per read of a batch. */
int groot_hip_rescue_pairs_enable(groot_ctx *ctx, int on);
/* Since the rule came on / groot_hip_ec_reset; zeros while it is off, but for launches.  Waits for everything in flight. */
int groot_hip_rescue_pairs_stats(groot_ctx *ctx, groot_rescue_pairs_stats *out);

/* ---- rescued reads in assigned coverage ----------------------------------------------------------------------------------
 * The assigned-coverage table piles up records, and a rescued read has none: with the rescued reads in the classes alone, the EM would
 * see them and the pileup would not.  With this on, every kept placement of a rescued read is a record of the table.  The definition:
 *
 *   S+(r), R(r), d*(r), kept placement (p, strand, x), path coordinate X: exactly as in "mismatch rescue" and "rescued reads in the equivalence
 *   classes".  ECs, canonical order, alpha, w(e,p): exactly as for --abundance --abundanceRescued (the run's ECs are the distinct non-empty S+(r)).
 *   A kept placement (p, strand, x) of a rescued read r of length len is one RESCUED RECORD of r on p covering [X, X + len - 1], both ends
 *   included -- the bases on which rescue's rdepth grows for that placement, and in the coordinate the exact records' Pos uses.  Every kept
 *   placement counts: both strands, every x, several on one path.  (An exact record covers [Pos, min(Pos + M, path_len - 1)], the report's
 *   interval, one base more than the read where the path allows: that stays.  The two kinds are not made alike.)
 *   The assigned-coverage table of a run with the feature on is the multiset of exact records AND rescued records grouped by
 *   (e = EC of S+(r), p, Pos, last): n(e, p, Pos, last), integers.  d_e[x], D_p[x], depth, breadth, cigar, called, --callSupport's and --rarefy's
 *   columns: computed from that table and those ECs by the existing host and device functions, unchanged.
 *   Reads placed with a gap (--indels) have no rescued record.  A pass that collect redoes counts once; a batch under kCovSkipFlags counts nothing.
 *   The table depends on the reads and the index alone: not on batch size, pipeline depth, align stage, --ctxPerGpu or --gpus.
 *
 * The exact pileup repeats a batch's claim and add at collect when the table was full; a rescued batch cannot be replayed (its inputs
 * are the ctx's, one batch at a time), so its records are claimed and added in one pass over the whole table.  The table grows at collect,
 * between batches: when the rescued records of the batches in flight find no room in the table as it stands, they are counted in `dropped`
 * and groot_hip_acov_export fails with GROOT_E_NOSPACE until groot_hip_acov_reset: start the table larger (min_slots).  No read is dropped
 * silently.  Off by default: then no allocation, launch or sync, and every kernel launched is the one launched without this feature. */
#define GROOT_RESCUE_ACOV_BYTES (8ull << 20)   /* per pipeline slot: the log (16 bytes a placement) of the kept placements of a batch's rescued reads in more than 4 graphs */
typedef struct groot_rescue_acov_stats {
    uint64_t records;       /* rescued records added to the table since enable / groot_hip_acov_reset, the host's among them */
    uint64_t host_records;  /* those of reads whose set lies in more than 4 graphs (1 under GROOT_TEST_SHARED_SLOW): folded on the host from the log */
    uint64_t dropped;       /* rescued records that found no room in the table: groot_hip_acov_export fails while this is not 0 */
    uint64_t log_rows;      /* log entries per batch: GROOT_RESCUE_ACOV_BYTES / 16, or GROOT_TEST_RESCUE_ACOV_LOG; 0 while off */
    uint64_t launches;      /* kernels launched for it since open, whether it is on now or not; the two that take the place of a kernel of the
                               rescued reads in the classes count in groot_rescue_ec_stats.launches */
} groot_rescue_acov_stats;
/* on != 0: on.  Needs mismatch rescue, equivalence classes and assigned coverage on (GROOT_E_STATE otherwise, with the reason), and
 * nothing in flight (GROOT_E_STATE); GROOT_E_UNSUPPORTED beside pairing.  It switches the rescued reads in the equivalence classes on
 * itself: the one way in which they and assigned coverage run together (groot_hip_rescue_ec_enable and groot_hip_acov_enable keep refusing
 * each other).  min_slots: 0, or a power of two (GROOT_E_INVALID otherwise): the table is grown to at least that many slots, also when the
 * feature is on already (it counts among groot_hip_acov_stats' grows).  on == 0 switches it and the rescued reads in the classes off;
 * so does switching mismatch rescue, the equivalence classes, the rescued reads in them or assigned coverage off.
 * groot_hip_acov_reset and groot_hip_ec_reset (which calls it) zero the table, the rescued records in it, `dropped` and these stats.
 * groot_hip_rescue_enable with another M and groot_hip_rescue_reset leave the table alone, as they leave the classes alone.
 * A batch whose rescued reads in more than 4 graphs have more kept placements than `log_rows` fails at collect with GROOT_E_NOSPACE (the
 * message names GROOT_TEST_RESCUE_ACOV_LOG).  groot_hip_acov_export / _stats then count the rescued records too (records, tuples);
 * slow_records there stays the exact records.  Device memory: 4 bytes per read of a batch, `log_rows` entries per pipeline slot. */
int groot_hip_rescue_acov_enable(groot_ctx *ctx, int on, uint64_t min_slots);
/* Waits for everything in flight; zeros while off, but for launches. */
int groot_hip_rescue_acov_stats(groot_ctx *ctx, groot_rescue_acov_stats *out);

/* ---- rescued mates in assigned coverage over fragments -----------------------------------------------------------------------
 * "Rescued reads in assigned coverage" is unpaired, "assigned coverage over fragments" knows exact records only, and "rescued mates in
 * paired-end units" refuses assigned coverage: its pileup had no rule for a fragment with a rescued mate.  This is the rule
 * (kernels_rescue_acov_pairs.hpp):
 *
 *   S(r), R(r), S+(r), candidate, rescued, d*, kept placement (p, strand, x), X, len: exactly as in "mismatch rescue" and "rescued reads in the
 *   equivalence classes".  Fragments, A = S+(r_2i), B = S+(r_2i+1), joined / split / single / none, units, ECs over units: exactly as in
 *   "rescued mates in paired-end units" (DESIGN §25).  Canonical order, alpha, w(e,p): as for --abundance over those ECs.
 *   U(r), the UNIT SET of a mate r with S+(r) non-empty:   A n B when r's fragment is joined (both mates the same set);  S+(r) when split or single.
 *   An exact record of r on p COUNTS when p is in U(r), covering [Pos, min(Pos + M, path_len(p) - 1)]           (§13 / §24's interval, unchanged).
 *   A kept placement (p, strand, x) of a rescued mate r COUNTS when p is in U(r), as one rescued record covering [X, X + len - 1]   (§19's interval).
 *   A record or placement on a path outside U(r) is LEFT OUT (w(e,p) is defined for p in e only).  Every counting one counts once: both mates,
 *   both strands, every x, several on one path, primary and secondary.  The two interval rules are not made alike.
 *   The table is the multiset of counting exact AND rescued records grouped by (e = EC of U(r), p, Pos, last): n(e,p,Pos,last), integers.
 *   A mate placed only with a gap, left unplaced, too short or with a non-ACGT base has the empty set and no record, as in §25.
 *   A pass that collect redoes counts once; a batch under kCovSkipFlags counts nothing; a batch that fails counts nothing anywhere.
 *   The table depends on the reads, their pairing and the index alone: not on batch size, pipeline depth, align stage, --ctxPerGpu or --gpus.
 *
 * So with no rescued mate in the run the table and the classes are those of assigned coverage over fragments; with split and single
 * fragments only they are those of the unpaired run with the rescued reads in assigned coverage; fragments (r, r) give that run's classes
 * with every n doubled.  The exact records whose filter needs exact records only (both mates exact; an exact mate that ends split or single)
 * are claimed and added by the ordinary count, which collect may repeat.  The kept placements, and the exact records of a mate joined
 * with a rescued partner, are filtered by a unit row that lives one batch long: they are claimed and added in one pass over the whole
 * table behind the batch's merge, and what finds no room is counted in `dropped`, on which groot_hip_acov_export fails with
 * GROOT_E_NOSPACE until groot_hip_acov_reset: start the table larger (min_slots).  A fragment on bitmaps (a mate in more than 4 graphs, 1
 * under GROOT_TEST_SHARED_SLOW) has no serial on the device: its records of both kinds come back in the slot's log as (bitmap row, p, Pos,
 * last) and are folded on the host at collect under the ID list of the unit's bitmap -- p in the list, or left out. */
typedef struct groot_rescue_acov_pairs_stats {
    uint64_t exact_records, exact_left_out;       /* exact records of a mate joined with a rescued partner, and of the exact mates of fragments on bitmaps: counted / left out */
    uint64_t rescued_records, rescued_left_out;   /* kept placements of rescued mates in a unit: counted as rescued records / left out */
    uint64_t host_records;  /* those of exact_records + rescued_records folded on the host from the log */
    uint64_t dropped;       /* records of either kind that found no room in the table: groot_hip_acov_export fails while this is not 0 */
    uint64_t log_rows;      /* log entries per batch: GROOT_RESCUE_ACOV_BYTES / 16, or GROOT_TEST_RESCUE_ACOV_LOG; 0 while off */
    uint64_t launches;      /* the three kernels behind the merge since open, whether the rule is on now or not; the two that take the place of
                               kernels of the rescued mates' rule count in groot_rescue_pairs_stats.launches */
} groot_rescue_acov_pairs_stats;
/* on != 0: puts the ctx into the rule above -- switches on whichever of the classes, pairing, the rescued classes, the rescued mates' rule,
 * assigned coverage and assigned coverage over fragments is off, then the rule; the unpaired "rescued reads in assigned coverage" goes
 * off if it was on (the rescued classes stay).  Needs mismatch rescue on (GROOT_E_STATE, with the reason) and nothing in flight
 * (GROOT_E_STATE).  min_slots: 0, or a power of two (GROOT_E_INVALID otherwise): the table is grown to at least that many slots, also when
 * the rule is on already.  GROOT_E_UNSUPPORTED, from whichever enable comes second, beside shared reads, assignment, and the gap-placed reads
 * in the classes or the pileup.  While the rule is off every other refusal is what it was, and no state has the rescued mates' rule and
 * assigned coverage both on without this rule.
 * on == 0: the rule, assigned coverage (with its rule over fragments) and the rescued records go; the classes, pairing, the rescued classes
 * and the rescued mates' rule stay.  groot_hip_acov_enable(ctx, 0) and groot_hip_acov_pairs_enable(ctx, 0) do the same.  Switching the
 * rescued mates' rule, the rescued classes, the classes, pairing or mismatch rescue off takes this rule with it (and leaves what that
 * call leaves otherwise: assigned coverage over fragments stays where pairing and the classes do).
 * groot_hip_acov_reset and groot_hip_ec_reset (which calls it) zero the table, `dropped` and these stats and leave the rule on, as they do
 * for the rescued reads in assigned coverage and for assigned coverage over fragments; groot_hip_rescue_reset leaves the table alone.
 * A batch whose fragments on bitmaps have more records than `log_rows`, or need more bitmaps than groot_rescue_ec_stats.rows, fails at collect
 * with GROOT_E_NOSPACE (the message names GROOT_TEST_RESCUE_ACOV_LOG / GROOT_TEST_RESCUE_EC_ROWS) and counts NOTHING in the classes, the
 * table or any stat.  groot_acov_pairs_stats.left_out stays the exact + exact fragments' count.  Device memory: 5 bytes per read of a
 * batch, `log_rows` entries per pipeline slot. */
int groot_hip_rescue_acov_pairs_enable(groot_ctx *ctx, int on, uint64_t min_slots);
/* Since the rule came on / groot_hip_acov_reset; zeros while it is off, but for launches.  Waits for everything in flight. */
int groot_hip_rescue_acov_pairs_stats(groot_ctx *ctx, groot_rescue_acov_pairs_stats *out);

/* ---- rescued records -------------------------------------------------------------------------------------------------------
 * Mismatch rescue piles its placements up in tables; the placements themselves are gone when the batch is.  With this on, every batch
 * also hands out one record per kept placement of its rescued reads: what a BAM record of the read needs.  The definition, integers only:
 *
 *   Candidate, placement (p, strand, x), d*(r), RESCUED, KEPT placement, path coordinate X = first Position of p + x: exactly as in
 *   "mismatch rescue".
 *   A RESCUED RECORD is one kept placement of a rescued read:
 *       read   = position of r in its batch
 *       path   = global path p
 *       pos    = X (0-based, the coordinate an exact record's Pos uses)
 *       strand = 0 / 1
 *       d      = d*(r)
 *       mm[3]  = the offsets i, ascending, in the ORIENTED read (the read for strand 0, its reverse complement for strand 1)
 *                with oriented[i] != text_p[x + i]; the d first entries are set, the rest are 0xFFFF.
 *   The rescued records of a batch are ALL kept placements of ALL its rescued reads (every path, both strands, every x, several on one
 *   path), each once, in ascending (read, path, strand, pos) order.
 *   A pass that collect redoes yields the records of its redo, once.  A batch under kCovSkipFlags (one that fails with GROOT_E_NOSPACE)
 *   yields none.  Gap-placed reads (gapped rescue) yield none, unless the gapped records below are on:
 *   then they yield those, in a list of their own.
 *   The list depends on the reads and the index alone: not on batch size, pipeline depth, align stage, results_on_device or the number
 *   of ctxs (cut a batch in pieces and the pieces' lists, with batch-relative `read`, concatenate to the batch's).
 *
 * On the device (kernels_rescue_rec.hpp): the count kernel of rescue also leaves every read's number of kept placements, an exclusive
 * scan over the batch's reads gives every read its segment, and rescue_rec_emit_kernel -- one thread per rescued read -- walks the
 * read's kept placements once more, writes them and sorts its segment.  The records live in a buffer of the pipeline slot and are copied
 * into pinned host memory at collect, as many as the batch has.  Rescue's tables and stats and every other counter stay what they are.
 * Off by default: then no allocation, launch or sync, and rescue_count_kernel is the one it is without this section. */
/* groot_rescue_record (20 bytes: read, path, pos, mm[3], strand, d) is declared in groot_host.h, beside the writer that takes it */
typedef struct groot_rescue_rec_stats {
    uint64_t records;     /* records handed out (of collected batches that did not fail) since enable */
    uint64_t reads;       /* rescued reads those records belong to */
    uint64_t failed;      /* batches that failed for room */
    uint64_t slots;       /* slots_per_batch (0 while off) */
    uint64_t launches;    /* the scan and rescue_rec_emit_kernel, launched since open, whether it is on now or not (the count kernel
                             counts in groot_rescue_stats.launches) */
} groot_rescue_rec_stats;
/* slots_per_batch > 0: on, with room for that many records per batch in every pipeline slot (a second call with another value
 * reallocates, the stats start over); 0: off, everything freed, nothing launched afterwards.  GROOT_E_STATE when mismatch rescue is off
 * or something is in flight; GROOT_E_UNSUPPORTED while assignment is on, as mismatch rescue itself is, and groot_hip_assign_enable
 * refuses while rescue is on.  groot_hip_rescue_enable(.., 0) switches it off too.  A batch with more records than slots_per_batch fails
 * at collect with GROOT_E_NOSPACE, and the message names slots_per_batch: no record is dropped silently; the batch's other results stay
 * readable, its records do not (groot_hip_rescue_rec_batch gives n = 0), and the next batch is not affected.  Device memory: 13 bytes per
 * read of a batch, and 20 slots_per_batch bytes per pipeline slot; pinned memory: 20 bytes per record of the largest batch so far, per slot. */
int groot_hip_rescue_rec_enable(groot_ctx *ctx, uint64_t slots_per_batch);
/* recs[0 .. *n) of a collected, unreleased batch (ticket 0: the batch groot_hip_wait collected), in pinned host memory that stays valid
 * until the batch is released; with results_on_device as well.  *n = 0 for an empty or a failed batch.  GROOT_E_STATE when the feature
 * was off when the batch was submitted. */
int groot_hip_rescue_rec_batch(groot_ctx *ctx, uint64_t ticket, const groot_rescue_record **recs, uint64_t *n);
/* Zeros while off, but for launches.  Counts collected batches only; does not wait. */
int groot_hip_rescue_rec_stats(groot_ctx *ctx, groot_rescue_rec_stats *out);

/* ---- gapped records --------------------------------------------------------------------------------------------------------
 * Gapped rescue adds its placements to gdepth and the event table; the placements themselves are gone when the batch is.  With this on,
 * every batch also hands out one record per kept gapped placement of its gap-rescued reads: what a BAM record with an I or D CIGAR
 * needs.  The definition, integers only:
 *
 *   Gap candidate, gapped placement (p, strand, x, type, g, k), d, k*, e = d + g, e*(r), GAP-RESCUED, KEPT gapped placement, oriented read R,
 *   T = text_p, path coordinate X = first Position of p + x: exactly as in "gapped rescue".
 *   A GAPPED RECORD is one kept gapped placement of a gap-rescued read:
 *       read   = position of r in its batch          path = global path p          pos = X (0-based, as an exact record's Pos)
 *       k      = k* (aligned read bases in front of the gap; the gap is left-aligned as the definition has it)
 *       strand = 0 / 1      d = its mismatches (<= M <= 3)      type = GROOT_GAP_DEL / GROOT_GAP_INS      g = 1..8
 *       mm[3]  = the offsets i, ascending, in the ORIENTED read at which an ALIGNED read base differs from the text base it lies on:
 *                i < k:  R[i] != T[x+i];    DEL, i >= k:  R[i] != T[x+g+i];    INS, i >= k+g:  R[i] != T[x+i-g].
 *                The inserted bases R[k, k+g) are never listed.  The d first entries are set, the rest are 0xFFFF.
 *   The gapped records of a batch are ALL kept gapped placements of ALL its gap-rescued reads, each (p, strand, x, type, g) once, in
 *   ascending (read, path, strand, pos, type, g) order.  (A read has rescued records or gapped records, never both: a gap candidate is
 *   not rescued.)
 *   A pass that collect redoes yields the records of its redo, once.  A batch under kCovSkipFlags yields none.
 *   The list depends on the reads and the index alone: not on batch size, pipeline depth, align stage, results_on_device or the number
 *   of ctxs (cut a batch in pieces and the pieces' lists, with batch-relative `read`, concatenate to the batch's).
 *
 * On the device (kernels_gap_rec.hpp): rescue_gap_rec_kernel -- rescue_gap_kernel's body with a sink -- also leaves every read's number
 * of kept gapped placements and every gap candidate's e*, an exclusive scan over the batch's reads gives every read its segment, and
 * gap_rec_emit_kernel -- one thread per gap-rescued read -- walks sweep 2 once more at e*, writes the placements and sorts its segment.
 * The records live in a buffer of the pipeline slot and are copied into pinned host memory at collect, as many as the batch has.
 * gdepth, the events, the stats and every other counter stay what they are.  Independent of the rescued records above: either, both or
 * neither may be on.  Off by default: then no allocation, launch or sync, and rescue_gap_kernel is the one it is without this section. */
/* groot_gap_record (24 bytes: read, path, pos, k, mm[3], strand, d, type, g) is declared in groot_host.h, beside the writer that takes it */
typedef struct groot_gap_rec_stats {
    uint64_t records;     /* records handed out (of collected batches that did not fail) since enable */
    uint64_t reads;       /* gap-rescued reads those records belong to */
    uint64_t failed;      /* batches that failed for room */
    uint64_t slots;       /* slots_per_batch (0 while off) */
    uint64_t launches;    /* the scan and gap_rec_emit_kernel, launched since open, whether it is on now or not (rescue_gap_rec_kernel
                             counts in groot_gap_stats.launches) */
} groot_gap_rec_stats;
/* slots_per_batch > 0: on, with room for that many records per batch in every pipeline slot (a second call with another value
 * reallocates, the stats start over); 0: off, everything freed, nothing launched afterwards.  GROOT_E_STATE when gapped rescue is off or
 * something is in flight; beyond 2^40 bytes GROOT_E_INVALID.  groot_hip_gap_enable(.., 0, ..) and groot_hip_rescue_enable(.., 0) switch
 * it off too; another G, another M or a reset leaves it on.  A batch with more records than slots_per_batch fails at collect with
 * GROOT_E_NOSPACE, and the message names slots_per_batch: no record is dropped silently; the batch's other results stay readable, the
 * rescued records included, its gapped records do not (groot_hip_gap_rec_batch gives n = 0), and the next batch is not affected.  Device
 * memory: 13 bytes per read of a batch, and 24 slots_per_batch bytes per pipeline slot; pinned memory: 24 bytes per record of the largest
 * batch so far, per slot. */
int groot_hip_gap_rec_enable(groot_ctx *ctx, uint64_t slots_per_batch);
/* recs[0 .. *n) of a collected, unreleased batch (ticket 0: the batch groot_hip_wait collected), in pinned host memory that stays valid
 * until the batch is released; with results_on_device as well.  *n = 0 for an empty or a failed batch.  GROOT_E_STATE when the feature
 * was off when the batch was submitted. */
int groot_hip_gap_rec_batch(groot_ctx *ctx, uint64_t ticket, const groot_gap_record **recs, uint64_t *n);
/* Zeros while off, but for launches.  Counts collected batches only; does not wait. */
int groot_hip_gap_rec_stats(groot_ctx *ctx, groot_gap_rec_stats *out);

/* ---- gap-placed reads in the equivalence classes ---------------------------------------------------------------------------
 * The rescued reads in the classes stop at the reads mismatch rescue places.  A read that lies across a frameshift, or across a codon
 * deletion or insertion, is placed by gapped rescue, and is in no class.  With this on, it is a unit of the classes with the set of
 * paths it was gap-placed on.  The definition:
 *
 *   S(r), R(r), S+(r): as in "rescued reads in the equivalence classes".  Gap candidate, kept gapped placement (p, strand, x, type, g, k*), e*:
 *   as in "gapped rescue".
 *   G(r)    for a read r that is GAP-RESCUED (a gap candidate with a kept gapped placement, e*(r) <= M + G): the set of global paths p for
 *           which r has a kept gapped placement -- any strand, x, type, g; each p once.  Not defined for any other read.
 *   S++(r)  = S(r) when r has a record;  R(r) when r is rescued ungapped;  G(r) when r is gap-rescued;  empty otherwise.
 *           (The three exclude each other: a candidate has no record, and a gap candidate is a candidate that ended unplaced.)
 *   With the feature on the run's ECs are the distinct non-empty S++(r) with their read counts.  Reads of the three kinds with the same set
 *   are one EC.
 *
 * A candidate that is rescued ungapped stays in R(r), even where a gapped placement would cost less (the rule of "gapped rescue").
 * Nothing else changes: records, BAMs, coverage, shared reads, the rescue and gap tables, events, and every stat that exists today keep
 * their values.  The ECs depend on the reads and the index alone: not on batch size, pipeline depth, align-stage variant,
 * results_on_device, or how the reads are spread over ctxs.  A pass that collect redoes counts once, a batch under the skip flags of
 * report coverage adds nothing.  Off by default: then no allocation, launch or sync, and the gap kernel is the one it is without this
 * section. */
typedef struct groot_gap_ec_stats {
    uint64_t reads;       /* gap-rescued reads added to the classes since enable / groot_hip_ec_reset */
    uint64_t slow_reads;  /* those among them whose set lies in more than 4 graphs (1 under GROOT_TEST_SHARED_SLOW): folded on the host from
                             bitmaps of the pool of groot_rescue_ec_stats.rows; groot_rescue_ec_stats.slow_reads stays the ungapped reads' alone */
    uint64_t launches;    /* gap_ec_slow_kernel and gap_ec_insert_kernel, launched since open, whether it is on now or not (rescue_gap_ec_kernel
                             counts in groot_gap_stats.launches) */
} groot_gap_ec_stats;
/* on != 0: on.  Needs gapped rescue and the rescued reads in the equivalence classes on (GROOT_E_STATE otherwise), and nothing in flight
 * (GROOT_E_STATE).  GROOT_E_UNSUPPORTED beside the rescued reads in assigned coverage, from whichever enable comes second: the pileup has
 * no rule for a gapped record, and a DEL covers two intervals (groot_hip_gap_acov_enable, below, is that rule and switches both on together).
 * groot_hip_gap_enable(.., 0, ..), groot_hip_rescue_ec_enable(.., 0),
 * mismatch rescue off and the equivalence classes off switch it off too; another G or another M leaves the classes alone;
 * groot_hip_ec_reset zeroes these stats with the classes.  The rescued and the gap-rescued reads of a batch in more than 4 graphs share
 * the slot's `rows` bitmaps: more of them together fail the batch at collect with GROOT_E_NOSPACE (the message names
 * GROOT_TEST_RESCUE_EC_ROWS).  Device memory: 1 byte per read of a batch. */
int groot_hip_gap_ec_enable(groot_ctx *ctx, int on);
/* Waits for everything in flight; zeros while off, but for launches. */
int groot_hip_gap_ec_stats(groot_ctx *ctx, groot_gap_ec_stats *out);

/* ---- gap-placed reads in assigned coverage -------------------------------------------------------------------------------
 * The gap-placed reads in the classes vote in the EM, and the rescued reads in assigned coverage stop at the reads mismatch rescue
 * places: a read placed with a deletion or an insertion is piled up nowhere, and the calls file has a hole of a read length on each side
 * of an indel the sample carries against every indexed allele.  With this on, every kept gapped placement is piled up on the text bases
 * gdepth grows on for it.  The definition:
 *
 *   S(r), R(r), G(r), S++(r), gap candidate, kept gapped placement (p, strand, x, type, g, k*), e*, X = first Position of p + x, len:
 *   exactly as in "gapped rescue" and "gap-placed reads in the equivalence classes".  ECs, canonical order, alpha, w(e,p): exactly as for
 *   --abundance --abundanceRescued --abundanceGapped (the run's ECs are the distinct non-empty S++(r)).
 *   A kept gapped placement of a gap-rescued read r is
 *      type DEL:  TWO gapped records of r on p, covering [X, X + k* - 1] and [X + k* + g, X + len + g - 1]
 *      type INS:  ONE gapped record of r on p, covering [X, X + len - g - 1]
 *   both ends included: the text bases on which gdepth grows for that placement.  The g deleted text bases of a DEL are covered by neither
 *   record (the pileup shows the deletion as the hole it is); the g inserted read bases of an INS cover nothing.  Every kept gapped placement
 *   counts: every path, both strands, every x, both types, every g, each (p, strand, x, type, g) once.
 *   The assigned-coverage table of a run with the feature on is the multiset of exact records, rescued records AND gapped records
 *   grouped by (e = EC of S++(r), p, Pos, last): n(e, p, Pos, last).  Everything computed from the table and the ECs (d_e[x], D_p[x], depth,
 *   breadth, cigar, called, --callSupport's and --rarefy's columns) is computed by the existing host and device functions, unchanged.
 *   A read that is rescued ungapped keeps its rescued records even where a gapped placement would cost less.  A pass that collect redoes counts
 *   once; a batch under kCovSkipFlags counts nothing.  The table depends on the reads and the index alone: not on batch size, pipeline depth,
 *   align stage, results_on_device, --ctxPerGpu or --gpus.
 *
 * Off by default: then no allocation, launch or sync, and every kernel launched is the one launched without this section. */
typedef struct groot_gap_acov_stats {
    uint64_t placements;    /* kept gapped placements piled up since enable / groot_hip_acov_reset, the host's among them */
    uint64_t records;       /* gapped records added (DEL two, INS one): placements + the DEL placements among them */
    uint64_t host_records;  /* those folded on the host from the log (the reads whose set lies in more than 4 graphs, 1 under GROOT_TEST_SHARED_SLOW) */
    uint64_t dropped;       /* gapped records that found no room: groot_hip_acov_export fails while this or groot_rescue_acov_stats.dropped is not 0 */
    uint64_t launches;      /* the four launches it adds to a batch's pass (gap_acov_slow_kernel, gap_ec_insert_kernel, gap_acov_serial_kernel,
                               gap_acov_kernel), since open, whether it is on now or not */
} groot_gap_acov_stats;
/* on != 0: on.  Needs gapped rescue and the rescued reads in assigned coverage on (GROOT_E_STATE otherwise, with the reason), and nothing
 * in flight (GROOT_E_STATE).  It switches the gap-placed reads in the equivalence classes on itself: the one way they and the rescued reads
 * in assigned coverage run together (groot_hip_gap_ec_enable and groot_hip_rescue_acov_enable keep refusing each other).  on == 0: off, and
 * the gap-placed reads in the classes with it; the rescued reads in assigned coverage stay.  It also goes off whenever gapped rescue, the
 * gap-placed classes, the rescued reads in assigned coverage, mismatch rescue, the classes, the rescued classes or assigned coverage goes
 * off.  Another G, another M and the rescue / gap resets leave the table alone; groot_hip_acov_reset (and groot_hip_ec_reset, which calls
 * it) zero these stats and the records.  groot_hip_acov_export / _stats count the gapped records in `records` and `tuples`
 * (slow_records stays the exact records'); groot_hip_gap_ec_stats counts as it does without this.  The log entries of a batch's rescued and
 * gap-rescued reads in more than 4 graphs share the slot's log (groot_rescue_acov_stats.log_rows): more of them together fail the batch at
 * collect with GROOT_E_NOSPACE (the message names GROOT_TEST_RESCUE_ACOV_LOG), before either kind is folded.  A gapped record that finds no
 * room in the table makes groot_hip_acov_export fail with GROOT_E_NOSPACE (min_slots / --callSlots) until groot_hip_acov_reset.
 * Device memory: 4 bytes per read of a batch. */
int groot_hip_gap_acov_enable(groot_ctx *ctx, int on);
/* Waits for everything in flight; zeros while off, but for launches. */
int groot_hip_gap_acov_stats(groot_ctx *ctx, groot_gap_acov_stats *out);

/* ---- bootstrap replicates of the abundance EM -----------------------------------------------------------------------
 * groot_host_em_bootstrap (groot_host.h, "bootstrap intervals": the resampling by splitmix64 draws, groot_host_em per replicate) on
 * the device, bit for bit in boot_count, alpha and iterations.  Quoted from there: draw j (0 <= j < n_draws; n_draws = 0 means N, the sum
 * of count) of replicate b, modulo 2^64,
 *     z = seed + (b * n_draws + j + 1) * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31);  t = high 64 bits of z * N;
 *     boot_count[b][e] += 1 for the EC e with cum[e] <= t < cum[e+1]   (cum = the running sum of count; count 0 is never drawn),
 * then alpha[b] = groot_host_em(n_paths, n_ec, off, ids, boot_count[b], min_iter, max_iter), iterations[b] its rounds.
 * Needs no ctx: it runs on the device with that ordinal, on a stream and in buffers of its own that are freed on return, and may be
 * called while ctxs have batches in flight.  The replicates are processed in chunks that bound the device memory taken; the draws
 * are one kernel (a thread per draw), the EM runs one workgroup per replicate, as many at a time as the device has compute units
 * (kernels_boot.hpp).  ECs in the order given (canonical order for the abundance file: groot_host_ecs_canonical).
 * boot_count[n_boot][n_ec] and iterations[n_boot] may be NULL; alpha[n_boot][n_paths].  GROOT_E_INVALID as groot_host_em_bootstrap
 * (n_boot = 0; N = 0 with n_ec > 0; the EM's errors), GROOT_E_UNSUPPORTED at 2^32 - 1 ECs or listed IDs and more, GROOT_E_DEVICE
 * without that HIP device; the message is groot_hip_last_error(NULL). */
int groot_hip_em_bootstrap(int device, uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                           uint32_t n_boot, uint64_t seed, uint64_t n_draws, uint32_t min_iter, uint32_t max_iter, uint64_t *boot_count,
                           double *alpha, uint32_t *iterations);

/* ---- rarefaction: nested subsamples without replacement, the EM at every depth ---------------------------------------------------
 * groot_host_em_rarefy (groot_host.h, "rarefaction curves") on the device, bit for bit in rare_count, alpha and iterations.  Quoted
 * from there:
 *
 * Input: canonical ECs (off, ids, count; groot_host_ecs_canonical), cum[0] = 0, cum[e+1] = cum[e] + count[e], N = cum[n_ec], 1 <= N < 2^62;
 * R >= 1 replicates; a 64-bit seed; n_depths >= 1 depths m[0] <= m[1] <= .. with 1 <= m[d] <= N.
 * Unit i (0 <= i < N) belongs to the EC e with cum[e] <= i < cum[e+1] (an EC with count 0 owns no unit).
 * sm(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)      (mod 2^64; the
 *         mixing steps of the bootstrap's draw)
 * h   = the smallest integer >= 1 with 2^(2h) >= N;  mask = 2^h - 1                       (domain 2^(2h) < 4 N for N > 4)
 * k_b = sm(seed + (b + 1) * 0x9E3779B97F4A7C15)
 * pi_b(j), 0 <= j < N:   x = j
 *     repeat:  L = x >> h;  Rr = x & mask
 *              for t = 0 .. 5:  F = sm(k_b + (((t << 32) | Rr) + 1) * 0x9E3779B97F4A7C15) >> (64 - h);   (L, Rr) = (Rr, L ^ F)
 *              x = (L << h) | Rr
 *     until x < N                                   (cycle walking: a Feistel network is a bijection of [0, 2^(2h)), so pi_b is a
 *                                                    bijection of [0, N) and the loop ends)
 * rare_count[b][d][e] = the number of j < m[d] with pi_b(j) in EC e.
 *
 * then alpha[b][d] = groot_host_em(n_paths, n_ec, off, ids, rare_count[b][d], min_iter, max_iter), iterations[b][d] its rounds.
 * Needs no ctx: like groot_hip_em_bootstrap it runs on the device with that ordinal, on a stream and in buffers of its own that are
 * freed on return, and may be called while ctxs have batches in flight.  On the device (kernels_rare.hpp): rare_draw_kernel, a thread
 * per draw j, one grid row per (replicate, depth interval [m[d-1], m[d])), counts the interval's units into the row's increments;
 * rare_cumsum_kernel adds the increments along the depths; boot_em_kernel then fits the n_rep * n_depths count vectors, one workgroup
 * each.  Replicates go in chunks that bound the device memory taken, as for the bootstrap; the result does not depend on them.
 * rare_count[n_rep][n_depths][n_ec] and iterations[n_rep][n_depths] may be NULL; alpha[n_rep][n_depths][n_paths].  GROOT_E_INVALID as
 * groot_host_em_rarefy (n_rep = 0; n_depths = 0; a depth of 0 or above N; depths that descend; N = 0; the EM's errors);
 * GROOT_E_UNSUPPORTED at N >= 2^62, at 2^32 - 1 ECs or listed IDs and more, above 65 535 depths or 4 GiB for one replicate's depths;
 * GROOT_E_DEVICE without that HIP device; the message is groot_hip_last_error(NULL). */
int groot_hip_em_rarefy(int device, uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t n_rep,
                        uint32_t n_depths, const uint64_t *depths, uint64_t seed, uint32_t min_iter, uint32_t max_iter, uint64_t *rare_count,
                        double *alpha, uint32_t *iterations);

/* ---- bootstrap support for the calls: per-replicate breadth ------------------------------------------------------------------
 * groot_host_call_support (groot_host.h, "bootstrap support for the calls") on the device, covered_out as u32 bit for bit.  Quoted
 * from there:
 *
 *   Inputs: canonical ECs (off, ids, count; count[e] > 0), the assigned-coverage table n(e,p,Pos,last), B >= 1 replicates:
 *   boot_count[b][e] and alpha_b[n_paths] exactly as groot_host_em_bootstrap / groot_hip_em_bootstrap return them, callDepth, covCutoff.
 *   d_e[x] for p in e: the number of records of (e,p,.,.) covering base x of p -- integers, as in §13.
 *   For replicate b, EC e and p in e.  Double precision, no FMA contraction.
 *       denom_b(e) = 0.0; denom_b(e) = denom_b(e) + alpha_b[q], q over e in ascending ID order
 *       w_b(e,p)   = alpha_b[p] / denom_b(e);  0.0 when boot_count[b][e] == 0 or denom_b(e) < 2^-52 (the EM's skip)
 *       s_b(e)     = (double)boot_count[b][e] / (double)count[e]            (one correctly rounded division)
 *       f_b(e,p)   = s_b(e) * w_b(e,p)                                      (one product)
 *       D_p^b[x]   = 0.0; D = D + (double)d_e[x] * f_b(e,p), over the ECs that hold p, in canonical EC order
 *       covered_b[p] = the number of x in [0, path_len(p)) with D_p^b[x] >= callDepth                       (u32: the only thing the device returns)
 *       called_b[p]  = ((double)covered_b[p] / (double)path_len(p) >= covCutoff), the writer's own expression; path_len 0: breadth 0.0
 *   Per path over b = 0 .. B-1:   support = (double)(number of b with called_b[p]) / (double)B
 *       v = covered_b[p] sorted ascending (integers), q = (25 * (B - 1)) / 1000 in integers (§11's rule)
 *       breadth_lo = (double)v[q] / (double)path_len,  breadth_hi = (double)v[B-1-q] / (double)path_len
 *   File: every line of the calls file gets three more tab-separated columns, "support (%.3f) \t breadth_lo (%.4f) \t breadth_hi (%.4f)"; the
 *   lines, their order and their first seven columns are the calls file's, byte for byte.
 *
 * Needs no ctx: like groot_hip_em_bootstrap it runs on the device with that ordinal, on a stream and in buffers of its own that are
 * freed on return, and may be called while ctxs have batches in flight.  Once, on the host: the tuples grouped by (e, p) into dense
 * rows of path_len + 1 integers, rows of a path in canonical EC order.  On the device (kernels_csup.hpp): csup_fill_kernel adds
 * +n at Pos and -n at last + 1 with integer atomics (u32 while every row's record sum is below 2^32, u64 otherwise or under
 * GROOT_TEST_CSUP_WIDE=1) and csup_scan_kernel turns each row into d_e[x]; csup_weight_kernel computes f_b per (replicate, EC);
 * csup_cover_kernel adds a path's rows in order for 8 replicates at a time and counts the covered bases.  Paths go in chunks of at
 * most 1 GiB of rows (GROOT_TEST_CSUP_BYTES=<n> sets the budget; a path is never split), replicates in chunks as for the
 * bootstrap; the result depends on neither.  Arguments and GROOT_E_INVALID as groot_host_call_support (no threads);
 * GROOT_E_UNSUPPORTED at 2^32 - 1 listed IDs, rows or tuples and more; GROOT_E_DEVICE without that HIP device; the message is
 * groot_hip_last_error(NULL). */
int groot_hip_call_support(int device, uint32_t n_paths, const uint32_t *path_len, uint64_t n_ec, const uint64_t *off, const uint32_t *ids,
                           const uint64_t *count, uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, uint32_t n_boot, const uint64_t *boot_count,
                           const double *alpha, double call_depth, uint32_t n_sel, const uint32_t *sel_paths, uint32_t *covered_out);
/* What the last groot_hip_call_support of this thread did (for logs and probes): rows, bytes per integer (4 or 8), path chunks. */
void groot_hip_call_support_info(uint64_t *rows, uint32_t *width, uint32_t *chunks);

/* Fine-grained mirror of Sequence.RunMinHash(k, s, false, nil) (seqio.go:40-68) for a batch of
 * sequences in host memory: out[i*s .. (i+1)*s) = KHF sketch of sequence i.  Only while nothing is in flight. */
int groot_hip_sketch(groot_ctx *ctx, const uint8_t *seq_concat, const uint64_t *seq_off, uint32_t n, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif
