/*
 * groot_host.h -- C ABI of libgroot_host.so: the host-side (no GPU) pieces either side of the
 * `groot align` hot path.  Plain C types only, so that a cgo / ctypes binding is a direct
 * transliteration (INTEGRATION.md shows the cgo stub).
 *
 *   index side   : what `groot index` produces and `groot align` loads
 *                  (cmd/index.go:57-133, src/pipeline/index.go:37-211, src/graph/graph.go:37-396)
 *   output side  : graph weighting / pruning / GFA + BAM writing after the device path returns
 *                  (src/graph/graph.go:401-525, src/graph/graphio.go:19-154, src/pipeline/boss.go:45-105)
 *
 * Every function returns 0 on success or a negative GROOT_E_* code; groot_host_last_error() gives
 * the message for the calling thread.
 */
#ifndef GROOT_HOST_H
#define GROOT_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "groot_index.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GROOT_OK 0
#define GROOT_E_INVALID (-1)   /* bad argument                                                    */
#define GROOT_E_IO (-2)        /* file could not be read / written                                */
#define GROOT_E_FORMAT (-3)    /* malformed MSA / GFA / FASTQ / index file                        */
#define GROOT_E_NOMEM (-4)
#define GROOT_E_DEVICE (-5)    /* HIP runtime error (device library only)                         */
#define GROOT_E_NOSPACE (-6)   /* caller buffer too small; the needed size is reported            */
#define GROOT_E_SHORT_READ (-7) /* read shorter than k: the reference panics (boss.go:164-166)    */
#define GROOT_E_REVCOMP (-8)   /* read byte > 'T' reached RevComplement: reference panics (seqio.go:126) */
#define GROOT_E_STATE (-9)     /* call sequence error (collect without submit, ...)               */
#define GROOT_E_UNSUPPORTED (-10)

typedef struct groot_index groot_index; /* owning handle; groot_index_view() borrows from it */

const char *groot_host_last_error(void);
/* CPUs this process may really use = min(affinity mask, cgroup CPU quota), or $GROOT_THREADS: what "0 = all cores"
 * means throughout this library (a container may show 256 hardware threads and grant 16) */
uint32_t groot_host_usable_cpus(void);
const char *groot_host_version(void); /* "1.1.2": must equal Info.Version (cmd/align.go:96) */

/* ---- index: `groot index` (cmd/index.go:44-52 defaults k=31 s=21 w=100 x=8 y=4) ---------------- */
typedef struct groot_index_params {
    uint32_t kmer_size;       /* -k */
    uint32_t sketch_size;     /* -s */
    uint32_t window_size;     /* -w */
    uint32_t num_part;        /* -x */
    uint32_t max_k;           /* -y */
    uint32_t max_sketch_span; /* --maxSketchSpan (never enforced by the reference: graph.go:33,225) */
    uint32_t n_threads;       /* -p ; 0 = all cores */
    uint32_t reserved;
} groot_index_params;

void groot_index_params_default(groot_index_params *p);

/* MSAconverter + GraphSketcher + SketchIndexer (src/pipeline/index.go:37-211) over every
 * cluster*.msa in msa_dir, graph ids = position in the lexically sorted file list
 * (filepath.Glob, cmd/index.go:143). */
int groot_index_build_msa_dir(const char *msa_dir, const groot_index_params *p, groot_index **out);
/* Same, with the window sketches (Sequence.RunMinHash on every path window, graph.go:292-296) computed by a
 * caller-supplied batch function -- e.g. groot_hip_sketch, which makes `groot index` sketch on the GPU while this
 * library stays free of device code.  fn gets n sequences (seq_off has n+1 entries) and fills out[n*sketch_size];
 * it is called from one thread at a time and returns 0 on success. */
typedef int (*groot_sketch_fn)(void *user, const uint8_t *seq_concat, const uint64_t *seq_off, uint32_t n, uint64_t *out);
int groot_index_build_msa_dir_with(const char *msa_dir, const groot_index_params *p, groot_sketch_fn fn, void *user,
                                   groot_index **out);
int groot_index_build_msa_files(const char *const *files, uint32_t n_files, const groot_index_params *p,
                                groot_index **out);
/* same pipeline starting from GFA files (graph.LoadGFA + CreateGrootGraph, graphio.go:115-138,
 * graph.go:37-147); used with the reference's src/graph/test.gfa fixture */
int groot_index_build_gfa_files(const char *const *files, uint32_t n_files, const groot_index_params *p,
                                groot_index **out);
int groot_index_save(const groot_index *idx, const char *path);   /* flat little-endian .gidx file */
int groot_index_load(const char *path, groot_index **out);
/* replaces Info.Load + ContainmentIndex.Load (src/pipeline/runtime.go:75-91, src/lshe/lshe.go:95-120; called at
 * cmd/align.go:93-107): reads an index directory written by the reference's `groot index` -- the Go encoding/gob
 * streams <dir>/groot.gg (pipeline.Info incl. graph.Store) and <dir>/groot.lshe (lshe.ContainmentIndex with its
 * WindowLookup map) -- into the flat index.  Window ids are assigned in the canonical order (GraphID, Key.Node,
 * Key.OffSet, the "-<i>" suffix of the WindowLookup key, src/pipeline/index.go:195-203).  GROOT_E_FORMAT for a stream
 * that does not decode or whose cross references do not resolve. */
int groot_index_load_gob(const char *gg_path, const char *lshe_path, groot_index **out);
/* the reverse: Info.Dump + ContainmentIndex.Dump (src/pipeline/runtime.go:64-72, src/lshe/lshe.go:71-92; cmd/index.go:96-106,
 * 130-131) -- writes <dir>/groot.gg and <dir>/groot.lshe with the fields `groot index` sets, so that the reference's own
 * subcommands can load an index built here.  The directory must exist. */
int groot_index_save_gob(const groot_index *idx, const char *dir, uint32_t max_sketch_span);
/* renders every top-level value of a gob stream as JSON text (structs as objects holding the fields present on the
 * wire, maps as [[key,value],...]): the decoder behind groot_index_load_gob, exposed for inspection and for the
 * known-answer tests on the byte vectors of the gob documentation.  *needed = bytes incl. the terminating NUL; the
 * text is written only when cap >= *needed. */
int groot_gob_to_json(const uint8_t *data, uint64_t n, char *out, uint64_t cap, uint64_t *needed);
void groot_index_get_view(const groot_index *idx, groot_index_view *view);
/* One O(n) consistency pass over a view (every node / edge / path / window index in range, offset arrays monotone and
 * ending at their payload, path_words wide enough): GROOT_E_FORMAT with the first inconsistency in
 * groot_host_last_error().  groot_index_load / groot_index_load_gob run it on what they read, groot_hip_open runs the
 * same pass on the view it is given before anything is uploaded. */
int groot_index_view_check(const groot_index_view *view);
void groot_index_free(groot_index *idx);

/* fine-grained mirror of Sequence.RunMinHash(k, s, false, nil) (src/seqio/seqio.go:40-68) used by
 * the index builder for graph windows (graph.go:292-296).  Host arithmetic; the align path uses
 * the device kernels in libgroot_hip.so instead. */
int groot_host_window_sketch(const uint8_t *seq, uint32_t len, uint32_t k, uint32_t s, uint64_t *sketch);

/* One successful traversal of performAlignment (alignment.go:162-193) together with the path ids
 * processTraversal (alignment.go:263-317) assigns to it: bit p of mask = local path id p.
 * AlignRead emits one sam.Record per set bit, ascending p, traversals in `ord` order; the record's
 * Pos = Position[p] of `node` + offset.  groot_host_expand_alns() does that expansion. */
typedef struct groot_trav {
    uint32_t read_id;
    uint32_t graph_id;
    uint32_t node;    /* global node index of the first node of the traversal            */
    uint32_t offset;  /* offset in that node where the alignment starts                   */
    uint16_t ord;     /* emission order within the read (graphs ascending, DFS order)     */
    uint8_t  flags;   /* GROOT_TRAV_* */
    uint8_t  reserved;
} groot_trav;
#define GROOT_TRAV_RC 1u          /* read.RC: the reverse complement aligned (sam.Reverse)           */
#define GROOT_TRAV_START_CLIP 2u  /* 1H before the M op (alignment.go:72-85)                          */
#define GROOT_TRAV_END_CLIP 4u    /* 1H after the M op (alignment.go:87-103)                          */
#define GROOT_TRAV_FIRST 8u       /* first traversal of its (read, graph) AlignRead call              */
#define GROOT_TRAV_MAPQ 16u       /* assignment (below): `reserved` holds the MAPQ of the traversal's records */

/* one sam.Record of AlignRead in id form (alignment.go:114-156) */
typedef struct groot_aln {
    uint32_t read_id;
    uint32_t graph_id;
    uint32_t path_id;   /* local path id: record.Ref = references[ID]                      */
    uint32_t ref_id;    /* global path index = position of its @SQ line (graph order)       */
    uint32_t pos;       /* record.Pos, 0-based                                              */
    uint8_t start_clip, end_clip, rc, secondary;
} groot_aln;

/* ---- traversal records -> alignment records ----------------------------------------------------- */
/* For every traversal, ascending set bit p of its mask: one record with Pos = Position[p] of the
 * traversal's first node + offset (alignment.go:296); Secondary on all but the first record of each
 * AlignRead call (alignment.go:147-149).  *n_out = records available; at most cap are written. */
int groot_host_expand_alns(const groot_index_view *idx, const groot_trav *travs, const uint64_t *masks, uint64_t n_trav,
                           groot_aln *out, uint64_t cap, uint64_t *n_out);

/* Path sets as groot_hip_collect hands them out (compact: max(1, ceil(paths of the traversal's graph / 8)) bytes per
 * traversal, back to back) -> path_words words per traversal, the layout groot_host_expand_alns takes. */
int groot_host_unpack_masks(const groot_index_view *idx, const groot_trav *travs, uint64_t n_trav, const uint8_t *compact_masks,
                            uint64_t *masks /*[n_trav * path_words]*/);

/* ---- graph weighting after alignment ------------------------------------------------------------ */
/* Replays GrootGraph.IncrementSubPath (graph.go:401-451) from the exact per-(kmerCount, window)
 * call counts the device accumulated: attempts[q * n_windows + w], q in [0, n_q).  Canonical order:
 * window ascending, kmerCount ascending, one floating-point add per call. */
int groot_host_weights(const groot_index_view *idx, const uint32_t *attempts, uint32_t n_q,
                       double *node_kmer_freq /*[n_nodes]*/, uint64_t *graph_kmer_total /*[n_graphs]*/);
/* The same replay from the compact table of groot_hip_attempts_export: row r holds the call counts of kmerCount
 * q_values[r] (strictly ascending), counts[r * n_windows + w]. */
int groot_host_weights_rows(const groot_index_view *idx, const uint32_t *q_values, uint32_t n_rows, const uint32_t *counts,
                            double *node_kmer_freq /*[n_nodes]*/, uint64_t *graph_kmer_total /*[n_graphs]*/);
/* GrootGraph.Prune (graph.go:455-525) over every graph */
int groot_host_prune(const groot_index_view *idx, const double *node_kmer_freq, double min_kmer_cov,
                     uint8_t *graph_kept /*[n_graphs]*/, uint8_t *path_kept /*[n_paths]*/,
                     uint8_t *node_removed /*[n_nodes]*/);
/* GrootGraph.SaveGraphAsGFA (graphio.go:19-112) for graph g after pruning; writes nothing and sets
 * *written=0 if no node has KmerFreq>0.  timestamp may be NULL (uses now). */
int groot_host_save_gfa(const groot_index_view *idx, uint32_t graph, const double *node_kmer_freq,
                        const uint8_t *path_kept, const uint8_t *node_removed, uint64_t total_kmers,
                        const char *timestamp, const char *file_name, int *written);

/* ---- FASTQ in (src/pipeline/sketch.go:41-77,175-238; seqio.go:173-188) -------------------------- */
typedef struct groot_fastq groot_fastq;
/* paths may end in .gz (sketch.go:60-68); n_files==0 reads stdin */
int groot_fastq_open(const char *const *files, uint32_t n_files, groot_fastq **out);
/* Fills caller buffers with up to max_reads reads: seq/qual/name are concatenations with offsets
 * (n+1 entries each).  Returns the number of reads (0 at end of input) or a negative error. */
int64_t groot_fastq_next_batch(groot_fastq *fq, uint32_t max_reads, uint8_t *seq, uint8_t *qual, uint64_t *seq_off,
                               uint64_t seq_cap, char *names, uint64_t *name_off, uint64_t name_cap);
void groot_fastq_close(groot_fastq *fq);

/* ---- BAM out (src/pipeline/boss.go:45-105,225-240; alignment.go:113-156) ------------------------ */
typedef struct groot_bam groot_bam;
typedef struct groot_aln_record {  /* one sam.Record of alignment.go:118-155 */
    const char *name; uint32_t name_len;        /* read.ID[1:]                                   */
    const uint8_t *seq; const uint8_t *qual;    /* read.Seq[0:seq_len], read.Qual[0:seq_len] raw  */
    uint32_t seq_len;
    uint32_t ref_id;                            /* index into the @SQ list (global path index)    */
    uint32_t pos;                               /* 0-based                                        */
    uint8_t start_clip, end_clip, reverse, secondary;
} groot_aln_record;
/* header: @HD VN:1.5, one @SQ per path (graphio.go:141-154), @PG ID:1 PN:groot CL:"groot align"
 * VN:1.1.2, @RG ID:readsID ... (boss.go:55-84).  path NULL or "-" = stdout.  date NULL = now. */
int groot_bam_open(const char *path, const groot_index_view *idx, const char *date, groot_bam **out);
int groot_bam_write(groot_bam *bam, const groot_aln_record *recs, uint64_t n);
/* BGZF write concurrency for large groot_bam_write calls (bam.NewWriter's third argument, boss.go:99); 0 = all cores */
int groot_bam_set_threads(groot_bam *bam, uint32_t n_threads);
/* Fast path of the collector: straight from the device's traversal records of one batch to BAM records (the
 * expansion of groot_host_expand_alns, the record fields of alignment.go:113-156 and the BGZF compression run in
 * parallel over chunks of traversals; output order = traversal order = read order).  The batch arrays are the ones
 * groot_fastq_next_batch filled. */
typedef struct groot_read_batch {
    const uint8_t *seq, *qual;     /* concatenated Seq / Qual (same offsets)           */
    const uint64_t *seq_off;       /* [n_reads+1]                                       */
    const char *names;             /* concatenated read.ID[1:]                          */
    const uint64_t *name_off;      /* [n_reads+1]                                       */
    uint32_t n_reads, first_read_id;
} groot_read_batch;
/* MAPQ: 30 (alignment.go:143), or travs[i].reserved for the records of a traversal that carries GROOT_TRAV_MAPQ (assignment); a
 * traversal with an empty path set writes no record.  The same holds for groot_bam_write_batch. */
int groot_bam_write_travs(groot_bam *bam, const groot_index_view *idx, const groot_read_batch *batch, const groot_trav *travs,
                          const uint64_t *masks, uint64_t n_trav, uint64_t *n_records);
int groot_bam_close(groot_bam *bam);
/* BGZF compression level: -1 = zlib default = what bgzf.NewWriter uses in the reference, 0 = stored .. 9;
 * -2 = structural: the records of a read (one per path of a traversal, alignment.go:113-156) are written as deflate back-references
 * to the first one with the differing header bytes as literals -- no match search; the inflated BAM is byte for byte the same,
 * the file about 4x larger than at level 1, the writer an order of magnitude faster */
int groot_bam_set_level(groot_bam *bam, int level);
uint64_t groot_bam_bytes_written(const groot_bam *bam);

/* ---- parallel FASTQ ingest (src/pipeline/sketch.go:41-77,213-236; seqio.go:173-188) --------------------------------
 * One reader thread per input file (the next few files are opened ahead, so several gzip streams inflate at once), the
 * calling thread frames the text at record boundaries, and n_threads workers find the line breaks, parse the records
 * and pack the bases into the wire format of groot_hip_submit_packed16.  Batches come out in input order; lines of
 * consecutive files form one stream; a trailing partial record is dropped (FastqHandler.Run).  Records hold positions
 * into the batch's own copy of the FASTQ text: nothing is copied per read. */
typedef struct groot_reads groot_reads;
typedef struct groot_reads_batch groot_reads_batch;
typedef struct groot_reads_view {
    uint32_t n_reads, max_len;
    uint64_t n_bases, n_exc;
    const uint8_t *packed;         /* 2-bit bases, (n_bases+3)/4 bytes                      */
    const uint16_t *seq_len;       /* [n_reads]                                             */
    const uint64_t *exc_pos;       /* [n_exc] bytes other than ACGT, ascending position     */
    const uint8_t *exc_byte;
    const uint8_t *text;           /* FASTQ text the positions below point into             */
    const uint32_t *name_pos, *name_len;   /* read.ID[1:] (the record name, alignment.go:119) */
    const uint32_t *seq_pos;       /* read.Seq, seq_len[i] bytes                            */
    const uint32_t *qual_pos, *qual_len;   /* read.Qual as it came                           */
} groot_reads_view;
/* n_files == 0 reads stdin; n_threads 0 = all cores; block_bytes 0 = 256 MB of text per block; a batch holds at most
 * max_batch_reads reads (0 = 1<<20) and max_batch_bases bases (0 = 256 per read) */
int groot_reads_open(const char *const *files, uint32_t n_files, uint32_t n_threads, uint64_t block_bytes, uint32_t max_batch_reads,
                     uint64_t max_batch_bases, groot_reads **out);
/* Paired-end input: batches of whole fragments with the mates interleaved, read 2i from files1 and read 2i+1 from files2, the two lists
 * read in lockstep (n_files2 == n_files1; the files of a list form one stream as above).  n_files2 == 0: files1 (or stdin) is ONE stream
 * that holds the mates alternately -- the same batches.  n_reads of every batch is even: a fragment is never cut by max_batch_reads (an
 * odd value is rounded down) or max_batch_bases.  Mate names must agree: the name runs up to the first whitespace and a trailing /1 or /2
 * is removed before comparing; GROOT_E_FORMAT names the 1-based fragment number and both names.  GROOT_E_FORMAT too for a list that ends
 * before its partner and for an interleaved stream with an odd number of records.  With two lists a batch's text is one stretch per
 * stream (the record arrays hold positions: nothing is copied per read); the packed bases are in read order. */
int groot_reads_open_paired(const char *const *files1, uint32_t n_files1, const char *const *files2, uint32_t n_files2, uint32_t n_threads,
                            uint64_t block_bytes, uint32_t max_batch_reads, uint64_t max_batch_bases, groot_reads **out);
int groot_reads_next(groot_reads *r, groot_reads_batch **out);   /* *out = NULL at the end of the input */
void groot_reads_batch_view(const groot_reads_batch *b, groot_reads_view *view);
void groot_reads_batch_free(groot_reads_batch *b);
uint64_t groot_reads_count(const groot_reads *r);
void groot_reads_close(groot_reads *r);
/* collector for such a batch: traversal records -> sam.Records -> BGZF, parallel like groot_bam_write_travs */
/* mask_ckpt != NULL: masks are the compact path sets of groot_hip_collect (bytes) with their checkpoints (every 256th traversal);
 * NULL: masks points at uint64_t words, path_words of them per traversal */
int groot_bam_write_batch(groot_bam *bam, const groot_index_view *idx, const groot_reads_view *reads, uint32_t first_read_id,
                          const groot_trav *travs, const void *masks, const uint32_t *mask_ckpt, uint64_t n_trav, uint64_t *n_records);

/* Rescued records (defined at groot_hip_rescue_rec_enable in groot_hip.h): one kept placement of a read that mismatch rescue placed --
 * batch-relative read, global path, 0-based path coordinate, strand, the distance d and the d offsets in the ORIENTED read (the read for
 * strand 0, its reverse complement for strand 1) at which it differs from the path, ascending, the rest 0xFFFF. */
typedef struct groot_rescue_record {
    uint32_t read, path, pos;
    uint16_t mm[3];
    uint8_t strand, d;
} groot_rescue_record;   /* 20 bytes */
/* One BAM record per rescued record of a batch, in list order (groot_hip_rescue_rec_batch: ascending by read, path, strand, pos), through
 * the record formatter and the BGZF path of the writer above, into a BAM opened with groot_bam_open:
 *   QNAME the read's name; FLAG 0x10 for strand 1, 0x100 on every record of a read but its first in the list; MAPQ 30; CIGAR <len>M, no
 *   clips; SEQ / QUAL oriented as a reverse record's are (reverse complement / reversed for strand 1); no mate; and two aux tags that
 *   the main BAM does not have: NM:i:d (written as a uint8), and MD:Z: the standard string -- the run of matching bases, then for every
 *   mismatch the PATH's base at pos + mm[i] and the next run, a run of 0 at either end and between neighbours included.
 * The path's bases come from the index view (a base outside every node of the path reads 'N').  GROOT_E_INVALID, with nothing of the
 * call written, for a record whose read is not in the batch, whose path is not in the index, that does not lie inside the path
 * (pos + len > path_len), with strand > 1, d > 3, or with offsets that are not d ascending values below the read's length followed by
 * 0xFFFF; GROOT_E_FORMAT for a name above 254 characters.  *n_records = records written. */
int groot_bam_write_rescued(groot_bam *bam, const groot_index_view *idx, const groot_reads_view *reads, const groot_rescue_record *recs,
                            uint64_t n, uint64_t *n_records);

/* Gapped records (defined at groot_hip_gap_rec_enable in groot_hip.h): one kept gapped placement of a read that gapped rescue placed --
 * as a rescued record, with k aligned read bases in front of one gap of g bases (type: GROOT_GAP_DEL 0 / GROOT_GAP_INS 1), and the d
 * offsets in the ORIENTED read at which an ALIGNED base differs from the path (never inside an insertion's bases [k, k + g)). */
typedef struct groot_gap_record {
    uint32_t read, path, pos;
    uint16_t k, mm[3];
    uint8_t strand, d, type, g;
} groot_gap_record;   /* 24 bytes */
/* One BAM record per entry of BOTH lists of a batch, merged by `read` (both arrive ascending; a read present in both lists is
 * GROOT_E_INVALID); with ng = 0 the bytes are exactly those of groot_bam_write_rescued.  A gapped record is written as a rescued one --
 * QNAME, FLAG 0x10 for strand 1 and 0x100 on every record of a read but its first in the merged list, MAPQ 30, POS = pos, SEQ / QUAL
 * oriented -- with
 *   CIGAR <k>M<g>D<len-k>M (DEL) or <k>M<g>I<len-k-g>M (INS); bin = reg2bin over the reference span, len + g (DEL) or len - g (INS);
 *   NM:i:d + g; MD:Z: the standard string over the aligned bases, runs and the PATH's base at every mismatch; a DEL carries ^ and the
 *   deleted path bases between the flanks, and a run of 0 behind them when the next aligned base mismatches (31^ACG0T67); an INS skips
 *   the inserted bases and the matching run goes on across them (50M1I49M with d = 0 gives MD:Z:99).
 * GROOT_E_INVALID, with nothing of the call written, for what groot_bam_write_rescued refuses in either list, and for a gapped record
 * whose window (len + g or len - g path bases at pos) does not lie inside the path, with strand > 1, d > 3, type > 1, g outside 1..8,
 * k below 16 or less than 16 aligned bases behind the gap, or offsets that are not d ascending values below the read's length, outside
 * [k, k + g) for an INS, followed by 0xFFFF.  *n_records = records written, of both lists. */
int groot_bam_write_rescued_gapped(groot_bam *bam, const groot_index_view *idx, const groot_reads_view *reads, const groot_rescue_record *recs,
                                   uint64_t n, const groot_gap_record *grecs, uint64_t ng, uint64_t *n_records);

/* ---- packing reads for groot_hip_submit_packed (include/groot_hip.h) ------------------------------------ */
/* packed[(n_bases+3)/4]; exceptions (bytes other than A C G T, e.g. N or lower case) in ascending position, at most
 * exc_cap of them: GROOT_E_NOSPACE with *n_exc = the number needed otherwise.  n_threads 0 = all cores. */
int groot_host_pack_reads(const uint8_t *seq_concat, uint64_t n_bases, uint8_t *packed, uint64_t *exc_pos, uint8_t *exc_byte,
                          uint64_t exc_cap, uint64_t *n_exc, uint32_t n_threads);

/* ---- after the hot path: the reference's own consumer of the BAM ---------------------------------- */
/* `groot report` (src/reporting/reporting.go:33-173, cmd/report.go:104-129): breadth of coverage per reference from the
 * BAM of `groot align` (bam_path NULL = stdin).  One line "name\tread count\tlength\tcoverage cigar" per reference whose
 * covered fraction is >= cov_cutoff, written to out_path (NULL = stdout) in BAM header order; low_cov != 0 uses the
 * cutoff 0.97 and drops references with internal uncovered stretches (cmd/report.go:119-122, reporting.go:151-153). */
int groot_host_report(const char *bam_path, double cov_cutoff, int low_cov, const char *out_path, uint64_t *n_reported);
/* The same report from counts instead of a BAM: records[p] = records on global path p, depth = the pileup of every path, path p
 * at sum_{q<p} path_len[q] (path_len[p] entries), as groot_hip_coverage_export hands them out.  A record of path p at Pos with
 * an M op of length M adds 1 to depth[Pos .. min(Pos + M, path_len[p] - 1)], both ends included (reporting.go:104-127).
 * Byte for byte the output groot_host_report writes for the BAM whose records give these counts. */
int groot_host_report_coverage(const groot_index_view *idx, const uint64_t *records, const uint64_t *depth, double cov_cutoff,
                               int low_cov, const char *out_path, uint64_t *n_reported);
/* Shared reads (the definition is at groot_hip_shared_enable in groot_hip.h): the file of "nameA \t nameB \t n" lines, one for every
 * pair a <= b of REPORTED references with n != 0 reads in common -- a = b included, n then being the distinct reads on a --
 * ascending by (a, b) in BAM header order, names as the report's first column prints them (the '*' stripped).  Empty when nothing is
 * reported.  The reported references are the lines groot_host_report_coverage writes for records / depth under the same cutoff and
 * low_cov.  The n_pairs triples (pa[i], pb[i], count[i]), pa <= pb < n_paths, come from groot_hip_shared_export, in any order; a pair
 * given more than once (the lists of several contexts) is summed.  out_path NULL = stdout; *n_lines = lines written. */
int groot_host_shared_from_counts(const groot_index_view *idx, const uint64_t *records, const uint64_t *depth, double cov_cutoff,
                                  int low_cov, uint64_t n_pairs, const uint32_t *pa, const uint32_t *pb, const uint64_t *count,
                                  const char *out_path, uint64_t *n_lines);
/* One pass over a BAM: the report, byte for byte what groot_host_report writes (report_out NULL = stdout), and the shared-reads file
 * above (shared_out, required).  Here a read is one QNAME: the records of a name are grouped wherever they lie in the BAM (the
 * reference's writer interleaves the records of different reads), so the device counts and these agree whenever read names are unique. */
int groot_host_report_shared(const char *bam_path, double cov_cutoff, int low_cov, const char *report_out, const char *shared_out,
                             uint64_t *n_reported, uint64_t *n_lines);

/* Variants (mismatch rescue, defined at groot_hip_rescue_enable in groot_hip.h): what the reads the exact aligner left unaligned say
 * differs from the indexed alleles.  rescued_depth[sum of path_len] and alt[4 * sum of path_len] (A, C, G, T per base) are the summed
 * groot_hip_rescue_export of every ctx, exact_depth the depth of groot_hip_coverage_export, path p at sum_{q<p} path_len[q].  One line
 *     name \t pos (1-based) \t ref \t alt \t alt_reads \t rescued_depth \t exact_depth \t share
 * per (path, position, alt base) with alt_reads >= max(min_reads, 1) and share = alt_reads / (rescued_depth + exact_depth) >= min_share
 * (one division in double, printed %.4f), ascending by global path, position and A, C, G, T; the name as the report prints it (the '*'
 * stripped), ref the path's base there.  out_path NULL = stdout; *n_lines = lines written.  GROOT_E_INVALID for an alt count above
 * the rescued depth of its base (no table of the device has one: a kept placement adds to the depth wherever it adds an alt). */
int groot_host_variants_write(const groot_index_view *idx, const uint64_t *rescued_depth, const uint64_t *alt, const uint64_t *exact_depth,
                              uint64_t min_reads, double min_share, const char *out_path, uint64_t *n_lines);

/* Indels (gapped rescue, defined at groot_hip_gap_enable in groot_hip.h): the gaps that reads left unplaced by mismatch rescue show
 * against the indexed alleles.  An event is one (path, position, type, length, inserted sequence) with the kept gapped placements
 * that show it, as groot_hip_gap_export gives them. */
#define GROOT_GAP_DEL 0
#define GROOT_GAP_INS 1
typedef struct groot_gap_event {
    uint32_t path, pos;  /* global path; path coordinate of the last text base before the gap */
    uint8_t type, len;   /* GROOT_GAP_DEL / GROOT_GAP_INS; the gap's bases, 1..8 */
    uint16_t seq;        /* INS: the inserted bases in path strand, 2 bits each, base i in bits 2i..2i+1, A C G T = 0 1 2 3; DEL: 0 */
    uint32_t reserved;
    uint64_t reads;      /* kept gapped placements that show it */
} groot_gap_event;
/* events[n_events] are the merged groot_hip_gap_export of every ctx (events by key), gdepth / rescued_depth / exact_depth[sum of path_len]
 * the summed gdepth of groot_hip_gap_export, depth of groot_hip_rescue_export and depth of groot_hip_coverage_export.  One line
 *     name \t pos (1-based, the base before the gap) \t type (DEL|INS) \t len \t seq \t reads \t gap_depth \t rescued_depth \t exact_depth \t share
 * per event with reads >= max(min_reads, 1) and share = reads / (gap_depth + rescued_depth + exact_depth) >= min_share (the three depths
 * at pos; one division in double, printed %.4f), in the order given (the export's: path, pos, type, len, seq).  seq: the deleted bases
 * of the path for a DEL, the inserted bases for an INS; the name as the report prints it.  out_path NULL = stdout; *n_lines = lines
 * written.  GROOT_E_INVALID, before anything is written, for an event outside its path (a DEL's bases included), with a type or length the
 * device never gives, or with more reads than the gap depth at its pos (every placement that shows an event covers that base). */
int groot_host_indels_write(const groot_index_view *idx, const groot_gap_event *events, uint64_t n_events, const uint64_t *gdepth,
                            const uint64_t *rescued_depth, const uint64_t *exact_depth, uint64_t min_reads, double min_share,
                            const char *out_path, uint64_t *n_lines);

/* ---- abundance by EM over equivalence classes ----------------------------------------------------------------------
 * ECs as defined at groot_hip_ec_enable in groot_hip.h (distinct non-empty S(r), ascending path IDs, in CSR form: EC i is
 * ids[off[i] .. off[i+1]) with count[i] reads).  groot_host_em restates src/em/em.go NewEM / Run / Return (lines 29-158) in double
 * precision over n_paths paths, visiting the ECs in the order given (canonical order: lexicographic on the ID lists; the reference
 * iterates a Go map): alpha starts at 1/n_paths; an EC with count 0, or whose denominator (the sum of alpha over it) is below 2^-52,
 * is skipped; next[p] += alpha[p] * (count / denom); a path has changed when next > 1e-2 and |next - alpha| / next > 1e-2; when no path
 * changed and the iteration index is above min_iter, alpha below 1e-7 / 10 is zeroed and one more round runs.  alpha_out[n_paths] =
 * the estimated reads of each path; *iterations = the rounds run (max_iter when it never settled).  GROOT_E_INVALID when
 * max_iter < min_iter or max_iter = 0 (the reference's errors), or an ID is >= n_paths. */
#define GROOT_EM_MIN_ITER 50      /* the reference's defaults (1_pipeline_test.go:49-54) */
#define GROOT_EM_MAX_ITER 10000
int groot_host_em(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t min_iter,
                  uint32_t max_iter, double *alpha_out, uint32_t *iterations);
/* The abundance file: "name \t reads \t em_reads \t fraction" for every path with alpha >= min_reads, in BAM header order; name as the
 * report prints it ('*' stripped), reads = the distinct reads with a record on the path (the diagonal of shared reads), em_reads =
 * alpha ("%.2f"), fraction = alpha / sum(alpha) ("%.6f").  Empty when there are no ECs.  The ECs come in any order, IDs in any order,
 * repeats summed (the lists of several contexts or GPUs); they are canonicalised, then groot_host_em runs with GROOT_EM_MIN_ITER /
 * GROOT_EM_MAX_ITER.  out_path NULL = stdout; *n_lines = lines written; iterations (may be NULL) = the EM's rounds. */
int groot_host_abundance_from_ecs(const groot_index_view *idx, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                                  double min_reads, const char *out_path, uint64_t *n_lines, uint32_t *iterations);
/* The same file from a BAM, a read being one QNAME (its records grouped wherever they lie, as groot_host_report_shared does): byte for
 * byte what the device path writes whenever read names are unique. */
int groot_host_report_abundance(const char *bam_path, double min_reads, const char *out_path, uint64_t *n_lines);

/* ---- bootstrap intervals of the abundance estimate ----------------------------------------------------------------
 * Input: ECs in canonical order as CSR (n_ec, off, ids, count over n_paths paths), N = the sum of count; n_boot = B replicates, a
 * 64-bit seed, n_draws draws per replicate (0 means N).
 * Resampling: cum[0] = 0, cum[e+1] = cum[e] + count[e].  Draw j (0 <= j < n_draws) of replicate b, all arithmetic modulo 2^64:
 *     z = seed + (b * n_draws + j + 1) * 0x9E3779B97F4A7C15
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z =  z ^ (z >> 31)
 *     t = high 64 bits of the 128-bit product z * N          (0 <= t < N)
 *     e = the EC with cum[e] <= t < cum[e+1]                 (an EC with count 0 is never drawn)
 *     boot_count[b][e] += 1
 * Only integers are involved: boot_count depends on (seed, b, n_draws, count) alone, not on the order of the draws or the number of
 * threads; the first three replicates of a run with B = 7 are the run with B = 3.
 * EM per replicate: alpha_b = groot_host_em(n_paths, n_ec, off, ids, boot_count[b], min_iter, max_iter), bit for bit, with its own
 * iteration count.  With n_ec = 0 every replicate is the EM of no ECs.
 * GROOT_E_INVALID: n_boot = 0; N = 0 with n_ec > 0; the errors of groot_host_em.
 * Statistics per path p over x_b = alpha_b[p], b = 0 .. B-1, in double precision without FMA contraction, sums in order of b:
 * boot_mean = (sum x_b) / B; boot_sd = sqrt(sum (x_b - boot_mean)^2 / (B - 1)), 0 when B = 1; with v = the x_b sorted ascending and
 * q = (25 * (B - 1)) / 1000 in integer arithmetic, boot_lo = v[q], boot_hi = v[B - 1 - q] (B = 100: v[2] and v[97]).
 * File: every line of the abundance file gets four more tab-separated columns, all "%.2f":
 * name \t reads \t em_reads \t fraction \t boot_mean \t boot_sd \t boot_lo \t boot_hi; the lines, their order and their first four
 * columns are those of the file without bootstraps. */
/* The contract above on the host, the replicates spread over `threads` (0 = 1).  boot_count[n_boot][n_ec] (may be NULL),
 * alpha[n_boot][n_paths], iterations[n_boot] (may be NULL).  groot_hip_em_bootstrap computes the same bits on the device. */
int groot_host_em_bootstrap(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t n_boot,
                            uint64_t seed, uint64_t n_draws, uint32_t min_iter, uint32_t max_iter, uint32_t threads, uint64_t *boot_count,
                            double *alpha, uint32_t *iterations);
/* The canonicalisation the abundance writers apply: ECs in any order, IDs in any order, repeats summed -> canonical order, IDs ascending
 * and unique, empty and count-0 ECs dropped.  out_off[n_ec + 1], out_ids[off[n_ec]], out_count[n_ec] (the input's sizes always
 * suffice); *n_out = the canonical ECs. */
int groot_host_ecs_canonical(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint64_t *out_off,
                             uint32_t *out_ids, uint64_t *out_count, uint64_t *n_out);
/* groot_host_abundance_from_ecs with the bootstrap columns: boot_alpha[n_boot][n_paths] = the replicates' alpha over the canonical ECs
 * (groot_host_ecs_canonical) with n_draws = 0 and GROOT_EM_MIN_ITER / GROOT_EM_MAX_ITER, as groot_hip_em_bootstrap returns them; NULL =
 * computed here with groot_host_em_bootstrap(seed, threads). */
int groot_host_abundance_boot_from_ecs(const groot_index_view *idx, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                                       double min_reads, uint32_t n_boot, uint64_t seed, const double *boot_alpha, uint32_t threads,
                                       const char *out_path, uint64_t *n_lines, uint32_t *iterations);
/* groot_host_report_abundance with the bootstrap columns, the replicates computed on `threads` host threads. */
int groot_host_report_abundance_boot(const char *bam_path, double min_reads, uint32_t n_boot, uint64_t seed, uint32_t threads, const char *out_path,
                                     uint64_t *n_lines);

/* ---- calls: assigned coverage, the EM-weighted pileup per path ------------------------------------------------------------
 * The pileup of the reads the abundance EM assigns to each path: every record of read r on path p gets the weight of r's posterior on
 * p, and a line says whether the assigned evidence covers the path.  The definition (groot_hip.h, README.md, DESIGN.md 13, the tests):
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
 * A table is (ECs as CSR in canonical order, tuples[4 n] = (EC index, path, Pos, last) ascending, tn[n] = records), as
 * groot_hip_acov_export hands it out.  The library is built without -march, so no product and sum are contracted. */
/* The exports of n_ctx contexts (arrays of n_ctx pointers / sizes; ECs in any order, tuples naming ECs by their index in the same
 * export) -> one table: ECs canonical as groot_host_ecs_canonical gives them, tuples renumbered, equal keys summed, ascending.  The
 * outputs need room for the sums of the inputs' sizes (out_off one more); *n_ec_out / *n_tuples_out = what was written. */
int groot_host_acov_merge(uint32_t n_paths, uint32_t n_ctx, const uint64_t *const *ec_off, const uint32_t *const *ec_ids, const uint64_t *const *ec_count,
                          const uint64_t *n_ec, const uint32_t *const *tuples, const uint64_t *const *tn, const uint64_t *n_tuples, uint64_t *out_off,
                          uint32_t *out_ids, uint64_t *out_count, uint32_t *out_tuples, uint64_t *out_tn, uint64_t *n_ec_out, uint64_t *n_tuples_out);
/* D_p of one path from a table (canonical ECs) and alpha[n_paths]: depth[path_len].  GROOT_E_INVALID for a tuple whose EC is outside
 * the list or whose path is not in its EC. */
int groot_host_acov_depth(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const double *alpha, uint64_t n_tuples,
                          const uint32_t *tuples, const uint64_t *tn, uint32_t path, uint32_t path_len, double *depth);
/* The calls file: one line per line of the abundance file (alpha >= min_reads, BAM header order; empty without ECs),
 * "name \t em_reads (%.2f) \t length \t depth (%.2f) \t breadth (%.4f) \t cigar \t called": cigar = the covered (M) / uncovered (D) runs as
 * the report writes them, called = 1 when breadth >= cov_cutoff.  ECs canonical (groot_host_acov_merge); alpha[n_paths], or NULL =
 * groot_host_em over the ECs with GROOT_EM_MIN_ITER / GROOT_EM_MAX_ITER.  out_path NULL = stdout; *n_lines / *n_called may be NULL. */
int groot_host_calls_from_table(const groot_index_view *idx, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                                const double *alpha, uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, double min_reads, double call_depth,
                                double cov_cutoff, const char *out_path, uint64_t *n_lines, uint64_t *n_called);
/* The same file from a BAM, a read being one QNAME (groot_host_report_abundance's grouping), through the same writer: byte for byte
 * what the device path writes whenever read names are unique.  *n_tuples (may be NULL) = distinct tuples of the table. */
int groot_host_report_calls(const char *bam_path, double min_reads, double call_depth, double cov_cutoff, const char *out_path, uint64_t *n_lines,
                            uint64_t *n_called, uint64_t *n_tuples);

/* ---- bootstrap support for the calls: per-replicate breadth ----------------------------------------------------------------
 * How far to trust `called`: the pileup above is redone for every bootstrap replicate of the abundance estimate, and a line says in
 * which share of the replicates the path is still called, and between which breadths it moves.  The definition (groot_hip.h,
 * README.md, DESIGN.md 13 and the tests quote it):
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
 * s_b(e) is the expectation of resampling the reads of e given how often the replicate drew e; positions inside an EC are not
 * resampled (a run keeps no per-read positions).  A term with d_e[x] == 0 leaves a non-negative D as it is: (e, p) without tuples
 * are skipped.  Record sums per (e, p) below 2^63. */
/* The definition itself, the replicates spread over `threads` (0 = 1): covered_out[n_boot][n_sel], the covered bases of the paths
 * sel_paths[n_sel] (any paths, any order) in every replicate.  path_len[n_paths]; the table as for groot_host_calls_from_table;
 * boot_count[n_boot][n_ec], alpha[n_boot][n_paths].  GROOT_E_INVALID: a tuple whose EC is outside the list, whose path is not in its
 * EC or whose last >= path_len; n_boot = 0; an EC with count 0 or IDs that do not ascend; a selected path outside the index.
 * groot_hip_call_support computes the same bits on the device. */
int groot_host_call_support(uint32_t n_paths, const uint32_t *path_len, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                            uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, uint32_t n_boot, const uint64_t *boot_count, const double *alpha,
                            double call_depth, uint32_t n_sel, const uint32_t *sel_paths, uint32_t threads, uint32_t *covered_out);
/* groot_host_calls_from_table with the three support columns, through the same writer.  boot_count[n_boot][n_ec] and
 * boot_alpha[n_boot][n_paths] = the replicates over these ECs with n_draws = 0 and GROOT_EM_MIN_ITER / GROOT_EM_MAX_ITER (used when
 * both are given; else computed here with groot_host_em_bootstrap(seed, threads)); covered[n_boot][lines] = groot_host_call_support /
 * groot_hip_call_support over the paths that get a line (alpha >= min_reads, ascending), NULL = computed here on `threads` threads. */
int groot_host_calls_support_from_table(const groot_index_view *idx, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                                        const double *alpha, uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, double min_reads,
                                        double call_depth, double cov_cutoff, uint32_t n_boot, uint64_t seed, uint32_t threads, const uint64_t *boot_count,
                                        const double *boot_alpha, const uint32_t *covered, const char *out_path, uint64_t *n_lines, uint64_t *n_called);
/* groot_host_report_calls with the three support columns, the replicates drawn, fitted and piled up on `threads` host threads. */
int groot_host_report_calls_support(const char *bam_path, double min_reads, double call_depth, double cov_cutoff, uint32_t n_boot, uint64_t seed,
                                    uint32_t threads, const char *out_path, uint64_t *n_lines, uint64_t *n_called, uint64_t *n_tuples);

/* ---- rarefaction curves: was the sample sequenced deeply enough? -----------------------------------------------------------
 * The run's units (reads; fragments with pairing) are subsampled WITHOUT replacement to a list of depths, nested, and the abundance
 * estimate is redone at every depth: a curve of detected ARGs against depth that has flattened says that more reads would turn up
 * little more.  Nothing but the ECs is needed.  The definition (groot_hip.h, README.md, DESIGN.md 15 and the tests quote it):
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
 * Only integers are involved: rare_count depends on (seed, b, count, m[d]) alone -- not on R, the other depths or the number of threads;
 * its sum over e is m[d]; rare_count[b][d][e] <= rare_count[b][d+1][e] <= count[e] (the depths are nested), and m[d] = N gives count.
 * The estimate of replicate b at depth d: alpha[b][d] = groot_host_em(n_paths, n_ec, off, ids, rare_count[b][d], min_iter, max_iter),
 * bit for bit, with its own iteration count.  (The ECs are taken in the order given; the file writers give them in canonical order.)
 *
 * The file (--rarefy): one line per depth step s = 1 .. D (D = n_steps), no header; m_s = (N / D) * s + ((N % D) * s) / D in integers, a
 * step with m_s = 0 is omitted.  "fraction (s/D, %.4f) \t units (m_s) \t args_mean (%.2f) \t args_lo \t args_hi": args of a replicate = the
 * number of paths with alpha[b][s] >= min_reads (the lines the abundance file would have at that depth); the mean summed in replicate
 * order; lo and hi = v[q] and v[R-1-q] of the sorted integers, q = (25 * (R - 1)) / 1000 (the bootstrap's rule).  The step s = D is not
 * drawn: its three values are the point estimate's line count.  With calls three more columns "called_mean (%.2f) \t called_lo \t
 * called_hi": called = the number of paths with alpha[b][s] >= min_reads and (double)covered / (double)path_len >= cov_cutoff (path_len 0:
 * breadth 0.0), covered = groot_host_call_support / groot_hip_call_support fed boot_count = rare_count, the rarefied alpha, call_depth and
 * sel_paths = every path detected (alpha >= min_reads) in at least one drawn (b, s), ascending; the step s = D from count and the point
 * estimate in the same way, which is the calls file's count of called lines. */
#define GROOT_RAREFY_STEPS 10
#define GROOT_RAREFY_REPS 20
/* m_s of the steps s = 1 .. n_steps into m[n_steps] (zeros included).  GROOT_E_INVALID for n_steps = 0. */
int groot_host_rarefy_depths(uint64_t n_units, uint32_t n_steps, uint64_t *m);
/* The definition on the host, the replicates spread over `threads` (0 = 1).  rare_count[n_rep][n_depths][n_ec] (may be NULL),
 * alpha[n_rep][n_depths][n_paths], iterations[n_rep][n_depths] (may be NULL).  GROOT_E_INVALID: n_rep = 0; n_depths = 0; a depth of 0 or
 * above N; depths that descend; N = 0; the errors of groot_host_em.  GROOT_E_UNSUPPORTED at N >= 2^62.  groot_hip_em_rarefy computes the
 * same bits on the device. */
int groot_host_em_rarefy(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t n_rep,
                         uint32_t n_depths, const uint64_t *depths, uint64_t seed, uint32_t min_iter, uint32_t max_iter, uint32_t threads,
                         uint64_t *rare_count, double *alpha, uint32_t *iterations);
/* The rarefaction file of a run's ECs (any order without calls: they are made canonical as the abundance writers do; with calls the
 * canonical ECs and the table of groot_host_acov_merge, as for groot_host_calls_from_table).  The drawn depths are the m_s > 0 of the steps
 * s < n_steps, n_drawn of them, in step order.  rare_alpha[n_rep][n_drawn][n_paths] and rare_count[n_rep][n_drawn][n_ec] as
 * groot_hip_em_rarefy returns them over the canonical ECs with GROOT_EM_MIN_ITER / GROOT_EM_MAX_ITER (rare_count is only read with calls
 * and without covered); rare_alpha NULL = both computed here with groot_host_em_rarefy(seed, threads).  with_calls != 0 adds the three
 * called columns; covered[n_rep * n_drawn][n_sel] = groot_hip_call_support over sel_paths as defined above, NULL = computed here on
 * `threads` threads (n_sel is then ignored).  GROOT_E_INVALID: n_rep = 0, n_steps = 0, cov_cutoff > 1 with calls, an n_sel that is not the
 * number of detected paths.  out_path NULL = stdout; *n_lines may be NULL. */
int groot_host_rarefy_from_ecs(const groot_index_view *idx, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                               double min_reads, uint32_t n_rep, uint32_t n_steps, uint64_t seed, uint32_t threads, const uint64_t *rare_count,
                               const double *rare_alpha, int with_calls, uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn,
                               double call_depth, double cov_cutoff, uint32_t n_sel, const uint32_t *covered, const char *out_path, uint64_t *n_lines);
/* The same file from a BAM, a read being one QNAME (groot_host_report_abundance's grouping; with calls the table of
 * groot_host_report_calls), everything computed on `threads` host threads: byte for byte what the device path writes whenever read
 * names are unique.  iter_range[2] (may be NULL) = the fewest and the most EM iterations among the drawn (replicate, depth) pairs, 0 0 without any. */
int groot_host_report_rarefy(const char *bam_path, double min_reads, uint32_t n_rep, uint32_t n_steps, uint64_t seed, uint32_t threads, int with_calls,
                             double call_depth, double cov_cutoff, const char *out_path, uint64_t *n_lines, uint32_t *iter_range);

/* ---- assignment: each read to its best allele by EM posterior ------------------------------------------------------------
 * A second `align` pass keeps, per read, only the records on the path with the largest posterior of a first pass's abundance estimate
 * (w(e,p) = alpha[p] / denom(e), so the argmax over S(r) is the argmax over alpha), each with a MAPQ derived from that posterior.  The
 * definition (groot_hip.h, README.md, DESIGN.md 14 and the tests quote it):
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
 * The result depends on alpha and the read's records alone.  The library is built without -march: no product and sum are contracted. */
typedef struct groot_assign_stats {
    uint64_t reads;        /* reads with records                                                         */
    uint64_t assigned, unassigned, below;
    uint64_t ties;         /* assigned reads whose largest alpha is shared by two or more paths of S(r)  */
    uint64_t records_in;   /* set bits of the path sets before                                           */
    uint64_t records_kept; /* ... and after: one per kept traversal                                      */
    uint64_t travs_emptied;
    uint64_t launches;     /* device only: kernels launched for the feature since the ctx was opened; 0 from the host call */
} groot_assign_stats;
/* The definition on the CPU, in place: travs[n_trav] in (read, ord) order with masks[n_trav * path_words]; a read's batch position is
 * read_id - first_read_id (< n_reads: GROOT_E_INVALID otherwise, as for alpha or min_posterior out of range and a traversal outside
 * the index; likewise for a list out of order: batch positions that fall, so also a read whose traversals are not one run, or graphs
 * that fall within a read).  best[n_reads], mapq[n_reads] and stats may be NULL.  libgroot_hip.so computes the same bytes (groot_hip_assign_enable). */
int groot_host_assign_travs(const groot_index_view *idx, const double *alpha, double min_posterior, groot_trav *travs, uint64_t *masks,
                            uint64_t n_trav, uint32_t first_read_id, uint32_t n_reads, uint32_t *best, uint8_t *mapq, groot_assign_stats *stats);
/* Reads an abundance file (4 columns, or 8 with bootstraps): alpha_out[n_paths] = em_reads (column 3, strtod) of the path named in
 * column 1 -- names as the report prints them, the '*' stripped --, 0 for paths the file does not name; *n_named (may be NULL) = its
 * lines.  GROOT_E_FORMAT for an unknown name, a name given twice, a name two paths share after stripping, a value that is not a finite
 * number in [0, 1e300], or a line with fewer than 3 columns; GROOT_E_IO when the file cannot be read. */
int groot_host_abundance_read(const groot_index_view *idx, const char *path, double *alpha_out, uint64_t *n_named);

#ifdef __cplusplus
}
#endif
#endif
