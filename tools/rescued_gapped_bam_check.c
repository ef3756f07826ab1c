/* rescued_gapped_bam_check.c -- groot_bam_write_rescued_gapped (include/groot_host.h, "Gapped records") on hand-made records, as a
 * stand-alone program: built with the host library's bam.cpp under -fsanitize=address,undefined (tests/test_rescued_gapped_bam.py) it
 * checks every refused input -- none of which may leave a byte in the file -- and then writes the records below to the BAM named by its
 * argument: a deletion with a mismatch right behind it and one right in front of it, an insertion without a mismatch and one with
 * mismatches on either side, gaps of 1 and of 8 bases, k at its smallest and its largest, a window that ends at the path's last base,
 * both strands, two records of one read, a quality line shorter than its sequence, and rescued records of other reads in between.  The
 * test inflates the file and compares it with its plain-Python restatement of the writer on the same tables. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "groot_host.h"

/* graph 0: one node of 80 bases, path "alpha"; graph 1: one node of 48 bases, path "beta" */
static const uint32_t graph_node_off[] = {0, 1, 2}, graph_path_off[] = {0, 1, 2};
static const uint32_t node_seq_off[] = {0, 80, 128}, node_np_off[] = {0, 1, 2};
static const uint32_t np_path[] = {0, 0}, np_pos[] = {0, 0};
static const uint32_t path_len[] = {80, 48}, path_name_off[] = {0, 5, 9};
static const char bases[] = "TGGTGTTAACCTTACTATACTCCCGCTCCGGGGTTTGGCTCATATGAACAAGTCTTTGCGCCCATAAATGTAGCCAGTGA"
                            "GCTTAGTTGGAGCAAGGGGTGCGGAAGCGCAACTCCGTCGCGCGGGTA";
static const char path_names[] = "alphabeta";

/* the batch: name, sequence, quality line of five reads, one after the other in one text (the writer takes the records on trust: what
 * a read's bases are does not matter to CIGAR, NM and MD) */
static const char text[] = "d0" "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT" "IIIIIIIIIIHHHHHHHHHHGGGGGGGGGGFFFFFFFFFF"
                           "ins/1" "CCCCCCCCCCCCCCCCCCCCAGGGGGGGGGGGGGGGGGGGG" "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmno"
                           "u" "CATGAATG" "JJJ"
                           "two" "TTTTTTTTTTTTTTTTAAAAAAAACCCCCCCCCCCCCCCC" "!!##%%"
                           "last" "GATTACAGATTACAGATTACAGATTACAGATTACA" "01234567890123456789012345678901234";
static const uint32_t name_pos[] = {0, 82, 169, 181, 230}, name_len[] = {2, 5, 1, 3, 4};
static const uint32_t seq_pos[] = {2, 87, 170, 184, 234}, qual_pos[] = {42, 128, 178, 224, 269}, qual_len[] = {40, 41, 3, 6, 35};
static const uint16_t seq_len[] = {40, 41, 8, 40, 35};

#define NONE 0xFFFF
static const groot_rescue_record plain[] = {
    {2, 1, 40, {4, NONE, NONE}, 0, 1},         /* u ungapped on beta[40 .. 47]: between the gapped reads in the merged list */
};
static const groot_gap_record good[] = {
    {0, 0, 2, 16, {16, NONE, NONE}, 0, 1, GROOT_GAP_DEL, 3},     /* d0: 16M3D24M at alpha 2, a mismatch right behind the gap: MD 16^..0.23 */
    {0, 0, 5, 24, {15, NONE, NONE}, 1, 1, GROOT_GAP_DEL, 8},     /* ... and reversed, 24M8D16M with a mismatch in front: secondary */
    {1, 0, 10, 20, {NONE, NONE, NONE}, 0, 0, GROOT_GAP_INS, 1},  /* ins/1: 20M1I20M, no mismatch: MD 40 */
    {1, 1, 0, 16, {0, 15, 40}, 1, 3, GROOT_GAP_INS, 8},          /* ... 16M8I17M on beta with mismatches at 0, 15 (the base in front of the gap) and 40 (the last) */
    {3, 0, 37, 24, {24, 25, NONE}, 0, 2, GROOT_GAP_DEL, 3},      /* two: 24M3D16M, its window ends at alpha's last base; a short quality line */
    {3, 1, 2, 16, {24, NONE, NONE}, 1, 1, GROOT_GAP_INS, 8},     /* ... 16M8I16M: the first aligned base behind the inserted ones */
    {4, 1, 3, 19, {NONE, NONE, NONE}, 0, 0, GROOT_GAP_DEL, 1},   /* last: 19M1D16M, k at its largest */
};

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    groot_index_view v;
    memset(&v, 0, sizeof v);
    v.n_graphs = 2; v.n_nodes = 2; v.n_paths = 2; v.n_bases = 128; v.n_np = 2; v.path_words = 1;
    v.graph_node_off = graph_node_off; v.graph_path_off = graph_path_off; v.node_seq_off = node_seq_off; v.node_np_off = node_np_off;
    v.np_path = np_path; v.np_pos = np_pos; v.path_len = path_len; v.path_name_off = path_name_off;
    v.bases = (const uint8_t *)bases; v.path_names = path_names;
    groot_reads_view rv;
    memset(&rv, 0, sizeof rv);
    rv.n_reads = 5; rv.max_len = 41; rv.n_bases = 164;
    rv.seq_len = seq_len; rv.text = (const uint8_t *)text; rv.name_pos = name_pos; rv.name_len = name_len; rv.seq_pos = seq_pos;
    rv.qual_pos = qual_pos; rv.qual_len = qual_len;
    groot_bam *bam = NULL;
    if (groot_bam_open(argv[1], &v, "2020-01-01T00:00:00Z", &bam)) { printf("open: %s\n", groot_host_last_error()); return 1; }
    const uint64_t before = groot_bam_bytes_written(bam);
    int bad = 0;
    uint64_t n = 7;
    const groot_gap_record refused[] = {
        {5, 0, 2, 16, {NONE, NONE, NONE}, 0, 0, 0, 3},        /* a read that is not in the batch */
        {0, 2, 2, 16, {NONE, NONE, NONE}, 0, 0, 0, 3},        /* a path that is not in the index */
        {0, 0, 38, 16, {NONE, NONE, NONE}, 0, 0, 0, 3},       /* 40 + 3 bases at 38 of 80: over the path's end by one */
        {0, 1, 10, 16, {NONE, NONE, NONE}, 0, 0, 1, 1},       /* 40 - 1 bases at 10 of 48: likewise */
        {0, 0, 2, 16, {NONE, NONE, NONE}, 2, 0, 0, 3},        /* no such strand */
        {0, 0, 2, 16, {1, 2, 3}, 0, 4, 0, 3},                 /* no such distance */
        {0, 0, 2, 16, {NONE, NONE, NONE}, 0, 0, 2, 3},        /* no such type */
        {0, 0, 2, 16, {NONE, NONE, NONE}, 0, 0, 0, 0},        /* a gap of no base */
        {0, 0, 2, 16, {NONE, NONE, NONE}, 0, 0, 0, 9},        /* ... and of nine */
        {0, 0, 2, 15, {NONE, NONE, NONE}, 0, 0, 0, 3},        /* k below 16 */
        {0, 0, 2, 25, {NONE, NONE, NONE}, 0, 0, 0, 3},        /* 15 bases behind a deletion */
        {0, 0, 2, 17, {NONE, NONE, NONE}, 0, 0, 1, 8},        /* 15 aligned bases behind an insertion */
        {2, 1, 0, 4, {NONE, NONE, NONE}, 0, 0, 1, 8},         /* a read of 8 bases, all of them inserted */
        {0, 0, 2, 16, {40, NONE, NONE}, 0, 1, 0, 3},          /* an offset at the read's length */
        {0, 0, 2, 16, {NONE, NONE, NONE}, 0, 1, 0, 3},        /* a missing offset */
        {0, 0, 2, 16, {3, 3, NONE}, 0, 2, 0, 3},              /* not ascending */
        {0, 0, 2, 16, {1, NONE, 2}, 0, 1, 0, 3},              /* an offset beyond d */
        {0, 0, 2, 16, {16, NONE, NONE}, 0, 1, 1, 3},          /* an inserted base listed: the first */
        {0, 0, 2, 16, {18, NONE, NONE}, 0, 1, 1, 3},          /* ... and the last */
    };
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) {
        groot_gap_record two[2] = {good[0], refused[i]};      /* behind a good record, and a rescued one: neither may be written */
        n = 7;
        if (groot_bam_write_rescued_gapped(bam, &v, &rv, plain, 1, two, 2, &n) != GROOT_E_INVALID || n != 0) { printf("refusal %zu differs\n", i); bad++; }
    }
    const groot_rescue_record both = {0, 0, 0, {NONE, NONE, NONE}, 0, 0};       /* a read in both lists */
    bad += groot_bam_write_rescued_gapped(bam, &v, &rv, &both, 1, good, 1, &n) != GROOT_E_INVALID || n != 0;
    const groot_rescue_record wrong = {2, 1, 41, {NONE, NONE, NONE}, 0, 0};     /* what groot_bam_write_rescued refuses, beside good gapped records */
    bad += groot_bam_write_rescued_gapped(bam, &v, &rv, &wrong, 1, good, 1, &n) != GROOT_E_INVALID || n != 0;
    bad += groot_bam_write_rescued_gapped(NULL, &v, &rv, plain, 1, good, 1, &n) != GROOT_E_INVALID;
    bad += groot_bam_write_rescued_gapped(bam, NULL, &rv, plain, 1, good, 1, &n) != GROOT_E_INVALID;
    bad += groot_bam_write_rescued_gapped(bam, &v, NULL, plain, 1, good, 1, &n) != GROOT_E_INVALID;
    bad += groot_bam_write_rescued_gapped(bam, &v, &rv, plain, 1, NULL, 1, &n) != GROOT_E_INVALID;
    bad += groot_bam_write_rescued_gapped(bam, &v, &rv, NULL, 0, NULL, 0, &n) != GROOT_OK || n != 0;      /* two empty lists are fine */
    bad += groot_bam_bytes_written(bam) != before;
    if (bad) { printf("%d refusals differ\n", bad); return 1; }
    /* two calls, as two batches: reads 0 .. 2 (the rescued record of read 2 behind the gapped ones of reads 0 and 1), then reads 3 and 4 */
    if (groot_bam_write_rescued_gapped(bam, &v, &rv, plain, 1, good, 4, &n) || n != 5) { printf("write: %s\n", groot_host_last_error()); return 1; }
    if (groot_bam_write_rescued_gapped(bam, &v, &rv, NULL, 0, good + 4, 3, &n) || n != 3) { printf("write: %s\n", groot_host_last_error()); return 1; }
    if (groot_bam_close(bam)) { printf("close: %s\n", groot_host_last_error()); return 1; }
    printf("ok\n");
    return 0;
}
