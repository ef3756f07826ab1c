/* rescued_bam_check.c -- groot_bam_write_rescued (include/groot_host.h, "Rescued records") on hand-made records, as a stand-alone program:
 * built with the host library's bam.cpp under -fsanitize=address,undefined (tests/test_rescued_bam.py) it checks every refused input --
 * none of which may leave a byte in the file -- and then writes the records below to the BAM named by its argument: d = 0 and d = 3, a
 * mismatch at the first and at the last base, two neighbouring mismatches, a record that ends at the path's last base, one that covers a
 * whole path, two records of one read, both strands, a quality line shorter than its sequence.  The test inflates the file and compares
 * it with its plain-Python restatement of the writer on the same tables. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "groot_host.h"

/* graph 0: nodes 0 "ACGTACGTTGCA", 1 "GGATCC", 2 "TTTAAA"; paths "*alpha" = 0,1 and "beta" = 0,2 (18 bases each).
 * graph 1: node 3 "CATGCATG", path "gamma" (8 bases). */
static const uint32_t graph_node_off[] = {0, 3, 4}, graph_path_off[] = {0, 2, 3};
static const uint32_t node_seq_off[] = {0, 12, 18, 24, 32}, node_np_off[] = {0, 2, 3, 4, 5};
static const uint32_t np_path[] = {0, 1, 0, 1, 0}, np_pos[] = {0, 0, 12, 12, 0};
static const uint32_t path_len[] = {18, 18, 8}, path_name_off[] = {0, 6, 10, 15};
static const char bases[] = "ACGTACGTTGCAGGATCCTTTAAACATGCATG", path_names[] = "*alphabetagamma";

/* the batch: name, sequence, quality line of four reads, one after the other in one text */
static const char text[] = "r0" "ACGTACGTTG" "IIIIIHHHHH" "read/1" "CGATACTT" "ABCDEFGH" "q" "CATGAATG" "JJJ" "r3" "ACTGTG" "!!##%%";
static const uint32_t name_pos[] = {0, 22, 44, 56}, name_len[] = {2, 6, 1, 2};
static const uint32_t seq_pos[] = {2, 28, 45, 58}, qual_pos[] = {12, 36, 53, 64}, qual_len[] = {10, 8, 3, 6};
static const uint16_t seq_len[] = {10, 8, 8, 6};

#define NONE 0xFFFF
static const groot_rescue_record good[] = {
    {0, 0, 0, {NONE, NONE, NONE}, 0, 0},      /* r0 on alpha and on beta, exact: the second record of the read is secondary */
    {0, 1, 0, {NONE, NONE, NONE}, 0, 0},
    {1, 0, 10, {0, 3, 7}, 1, 3},               /* read/1 reversed on alpha[10 .. 17], the path's last base: mismatches at its first, a middle and its last base */
    {2, 2, 0, {4, NONE, NONE}, 0, 1},          /* q covers gamma; its quality line is short */
    {3, 1, 4, {2, 3, NONE}, 0, 2},             /* r3 on beta[4 .. 9]: two neighbouring mismatches */
    {3, 1, 4, {2, 3, NONE}, 1, 2},             /* ... and the same placement on the other strand: secondary, reversed */
};

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    groot_index_view v;
    memset(&v, 0, sizeof v);
    v.n_graphs = 2; v.n_nodes = 4; v.n_paths = 3; v.n_bases = 32; v.n_np = 5; v.path_words = 1;
    v.graph_node_off = graph_node_off; v.graph_path_off = graph_path_off; v.node_seq_off = node_seq_off; v.node_np_off = node_np_off;
    v.np_path = np_path; v.np_pos = np_pos; v.path_len = path_len; v.path_name_off = path_name_off;
    v.bases = (const uint8_t *)bases; v.path_names = path_names;
    groot_reads_view rv;
    memset(&rv, 0, sizeof rv);
    rv.n_reads = 4; rv.max_len = 10; rv.n_bases = 32;
    rv.seq_len = seq_len; rv.text = (const uint8_t *)text; rv.name_pos = name_pos; rv.name_len = name_len; rv.seq_pos = seq_pos;
    rv.qual_pos = qual_pos; rv.qual_len = qual_len;
    groot_bam *bam = NULL;
    if (groot_bam_open(argv[1], &v, "2020-01-01T00:00:00Z", &bam)) { printf("open: %s\n", groot_host_last_error()); return 1; }
    const uint64_t before = groot_bam_bytes_written(bam);
    int bad = 0;
    uint64_t n = 7;
    const groot_rescue_record refused[] = {
        {4, 0, 0, {NONE, NONE, NONE}, 0, 0},      /* a read that is not in the batch */
        {0, 3, 0, {NONE, NONE, NONE}, 0, 0},      /* a path that is not in the index */
        {0, 0, 9, {NONE, NONE, NONE}, 0, 0},      /* 10 bases at 9 of 18: over the path's end */
        {2, 2, 1, {NONE, NONE, NONE}, 0, 0},      /* ... by one base */
        {0, 0, 0, {NONE, NONE, NONE}, 2, 0},      /* no such strand */
        {0, 0, 0, {1, 2, 3}, 0, 4},               /* no such distance */
        {0, 0, 0, {10, NONE, NONE}, 0, 1},        /* an offset at the read's length */
        {0, 0, 0, {65534, NONE, NONE}, 0, 1},     /* ... and what a read of 65 535 bases could have: not this one */
        {0, 0, 0, {NONE, NONE, NONE}, 0, 1},      /* a missing offset */
        {0, 0, 0, {3, 3, NONE}, 0, 2},            /* not ascending */
        {0, 0, 0, {5, 2, NONE}, 0, 2},
        {0, 0, 0, {1, NONE, 2}, 0, 1},            /* an offset beyond d */
        {0, 0, 0, {1, 2, NONE}, 0, 1},
    };
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) {
        groot_rescue_record two[2] = {good[0], refused[i]};       /* behind a good record: that one must not be written either */
        n = 7;
        if (groot_bam_write_rescued(bam, &v, &rv, two, 2, &n) != GROOT_E_INVALID || n != 0) { printf("refusal %zu differs\n", i); bad++; }
    }
    bad += groot_bam_write_rescued(NULL, &v, &rv, good, 1, &n) != GROOT_E_INVALID;
    bad += groot_bam_write_rescued(bam, NULL, &rv, good, 1, &n) != GROOT_E_INVALID;
    bad += groot_bam_write_rescued(bam, &v, NULL, good, 1, &n) != GROOT_E_INVALID;
    bad += groot_bam_write_rescued(bam, &v, &rv, NULL, 1, &n) != GROOT_E_INVALID;
    bad += groot_bam_write_rescued(bam, &v, &rv, NULL, 0, &n) != GROOT_OK || n != 0;      /* an empty list is fine */
    bad += groot_bam_bytes_written(bam) != before;
    if (bad) { printf("%d refusals differ\n", bad); return 1; }
    /* two calls, as two batches: the first record of a call is never secondary */
    if (groot_bam_write_rescued(bam, &v, &rv, good, 3, &n) || n != 3) { printf("write: %s\n", groot_host_last_error()); return 1; }
    if (groot_bam_write_rescued(bam, &v, &rv, good + 3, 3, &n) || n != 3) { printf("write: %s\n", groot_host_last_error()); return 1; }
    if (groot_bam_close(bam)) { printf("close: %s\n", groot_host_last_error()); return 1; }
    printf("ok\n");
    return 0;
}
