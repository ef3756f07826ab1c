/* indels_check.c -- groot_host_indels_write (include/groot_host.h, "Indels") on hand-made tables, as a stand-alone program: built with
 * the host library's report.cpp under -fsanitize=address,undefined (tests/test_indels.py) it writes the file of the three-path view of
 * tools/variants_check.c (a name with the '*' mark, an 'N' among the deleted bases, a DEL of a path's last base, an INS behind a path's
 * last base, an INS of eight bases, two events at one position, the share 0.1 met exactly) under several thresholds to stdout, one
 * "== case" line ahead of each, and checks every refused input.  The test compares the bytes with its plain-Python restatement of the
 * writer on the same tables. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "groot_host.h"

/* graph 0: nodes 0 "ACGTN", 1 "GGA", 2 "TTT"; paths "*alpha" = 0,1 and "beta" = 0,2 (8 bases each).  graph 1: node 3 "CAT", path "gamma". */
static const uint32_t graph_node_off[] = {0, 3, 4}, graph_path_off[] = {0, 2, 3};
static const uint32_t node_seq_off[] = {0, 5, 8, 11, 14}, node_np_off[] = {0, 2, 3, 4, 5};
static const uint32_t np_path[] = {0, 1, 0, 1, 0}, np_pos[] = {0, 0, 5, 5, 0};
static const uint32_t path_len[] = {8, 8, 3}, path_name_off[] = {0, 6, 10, 15};
static const char bases[] = "ACGTNGGATTTCAT", path_names[] = "*alphabetagamma";

/* per path base: gap depth, rescued depth, exact depth */
static const uint64_t gdepth[19] = {0, 5, 0, 2, 0, 9, 1, 0, /**/ 0, 10, 0, 0, 0, 0, 0, 0, /**/ 5, 0, 2};
static const uint64_t rescued[19] = {0, 1, 0, 0, 0, 3, 0, 0, /**/ 0, 0, 0, 0, 0, 0, 0, 0, /**/ 0, 0, 6};
static const uint64_t exact[19] = {0, 4, 0, 16, 0, 0, 0, 0, /**/ 0, 30, 0, 0, 0, 0, 0, 0, /**/ 5, 0, 0};
/* path, pos, type, len, seq, reserved, reads */
static const groot_gap_event events[8] = {
    {0, 1, GROOT_GAP_DEL, 2, 0, 0, 3}, {0, 3, GROOT_GAP_DEL, 1, 0, 0, 2}, {0, 5, GROOT_GAP_INS, 3, 11, 0, 4}, {0, 6, GROOT_GAP_DEL, 1, 0, 0, 1},
    {1, 1, GROOT_GAP_INS, 1, 1, 0, 4}, {1, 1, GROOT_GAP_INS, 8, 58596, 0, 6}, {2, 0, GROOT_GAP_DEL, 2, 0, 0, 5}, {2, 2, GROOT_GAP_INS, 1, 3, 0, 2}};

int main(void)
{
    groot_index_view v;
    memset(&v, 0, sizeof v);
    v.n_graphs = 2; v.n_nodes = 4; v.n_paths = 3; v.n_bases = 14; v.n_np = 5; v.path_words = 1;
    v.graph_node_off = graph_node_off; v.graph_path_off = graph_path_off; v.node_seq_off = node_seq_off; v.node_np_off = node_np_off;
    v.np_path = np_path; v.np_pos = np_pos; v.path_len = path_len; v.path_name_off = path_name_off;
    v.bases = (const uint8_t *)bases; v.path_names = path_names;
    const struct { uint64_t min_reads; double min_share; } cases[] = {{1, 0.0}, {0, 0.0}, {2, 0.1}, {3, 0.5}, {1, 0.1}, {1, 1.0}, {100, 0.0}};
    for (size_t i = 0; i < sizeof cases / sizeof cases[0]; i++) {
        uint64_t n = ~0ull;
        printf("== case %llu %.4f\n", (unsigned long long)cases[i].min_reads, cases[i].min_share);
        fflush(stdout);
        const int rc = groot_host_indels_write(&v, events, 8, gdepth, rescued, exact, cases[i].min_reads, cases[i].min_share, NULL, &n);
        if (rc) { printf("error %d: %s\n", rc, groot_host_last_error()); return 1; }
        printf("== %llu lines\n", (unsigned long long)n);
    }
    uint64_t n = ~0ull;                      /* no events: an empty file */
    if (groot_host_indels_write(&v, NULL, 0, gdepth, rescued, exact, 1, 0.0, NULL, &n) || n) { printf("no events: %llu lines\n", (unsigned long long)n); return 1; }
    int bad = 0;
    bad += groot_host_indels_write(NULL, events, 8, gdepth, rescued, exact, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_indels_write(&v, NULL, 8, gdepth, rescued, exact, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_indels_write(&v, events, 8, NULL, rescued, exact, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_indels_write(&v, events, 8, gdepth, NULL, exact, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_indels_write(&v, events, 8, gdepth, rescued, NULL, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_indels_write(&v, events, 8, gdepth, rescued, exact, 1, -0.1, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_indels_write(&v, events, 8, gdepth, rescued, exact, 1, 1.5, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_indels_write(&v, events, 8, gdepth, rescued, exact, 1, 0.0, "/nonexistent-dir/x.tsv", NULL) != GROOT_E_IO;
    /* one event each that no device gives: a path and a pos outside the index, a DEL that runs over the end of its path, a type, two lengths, a
     * DEL with a sequence, an INS with more sequence than bases, more reads than the gap depth at pos */
    const groot_gap_event wrong[] = {{3, 0, GROOT_GAP_DEL, 1, 0, 0, 1}, {0, 8, GROOT_GAP_INS, 1, 0, 0, 1}, {0, 6, GROOT_GAP_DEL, 2, 0, 0, 1}, {0, 1, 2, 1, 0, 0, 1},
                                     {0, 1, GROOT_GAP_DEL, 0, 0, 0, 1}, {0, 1, GROOT_GAP_INS, 9, 0, 0, 1}, {0, 1, GROOT_GAP_DEL, 1, 1, 0, 1}, {0, 1, GROOT_GAP_INS, 1, 4, 0, 1},
                                     {0, 1, GROOT_GAP_DEL, 1, 0, 0, 6}};
    for (size_t i = 0; i < sizeof wrong / sizeof wrong[0]; i++) {
        groot_gap_event ev[8];
        memcpy(ev, events, sizeof ev);
        ev[7] = wrong[i];
        if (groot_host_indels_write(&v, ev, 8, gdepth, rescued, exact, 1, 0.0, NULL, NULL) != GROOT_E_INVALID) { printf("wrong event %zu was taken\n", i); bad++; }
    }
    if (bad) { printf("%d refusals differ\n", bad); return 1; }
    printf("ok\n");
    return 0;
}
