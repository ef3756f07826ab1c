/* variants_check.c -- groot_host_variants_write (include/groot_host.h, "Variants") on hand-made tables, as a stand-alone program: built
 * with the host library's report.cpp under -fsanitize=address,undefined (tests/test_variants.py) it writes the file of a three-path view
 * (a name with the '*' mark, an 'N' as ref, a path of three bases, counts at the first and last base of a path) under several
 * thresholds to stdout, one "== case" line ahead of each, and checks every refused input.  The test compares the bytes with its
 * plain-Python restatement of the writer on the same tables. */
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

/* per path base: rescued depth, exact depth, alt A C G T */
static const uint64_t rescued[19] = {3, 0, 4, 4, 9, 2, 0, 5, /**/ 0, 10, 0, 0, 1, 0, 0, 20, /**/ 6, 0, 7};
static const uint64_t exact[19] = {0, 7, 0, 16, 1, 0, 0, 5, /**/ 0, 30, 0, 0, 0, 0, 0, 0, /**/ 0, 0, 3};
static const uint64_t alt[76] = {0, 3, 0, 0, /**/ 0, 0, 0, 0, /**/ 1, 0, 0, 3, /**/ 2, 0, 2, 0, /**/ 4, 0, 5, 0, /**/ 0, 0, 0, 2, /**/ 0, 0, 0, 0, /**/ 0, 0, 0, 1,
                                0, 0, 0, 0, /**/ 4, 0, 0, 0, /**/ 0, 0, 0, 0, /**/ 0, 0, 0, 0, /**/ 0, 1, 0, 0, /**/ 0, 0, 0, 0, /**/ 0, 0, 0, 0, /**/ 2, 18, 0, 0,
                                0, 0, 6, 0, /**/ 0, 0, 0, 0, /**/ 0, 1, 0, 6};

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
        const int rc = groot_host_variants_write(&v, rescued, alt, exact, cases[i].min_reads, cases[i].min_share, NULL, &n);
        if (rc) { printf("error %d: %s\n", rc, groot_host_last_error()); return 1; }
        printf("== %llu lines\n", (unsigned long long)n);
    }
    int bad = 0;
    bad += groot_host_variants_write(NULL, rescued, alt, exact, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_variants_write(&v, NULL, alt, exact, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_variants_write(&v, rescued, NULL, exact, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_variants_write(&v, rescued, alt, NULL, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_variants_write(&v, rescued, alt, exact, 1, -0.1, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_variants_write(&v, rescued, alt, exact, 1, 1.5, NULL, NULL) != GROOT_E_INVALID;
    bad += groot_host_variants_write(&v, rescued, alt, exact, 1, 0.0, "/nonexistent-dir/x.tsv", NULL) != GROOT_E_IO;
    uint64_t alt2[76];                       /* an alt count above the rescued depth of its base */
    memcpy(alt2, alt, sizeof alt2);
    alt2[4 * 5 + 3] = 3;
    bad += groot_host_variants_write(&v, rescued, alt2, exact, 1, 0.0, NULL, NULL) != GROOT_E_INVALID;
    if (bad) { printf("%d refusals differ\n", bad); return 1; }
    printf("ok\n");
    return 0;
}
