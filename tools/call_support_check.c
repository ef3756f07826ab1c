/* call_support_check.c -- groot_host_call_support (include/groot_host.h, "bootstrap support for the calls") on hand-made tables, as a
 * stand-alone program: built with the host library's report.cpp under -fsanitize=address,undefined (tests/test_call_support.py) it shows
 * that the pileup stays inside its buffers at path lengths 1, 63, 64, 65 and 129, with records clipped at path_len - 1, overlapping
 * intervals, an EC no replicate drew, an EC the EM skips, n = 2^33, one and several threads, and on every refused input.  The expected
 * counts are those of the plain-Python restatement in that test file.  Prints "ok <tables>" and exits 0, or says what differs. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "groot_host.h"

/* shapes */
static const uint32_t t0_len[] = {1, 63, 64, 65, 129, 50};
static const uint64_t t0_off[] = {0ull, 1ull, 3ull, 4ull, 7ull, 9ull, 10ull, 12ull, 13ull, 16ull, 18ull, 19ull, 21ull, 22ull};
static const uint32_t t0_ids[] = {0, 0, 5, 1, 1, 2, 5, 1, 5, 2, 2, 5, 3, 3, 4, 5, 3, 5, 4, 4, 5, 5};
static const uint64_t t0_cnt[] = {2ull, 3ull, 5ull, 2ull, 6ull, 6ull, 4ull, 4ull, 8ull, 9ull, 7ull, 7ull, 5ull};
static const uint32_t t0_tup[] = {0, 0, 0, 0, 1, 0, 0, 0, 1, 5, 0, 49, 2, 1, 0, 40, 2, 1, 20, 62, 3, 1, 5, 50, 3, 2, 5, 50, 3, 5, 5, 45, 4, 1, 0, 62, 4, 1, 30, 62, 4, 5, 3, 40, 5, 2, 1, 63, 6, 2, 0, 63, 6, 2, 63, 63, 6, 5, 10, 49, 7, 3, 0, 63, 8, 3, 0, 64, 8, 4, 0, 128, 8, 4, 127, 128, 8, 5, 49, 49, 9, 3, 0, 64, 9, 3, 1, 63, 9, 5, 0, 20, 10, 4, 0, 100, 10, 4, 64, 128, 11, 4, 10, 80, 11, 4, 40, 128, 11, 4, 64, 64, 11, 5, 25, 49, 12, 5, 0, 49, 12, 5, 7, 7};
static const uint64_t t0_tn[] = {2ull, 2ull, 3ull, 3ull, 2ull, 1ull, 1ull, 2ull, 4ull, 2ull, 1ull, 6ull, 3ull, 1ull, 2ull, 4ull, 3ull, 3ull, 5ull, 8ull, 5ull, 4ull, 2ull, 4ull, 3ull, 3ull, 4ull, 1ull, 2ull, 5ull, 1ull};
static const uint64_t t0_bc[] = {8ull, 11ull, 10ull, 6ull, 11ull, 11ull, 11ull, 0ull, 5ull, 7ull, 3ull, 4ull, 7ull, 9ull, 6ull, 2ull, 8ull, 10ull, 2ull, 6ull, 4ull, 10ull, 0ull, 5ull, 10ull, 5ull, 1ull, 9ull, 11ull, 11ull, 11ull, 0ull, 8ull, 11ull, 6ull, 11ull, 7ull, 2ull, 5ull};
static const double t0_alpha[] = {6.344, 8.485, 5.991, 1.201, 4.481, 4.443, 0.0, 8.627, 3.149, 2.014, 4.699, 5.771, 8.452, 5.238, 2.411, 8.368, 4.426, 6.082};
static const uint32_t t0_sel[] = {0, 1, 2, 3, 4, 5};
static const uint32_t t0_want[] = {1, 63, 64, 0, 119, 50, 0, 63, 63, 64, 129, 50, 1, 63, 0, 65, 129, 50};

/* skipped EC */
static const uint32_t t1_len[] = {40, 40, 40};
static const uint64_t t1_off[] = {0ull, 1ull, 3ull, 5ull};
static const uint32_t t1_ids[] = {0, 0, 1, 1, 2};
static const uint64_t t1_cnt[] = {9ull, 2ull, 4ull};
static const uint32_t t1_tup[] = {0, 0, 0, 30, 1, 0, 2, 9, 1, 1, 2, 9, 2, 1, 0, 30, 2, 2, 4, 20};
static const uint64_t t1_tn[] = {9ull, 2ull, 2ull, 4ull, 4ull};
static const uint64_t t1_bc[] = {9ull, 2ull, 4ull, 8ull, 3ull, 4ull};
static const double t1_alpha[] = {11.0, 5.551115123125783e-17, 5.551115123125783e-17, 5.0, 3.0, 1.0};
static const uint32_t t1_sel[] = {0, 1, 2};
static const uint32_t t1_want[] = {31, 0, 0, 31, 31, 17};

/* D == f = 1/2 */
static const uint32_t t2_len[] = {10, 3};
static const uint64_t t2_off[] = {0ull, 1ull};
static const uint32_t t2_ids[] = {0};
static const uint64_t t2_cnt[] = {2ull};
static const uint32_t t2_tup[] = {0, 0, 2, 6};
static const uint64_t t2_tn[] = {1ull};
static const uint64_t t2_bc[] = {1ull};
static const double t2_alpha[] = {1.0, 0.0};
static const uint32_t t2_sel[] = {0, 1};
static const uint32_t t2_want[] = {0, 0};

/* D == f = 2/1 */
static const uint32_t t3_len[] = {10, 3};
static const uint64_t t3_off[] = {0ull, 1ull};
static const uint32_t t3_ids[] = {0};
static const uint64_t t3_cnt[] = {1ull};
static const uint32_t t3_tup[] = {0, 0, 2, 6};
static const uint64_t t3_tn[] = {1ull};
static const uint64_t t3_bc[] = {2ull};
static const double t3_alpha[] = {2.0, 0.0};
static const uint32_t t3_sel[] = {0, 1};
static const uint32_t t3_want[] = {5, 0};

/* n = 2^33 */
static const uint32_t t4_len[] = {20, 20};
static const uint64_t t4_off[] = {0ull, 1ull, 3ull};
static const uint32_t t4_ids[] = {0, 0, 1};
static const uint64_t t4_cnt[] = {8589934592ull, 4ull};
static const uint32_t t4_tup[] = {0, 0, 0, 15, 0, 0, 10, 19, 1, 0, 3, 12, 1, 1, 3, 12};
static const uint64_t t4_tn[] = {8589934592ull, 5ull, 2ull, 2ull};
static const uint64_t t4_bc[] = {1ull, 4ull, 3ull, 0ull};
static const double t4_alpha[] = {7.0, 1.0, 2.0, 2.0};
static const uint32_t t4_sel[] = {0, 1};
static const uint32_t t4_want[] = {16, 0, 16, 0};

struct table {
    const char *name;
    uint32_t n_paths;
    const uint32_t *len;
    uint64_t n_ec;
    const uint64_t *off;
    const uint32_t *ids;
    const uint64_t *cnt;
    uint64_t n_tuples;
    const uint32_t *tup;
    const uint64_t *tn;
    uint32_t n_boot;
    const uint64_t *bc;
    const double *alpha;
    double call_depth;
    uint32_t n_sel;
    const uint32_t *sel;
    const uint32_t *want;
};

static const struct table tables[] = {
    {"shapes", 6, t0_len, 13, t0_off, t0_ids, t0_cnt, 31, t0_tup, t0_tn, 3, t0_bc, t0_alpha, 3.0, 6, t0_sel, t0_want},
    {"skipped EC", 3, t1_len, 3, t1_off, t1_ids, t1_cnt, 5, t1_tup, t1_tn, 2, t1_bc, t1_alpha, 0.5, 3, t1_sel, t1_want},
    {"D == f = 1/2", 2, t2_len, 1, t2_off, t2_ids, t2_cnt, 1, t2_tup, t2_tn, 1, t2_bc, t2_alpha, 1.0, 2, t2_sel, t2_want},
    {"D == f = 2/1", 2, t3_len, 1, t3_off, t3_ids, t3_cnt, 1, t3_tup, t3_tn, 1, t3_bc, t3_alpha, 1.0, 2, t3_sel, t3_want},
    {"n = 2^33", 2, t4_len, 2, t4_off, t4_ids, t4_cnt, 4, t4_tup, t4_tn, 2, t4_bc, t4_alpha, 1.0, 2, t4_sel, t4_want},
};

static int run(const struct table *t, uint32_t threads, const uint32_t *tup, uint64_t n_tuples, uint32_t n_boot, uint32_t *got)
{
    return groot_host_call_support(t->n_paths, t->len, t->n_ec, t->off, t->ids, t->cnt, n_tuples, tup, t->tn, n_boot, t->bc, t->alpha, t->call_depth, t->n_sel,
                                   t->sel, threads, got);
}

int main(void)
{
    const size_t n_tables = sizeof tables / sizeof tables[0];
    for (size_t k = 0; k < n_tables; k++) {
        const struct table *t = &tables[k];
        const size_t n = (size_t)t->n_boot * t->n_sel;
        for (uint32_t threads = 1; threads <= 4; threads += 3) {
            uint32_t *got = malloc(n * sizeof *got);          /* exactly n_boot x n_sel: a write past it is the sanitizer's to find */
            if (!got) return 2;
            const int rc = run(t, threads, t->tup, t->n_tuples, t->n_boot, got);
            if (rc) { printf("%s: error %d: %s\n", t->name, rc, groot_host_last_error()); return 1; }
            for (size_t i = 0; i < n; i++)
                if (got[i] != t->want[i]) { printf("%s, %u thread(s): covered[%zu] = %u, expected %u\n", t->name, threads, i, got[i], t->want[i]); return 1; }
            free(got);
        }
    }
    /* the refused inputs, on the first table: an EC outside the list, a path that is not in its EC, last >= path_len, no replicates */
    const struct table *t = &tables[0];
    const uint32_t bad[3][4] = {{(uint32_t)t->n_ec, 5, 0, 3}, {0, 1, 0, 0}, {0, 0, 0, 1}};
    uint32_t *got = malloc((size_t)t->n_boot * t->n_sel * sizeof *got);
    if (!got) return 2;
    for (int i = 0; i < 3; i++)
        if (run(t, 2, bad[i], 1, t->n_boot, got) != GROOT_E_INVALID) { printf("bad tuple %d was not refused\n", i); return 1; }
    if (run(t, 2, t->tup, t->n_tuples, 0, got) != GROOT_E_INVALID) { printf("n_boot = 0 was not refused\n"); return 1; }
    free(got);
    printf("ok %zu\n", n_tables);
    return 0;
}
