// rescue_fold_check.cpp -- the two host folds of groot_amd/csrc/hip/rescue_fold.hpp (what rescue.hip does at collect with the bitmaps and
// the logs of a batch's slow rescued and gap-rescued reads) at their edges, as a stand-alone program on a CPU.  Every expected value is
// written out by hand.  Build and run from the repository root, under the sanitizers:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//         -Igroot_amd/csrc/hip -o build/rescue_fold_check tools/rescue_fold_check.cpp && build/rescue_fold_check
// (exit 0 and "rescue_fold_check: ok": every check held)
#include <cstdio>
#include <vector>

#include "rescue_fold.hpp"

using namespace groot;

static int failures = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

using Ids = std::vector<uint32_t>;
using Rows = std::vector<Ids>;
constexpr uint32_t kSecond = 0x80000000u;   // kGapAcovSecond (kernels_gap_acov.hpp)
constexpr uint64_t kAll = ~0ull;

static Ids range(uint32_t a, uint32_t b)    // a, a + 1, ..., b - 1
{
    Ids v;
    for (uint32_t i = a; i < b; i++) v.push_back(i);
    return v;
}

static void check_unfold()
{
    {   // no rows: nothing is read (bits may be null), nothing counted
        EcHost ec;
        uint64_t slow = 5;
        CHECK(unfold_rows(nullptr, 0, 3, 130, ec, slow).empty() && ec.empty() && slow == 5);
    }
    {   // one path, one word: bit 0 is the path, every other bit lies above n_paths
        const uint64_t bits[3] = {kAll, 1, kAll - 1};
        EcHost ec;
        uint64_t slow = 0;
        const Rows r = unfold_rows(bits, 3, 1, 1, ec, slow);
        CHECK((r == Rows{{0}, {0}, {}}));
        CHECK((ec == EcHost{{{0}, 2}}));                  // the row without an ID is no class ...
        CHECK(slow == 3);                                 // ... and a slow read all the same
    }
    {   // 63 paths: bit 62 is the last one, bit 63 is set and dropped
        const uint64_t bits[2] = {(1ull << 63) | (1ull << 62) | 1, 1ull << 63};
        EcHost ec;
        uint64_t slow = 0;
        CHECK((unfold_rows(bits, 2, 1, 63, ec, slow) == Rows{{0, 62}, {}}));
        CHECK((ec == EcHost{{{0, 62}, 1}}) && slow == 2);
    }
    {   // 64 paths fill the word: every bit counts, ascending; an all-zero row among them
        const uint64_t bits[3] = {kAll, 0, (1ull << 63) | 2};
        EcHost ec;
        uint64_t slow = 10;
        const Rows r = unfold_rows(bits, 3, 1, 64, ec, slow);
        CHECK(r.size() == 3 && r[0] == range(0, 64) && r[1].empty() && (r[2] == Ids{1, 63}));
        CHECK((ec == EcHost{{range(0, 64), 1}, {{1, 63}, 1}}) && slow == 13);
    }
    {   // 65 paths, two words: ID 64 is bit 0 of the second word, ID 65 (bit 1) is at n_paths and dropped; two rows with one set count twice
        const uint64_t bits[6] = {1ull << 63, 3, 0, 2, 1ull << 63, 1};
        EcHost ec;
        uint64_t slow = 0;
        CHECK((unfold_rows(bits, 3, 2, 65, ec, slow) == Rows{{63, 64}, {}, {63, 64}}));
        CHECK((ec == EcHost{{{63, 64}, 2}}) && slow == 3);
    }
    {   // 130 paths, three words: IDs 128 and 129 are bits 0 and 1 of the third word, bit 2 (ID 130) and everything above are dropped
        const uint64_t bits[6] = {1, 1, kAll, 0, 1ull << 63, 4};
        EcHost ec{{{0, 64, 128, 129}, 7}};                // (the map had this class already)
        uint64_t slow = 0;
        CHECK((unfold_rows(bits, 2, 3, 130, ec, slow) == Rows{{0, 64, 128, 129}, {127}}));
        CHECK((ec == EcHost{{{0, 64, 128, 129}, 8}, {{127}, 1}}) && slow == 2);
    }
}

static void check_fold()
{
    const Rows rows{{3, 5}, {}, {7}};
    {   // no entries: nothing is read (log may be null)
        AcovHost ac;
        uint64_t rec = 0, pl = 0;
        CHECK(fold_log(nullptr, 0, rows, kSecond, ac, rec, pl) == -1 && ac.empty() && rec == 0 && pl == 0);
    }
    {   // a DEL of row 0 (its second record carries the flag: two records, one placement), the same tuple twice, an INS of row 2
        const uint4 log[4] = {{0, 3, 10, 19}, {0 | kSecond, 3, 22, 40}, {0, 3, 10, 19}, {2, 7, 1, 2}};
        AcovHost ac;
        uint64_t rec = 100, pl = 200;
        CHECK(fold_log(log, 4, rows, kSecond, ac, rec, pl) == -1);
        CHECK((ac == AcovHost{{{3, 5}, {{{3, 10, 19}, 2}, {{3, 22, 40}, 1}}}, {{7}, {{{7, 1, 2}, 1}}}}));
        CHECK(rec == 104 && pl == 203);
    }
    {   // a log without the flag (the rescued reads'): every entry is a placement, and bit 31 is part of the row
        const uint4 log[2] = {{2, 7, 4, 9}, {0 | kSecond, 3, 1, 2}};
        AcovHost ac;
        uint64_t rec = 0, pl = 0;
        CHECK(fold_log(log, 2, rows, 0, ac, rec, pl) == (int64_t)kSecond);      // (no such row)
        CHECK((ac == AcovHost{{{7}, {{{7, 4, 9}, 1}}}}) && rec == 1 && pl == 1);
    }
    {   // an entry that names row n: the entries ahead of it are folded, none behind it
        const uint4 log[3] = {{0, 5, 1, 2}, {3, 5, 1, 2}, {2, 7, 1, 2}};
        AcovHost ac;
        uint64_t rec = 0, pl = 0;
        CHECK(fold_log(log, 3, rows, kSecond, ac, rec, pl) == 3);
        CHECK((ac == AcovHost{{{3, 5}, {{{5, 1, 2}, 1}}}}) && rec == 1 && pl == 1);
    }
    {   // an entry that names an empty row, with the flag: the row is reported without it
        const uint4 log[1] = {{1 | kSecond, 5, 1, 2}};
        AcovHost ac;
        uint64_t rec = 0, pl = 0;
        CHECK(fold_log(log, 1, rows, kSecond, ac, rec, pl) == 1 && ac.empty() && rec == 0 && pl == 0);
    }
    {   // no rows at all
        const uint4 log[1] = {{0, 0, 0, 0}};
        AcovHost ac;
        uint64_t rec = 0, pl = 0;
        CHECK(fold_log(log, 1, Rows{}, kSecond, ac, rec, pl) == 0 && ac.empty());
    }
}

// the log of the fragments on bitmaps (rescued mates in assigned coverage over fragments): an entry counts when its path is in its row's list
static void check_fold_units()
{
    const Rows rows{{3, 5}, {}, {7}};
    {   // no entries: nothing is read (log may be null)
        AcovHost ac;
        uint64_t n[4] = {1, 2, 3, 4};
        CHECK(fold_log_units(nullptr, 0, rows, kSecond, ac, n) == -1 && ac.empty() && n[0] == 1 && n[1] == 2 && n[2] == 3 && n[3] == 4);
    }
    {   // row 0 = {3, 5}: an exact record on 3 and a placement on 5 count, an exact record on 4 and placements on 2 and 6 (below, between
        // and above the list) are left out; the same tuple from both kinds lands in one cell
        const uint4 log[7] = {{0 | kSecond, 3, 10, 19}, {0, 5, 1, 9}, {0 | kSecond, 4, 10, 19}, {0, 2, 1, 9}, {0, 6, 1, 9}, {0, 3, 10, 19}, {2, 7, 0, 0}};
        AcovHost ac;
        uint64_t n[4] = {0, 0, 0, 0};
        CHECK(fold_log_units(log, 7, rows, kSecond, ac, n) == -1);
        CHECK((ac == AcovHost{{{3, 5}, {{{3, 10, 19}, 2}, {{5, 1, 9}, 1}}}, {{7}, {{{7, 0, 0}, 1}}}}));
        CHECK(n[0] == 1 && n[1] == 1 && n[2] == 3 && n[3] == 2);
    }
    {   // an entry that names row n, and one that names an empty row with the flag: reported without it, the entries ahead are folded
        const uint4 log[3] = {{2 | kSecond, 7, 1, 2}, {3, 5, 1, 2}, {2, 7, 1, 2}};
        AcovHost ac;
        uint64_t n[4] = {0, 0, 0, 0};
        CHECK(fold_log_units(log, 3, rows, kSecond, ac, n) == 3);
        CHECK((ac == AcovHost{{{7}, {{{7, 1, 2}, 1}}}}) && n[0] == 1 && n[1] == 0 && n[2] == 0 && n[3] == 0);
        const uint4 empty[1] = {{1 | kSecond, 5, 1, 2}};
        CHECK(fold_log_units(empty, 1, rows, kSecond, ac, n) == 1 && n[0] == 1 && n[1] == 0);
        CHECK(fold_log_units(empty, 1, Rows{}, kSecond, ac, n) == 1);
    }
}

int main()
{
    check_unfold();
    check_fold();
    check_fold_units();
    if (failures) { printf("rescue_fold_check: %d checks FAILED\n", failures); return 1; }
    printf("rescue_fold_check: ok\n");
    return 0;
}
