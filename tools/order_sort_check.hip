// order_sort_check.hip -- the processing-order sort (groot_amd/csrc/hip/order_sort.hpp) against std::stable_sort, alone: no ctx, no library.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -Igroot_amd/csrc/hip -o build/order_sort_check tools/order_sort_check.hip && build/order_sort_check
//
// Every sort goes through ONE scratch block, and the only fills of that block are the driver's own: the one at allocation and the one
// order_sort::clear behind each sort.  A clear that is sized for another batch than the one that dirtied the block leaves look-back states or
// a block id behind, and the next sort through the block ranks against them: perm differs from the stable sort (or the sort's look-back reads
// a prefix that no workgroup of THIS sort wrote).  Sizes: 2 049, one onesweep tile and its two neighbours, 8 193, three tiles + 1, 100 000;
// keys: all equal, all 0xFFFFFFFF, two values, random 24-bit with a tenth 0xFFFFFFFF; bits [2, 8 | 9 | 10 | 16 | 17 | 18 | 26): one, two and
// three iterations with a partial last digit.  Then 100 000 -> 4 097 -> 100 000 through a fresh block.
// (tests/test_order_sort.py builds and runs it)
#include "order_sort.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

namespace os = groot::order_sort;

#define CHECK(expr)                                                                                  \
    do {                                                                                             \
        hipError_t e__ = (expr);                                                                     \
        if (e__ != hipSuccess) {                                                                     \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
            std::exit(2);                                                                            \
        }                                                                                            \
    } while (0)

static constexpr uint32_t kGuard = 64, kGuardWord = 0xA5A5A5A5u;
static constexpr unsigned kBeginBit = 2;

struct Bufs {
    uint32_t *keys_in = nullptr, *keys_out = nullptr, *vals_in = nullptr, *vals_out = nullptr;
    size_t cap = 0;
    void alloc(size_t n)
    {
        cap = n;
        CHECK(hipMalloc((void **)&keys_in, n * 4));
        CHECK(hipMalloc((void **)&vals_in, n * 4));
        CHECK(hipMalloc((void **)&keys_out, (n + kGuard) * 4));
        CHECK(hipMalloc((void **)&vals_out, (n + kGuard) * 4));
    }
};

enum KeyKind { kAllEqual, kAllOnes, kTwoValues, kRandom24, kKinds };
static const char *kind_name[kKinds] = {"all-equal", "all-ones", "two-values", "random24+ones"};

static std::vector<uint32_t> make_keys(KeyKind kind, uint32_t n, uint32_t seed)
{
    std::vector<uint32_t> k(n);
    std::mt19937 rng(seed);
    for (uint32_t i = 0; i < n; ++i) {
        switch (kind) {
        case kAllEqual: k[i] = 0x00123454u; break;
        case kAllOnes: k[i] = 0xFFFFFFFFu; break;
        case kTwoValues: k[i] = rng() & 1u ? 0x0003FFFCu : 0x00000404u; break;
        default: k[i] = rng() % 10u == 0 ? 0xFFFFFFFFu : rng() & 0x00FFFFFFu; break;
        }
    }
    return k;
}

// one sort of keys through sc (its state all zero), the driver's clear behind it, and the comparison; returns the number of failed checks
static int run_case(const os::Scratch &sc, const Bufs &b, const std::vector<uint32_t> &keys, unsigned end_bit, hipStream_t st, const char *what)
{
    const uint32_t n = (uint32_t)keys.size();
    std::vector<uint32_t> iota(n);
    std::iota(iota.begin(), iota.end(), 0u);
    CHECK(hipMemcpyAsync(b.keys_in, keys.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    CHECK(hipMemcpyAsync(b.vals_in, iota.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    CHECK(hipMemsetAsync(b.keys_out, 0xA5, ((size_t)n + kGuard) * 4, st));
    CHECK(hipMemsetAsync(b.vals_out, 0xA5, ((size_t)n + kGuard) * 4, st));
    CHECK(os::sort_pairs(sc, b.keys_in, b.keys_out, b.vals_in, b.vals_out, n, kBeginBit, end_bit, st));
    CHECK(os::clear(sc, n, kBeginBit, end_bit, st));
    std::vector<uint32_t> got_k((size_t)n + kGuard), got_v((size_t)n + kGuard), in_k(n), in_v(n);
    CHECK(hipMemcpyAsync(got_k.data(), b.keys_out, got_k.size() * 4, hipMemcpyDeviceToHost, st));
    CHECK(hipMemcpyAsync(got_v.data(), b.vals_out, got_v.size() * 4, hipMemcpyDeviceToHost, st));
    CHECK(hipMemcpyAsync(in_k.data(), b.keys_in, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    CHECK(hipMemcpyAsync(in_v.data(), b.vals_in, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    CHECK(hipStreamSynchronize(st));

    const uint32_t mask = (uint32_t)((1ull << (end_bit - kBeginBit)) - 1);
    auto digit = [&](uint32_t r) { return (keys[r] >> kBeginBit) & mask; };
    std::vector<uint32_t> want = iota;
    std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return digit(x) < digit(y); });
    int bad = 0;
    auto fail = [&](const char *msg, uint32_t i) {
        if (bad++ < 4) std::fprintf(stderr, "FAIL %s n=%u end_bit=%u: %s at %u\n", what, n, end_bit, msg, i);
    };
    for (uint32_t i = 0; i < n; ++i) {
        if (got_v[i] != want[i]) { fail("perm differs from the stable sort", i); break; }
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (got_k[i] != keys[want[i]]) { fail("sorted key is not the key of perm", i); break; }
    }
    for (uint32_t i = 0; i < kGuard; ++i) {
        if (got_k[n + i] != kGuardWord || got_v[n + i] != kGuardWord) { fail("write past the end of the output", n + i); break; }
    }
    if (in_k != keys) fail("input keys changed", 0);
    if (in_v != iota) fail("input values changed", 0);
    if (end_bit == 26) {      // every bit of the sorted range is set in 0xFFFFFFFF and in no 24-bit key: reads without seeds come last
        const uint32_t ones = (uint32_t)std::count(keys.begin(), keys.end(), 0xFFFFFFFFu);
        if (ones < n) {
            for (uint32_t i = 0; i < n; ++i) {
                if ((got_k[i] == 0xFFFFFFFFu) != (i >= n - ones)) { fail("0xFFFFFFFF is not last", i); break; }
            }
        }
    }
    return bad ? 1 : 0;
}

// the whole state of sc is zero again (what every sort relies on)
static int state_is_zero(const os::Scratch &sc, hipStream_t st, const char *what)
{
    std::vector<uint32_t> h(sc.state_bytes() / 4);
    CHECK(hipMemcpyAsync(h.data(), sc.base, sc.state_bytes(), hipMemcpyDeviceToHost, st));
    CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < h.size(); ++i) {
        if (h[i]) {
            std::fprintf(stderr, "FAIL %s: state word %zu is 0x%08x behind the clear\n", what, i, h[i]);
            return 1;
        }
    }
    return 0;
}

int main()
{
    const uint32_t sizes[] = {2049, 4095, 4096, 4097, 8193, 3 * 4096 + 1, 100000};
    const unsigned end_bits[] = {8, 9, 10, 16, 17, 18, 26};
    static_assert(os::kTile == 4096, "the sizes above are one onesweep tile and its neighbours");
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    Bufs b;
    b.alloc(100000);
    int failed = 0, cases = 0;
    {
        os::Scratch sc;
        CHECK(os::reserve(sc, 100000, st));
        for (uint32_t n : sizes) {
            for (int kind = 0; kind < kKinds; ++kind) {
                const std::vector<uint32_t> keys = make_keys((KeyKind)kind, n, 1234u + n + (uint32_t)kind);
                for (unsigned eb : end_bits) {
                    failed += run_case(sc, b, keys, eb, st, kind_name[kind]);
                    ++cases;
                }
            }
        }
        failed += state_is_zero(sc, st, "all cases through one block");
        os::release(sc);
    }
    {
        // a large batch, a small one, a large one through a fresh block that starts smaller than the first batch: grown once, then only the driver's clears
        os::Scratch sc;
        CHECK(os::reserve(sc, 5000, st));
        CHECK(hipStreamSynchronize(st));
        CHECK(os::reserve(sc, 100000, st));
        const uint32_t seq[] = {100000, 4097, 100000};
        for (int i = 0; i < 3; ++i) {
            const std::vector<uint32_t> keys = make_keys(kRandom24, seq[i], 99u + (uint32_t)i);
            failed += run_case(sc, b, keys, 26, st, "sequence");
            ++cases;
        }
        failed += state_is_zero(sc, st, "sequence");
        os::release(sc);
    }
    std::printf("order_sort_check: %d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
