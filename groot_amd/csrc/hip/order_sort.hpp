// order_sort.hpp -- the processing-order sort under the project's own launcher.
//
// rocprim's onesweep radix sort of (u32 key, u32 value) pairs, device code unchanged: rocprim::detail::onesweep_histograms,
// onesweep_scan_histograms and onesweep_iteration at 256 threads x GROOT_SORT_ITEMS items, 8-bit digits, block_radix_rank_algorithm::match,
// ordered block ids -- the same digits and the same stable rank as rocprim::radix_sort_pairs<OrderSortConfig>, so the result is bit-identical.
// What differs is the host side.  rocprim's host loop clears its scratch between the kernels (one hipMemsetAsync of the histograms, then per
// iteration one of the look-back states and one of the block id): seven fills per three-digit sort, each between two dependent kernels.  Here
// the histograms, one look-back array per iteration and one block-id word per iteration lie in ONE contiguous run of words, the "state", which
// is all zero between two sorts: a sort dirties a prefix of it (laid out for its own n and digit count), and ONE hipMemsetAsync
// (order_sort::clear) zeroes that prefix again, whenever the caller likes after the last iteration.  No fill sits between two sort kernels.
//
// Self-contained: HIP + rocprim only, no ctx types (tools/order_sort_check.hip includes it alone).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>      // (rocprim's texture_cache_iterator.hpp calls memset without including it)

#include <rocprim/rocprim.hpp>

#ifndef GROOT_SORT_ITEMS
#define GROOT_SORT_ITEMS 16
#endif

namespace groot {
namespace order_sort {

constexpr unsigned kThreads = 256, kItems = GROOT_SORT_ITEMS, kRadixBits = 8, kRadix = 1u << kRadixBits, kTile = kThreads * kItems;
constexpr unsigned kMaxPlaces = (32 + kRadixBits - 1) / kRadixBits;
constexpr uint32_t kMaxItems = (1u << 30) - (1u << 30) % kTile;      // one launch per iteration (rocprim cuts larger inputs into batches of this size)

using BlockId = rocprim::detail::block_id_wrapper<unsigned int, true>;   // ordered (atomic) block ids: what rocprim takes on gfx942 / gfx950
using Lookback = rocprim::detail::onesweep_lookback_state;
static_assert(sizeof(Lookback) == sizeof(uint32_t), "the state is laid out in 32-bit words");

inline unsigned places(unsigned begin_bit, unsigned end_bit) { return (end_bit - begin_bit + kRadixBits - 1) / kRadixBits; }
inline size_t tiles(size_t n) { return (n + kTile - 1) / kTile; }
// words of the state a sort of n items over `places` digits dirties: the histograms, a look-back array per iteration, a block-id word per iteration
inline size_t state_words(size_t n, unsigned places) { return (size_t)places * kRadix + (size_t)places * kRadix * tiles(n) + places; }

// One allocation for sorts of up to cap items (a view: whoever allocated base frees it): [ state (zero between sorts) | 256 offsets the last workgroup writes, never read | keys_tmp | vals_tmp ]
struct Scratch {
    uint32_t *base = nullptr;
    size_t cap = 0;                                           // items
    static size_t bytes(size_t cap) { return (state_words(cap, kMaxPlaces) + kRadix + 2 * cap) * sizeof(uint32_t); }
    size_t state_bytes() const { return state_words(cap, kMaxPlaces) * sizeof(uint32_t); }
    uint32_t *offs_out() const { return base + state_words(cap, kMaxPlaces); }
    uint32_t *keys_tmp() const { return offs_out() + kRadix; }
    uint32_t *vals_tmp() const { return keys_tmp() + cap; }
};

static __global__ __launch_bounds__(kThreads) void hist_kernel(const uint32_t *keys, uint32_t *hist, uint32_t n, uint32_t full_tiles, unsigned begin_bit, unsigned end_bit)
{
    rocprim::detail::onesweep_histograms<kThreads, kItems, kRadixBits, false>(keys, hist, n, full_tiles, rocprim::identity_decomposer{}, begin_bit, end_bit);
}

static __global__ __launch_bounds__(kThreads) void scan_kernel(uint32_t *hist) { rocprim::detail::onesweep_scan_histograms<kThreads, kRadixBits>(hist); }

static __global__ __launch_bounds__(kThreads) void iteration_kernel(const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *vals_in, uint32_t *vals_out, uint32_t n,
                                                             uint32_t *offs_in, uint32_t *offs_out, Lookback *lookback, unsigned bit, unsigned radix_bits,
                                                             uint32_t full_tiles, BlockId bid)
{
    rocprim::detail::onesweep_iteration<kThreads, kItems, kRadixBits, false, rocprim::block_radix_rank_algorithm::match>(
        keys_in, keys_out, vals_in, vals_out, n, offs_in, offs_out, lookback, rocprim::identity_decomposer{}, bit, radix_bits, full_tiles, bid);
}

// Sorts (keys_in, vals_in)[0, n) by the bits [begin_bit, end_bit) of the key, stable, into (keys_out, vals_out).  The inputs are left as they are and
// may not overlap the outputs.  The state of sc must be all zero; it is not afterwards: order_sort_clear with the same n and bits, on the same
// stream or behind this sort, before the next one.
inline hipError_t sort_pairs(const Scratch &sc, const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *vals_in, uint32_t *vals_out, uint32_t n,
                             unsigned begin_bit, unsigned end_bit, hipStream_t stream)
{
    if (n == 0 || end_bit <= begin_bit) return hipSuccess;
    if (!sc.base || n > sc.cap || n > kMaxItems || end_bit > 32) return hipErrorInvalidValue;
    const unsigned np = places(begin_bit, end_bit);
    const uint32_t nt = (uint32_t)tiles(n), full = n % kTile == 0 ? nt : nt - 1;
    uint32_t *hist = sc.base;
    uint32_t *lookback = hist + (size_t)np * kRadix;
    uint32_t *bid = lookback + (size_t)np * kRadix * nt;
    hipLaunchKernelGGL(hist_kernel, dim3(nt), dim3(kThreads), 0, stream, keys_in, hist, n, full, begin_bit, end_bit);
    hipLaunchKernelGGL(scan_kernel, dim3(np), dim3(kThreads), 0, stream, hist);
    // the last iteration writes the outputs; the ones before it alternate between the outputs and the scratch copies
    bool to_output = (np - 1) % 2 == 0;
    const uint32_t *kin = keys_in, *vin = vals_in;
    for (unsigned p = 0, bit = begin_bit; p < np; ++p, bit += kRadixBits) {
        uint32_t *kout = to_output ? keys_out : sc.keys_tmp(), *vout = to_output ? vals_out : sc.vals_tmp();
        const unsigned radix_bits = end_bit - bit < kRadixBits ? end_bit - bit : kRadixBits;
        hipLaunchKernelGGL(iteration_kernel, dim3(nt), dim3(kThreads), 0, stream, kin, kout, vin, vout, n, hist + (size_t)p * kRadix, sc.offs_out(),
                           reinterpret_cast<Lookback *>(lookback + (size_t)p * kRadix * nt), bit, radix_bits, full, BlockId::create(bid + p));
        kin = kout; vin = vout;
        to_output = !to_output;
    }
    return hipGetLastError();
}

// the ONE fill per sort: zeroes what sort_pairs(sc, ..., n, begin_bit, end_bit) dirtied
inline hipError_t clear(const Scratch &sc, uint32_t n, unsigned begin_bit, unsigned end_bit, hipStream_t stream)
{
    if (n == 0 || end_bit <= begin_bit || !sc.base) return hipSuccess;
    return hipMemsetAsync(sc.base, 0, state_words(n, places(begin_bit, end_bit)) * sizeof(uint32_t), stream);
}

// (re)allocates for cap items and zeroes the state.  The caller makes sure that nothing that uses the old block is still in flight.
inline hipError_t reserve(Scratch &sc, size_t cap, hipStream_t stream)
{
    if (sc.base && cap <= sc.cap) return hipSuccess;
    if (sc.base) (void)hipFree(sc.base);
    sc.base = nullptr;
    sc.cap = 0;
    hipError_t e = hipMalloc((void **)&sc.base, Scratch::bytes(cap));
    if (e != hipSuccess) return e;
    sc.cap = cap;
    return hipMemsetAsync(sc.base, 0, sc.state_bytes(), stream);
}

inline void release(Scratch &sc)
{
    if (sc.base) (void)hipFree(sc.base);
    sc.base = nullptr;
    sc.cap = 0;
}

} // namespace order_sort
} // namespace groot
