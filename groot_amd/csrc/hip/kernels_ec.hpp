// kernels_ec.hpp -- equivalence classes of reads on the device (groot_hip_ec_*): for every distinct S(r) (kernels_shared.hpp) the
// number of reads with exactly that set, accumulated over the whole run in a ctx-owned open-addressing table in HBM.
//
// The per-batch table of kernels_shared.hpp has already reduced the batch's fast-path reads to their distinct sets, one owner read
// each.  ec_merge_kernel (one thread per slot of that table, after insert and before expand) folds each owner's set into the run-wide
// table: a slot = a claim word (the epoch of the launch that claimed it, 0 = free), a fixed-size key (kSharedSegs graphs + kSharedSegs * pw
// mask words, unused segments kSharedEmpty / 0) and a u64 count.  No two threads of one launch carry the same key (the batch's sets
// are distinct), so a probe that meets a slot claimed in the current epoch moves on without comparing; a slot of an older epoch is
// complete (a kernel boundary lies between) and is compared word for word.  No lane ever waits for another.
//
// The host keeps the table at >= 2 x (keys it can hold after every batch in flight) slots and grows it, between two merges in
// align-stream order, by ec_rehash_kernel.  Slow-path reads (kernels_shared.hpp) are not in the table: ec_merge_kernel copies the
// batch's slow list (first and end traversal of each read) into a buffer the slot owns, and the host folds those reads' exact sets
// in at collect.  Every kernel reads the pass's status word first: a pass collect redoes is not counted.
// In paired mode (kernels_shared.hpp) the rows are units and ec_merge_kernel<true> lists the slow-path units: a read, or a fragment
// whose set is the intersection of its mates' sets (three words each, the host intersects).
#pragma once

#include "kernels_shared.hpp"

namespace groot {

struct EcTable {
    uint32_t *claim;               // [cap] epoch of the launch that claimed the slot, 0 = free
    uint32_t *graph;               // [cap * kSharedSegs]
    uint64_t *mask;                // [cap * kSharedSegs * pw]
    unsigned long long *cnt;       // [cap]
    uint32_t *serial;              // [cap] the slot's serial number: the table's fill when it was claimed (kernels_acov.hpp keys its tuples by it)
    uint32_t cap_mask;             // cap - 1 (cap a power of two)
};

__device__ __forceinline__ uint64_t ec_hash(const uint32_t *g, const uint64_t *m, uint32_t pw)
{
    uint64_t h = 0x2545F4914F6CDD1Dull;
    for (uint32_t k = 0; k < kSharedSegs && g[k] != kSharedEmpty; k++) {
        h ^= g[k] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        for (uint32_t w = 0; w < pw; w++) {
            h ^= m[k * pw + w] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
            h ^= h >> 31; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 29;
        }
    }
    h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33;
    return h;
}

// key (g, m) == the key of slot s
__device__ __forceinline__ bool ec_same(const EcTable &t, uint32_t s, const uint32_t *g, const uint64_t *m, uint32_t pw)
{
    for (uint32_t k = 0; k < kSharedSegs; k++) {
        const uint32_t x = t.graph[(size_t)s * kSharedSegs + k];
        if (x != g[k]) return false;
        if (x == kSharedEmpty) return true;
        const uint64_t *y = t.mask + ((size_t)s * kSharedSegs + k) * pw;
        for (uint32_t w = 0; w < pw; w++)
            if (y[w] != m[k * pw + w]) return false;
    }
    return true;
}

// adds c to key (g, m): an older slot with the key, or the first free one (claimed with `epoch`); fill counts claimed slots and
// numbers them (a rehash has no fill and carries the serial `ser`).  Returns the slot's serial.
__device__ __forceinline__ uint32_t ec_add(const EcTable &t, const uint32_t *g, const uint64_t *m, uint32_t pw, unsigned long long c, uint32_t epoch,
                                           bool compare, uint32_t *fill, uint32_t ser)
{
    // the host keeps at least half the slots free: the probe ends
    for (uint32_t s = (uint32_t)ec_hash(g, m, pw) & t.cap_mask;; s = (s + 1) & t.cap_mask) {
        uint32_t cur = __hip_atomic_load(t.claim + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(t.claim + s, 0u, epoch);
            if (cur == 0) {
                uint32_t k = 0;
                for (; k < kSharedSegs && g[k] != kSharedEmpty; k++) {
                    t.graph[(size_t)s * kSharedSegs + k] = g[k];
                    for (uint32_t w = 0; w < pw; w++) t.mask[((size_t)s * kSharedSegs + k) * pw + w] = m[k * pw + w];
                }
                for (; k < kSharedSegs; k++) {
                    t.graph[(size_t)s * kSharedSegs + k] = kSharedEmpty;
                    for (uint32_t w = 0; w < pw; w++) t.mask[((size_t)s * kSharedSegs + k) * pw + w] = 0;
                }
                t.cnt[s] = c;
                if (fill) ser = atomicAdd(fill, 1u);
                t.serial[s] = ser;
                return ser;
            }
        }
        if (cur == epoch || !compare) continue;   // claimed by this launch: another key
        if (ec_same(t, s, g, m, pw)) { atomicAdd(t.cnt + s, c); return t.serial[s]; }
    }
}

// one thread per slot of the batch's set table (tab_size slots); block 0 also lists the batch's slow-path reads:
// slow_out[0] = their number, then (first traversal, end traversal) per read.
// kPaired: three words per slow-path unit, (first traversal, end of the even mate's records, end traversal); the middle word equals
// the last for a read that is a unit by itself, and the host folds the intersection of the two ranges' sets otherwise.
// tab_ser (assigned coverage on, else null): [tab_size] the serial of every occupied slot's EC.
template <bool kPaired>
__global__ __launch_bounds__(kBlock) void ec_merge_kernel(SharedArgs a, EcTable t, uint32_t tab_size, uint32_t epoch, uint32_t *fill, uint32_t *slow_out,
                                                          uint32_t *tab_ser)
{
    if (!shared_live(a)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) slow_out[0] = 0;
        return;
    }
    const uint32_t n = min(a.ctr->n_trav, a.cap), n_reads = a.batch[2], n_slow = n_reads + (kPaired ? a.batch[6] : 0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) slow_out[0] = n_slow;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_slow; i += gridDim.x * kBlock) {
        if (kPaired && i >= n_reads) {
            const uint32_t t0 = a.slow[a.slow_cap - 1 - (i - n_reads)];
            uint32_t tm, t1;
            frag_span(a, t0, n, tm, t1);
            slow_out[1 + 3 * i] = t0;
            slow_out[2 + 3 * i] = tm;
            slow_out[3 + 3 * i] = t1;
            continue;
        }
        const uint32_t t0 = a.slow[i], rid = a.trav[t0].read_id;
        uint32_t t1 = t0 + 1;
        while (t1 < n && a.trav[t1].read_id == rid) t1++;
        if (kPaired) {
            slow_out[1 + 3 * i] = t0;
            slow_out[2 + 3 * i] = t1;
            slow_out[3 + 3 * i] = t1;
            continue;
        }
        slow_out[1 + 2 * i] = t0;
        slow_out[2 + 2 * i] = t1;
    }
    for (uint32_t slot = blockIdx.x * kBlock + threadIdx.x; slot < tab_size; slot += gridDim.x * kBlock) {
        const uint32_t r = a.tab_rep[slot];
        if (r == kSharedEmpty) continue;
        const uint32_t ser = ec_add(t, a.set_graph + (size_t)r * kSharedSegs, a.set_mask + (size_t)r * kSharedSegs * a.pw, a.pw, a.tab_cnt[slot], epoch, true, fill, 0);
        if (tab_ser) tab_ser[slot] = ser;
    }
}

// every key of `from` into the (empty, larger) table `to`: keys are distinct, so nothing is compared
__global__ __launch_bounds__(kBlock) void ec_rehash_kernel(EcTable from, uint32_t from_cap, EcTable to, uint32_t pw, uint32_t epoch)
{
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < from_cap; s += gridDim.x * kBlock) {
        if (!from.claim[s]) continue;
        ec_add(to, from.graph + (size_t)s * kSharedSegs, from.mask + (size_t)s * kSharedSegs * pw, pw, from.cnt[s], epoch, false, nullptr, from.serial[s]);
    }
}

// the occupied slots, compacted (in no particular order) into out_* (room for cap_out keys); *n_out counts them
__global__ __launch_bounds__(kBlock) void ec_export_kernel(EcTable t, uint32_t cap, uint32_t pw, uint32_t *out_graph, uint64_t *out_mask,
                                                           unsigned long long *out_cnt, uint32_t *out_ser, uint32_t *n_out, uint32_t cap_out)
{
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < cap; s += gridDim.x * kBlock) {
        if (!t.claim[s]) continue;
        const uint32_t i = atomicAdd(n_out, 1u);
        if (i >= cap_out) continue;
        for (uint32_t k = 0; k < kSharedSegs; k++) out_graph[(size_t)i * kSharedSegs + k] = t.graph[(size_t)s * kSharedSegs + k];
        for (uint32_t w = 0; w < kSharedSegs * pw; w++) out_mask[(size_t)i * kSharedSegs * pw + w] = t.mask[(size_t)s * kSharedSegs * pw + w];
        out_cnt[i] = t.cnt[s];
        out_ser[i] = t.serial[s];
    }
}

} // namespace groot
