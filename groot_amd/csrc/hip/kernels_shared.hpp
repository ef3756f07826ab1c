// kernels_shared.hpp -- reads shared between references on the device (groot_hip_shared_*): for every pair of global paths a <= b the
// number of reads with at least one record on a and one on b, accumulated batch by batch behind the order stage.
//
// S(r) = the global paths that carry a record of read r: every set bit p of every traversal's path set, at graph_path_off[graph] + p
// (groot_host_expand_alns emits exactly one record per set bit).  The traversals of a read are contiguous and in (graph ascending,
// DFS) order, so S(r) is a list of segments (g, the OR of the path sets of r's traversals in g), one per graph, ascending: pw words
// per segment, whatever the size of the set.  Reads in up to kSharedSegs graphs take the fast path (on arg-annot.90, 100 bp reads:
// 97.5 % in one graph, the rest in two or three); reads in more graphs take the slow path.
//
// Per batch, four kernels on the align stream:
//   shared_gather_kernel   one thread per read (the thread of its first traversal): writes read r's segments, or lists the read for
//                          the slow path.
//   shared_insert_kernel   the same threads: hash the set into an open-addressing table of 2^k >= 2 n_reads slots; the first read of
//                          a set owns a slot (CAS), the others compare their set word for word with the owner's and add 1 to its count.
//                          Different sets with one hash probe on: a collision costs a probe, never a wrong count.
//   shared_slow_kernel     one wave per listed read: the exact set from its traversals, 1 added to every pair (a, b), a <= b.
//   shared_expand_kernel   one thread per table slot: count added to every pair of the owner's set, then the slot is cleared.
// With equivalence classes on (kernels_ec.hpp) gather and insert run too, and ec_merge_kernel between insert and expand; with shared
// reads off, expand only clears the table.
// So the triangle sees one u64 atomic per (distinct set, pair) and per (slow read, pair), not one per (read, pair).
// Every kernel reads the pass's status word first: a pass collect redoes, or a batch that fails with NOSPACE, is not counted.
#pragma once

#include "kernels_common.hpp"
#include "kernels_cov.hpp"   // kCovSkipFlags

namespace groot {

constexpr uint32_t kSharedEmpty = 0xFFFFFFFFu;   // table slot without an owner / unused segment / (segment 0) read on the slow path
constexpr uint32_t kSharedSegs = 4;              // graphs per read on the fast path

struct SharedArgs {
    const groot_trav *trav;        // the batch's records in (read, ord) order
    const uint64_t *mask;          // their path sets, pw words each
    const DeviceCounters *ctr;     // n_trav + flags of the pass
    const uint32_t *graph_path_off;
    uint32_t *set_graph;           // [max_batch_reads * kSharedSegs] graph of segment k of read r, kSharedEmpty = none
    uint64_t *set_mask;            // [max_batch_reads * kSharedSegs * pw] its path set (the OR over r's traversals in that graph)
    uint32_t *tab_rep;             // [tab_size] read owning the slot, kSharedEmpty = free
    uint32_t *tab_cnt;             // [tab_size] reads with the owner's set
    uint32_t *slow;                // [max_batch_reads] first traversal of every slow-path read
    uint32_t *batch;               // [3] of this batch: reads with a record, distinct fast-path sets, slow-path reads
    unsigned long long *tri;       // upper triangle, row a = pairs (a, a..n_paths-1)
    unsigned long long *stats;     // [3] totals of `batch` since enable / reset
    uint32_t cap, pw, first_read_id, n_paths, tab_mask;
    uint32_t max_segs;             // graphs per read on the fast path: kSharedSegs (1 under GROOT_TEST_SHARED_SLOW)
    uint32_t pairs;                // shared reads are on: expand adds to the triangle (else it only clears the table: equivalence classes)
};

__device__ __forceinline__ bool shared_live(const SharedArgs &a) { return !(a.ctr->flags & kCovSkipFlags); }

__device__ __forceinline__ uint64_t tri_index(uint64_t x, uint64_t y, uint64_t n) { return x * n - x * (x - 1) / 2 + (y - x); }

// (x, y) += c; x <= y as the segments ascend (a bit past the index's paths is never set: dropped rather than written out of bounds)
__device__ __forceinline__ void shared_add(const SharedArgs &a, uint64_t x, uint64_t y, unsigned long long c)
{
    const uint64_t lo = min(x, y), hi = max(x, y);
    if (hi < a.n_paths) atomicAdd(a.tri + tri_index(lo, hi, a.n_paths), c);
}

// t starts a read: its first traversal
__device__ __forceinline__ bool read_start(const SharedArgs &a, uint32_t t) { return t == 0 || a.trav[t].read_id != a.trav[t - 1].read_id; }

__device__ __forceinline__ uint64_t shared_hash(const SharedArgs &a, uint32_t r)
{
    uint64_t h = 0x9E3779B97F4A7C15ull;
    auto mix = [&](uint64_t v) {
        h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
        h ^= h >> 31; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 29;
    };
    for (uint32_t k = 0; k < kSharedSegs && a.set_graph[r * kSharedSegs + k] != kSharedEmpty; k++) {
        mix(a.set_graph[r * kSharedSegs + k]);
        const uint64_t *m = a.set_mask + ((size_t)r * kSharedSegs + k) * a.pw;
        for (uint32_t w = 0; w < a.pw; w++) mix(m[w]);
    }
    return h;
}

__device__ __forceinline__ bool same_set(const SharedArgs &a, uint32_t r, uint32_t q)
{
    for (uint32_t k = 0; k < kSharedSegs; k++) {
        const uint32_t g = a.set_graph[r * kSharedSegs + k];
        if (g != a.set_graph[q * kSharedSegs + k]) return false;
        if (g == kSharedEmpty) return true;
        const uint64_t *x = a.set_mask + ((size_t)r * kSharedSegs + k) * a.pw, *y = a.set_mask + ((size_t)q * kSharedSegs + k) * a.pw;
        for (uint32_t w = 0; w < a.pw; w++)
            if (x[w] != y[w]) return false;
    }
    return true;
}

// sum of v over the block, added once to *dst
__device__ __forceinline__ void block_add(uint32_t v, uint32_t *dst)
{
    __shared__ uint32_t acc;
    if (threadIdx.x == 0) acc = 0;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&acc, v);
    __syncthreads();
    if (threadIdx.x == 0 && acc) atomicAdd(dst, acc);
}

__global__ __launch_bounds__(kBlock) void shared_gather_kernel(SharedArgs a)
{
    if (!shared_live(a)) return;
    const uint32_t n = min(a.ctr->n_trav, a.cap);
    uint32_t reads = 0;
    for (uint32_t t0 = blockIdx.x * kBlock + threadIdx.x; t0 < n; t0 += gridDim.x * kBlock) {
        if (!read_start(a, t0)) continue;
        const uint32_t rid = a.trav[t0].read_id, r = rid - a.first_read_id;
        uint32_t t1 = t0 + 1, segs = 1;
        for (; t1 < n && a.trav[t1].read_id == rid; t1++) segs += a.trav[t1].graph_id != a.trav[t1 - 1].graph_id;
        reads++;
        uint32_t *sg = a.set_graph + (size_t)r * kSharedSegs;
        if (segs > a.max_segs) {
            sg[0] = kSharedEmpty;
            a.slow[atomicAdd(&a.batch[2], 1u)] = t0;   // (slow-path reads are rare: one atomic each)
            continue;
        }
        uint32_t k = 0;
        for (uint32_t s = t0; s < t1; k++) {
            uint32_t e = s + 1;
            while (e < t1 && a.trav[e].graph_id == a.trav[s].graph_id) e++;
            sg[k] = a.trav[s].graph_id;
            for (uint32_t w = 0; w < a.pw; w++) {
                uint64_t m = 0;
                for (uint32_t t = s; t < e; t++) m |= a.mask[(size_t)t * a.pw + w];
                a.set_mask[((size_t)r * kSharedSegs + k) * a.pw + w] = m;
            }
            s = e;
        }
        for (; k < kSharedSegs; k++) sg[k] = kSharedEmpty;
    }
    block_add(reads, &a.batch[0]);
}

__global__ __launch_bounds__(kBlock) void shared_insert_kernel(SharedArgs a)
{
    if (!shared_live(a)) return;
    const uint32_t n = min(a.ctr->n_trav, a.cap);
    uint32_t owned = 0;
    for (uint32_t t0 = blockIdx.x * kBlock + threadIdx.x; t0 < n; t0 += gridDim.x * kBlock) {
        if (!read_start(a, t0)) continue;
        const uint32_t r = a.trav[t0].read_id - a.first_read_id;
        if (a.set_graph[(size_t)r * kSharedSegs] == kSharedEmpty) continue;
        // the table holds at most n_reads owners in >= 2 n_reads slots: the probe ends
        for (uint32_t slot = (uint32_t)shared_hash(a, r) & a.tab_mask;; slot = (slot + 1) & a.tab_mask) {
            uint32_t cur = __hip_atomic_load(a.tab_rep + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kSharedEmpty) {
                cur = atomicCAS(a.tab_rep + slot, kSharedEmpty, r);
                if (cur == kSharedEmpty) { atomicAdd(a.tab_cnt + slot, 1u); owned++; break; }
            }
            if (same_set(a, cur, r)) { atomicAdd(a.tab_cnt + slot, 1u); break; }
        }
    }
    block_add(owned, &a.batch[1]);
}

// one wave per slow-path read: S(r) = the concatenation, graph after graph (ascending), of the OR of each graph's path sets.  Lane l
// takes the elements k = l, l + 64, ... of S(r) as a and adds 1 to (a, b) for every element b >= a.
__global__ __launch_bounds__(kBlock) void shared_slow_kernel(SharedArgs a)
{
    if (!shared_live(a)) return;
    const uint32_t n = min(a.ctr->n_trav, a.cap), n_slow = a.batch[2];
    const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * (kBlock / 64);
    for (uint32_t i = blockIdx.x * (kBlock / 64) + threadIdx.x / 64; i < n_slow; i += waves) {
        const uint32_t t0 = a.slow[i], rid = a.trav[t0].read_id;
        uint32_t t1 = t0 + 1;
        while (t1 < n && a.trav[t1].read_id == rid) t1++;
        // word w of the segment of graph starting at traversal s (traversals s..e-1 of one graph)
        auto seg_word = [&](uint32_t s, uint32_t e, uint32_t w) {
            uint64_t m = 0;
            for (uint32_t t = s; t < e; t++) m |= a.mask[(size_t)t * a.pw + w];
            return m;
        };
        auto seg_end = [&](uint32_t s) {
            uint32_t e = s + 1;
            while (e < t1 && a.trav[e].graph_id == a.trav[s].graph_id) e++;
            return e;
        };
        uint32_t k = 0;
        for (uint32_t s = t0; s < t1;) {
            const uint32_t e = seg_end(s), ga = a.graph_path_off[a.trav[s].graph_id];
            for (uint32_t wa = 0; wa < a.pw; wa++) {
                for (uint64_t ma = seg_word(s, e, wa); ma; ma &= ma - 1, k++) {
                    if ((k & 63) != lane) continue;
                    const uint32_t pa = wa * 64 + (uint32_t)__builtin_ctzll(ma);
                    const uint64_t x = ga + pa;
                    // b in the same segment from a on, then every later segment
                    for (uint32_t s2 = s; s2 < t1;) {
                        const uint32_t e2 = s2 == s ? e : seg_end(s2), gb = a.graph_path_off[a.trav[s2].graph_id];
                        for (uint32_t wb = s2 == s ? wa : 0; wb < a.pw; wb++) {
                            uint64_t mb = seg_word(s2, e2, wb);
                            if (s2 == s && wb == wa) mb &= ~0ull << (pa & 63);
                            for (; mb; mb &= mb - 1) shared_add(a, x, gb + wb * 64 + (uint32_t)__builtin_ctzll(mb), 1ull);
                        }
                        s2 = e2;
                    }
                }
            }
            s = e;
        }
    }
}

__global__ __launch_bounds__(kBlock) void shared_expand_kernel(SharedArgs a, uint32_t tab_size)
{
    if (!shared_live(a)) return;
    for (uint32_t slot = blockIdx.x * kBlock + threadIdx.x; slot < tab_size; slot += gridDim.x * kBlock) {
        const uint32_t r = a.tab_rep[slot];
        if (r == kSharedEmpty) continue;
        const unsigned long long c = a.tab_cnt[slot];
        const uint32_t *sg = a.set_graph + (size_t)r * kSharedSegs;
        const uint64_t *m = a.set_mask + (size_t)r * kSharedSegs * a.pw;
        for (uint32_t i = 0; a.pairs && i < kSharedSegs && sg[i] != kSharedEmpty; i++) {
            const uint64_t gi = a.graph_path_off[sg[i]];
            for (uint32_t wa = 0; wa < a.pw; wa++) {
                for (uint64_t ma = m[i * a.pw + wa]; ma; ma &= ma - 1) {
                    const uint32_t pa = (uint32_t)__builtin_ctzll(ma);
                    const uint64_t x = gi + wa * 64 + pa;
                    // b: the rest of this segment from a on, then every later one
                    for (uint32_t j = i; j < kSharedSegs && sg[j] != kSharedEmpty; j++) {
                        const uint64_t gj = a.graph_path_off[sg[j]];
                        for (uint32_t wb = j == i ? wa : 0; wb < a.pw; wb++) {
                            uint64_t mb = m[j * a.pw + wb];
                            if (j == i && wb == wa) mb &= ~0ull << pa;
                            for (; mb; mb &= mb - 1) shared_add(a, x, gj + wb * 64 + (uint32_t)__builtin_ctzll(mb), c);
                        }
                    }
                }
            }
        }
        a.tab_rep[slot] = kSharedEmpty;
        a.tab_cnt[slot] = 0;
    }
    // the batch's counters into the totals, and zeroed for the next batch (every kernel of this batch before this one has ended)
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        a.stats[threadIdx.x] += a.batch[threadIdx.x];
        a.batch[threadIdx.x] = 0;
    }
}

} // namespace groot
