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
//
// Paired mode (groot_hip_pairs_enable): shared_gather_paired_kernel takes the place of shared_gather_kernel and makes one row per
// unit -- a fragment's two mates intersected, or either mate alone -- and the slow, merge and expand kernels run as their kPaired
// instantiations, which also know the batch's slow fragments.  Insert, and everything that works on rows, is the same code either way;
// with pairing off the launches are the ones above, compiled from the same text as before (kPaired = false drops every branch).
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
    uint32_t slow_cap;             // paired mode: entries of `slow`; slow fragments are listed from its end down (batch[6] of them)
};

// `batch` and `stats` beyond [3], written in paired mode only (kPaired kernels): fragments joined, split, single; batch[6] = the
// batch's slow-path fragments (into stats[2] with the slow-path reads)
constexpr uint32_t kSharedStats = 6, kSharedBatch = 7;
constexpr uint32_t kSharedPairStats = 3;   // (host) stats[kSharedPairStats .. kSharedStats): the pairing counts -- joined, split, single

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

// ---- paired mode (groot_hip_pairs_enable) ----------------------------------------------------------------------------
// With pairing on, reads 2i and 2i+1 of a batch are the mates of fragment i (batch-relative: read_id - first_read_id).  With
// A = S(r_2i), B = S(r_2i+1): joined (A n B not empty: one unit, A n B), split (both non-empty, A n B empty: two units, A and B),
// single (one of them non-empty: one unit), none.  A fragment's records are contiguous, read 2i's before read 2i+1's, so one thread
// owns a fragment -- the thread of its first traversal -- and nobody else writes either mate's row.  A joined unit goes to the even
// mate's row; the odd mate's row gets kSharedEmpty as its first graph, which is what shared_insert_kernel skips at that read start.

// t starts a fragment: its first traversal
__device__ __forceinline__ bool frag_start(const SharedArgs &a, uint32_t t)
{
    return t == 0 || ((a.trav[t].read_id - a.first_read_id) >> 1) != ((a.trav[t - 1].read_id - a.first_read_id) >> 1);
}

// the fragment whose first traversal is t0: the even mate's records are [t0, tm), the odd mate's [tm, t1) (either may be empty, not both)
__device__ __forceinline__ void frag_span(const SharedArgs &a, uint32_t t0, uint32_t n, uint32_t &tm, uint32_t &t1)
{
    const uint32_t even = a.first_read_id + ((a.trav[t0].read_id - a.first_read_id) & ~1u);
    for (tm = t0; tm < n && a.trav[tm].read_id == even; tm++) {}
    for (t1 = tm; t1 < n && a.trav[t1].read_id == even + 1; t1++) {}
}

// the end of the run of records of one graph that starts at s (records [s, lim) of one read)
__device__ __forceinline__ uint32_t seg_end(const SharedArgs &a, uint32_t s, uint32_t lim)
{
    uint32_t e = s + 1;
    while (e < lim && a.trav[e].graph_id == a.trav[s].graph_id) e++;
    return e;
}

// word w of the OR of the path sets of records [s, e)
__device__ __forceinline__ uint64_t seg_or(const SharedArgs &a, uint32_t s, uint32_t e, uint32_t w)
{
    uint64_t m = 0;
    for (uint32_t t = s; t < e; t++) m |= a.mask[(size_t)t * a.pw + w];
    return m;
}

// word w of the OR of the path sets of those records of [s, e) that lie in graph g (0 when there is none)
__device__ __forceinline__ uint64_t graph_or(const SharedArgs &a, uint32_t s, uint32_t e, uint32_t g, uint32_t w)
{
    uint64_t m = 0;
    for (uint32_t t = s; t < e; t++)
        if (a.trav[t].graph_id == g) m |= a.mask[(size_t)t * a.pw + w];
    return m;
}

// one read as a unit, as shared_gather_kernel does it: the row of read r from records [t0, t1), or the read on the slow list
__device__ __forceinline__ void gather_read(const SharedArgs &a, uint32_t t0, uint32_t t1, uint32_t r)
{
    uint32_t segs = 0;
    for (uint32_t s = t0; s < t1; s = seg_end(a, s, t1)) segs++;
    uint32_t *sg = a.set_graph + (size_t)r * kSharedSegs;
    if (segs > a.max_segs) {
        sg[0] = kSharedEmpty;
        a.slow[atomicAdd(&a.batch[2], 1u)] = t0;
        return;
    }
    uint32_t k = 0;
    for (uint32_t s = t0; s < t1; k++) {
        const uint32_t e = seg_end(a, s, t1);
        sg[k] = a.trav[s].graph_id;
        for (uint32_t w = 0; w < a.pw; w++) a.set_mask[((size_t)r * kSharedSegs + k) * a.pw + w] = seg_or(a, s, e, w);
        s = e;
    }
    for (; k < kSharedSegs; k++) sg[k] = kSharedEmpty;
}

// one thread per fragment.  The two mates' ascending segment lists are merged: graphs in common only, masks ANDed word by word,
// segments whose AND is all zero dropped -- so the row is a canonical key (graphs ascend, no segment is empty, kSharedEmpty ends it).
// The first max_segs segments of the intersection are written as they are met; a fragment is a slow-path unit only when the
// intersection itself has more, whatever the mates have alone.
// kDefer (rescued mates in paired-end units: kernels_rescue_pairs.hpp): a fragment with records on one mate only makes no unit here and is
// not counted -- that mate's row starts with kSharedEmpty, which shared_insert_kernel skips, and rescue_pair_kernel makes the unit once
// the other mate's rescued set exists.  <false> is the kernel as it was, and the only one launched while that rule is off.
template <bool kDefer>
__global__ __launch_bounds__(kBlock) void shared_gather_paired_kernel(SharedArgs a)
{
    if (!shared_live(a)) return;
    const uint32_t n = min(a.ctr->n_trav, a.cap);
    uint32_t units = 0, joined = 0, split = 0, single = 0;
    for (uint32_t t0 = blockIdx.x * kBlock + threadIdx.x; t0 < n; t0 += gridDim.x * kBlock) {
        if (!frag_start(a, t0)) continue;
        uint32_t tm, t1;
        frag_span(a, t0, n, tm, t1);
        const uint32_t r0 = (a.trav[t0].read_id - a.first_read_id) & ~1u;     // the even mate's row; r0 + 1 the odd mate's
        if (tm == t0 || t1 == tm) {     // "has records" is decided here, from the traversals: the other mate's row is stale and stays unread
            if (kDefer) {
                a.set_graph[(size_t)(tm == t0 ? r0 + 1 : r0) * kSharedSegs] = kSharedEmpty;
                continue;
            }
            gather_read(a, t0, t1, tm == t0 ? r0 + 1 : r0);
            single++; units++;
            continue;
        }
        uint32_t *sg = a.set_graph + (size_t)r0 * kSharedSegs;
        uint32_t k = 0;
        for (uint32_t sa = t0, sb = tm; sa < tm && sb < t1;) {
            const uint32_t ga = a.trav[sa].graph_id, gb = a.trav[sb].graph_id;
            if (ga < gb) { sa = seg_end(a, sa, tm); continue; }
            if (gb < ga) { sb = seg_end(a, sb, t1); continue; }
            const uint32_t ea = seg_end(a, sa, tm), eb = seg_end(a, sb, t1);
            uint64_t any = 0;
            for (uint32_t w = 0; w < a.pw; w++) {
                const uint64_t m = seg_or(a, sa, ea, w) & seg_or(a, sb, eb, w);
                any |= m;
                if (k < a.max_segs) a.set_mask[((size_t)r0 * kSharedSegs + k) * a.pw + w] = m;     // (kept only if any: else segment k is written again)
            }
            if (any) {
                if (k < a.max_segs) sg[k] = ga;
                k++;
            }
            sa = ea; sb = eb;
        }
        if (k == 0) {                   // split: the two reads as today, each on its own path
            gather_read(a, t0, tm, r0);
            gather_read(a, tm, t1, r0 + 1);
            split++; units += 2;
            continue;
        }
        joined++; units++;
        sg[kSharedSegs] = kSharedEmpty;     // the odd mate: a read start without a unit, and not on the slow list
        if (k > a.max_segs) {
            sg[0] = kSharedEmpty;
            a.slow[a.slow_cap - 1 - atomicAdd(&a.batch[6], 1u)] = t0;
            continue;
        }
        for (; k < kSharedSegs; k++) sg[k] = kSharedEmpty;
    }
    block_add(units, &a.batch[0]);
    block_add(joined, &a.batch[3]);
    block_add(split, &a.batch[4]);
    block_add(single, &a.batch[5]);
}

// row r into the batch's table: the first row of a set owns a slot, the others add 1 to its count.  -> r owns its slot
// (also what kernels_rescue_ec.hpp does with the rows of the rescued reads, behind shared_expand_kernel)
__device__ __forceinline__ bool shared_insert_row(const SharedArgs &a, uint32_t r)
{
    // the table holds at most n_reads owners in >= 2 n_reads slots: the probe ends
    for (uint32_t slot = (uint32_t)shared_hash(a, r) & a.tab_mask;; slot = (slot + 1) & a.tab_mask) {
        uint32_t cur = __hip_atomic_load(a.tab_rep + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kSharedEmpty) {
            cur = atomicCAS(a.tab_rep + slot, kSharedEmpty, r);
            if (cur == kSharedEmpty) { atomicAdd(a.tab_cnt + slot, 1u); return true; }
        }
        if (same_set(a, cur, r)) { atomicAdd(a.tab_cnt + slot, 1u); return false; }
    }
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
        owned += shared_insert_row(a, r);
    }
    block_add(owned, &a.batch[1]);
}

// one wave per slow-path read: S(r) = the concatenation, graph after graph (ascending), of the OR of each graph's path sets.  Lane l
// takes the elements k = l, l + 64, ... of S(r) as a and adds 1 to (a, b) for every element b >= a.
// kPaired: entries i >= batch[2] are the batch's slow fragments (listed from the end of `slow` down).  The wave walks the even mate's
// segments, each ANDed with the odd mate's OR in the same graph: a graph the odd mate lacks, or an all-zero AND, has no element.
template <bool kPaired>
__global__ __launch_bounds__(kBlock) void shared_slow_kernel(SharedArgs a)
{
    if (!shared_live(a)) return;
    const uint32_t n = min(a.ctr->n_trav, a.cap), n_reads = a.batch[2], n_slow = n_reads + (kPaired ? a.batch[6] : 0u);
    const uint32_t lane = threadIdx.x & 63, waves = gridDim.x * (kBlock / 64);
    for (uint32_t i = blockIdx.x * (kBlock / 64) + threadIdx.x / 64; i < n_slow; i += waves) {
        const uint32_t t0 = a.slow[kPaired && i >= n_reads ? a.slow_cap - 1 - (i - n_reads) : i], rid = a.trav[t0].read_id;
        uint32_t t1 = t0 + 1, m0 = 0, m1 = 0;      // [m0, m1): the odd mate's records, for a fragment
        if (kPaired && i >= n_reads) {
            frag_span(a, t0, n, t1, m1);
            m0 = t1;
        } else {
            while (t1 < n && a.trav[t1].read_id == rid) t1++;
        }
        // word w of the segment of graph starting at traversal s (traversals s..e-1 of one graph)
        auto seg_word = [&](uint32_t s, uint32_t e, uint32_t w) {
            uint64_t m = 0;
            for (uint32_t t = s; t < e; t++) m |= a.mask[(size_t)t * a.pw + w];
            if (kPaired && m1 > m0) m &= graph_or(a, m0, m1, a.trav[s].graph_id, w);
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

template <bool kPaired>
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
    if (blockIdx.x == 0 && threadIdx.x < (kPaired ? kSharedStats : 3u)) {
        a.stats[threadIdx.x] += a.batch[threadIdx.x];
        a.batch[threadIdx.x] = 0;
        if (kPaired && threadIdx.x == 2) {     // slow units = slow reads + slow fragments
            a.stats[2] += a.batch[6];
            a.batch[6] = 0;
        }
    }
}

} // namespace groot
