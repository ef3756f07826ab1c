// kernels_assign.hpp -- each read to its best allele by EM posterior on the device (groot_hip_assign_*; the definition is in
// include/groot_hip.h, "assignment").
//
// assign_kernel: one thread per read of the batch, on the tail stream right behind order_ovf_kernel: the batch's records are in
// (read, ord) order then, read r's at trav_off[r] .. + trav_cnt[r], ascending by graph, and nothing downstream has read them yet.
//   sweep 1  per graph of the read (a run of its traversals) and per mask word, the OR of the run's path sets; its set bits upward are
//            S(r) in ascending global ID: denom = denom + alpha[p] one after the other, the maximum tracked with a strict > (so the lowest
//            ID wins among equals), the paths that share the maximum counted for the `ties` stat.
//   sweep 2  every traversal's path set becomes {best} or empty (all pw words), GROOT_TRAV_FIRST moves to the first kept traversal, kept
//            ones get GROOT_TRAV_MAPQ and reserved = mapq; best[r] / mapq[r] for every read of the batch, with or without records.
// One thread walks a read whatever its width: the walk keeps no per-graph state (the OR is recomputed per word), so seven graphs and
// 477 paths over three words are 21 short loops, not an array.  alpha lies in LDS when it fits (kLds: 14 KB on arg-annot.90, every
// workgroup stages it once and its reads then hit LDS for each of their ~18 paths), in global memory otherwise.
// The floating point is compiled without contraction and every product by 2^k is exact, so best, mapq and the stats equal
// groot_host_assign_travs bit for bit.  f64 denormals are on (the target's default).
// The filter is NOT idempotent (a second application would see S(r) = {best} and give MAPQ 60): it runs once per pass, on records the
// order stage has just written, and returns at once under kCovSkipFlags as every counter does -- a pass that collect redoes is filtered,
// and counted, by its redo.
#pragma once

#include "kernels_common.hpp"
#include "kernels_cov.hpp"   // kCovSkipFlags

namespace groot {

constexpr uint32_t kAssignLdsPaths = 6144;       // alpha of up to this many paths is staged in LDS (48 KB)
constexpr uint32_t kAssignNone = 0xFFFFFFFFu;    // best[r] of a read that keeps no record
// stats[]: reads with records, assigned, unassigned, below, ties, records in, records kept, traversals emptied (groot_assign_stats order)
constexpr uint32_t kAssignStats = 8;

struct AssignArgs {
    groot_trav *trav;              // the batch's records in (read, ord) order, rewritten in place
    uint64_t *mask;                // their path sets, pw words each, likewise
    const DeviceCounters *ctr;     // n_trav + flags of the pass
    const uint32_t *off, *cnt;     // [n_reads] read r's records: off[r] .. off[r] + cnt[r]
    const uint32_t *graph_path_off;
    const double *alpha;           // [n_paths]
    uint32_t *best;                // [n_reads]
    uint8_t *mapq;                 // [n_reads]
    unsigned long long *stats;     // [kAssignStats] run totals
    double min_post;
    uint32_t n_reads, cap, pw, n_paths, n_graphs;
};

// mapq of an assigned read: 3 per k in 1..20 with rest * 2^k <= denom
__device__ __forceinline__ uint32_t assign_mapq(double denom, double rest)
{
#pragma clang fp contract(off)
    uint32_t j = 0;
    double s = 1.0;
    for (int k = 1; k <= 20; k++) {
        s = s * 2.0;
        if (rest * s <= denom) j++;
    }
    return 3u * j;
}

template <bool kLds> __global__ __launch_bounds__(kBlock) void assign_kernel(AssignArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char assign_lds[];
    __shared__ unsigned long long acc[kAssignStats];
    if (a.ctr->flags & kCovSkipFlags) return;              // (uniform: ahead of the barriers)
    const double *alpha = a.alpha;
    if (kLds) {
        double *l = reinterpret_cast<double *>(assign_lds);
        for (uint32_t p = threadIdx.x; p < a.n_paths; p += kBlock) l[p] = a.alpha[p];
        alpha = l;
    }
    if (threadIdx.x < kAssignStats) acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n = min(a.ctr->n_trav, a.cap), pw = a.pw;
    uint32_t st[kAssignStats] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t r = blockIdx.x * kBlock + threadIdx.x; r < a.n_reads; r += gridDim.x * kBlock) {
        const uint32_t t0 = a.off[r], c = a.cnt[r];
        uint32_t best = kAssignNone, mq = 0;
        if (c == 0 || t0 >= n || c > n - t0) {              // no records (or a run past the batch's records: never in a pass that is counted)
            a.best[r] = best; a.mapq[r] = 0;
            continue;
        }
        const uint32_t t1 = t0 + c;
        st[0]++;
        // sweep 1: S(r) in ascending global ID
        double denom = 0.0, bestv = -1.0;
        uint32_t bg = 0, bl = 0, nties = 0;
        for (uint32_t s = t0; s < t1;) {
            const uint32_t g = a.trav[s].graph_id;
            uint32_t e = s + 1;
            while (e < t1 && a.trav[e].graph_id == g) e++;
            const uint32_t p0 = g < a.n_graphs ? a.graph_path_off[g] : a.n_paths;
            for (uint32_t w = 0; w < pw; w++) {
                uint64_t m = 0;
                for (uint32_t t = s; t < e; t++) {
                    const uint64_t x = a.mask[(size_t)t * pw + w];
                    st[5] += (uint32_t)__popcll(x);
                    m |= x;
                }
                while (m) {
                    const uint32_t l = w * 64u + (uint32_t)__ffsll((unsigned long long)m) - 1u;
                    m &= m - 1;
                    const uint32_t p = p0 + l;
                    if (p >= a.n_paths) continue;              // (a bit past the index's paths is never set: dropped rather than read out of bounds)
                    const double v = alpha[p];
                    denom = denom + v;
                    if (v > bestv) { bestv = v; bg = g; bl = l; nties = 1; }
                    else if (v == bestv) nties++;
                }
            }
            s = e;
        }
        bool keep = false;
        if (bestv < 0.0 || denom == 0.0) st[2]++;
        else if (!(bestv >= a.min_post * denom)) st[3]++;
        else {
            keep = true;
            st[1]++;
            if (nties > 1) st[4]++;
            best = a.graph_path_off[bg] + bl;
            mq = assign_mapq(denom, denom - bestv);
        }
        // sweep 2: rewrite
        const uint32_t bw = bl >> 6;
        const uint64_t bb = 1ull << (bl & 63u);
        bool first = true;
        for (uint32_t t = t0; t < t1; t++) {
            groot_trav *tr = a.trav + t;
            uint64_t *mk = a.mask + (size_t)t * pw;
            const bool kept = keep && tr->graph_id == bg && (mk[bw] & bb);
            for (uint32_t w = 0; w < pw; w++) mk[w] = kept && w == bw ? bb : 0ull;
            uint8_t fl = tr->flags & (uint8_t)~(GROOT_TRAV_FIRST | GROOT_TRAV_MAPQ);
            if (kept) {
                fl |= GROOT_TRAV_MAPQ;
                if (first) fl |= GROOT_TRAV_FIRST;
                first = false;
                st[6]++;
            } else st[7]++;
            tr->flags = fl;
            tr->reserved = kept ? (uint8_t)mq : (uint8_t)0;
        }
        a.best[r] = best; a.mapq[r] = (uint8_t)mq;
    }
    // the workgroup's sums, once each
    for (uint32_t i = 0; i < kAssignStats; i++) {
        uint32_t v = st[i];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&acc[i], (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x < kAssignStats && acc[threadIdx.x]) atomicAdd(a.stats + threadIdx.x, acc[threadIdx.x]);
}

} // namespace groot
