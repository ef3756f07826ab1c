// kernels_rescue_rec.hpp -- rescued records (groot_hip_rescue_rec_*; the definition is in include/groot_hip.h, "rescued records"): every
// kept placement of every rescued read of a batch as one 20-byte record (read, path, pos, mm[3], strand, d), in ascending
// (read, path, strand, pos) order, in a buffer the pipeline slot owns.  Three steps per batch on the tail stream, behind the rescue
// kernels' inputs and launched only while the feature is on:
//
// rescue_count_rec_kernel  takes the place of rescue_count_kernel / rescue_count_ec_kernel: the same body, whose sink (RescueRecCount, on
//                          top of the sink the launch would have had) also counts the candidate's kept placements and leaves them at
//                          n_kept[r] -- indexed by READ, zeroed ahead of the launch, so a read that is no candidate holds 0 -- and d* at
//                          rec_d[i].  <kGap, kEc>: beside gapped rescue, beside the rescued reads in the classes, beside both, or alone.
// the scan                 rocprim::exclusive_scan of n_kept[0 .. n_reads] (one slot more than reads: the last output is the batch's
//                          total) into rec_off, 64-bit.  Indexed by read, a segment's start does not depend on the order in which the
//                          wavefronts built the candidate list.
// rescue_rec_emit_kernel   one thread per candidate with d* <= M: walks its kept placements at the stored d* once more
//                          (rescue_each_kept_strand), writes placement k to rec[rec_off[r] + k] with the mismatch offsets re-derived
//                          from rescue_diff (word k, bit / 2: ascending by construction), then sorts its own segment by
//                          (path, strand, pos) in place: an insertion sort over global memory, no other thread touches the segment.
//                          A segment that would end past `cap` is not written at all; the total tells the host, which fails the batch.
// The record travels as five dwords (the layout of groot_rescue_record on a little-endian host): the mismatch offsets are kept in one
// 64-bit register and shifted in, so that no per-thread array is indexed dynamically.  Plain loads and stores only, and every kernel reads
// the pass's status word first: a pass that collect redoes, or a batch that fails, leaves the total at 0.
#pragma once

#include "kernels_rescue_ec.hpp"

namespace groot {

constexpr uint32_t kRescueRecWords = 5;      // sizeof(groot_rescue_record) / 4

// the sink of a count launch with the records on: Base's work (nothing, or the set row), and the number of kept placements
template <class Base> struct RescueRecCount : Base {
    uint32_t n;
    __device__ __forceinline__ void kept(const RescueArgs &a, uint32_t r, uint32_t p) { Base::kept(a, r, p); n++; }
    __device__ __forceinline__ void done(const RescueArgs &a, uint32_t r, uint32_t i, uint32_t best)
    {
        Base::done(a, r, i, best);
        const bool rescued = best <= a.max_mismatch;
        a.rec_d[i] = rescued ? (uint8_t)best : kRescueUnplaced;
        if (rescued) a.n_kept[r] = n;
    }
};

template <bool kGap, bool kEc> __global__ __launch_bounds__(kBlock) void rescue_count_rec_kernel(RescueArgs a)
{
    if (kEc) rescue_count_body<kGap, RescueRecCount<RescueRow>>(a);
    else rescue_count_body<kGap, RescueRecCount<RescueNoSink>>(a);
}

struct RescueRecArgs {
    RescueArgs r;
    const uint64_t *off;           // [n_reads + 1] first record of read r, the batch's total behind the last read
    uint32_t *rec;                 // [cap][kRescueRecWords] (slot-owned)
    uint64_t cap;
};

// (path, strand, pos) of record x before that of record y; w1 = path, w2 = pos, w4 = mm[2] | strand << 16 | d << 24
__device__ __forceinline__ bool rescue_rec_before(uint32_t x1, uint32_t x2, uint32_t x4, uint32_t y1, uint32_t y2, uint32_t y4)
{
    if (x1 != y1) return x1 < y1;
    const uint32_t xs = (x4 >> 16) & 0xFFu, ys = (y4 >> 16) & 0xFFu;
    if (xs != ys) return xs < ys;
    return x2 < y2;
}

__global__ __launch_bounds__(kBlock) void rescue_rec_emit_kernel(RescueRecArgs a)
{
    if (a.r.ctr->flags & kCovSkipFlags) return;
    const uint32_t n = min(*a.r.n_cand, a.r.n_reads);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t d = a.r.rec_d[i];
        if (d == kRescueUnplaced) continue;
        const uint32_t r = a.r.cand[i], nk = a.r.n_kept[r];
        const uint64_t first = a.off[r];
        if (first + nk > a.cap) continue;                  // no room: nothing of the read is written, the total fails the batch at collect
        const uint64_t o = a.r.seq_off[r];
        const uint32_t len = (uint32_t)(a.r.seq_off[r + 1] - o), nw = (len + 31u) >> 5;
        const uint64_t w0 = ((o - a.r.seq_off[0]) >> 5) + r;
        uint32_t *seg = a.rec + first * kRescueRecWords;
        uint32_t k = 0;
        rescue_each_kept_strand(a.r, r, d, [&](uint32_t p, uint32_t to, uint32_t strand) {
            if (k >= nk) return;                           // (the walk is the count's: never taken; a segment is never left)
            const uint4 pi = a.r.path[p];
            const unsigned long long *rd = a.r.rbuf + strand * a.r.rcap + w0;
            unsigned long long mm = 0xFFFFFFFFFFFFull;
            uint32_t c = 0;
            for (uint32_t w = 0; d && w < nw; w++) {
                bool nn;
                for (unsigned long long m = rescue_diff(a.r, rd, len, pi.x + to, w, nn); m; m &= m - 1) {
                    const unsigned long long at = 32u * w + (((uint32_t)__ffsll(m) - 1u) >> 1);
                    if (c < 3u) mm = (mm & ~(0xFFFFull << (16u * c))) | (at << (16u * c));
                    c++;
                }
            }
            uint32_t *x = seg + (size_t)k * kRescueRecWords;
            x[0] = r; x[1] = p; x[2] = pi.z + to; x[3] = (uint32_t)mm;
            x[4] = (uint32_t)(mm >> 32) | (strand << 16) | (d << 24);
            k++;
        });
        for (uint32_t j = 1; j < nk; j++) {                // the thread's own segment into (path, strand, pos) order
            uint32_t *x = seg + (size_t)j * kRescueRecWords;
            const uint32_t c1 = x[1], c2 = x[2], c3 = x[3], c4 = x[4];
            uint32_t at = j;
            while (at > 0) {
                const uint32_t *y = seg + (size_t)(at - 1) * kRescueRecWords;
                const uint32_t y1 = y[1], y2 = y[2], y3 = y[3], y4 = y[4];
                if (!rescue_rec_before(c1, c2, c4, y1, y2, y4)) break;
                uint32_t *z = seg + (size_t)at * kRescueRecWords;
                z[1] = y1; z[2] = y2; z[3] = y3; z[4] = y4;    // (word 0, the read, is the same all over the segment)
                at--;
            }
            if (at != j) {
                uint32_t *z = seg + (size_t)at * kRescueRecWords;
                z[1] = c1; z[2] = c2; z[3] = c3; z[4] = c4;
            }
        }
    }
}

} // namespace groot
