// kernels_gap_ec.hpp -- gap-placed reads in the equivalence classes (groot_hip_gap_ec_*; the definition is in include/groot_hip.h,
// "gap-placed reads in the equivalence classes"): G(r), the global paths a gap-rescued read has a kept gapped placement on, becomes a
// unit of the run-wide table of kernels_ec.hpp, as S(r) of a read with a record and R(r) of a rescued read are.  Three kernels per batch
// on the tail stream, launched only while the feature is on; rescue_gap_ec_kernel takes the place of rescue_gap_kernel /
// rescue_gap_rec_kernel, the other two run between the kernels of kernels_rescue_ec.hpp:
//
// rescue_gap_ec_kernel  the same body (rescue_gap_body, kernels_gap.hpp), whose sink (GapEcRow, on top of the sink the launch would have
//                       had: <kRec> beside the gapped records or not) also writes the candidate's set into row r of set_graph / set_mask
//                       with RescueRow's logic (kernels_rescue_ec.hpp): graph ascending, up to max_segs segments, the (segment, word) in
//                       hand in registers, plain loads and stores.  A gap candidate is a candidate that ended unplaced: rescue_count_ec_kernel
//                       ended its row as empty, begin() starts it again.  A set in more than max_segs graphs marks the row slow.  e* of
//                       every gap candidate is kept, one byte (kGapRecNone: not gap-rescued).
// gap_ec_slow_kernel    one thread per gap candidate, behind rescue_ec_slow_kernel; a gap-rescued one with a slow row takes a bitmap from
//                       the slot's pool behind those the rescued reads took (their count is final: the same stream), walks gap_sweep
//                       (sweep 1 at the stored e*) and ORs bit p in.  The batch's slow gap-rescued reads are counted whether they found
//                       a bitmap or not: more than `rows` of both kinds together fail the batch at collect.
// gap_ec_insert_kernel  one thread per gap candidate, behind rescue_ec_insert_kernel and ahead of the batch's one rescue_ec_merge_kernel
//                       launch; a gap-rescued one with a fast row goes into the per-batch table (shared_insert_row), where a rescued
//                       read with the same set already owns the slot or finds this one: the merge folds both kinds under one epoch.
// No per-thread array is indexed dynamically, integer sums only, and every kernel reads the pass's status word first: a pass collect
// redoes, or a batch that fails, adds nothing.
#pragma once

#include "kernels_gap_rec.hpp"
#include "kernels_rescue_ec.hpp"

namespace groot {

// stats[]: gap-rescued reads that went through the per-batch table (the slow ones are counted at collect)
constexpr uint32_t kGapEcStats = 1;

struct GapEcCountArgs {
    GapRecArgs g;                  // the gap kernel's own, with the gapped records' (unused while <kRec> is false)
    uint8_t *e;                    // [n_reads] e* of gap candidate c, kGapRecNone when it is not gap-rescued
};

// the sink of rescue_gap_body with the feature on: Base's work (nothing, or the count of the gapped records), and the set row
template <class Base> struct GapEcRow : Base {
    RescueRow row;
    uint8_t *e;
    __device__ __forceinline__ void begin() { Base::begin(); row = RescueRow{}; }
    __device__ __forceinline__ void kept(const RescueArgs &a, uint32_t r, uint32_t p) { Base::kept(a, r, p); row.kept(a, r, p); }
    __device__ __forceinline__ void done(const RescueArgs &a, uint32_t c, uint32_t r, uint32_t best, bool rescued)
    {
        Base::done(a, c, r, best, rescued);
        row.end(a, r);             // (not gap-rescued: no sweep 2, no segment, the row ends empty again)
        e[c] = rescued ? (uint8_t)best : kGapRecNone;
    }
};

template <bool kRec> __global__ __launch_bounds__(kBlock) void rescue_gap_ec_kernel(GapEcCountArgs a)
{
    if (kRec) {
        GapEcRow<GapRecCount> sink;
        sink.n_gkept = a.g.n_gkept; sink.gap_e = a.g.gap_e; sink.n = 0; sink.e = a.e;
        rescue_gap_body(a.g.g, sink);
    } else {
        GapEcRow<GapNoSink> sink;
        sink.e = a.e;
        rescue_gap_body(a.g.g, sink);
    }
}

struct GapEcArgs {
    GapArgs g;
    SharedArgs s;                  // the rows and the per-batch table (trav, mask, slow, batch, tri and stats stay unused)
    const uint8_t *e;              // GapEcCountArgs::e
    unsigned long long *bits;      // RescueEcArgs::bits: [rows][bw], the rescued reads' bitmaps first
    const uint32_t *n_rslow;       // [1] RescueEcArgs::n_slow: final, rescue_ec_slow_kernel ran ahead on this stream
    uint32_t *n_gslow;             // [1] the batch's slow gap-rescued reads, with or without a bitmap (slot-owned, zeroed ahead of the launch)
    unsigned long long *stats;     // [kGapEcStats]
    uint32_t rows, bw;
};

// what gap_ec_slow_body tells of every kept tuple beyond the bitmap: nothing here, the tuple's intervals to the slot's log in
// kernels_gap_acov.hpp (GapAcovLog); `at` is the read's bitmap among the gap-rescued reads' (behind the rescued reads' in the pool)
struct GapNoLog {
    __device__ __forceinline__ void kept(const GapEcArgs &, uint32_t, uint32_t, const uint4 &, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) const {}
};

template <class Log> __device__ __forceinline__ void gap_ec_slow_body(const GapEcArgs &a, const Log &log)
{
    if (!shared_live(a.s)) return;
    const RescueArgs &ra = a.g.r;
    const uint32_t n = min(*a.g.n_gcand, ra.n_reads), G = a.g.max_gap;
    const uint32_t first = min(*a.n_rslow, a.rows);            // (above rows: the batch fails at collect, no bitmap is left)
    const uint64_t off0 = ra.seq_off[0];
    for (uint32_t c = blockIdx.x * kBlock + threadIdx.x; c < n; c += gridDim.x * kBlock) {
        uint32_t best = a.e[c];
        if (best == kGapRecNone) continue;
        const uint32_t r = a.g.gcand[c];
        if (a.s.set_graph[(size_t)r * kSharedSegs] != kSharedEmpty) continue;
        const uint32_t at = atomicAdd(a.n_gslow, 1u);          // (slow gap-rescued reads are rare: one atomic each)
        if (at >= a.rows - first) continue;                     // no bitmap left: the count tells the host, which fails the batch
        unsigned long long *b = a.bits + (size_t)(first + at) * a.bw;
        for (uint32_t w = 0; w < a.bw; w++) b[w] = 0;
        const uint64_t o = ra.seq_off[r];
        const uint32_t len = (uint32_t)(ra.seq_off[r + 1] - o);
        const uint64_t w0 = ((o - off0) >> 5) + r;
        gap_sweep(ra, G, w0, len, 1u, best, [&](uint32_t p, const uint4 &pi, uint32_t, uint32_t x, uint32_t ins, uint32_t g, uint32_t ks, uint32_t, const unsigned long long *) {
            if (p >= a.s.n_paths) return;
            b[p >> 6] |= 1ull << (p & 63u);
            log.kept(a, at, p, pi, x, ins, g, ks, len);
        });
    }
}

__global__ __launch_bounds__(kBlock) void gap_ec_slow_kernel(GapEcArgs a) { gap_ec_slow_body(a, GapNoLog{}); }

__global__ __launch_bounds__(kBlock) void gap_ec_insert_kernel(GapEcArgs a)
{
    if (!shared_live(a.s)) return;
    const uint32_t n = min(*a.g.n_gcand, a.g.r.n_reads);
    uint32_t st[1] = {0};
    for (uint32_t c0 = blockIdx.x * kBlock; c0 < n; c0 += gridDim.x * kBlock) {      // (uniform per wavefront: the shuffles of the stats)
        const uint32_t c = c0 + threadIdx.x;
        if (c >= n || a.e[c] == kGapRecNone) continue;
        const uint32_t r = a.g.gcand[c];
        if (a.s.set_graph[(size_t)r * kSharedSegs] == kSharedEmpty) continue;
        shared_insert_row(a.s, r);
        st[0]++;
    }
    const uint32_t where[1] = {0};
    rescue_add_stats(a.stats, st, where);
}

} // namespace groot
