// kernels_gap_acov.hpp -- gap-placed reads in assigned coverage (groot_hip_gap_acov_*; the definition is in include/groot_hip.h,
// "gap-placed reads in assigned coverage"): every kept gapped placement (p, strand, x, type, g, k*) of a gap-rescued read r of length len
// is, with X = first Position of p + x, TWO GAPPED RECORDS of r on p for a DEL, covering [X, X + k* - 1] and [X + k* + g, X + len + g - 1],
// and ONE for an INS, covering [X, X + len - g - 1]: the text bases gdepth grows on (rescue_gap_body, kernels_gap.hpp).  They are grouped
// in the run-wide table of kernels_acov.hpp under (EC of S++(r), p, Pos, last) beside the exact and the rescued records.  Four kernels per
// batch on the tail stream, between and behind those of kernels_rescue_acov.hpp, launched only while the feature is on:
//
// gap_acov_slow_kernel    gap_ec_slow_kernel (gap_ec_slow_body, kernels_gap_ec.hpp), whose walk also appends every record of a slow
//                         gap-rescued read as (bitmap, p, Pos, last) to the slot's log behind the rescued reads' entries (their count is
//                         final: rescue_acov_slow_kernel ran ahead on this stream); bitmap = the read's among the gap-rescued reads', the
//                         second entry of a DEL marked kGapAcovSecond.  Entries are counted whether they found room or not: more than the
//                         log holds of both kinds together fail the batch at collect.
// gap_acov_serial_kernel  one thread per gap candidate, behind rescue_acov_merge_kernel (which follows gap_ec_insert_kernel here and leaves
//                         tab_ser[]); a gap-rescued one with a fast row probes the per-batch table as rescue_acov_serial_kernel does and
//                         keeps its EC's serial in gcand_ser[c]; kAcovNone for every other gap candidate.  rescue_acov_clear_kernel runs
//                         behind both serial kernels.
// gap_acov_kernel         one thread per gap candidate with a serial: one walk at the stored e* (gap_sweep, sweep 1: the tuples
//                         rescue_gap_body's second sweep and gap_rec_emit_kernel visit, in their order); claims k0 = (ser + 1) << 32 | p
//                         with k1 = Pos << 32 | last per record and adds one.
//
// Claim and add in one pass, here and never at collect, for rescue_acov_kernel's reason: the gap kernel's inputs (the 2-bit reads, the gap
// candidates, e*) are the ctx's, one batch at a time.  A record that finds no room in the whole table is counted in
// stats[kGapAcovDropped], and groot_hip_acov_export fails while that is not zero.
// No per-thread array is indexed dynamically, integer sums only, and every kernel reads the pass's status word first: a pass collect
// redoes, or a batch that fails, adds nothing.
#pragma once

#include "kernels_gap_ec.hpp"
#include "kernels_rescue_acov.hpp"

namespace groot {

// stats[]: kept gapped placements piled up on the device, gapped records added to the device table, records that found no room
constexpr uint32_t kGapAcovStats = 3;
constexpr uint32_t kGapAcovRecords = 1;
constexpr uint32_t kGapAcovDropped = 2;
constexpr uint32_t kGapAcovSecond = 0x80000000u;      // log entry .x: the record behind the gap of a DEL (its placement is counted at the first)

struct GapAcovArgs {
    GapEcArgs e;
    const uint32_t *tab_ser;       // RescueAcovArgs::tab_ser
    uint32_t *gcand_ser;           // [n_reads] the EC serial of gap candidate c, kAcovNone when it is not gap-rescued or its row is slow
    uint32_t *fill;                // claimed slots of the assigned-coverage table
    unsigned long long *stats;     // [kGapAcovStats]
    uint4 *log;                    // RescueAcovArgs::log: the rescued reads' entries first
    const uint32_t *n_rlog;        // [1] RescueAcovArgs::n_log: final, rescue_acov_slow_kernel ran ahead on this stream
    uint32_t *n_glog;              // [1] the entries of the batch's slow gap-rescued reads, logged or not (slot-owned, zeroed ahead of the launch)
    uint32_t log_cap;
};

// the records of the tuple (x, type, g, k*) of a read of len bases on a path whose first Position is pos0: f(Pos, last), once or twice
template <class F> __device__ __forceinline__ void gap_acov_records(uint32_t pos0, uint32_t x, uint32_t ins, uint32_t g, uint32_t ks, uint32_t len, F &&f)
{
    const uint32_t X = pos0 + x;
    if (ins) { f(X, X + len - g - 1u); return; }
    f(X, X + ks - 1u);
    f(X + ks + g, X + len + g - 1u);
}

struct GapAcovLog {
    uint4 *log;
    const uint32_t *n_rlog;
    uint32_t *n_glog;
    uint32_t log_cap;
    __device__ __forceinline__ void kept(const GapEcArgs &, uint32_t row, uint32_t p, const uint4 &pi, uint32_t x, uint32_t ins, uint32_t g, uint32_t ks, uint32_t len) const
    {
        const uint32_t first = min(*n_rlog, log_cap);       // (above log_cap: the batch fails at collect, no room is left)
        uint32_t at = atomicAdd(n_glog, ins ? 1u : 2u);     // (slow gap-rescued reads are rare: one atomic per placement)
        uint32_t mark = 0;
        gap_acov_records(pi.z, x, ins, g, ks, len, [&](uint32_t pos, uint32_t last) {
            if (at < log_cap - first) log[first + at] = make_uint4(row | mark, p, pos, last);      // no room: the count tells the host
            at++;
            mark = kGapAcovSecond;
        });
    }
};

__global__ __launch_bounds__(kBlock) void gap_acov_slow_kernel(GapAcovArgs a) { gap_ec_slow_body(a.e, GapAcovLog{a.log, a.n_rlog, a.n_glog, a.log_cap}); }

__global__ __launch_bounds__(kBlock) void gap_acov_serial_kernel(GapAcovArgs a)
{
    const SharedArgs &s = a.e.s;
    if (!shared_live(s)) return;
    const uint32_t n = min(*a.e.g.n_gcand, a.e.g.r.n_reads);
    for (uint32_t c = blockIdx.x * kBlock + threadIdx.x; c < n; c += gridDim.x * kBlock) {
        uint32_t ser = kAcovNone;
        const uint32_t r = a.e.g.gcand[c];
        if (a.e.e[c] != kGapRecNone && s.set_graph[(size_t)r * kSharedSegs] != kSharedEmpty) {
            uint32_t slot = (uint32_t)shared_hash(s, r) & s.tab_mask;
            for (uint32_t k = 0; k <= s.tab_mask; k++, slot = (slot + 1) & s.tab_mask) {
                const uint32_t cur = s.tab_rep[slot];
                if (cur == kSharedEmpty) break;            // (insert put every row in: never met)
                if (cur == r || same_set(s, cur, r)) { ser = a.tab_ser[slot]; break; }
            }
        }
        a.gcand_ser[c] = ser;
    }
}

__global__ __launch_bounds__(kBlock) void gap_acov_kernel(GapAcovArgs a, AcovTable t)
{
    if (!shared_live(a.e.s)) return;
    const RescueArgs &ra = a.e.g.r;
    const uint32_t n = min(*a.e.g.n_gcand, ra.n_reads), n_paths = a.e.s.n_paths, G = a.e.g.max_gap;
    const uint64_t off0 = ra.seq_off[0];
    uint32_t placed = 0, added = 0, dropped = 0;
    for (uint32_t c0 = blockIdx.x * kBlock; c0 < n; c0 += gridDim.x * kBlock) {      // (uniform per wavefront: the shuffles of the stats)
        const uint32_t c = c0 + threadIdx.x;
        if (c >= n) continue;
        const uint32_t ser = a.gcand_ser[c];
        if (ser == kAcovNone) continue;
        uint32_t best = a.e.e[c];
        const uint32_t r = a.e.g.gcand[c];
        const uint64_t o = ra.seq_off[r];
        const uint32_t len = (uint32_t)(ra.seq_off[r + 1] - o);
        const uint64_t w0 = ((o - off0) >> 5) + r;
        gap_sweep(ra, G, w0, len, 1u, best, [&](uint32_t p, const uint4 &pi, uint32_t, uint32_t x, uint32_t ins, uint32_t g, uint32_t ks, uint32_t, const unsigned long long *) {
            if (p >= n_paths) return;
            placed++;
            const unsigned long long k0 = ((unsigned long long)(ser + 1u) << 32) | p;
            gap_acov_records(pi.z, x, ins, g, ks, len, [&](uint32_t pos, uint32_t last) {
                const uint32_t s = acov_claim(t, k0, ((unsigned long long)pos << 32) | last, a.fill, ~0u);
                const bool room = s != kAcovNone;
                added += room;
                dropped += !room;
                if (room) atomicAdd(t.cnt + s, 1ull);
            });
        });
    }
    const uint32_t st[3] = {placed, added, dropped}, where[3] = {0, kGapAcovRecords, kGapAcovDropped};
    rescue_add_stats(a.stats, st, where);
}

} // namespace groot
