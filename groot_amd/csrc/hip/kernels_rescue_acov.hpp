// kernels_rescue_acov.hpp -- rescued reads in assigned coverage (groot_hip_rescue_acov_*; the definition is in include/groot_hip.h,
// "rescued reads in assigned coverage"): every kept placement (p, strand, x) of a rescued read r of length len is one RESCUED RECORD of r on
// p covering [X, X + len - 1], grouped in the run-wide table of kernels_acov.hpp under (EC of S+(r), p, X, X + len - 1) beside the exact
// records.  The kernels run on the tail stream behind rescue_ec_insert_kernel, and only while the feature is on; two of them take the place
// of a kernel of kernels_rescue_ec.hpp, the other three follow:
//
// rescue_acov_slow_kernel    rescue_ec_slow_kernel, whose walk also appends every kept placement of a slow rescued read as
//                            (bitmap row, p, X, last) to a log of fixed size that the slot owns.  Such a read has no serial on the device:
//                            the host folds the log at collect under the ID list of the row's bitmap.  Placements are counted whether
//                            they found room or not: more than the log holds fail the batch at collect.
// rescue_acov_merge_kernel   rescue_ec_merge_kernel, which also leaves the serial of every occupied slot's EC in tab_ser[] (as
//                            ec_merge_kernel does for the exact reads) and does not clear the slots.
// rescue_acov_serial_kernel  one thread per candidate; a rescued one with a fast row probes the per-batch table as acov_serial_kernel does
//                            and keeps its EC's serial in cand_ser[i]; kAcovNone for every other candidate.
// rescue_acov_clear_kernel   one thread per slot of the per-batch table: cleared, behind the probe.
// rescue_acov_kernel         one thread per candidate with a serial: walks its kept placements at the stored d* (rescue_each_kept), claims
//                            (k0 = (ser + 1) << 32 | p, k1 = X << 32 | X + len - 1) and adds one.
//
// Exactly once, without a redo.  The exact pileup claims first and adds in a second launch, and collect repeats both when the table was
// full: the slot still owns its records.  Rescue's inputs (the 2-bit reads, the candidate list, d*) are the ctx's, one batch at a time, so
// a rescued batch cannot be replayed at collect.  rescue_acov_kernel therefore claims and adds in one pass and probes the whole table.
// Its claims bump the fill that collect reads, so collect's "more than half full: double" makes room for the next batch, and
// acov_rehash_kernel carries these keys like any others.  A key that finds no room in the whole table is counted in stats[kRescueAcovDropped],
// and groot_hip_acov_export fails while that is not zero: no read is dropped silently.  acov_count_kernel, which collect may launch again,
// knows nothing of rescued reads.
// Integer sums only, and every kernel reads the pass's status word first: a pass collect redoes, or a batch that fails, adds nothing.
#pragma once

#include "kernels_acov.hpp"
#include "kernels_rescue_ec.hpp"

namespace groot {

// stats[]: rescued records added to the device table, keys that found no room
constexpr uint32_t kRescueAcovStats = 2;
constexpr uint32_t kRescueAcovDropped = 1;

struct RescueAcovArgs {
    RescueEcArgs e;
    const uint32_t *tab_ser;       // [tab_size] the EC serial of every occupied slot of the per-batch table (rescue_acov_merge_kernel)
    uint32_t *cand_ser;            // [n_reads] the EC serial of candidate i, kAcovNone when it is not rescued or its row is slow
    uint32_t *fill;                // claimed slots of the assigned-coverage table
    unsigned long long *stats;     // [kRescueAcovStats]
    uint4 *log;                    // [log_cap] (bitmap row, p, X, last) of the kept placements of the batch's slow rescued reads (slot-owned)
    uint32_t *n_log;               // [1] their number, logged or not (slot-owned, zeroed ahead of the launch)
    uint32_t log_cap;
};

// X of the placement of a read on global path p at text offset `to`: the coordinate of the exact records' Pos (rescue_place's slot)
__device__ __forceinline__ uint32_t rescue_acov_x(const RescueArgs &a, uint32_t p, uint32_t to) { return a.path[p].z + to; }

struct RescueAcovLog {
    uint4 *log;
    uint32_t *n_log;
    uint32_t log_cap;
    __device__ __forceinline__ void kept(const RescueEcArgs &a, uint32_t r, uint32_t row, uint32_t p, uint32_t to) const
    {
        const uint32_t at = atomicAdd(n_log, 1u);           // (slow rescued reads are rare: one atomic per placement)
        if (at >= log_cap) return;                          // no room left: the count tells the host, which fails the batch
        const uint32_t len = (uint32_t)(a.r.seq_off[r + 1] - a.r.seq_off[r]), x = rescue_acov_x(a.r, p, to);
        log[at] = make_uint4(row, p, x, x + len - 1u);
    }
};

__global__ __launch_bounds__(kBlock) void rescue_acov_slow_kernel(RescueAcovArgs a) { rescue_ec_slow_body(a.e, RescueAcovLog{a.log, a.n_log, a.log_cap}); }

__global__ __launch_bounds__(kBlock) void rescue_acov_merge_kernel(SharedArgs a, EcTable t, uint32_t tab_size, uint32_t epoch, uint32_t *fill, uint32_t *tab_ser)
{
    rescue_ec_merge_body<true>(a, t, tab_size, epoch, fill, tab_ser);
}

__global__ __launch_bounds__(kBlock) void rescue_acov_serial_kernel(RescueAcovArgs a)
{
    const SharedArgs &s = a.e.s;
    if (!shared_live(s)) return;
    const uint32_t n = min(*a.e.r.n_cand, a.e.r.n_reads);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        uint32_t ser = kAcovNone;
        const uint32_t r = a.e.r.cand[i];
        if (rescue_ec_rescued(a.e, i) && s.set_graph[(size_t)r * kSharedSegs] != kSharedEmpty) {
            uint32_t slot = (uint32_t)shared_hash(s, r) & s.tab_mask;
            for (uint32_t k = 0; k <= s.tab_mask; k++, slot = (slot + 1) & s.tab_mask) {
                const uint32_t cur = s.tab_rep[slot];
                if (cur == kSharedEmpty) break;            // (insert put every row in: never met)
                if (cur == r || same_set(s, cur, r)) { ser = a.tab_ser[slot]; break; }
            }
        }
        a.cand_ser[i] = ser;
    }
}

__global__ __launch_bounds__(kBlock) void rescue_acov_clear_kernel(SharedArgs a, uint32_t tab_size)
{
    if (!shared_live(a)) return;
    for (uint32_t slot = blockIdx.x * kBlock + threadIdx.x; slot < tab_size; slot += gridDim.x * kBlock) {
        a.tab_rep[slot] = kSharedEmpty;
        a.tab_cnt[slot] = 0;
    }
}

// which placements of a candidate count: all of them here; those on a path of the unit of the mate's fragment in
// kernels_rescue_acov_pairs.hpp (RescueAcovUnit), which sums the others in `left`
struct RescueAcovAll {
    static constexpr bool kFilter = false;
    __device__ __forceinline__ uint32_t row(uint32_t r) const { return r; }
    __device__ __forceinline__ bool has(const RescueEcArgs &, uint32_t, uint32_t) const { return true; }
};

template <class Unit> __device__ __forceinline__ void rescue_acov_body(const RescueAcovArgs &a, const AcovTable &t, const Unit &unit, unsigned long long *left_out)
{
    const RescueArgs &ra = a.e.r;
    const uint32_t n = min(*ra.n_cand, ra.n_reads), n_paths = a.e.s.n_paths;
    uint32_t added = 0, dropped = 0, left = 0;
    for (uint32_t i0 = blockIdx.x * kBlock; i0 < n; i0 += gridDim.x * kBlock) {      // (uniform per wavefront: the shuffles of the stats)
        const uint32_t i = i0 + threadIdx.x;
        if (i >= n) continue;
        const uint32_t ser = a.cand_ser[i];
        if (ser == kAcovNone) continue;
        const uint32_t r = ra.cand[i], len = (uint32_t)(ra.seq_off[r + 1] - ra.seq_off[r]);
        const uint32_t row = unit.row(r);
        rescue_each_kept(ra, r, ra.dstar[i], [&](uint32_t p, uint32_t to) {
            if (p >= n_paths) return;
            if (Unit::kFilter && !unit.has(a.e, row, p)) { left++; return; }
            const uint32_t x = rescue_acov_x(ra, p, to);
            const uint32_t s = acov_claim(t, ((unsigned long long)(ser + 1u) << 32) | p, ((unsigned long long)x << 32) | (x + len - 1u), a.fill, ~0u);
            const bool room = s != kAcovNone;                // (both counts without a branch: an early return here costs the kernel 12 bytes of scratch)
            added += room;
            dropped += !room;
            if (room) atomicAdd(t.cnt + s, 1ull);
        });
    }
    const uint32_t st[2] = {added, dropped}, where[2] = {0, kRescueAcovDropped};
    rescue_add_stats(a.stats, st, where);
    if (Unit::kFilter) {
        const uint32_t lst[1] = {left}, lwhere[1] = {0};
        rescue_add_stats(left_out, lst, lwhere);
    }
}

__global__ __launch_bounds__(kBlock) void rescue_acov_kernel(RescueAcovArgs a, AcovTable t)
{
    if (!shared_live(a.e.s)) return;
    rescue_acov_body(a, t, RescueAcovAll{}, nullptr);
}

} // namespace groot
