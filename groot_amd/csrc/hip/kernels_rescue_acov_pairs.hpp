// kernels_rescue_acov_pairs.hpp -- rescued mates in assigned coverage over fragments (groot_hip_rescue_acov_pairs_*; the rule is in
// include/groot_hip.h, "rescued mates in assigned coverage over fragments"): with the rescued mates in the fragments' units
// (kernels_rescue_pairs.hpp) and assigned coverage over fragments (the kPaired kernels of kernels_acov.hpp) both on, a record or a kept
// placement of mate r on path p counts when p is in U(r) -- the fragment's unit when it is joined, S+(r) otherwise -- under the EC of U(r).
//
// Three kinds of record.  (a) Exact records whose filter needs exact records only -- fragments exact + exact, exact mates that end single or
// split -- go through acov_serial_paired_kernel and acov_count_kernel<., true> as they are, and collect may redo them.  (b) The kept
// placements of a rescued mate and (c) the exact records of a mate joined with a rescued partner are filtered by a unit row that is the
// ctx's and is gone when collect redoes a count: they are claimed and added in ONE pass while the row is live, probing the whole table, as
// kernels_rescue_acov.hpp does for the same reason; what finds no room is counted in `dropped` and fails the export.  The reads of kind (c)
// keep kAcovNone in read_ser[], so neither the ordinary count nor its redo touches them.
//
// On the tail stream, launched only while the rule is on.  In rescue_launch, in the place of the two kernels of kernels_rescue_pairs.hpp:
// rescue_acov_pair_kernel         rescue_pair_kernel, which also leaves every fragment's class in fclass[] (joined / own rows / bitmaps) and
//                                 appends the records of a fragment on bitmaps -- placements and exact records alike -- as (bitmap row [|
//                                 kRapExact], p, Pos, last) to the slot's log; the host folds the log at collect under the ID list of the
//                                 row's bitmap, p in the list or left out.  Entries are counted whether they found room or not.
// rescue_acov_pair_insert_kernel  rescue_pair_insert_kernel, for which a batch with more entries than the log holds has no room either: the
//                                 batch counts nothing, and the host fails it at collect.
// Behind ec_merge_kernel<true>, which leaves the units' serials in tab_ser[], and acov_serial_paired_kernel (counters.hip, acov_launch):
// rescue_acov_pairs_serial_kernel one thread per candidate: the serial of the unit row of a rescued mate (the even mate's row when the
//                                 fragment is joined, its own otherwise) into cand_ser[], by rescue_acov_serial_kernel's probe.
// rescue_acov_pairs_exact_kernel  one thread per fragment: kind (c), and kAcovNone into read_ser[] of the exact mates whose records are not
//                                 the ordinary count's (kind (c), fragments on bitmaps).
// rescue_acov_pairs_kernel        rescue_acov_kernel with one test more: kind (b).
// acov_count_kernel<., true> follows, then shared_expand_kernel<true> clears the table.
// Integer sums only, and every kernel reads the pass's status word first: a pass collect redoes, or a batch that fails, adds nothing.
#pragma once

#include "kernels_rescue_acov.hpp"
#include "kernels_rescue_pairs.hpp"

namespace groot {

// stats[]: exact records of kind (c) counted / left out, rescued records counted, keys of either kind that found no room, rescued records left out
constexpr uint32_t kRescueAcovPairStats = 5;
constexpr uint32_t kRapExact = 0, kRapExactLeft = 1, kRapRescued = 2, kRapDropped = 3, kRapRescuedLeft = 4;
constexpr uint32_t kRapLogExact = 0x80000000u;         // flag of a log entry's row word: an exact record (else a kept placement)
constexpr uint8_t kRapNone = 0, kRapJoined = 1, kRapOwn = 2, kRapBitmap = 3;      // fclass[]: no unit made here / unit in the even mate's row / own rows / bitmaps

// the position tables of kernels_acov.hpp, for the exact records
struct RapIndex {
    const uint32_t *node_np_off;
    const uint2 *np;
    const uint32_t *path_len;
};

// every record of read r's traversals [t0, t1): f(graph, local path, global path, Pos, last) -- acov_count_kernel's enumeration
template <class F> __device__ __forceinline__ void rap_each_record(const SharedArgs &s, const RapIndex &ix, const uint64_t *seq_off, uint32_t r, uint32_t t0, uint32_t t1, F &&f)
{
    const uint64_t len = seq_off[r + 1] - seq_off[r];
    for (uint32_t t = t0; t < t1; t++) {
        const groot_trav tr = s.trav[t];
        const uint64_t m = len - ((tr.flags & GROOT_TRAV_START_CLIP) ? 1u : 0u) - ((tr.flags & GROOT_TRAV_END_CLIP) ? 1u : 0u);
        const uint32_t g0 = s.graph_path_off[tr.graph_id];
        const uint64_t *mk = s.mask + (size_t)t * s.pw;
        for (uint32_t j = ix.node_np_off[tr.node]; j < ix.node_np_off[tr.node + 1]; j++) {
            const uint2 e = ix.np[j];
            if (!((mk[e.x >> 6] >> (e.x & 63)) & 1ull)) continue;
            const uint32_t gp = g0 + e.x;
            if (gp >= s.n_paths) continue;
            const uint64_t plen = ix.path_len[gp], pos = (uint64_t)e.y + tr.offset;
            if (plen == 0 || pos > 0xFFFFFFFEull) continue;
            f(tr.graph_id, e.x, gp, (uint32_t)pos, (uint32_t)min(pos + m, plen - 1));
        }
    }
}

// local path `bit` of graph g is in unit row `row`
__device__ __forceinline__ bool rap_in_row(const SharedArgs &s, uint32_t row, uint32_t g, uint32_t bit)
{
    const uint32_t *sg = s.set_graph + (size_t)row * kSharedSegs;
    for (uint32_t k = 0; k < kSharedSegs; k++)
        if (sg[k] == g) return (s.set_mask[((size_t)row * kSharedSegs + k) * s.pw + (bit >> 6)] >> (bit & 63u)) & 1ull;
    return false;
}

struct RescueAcovPairSink {
    RapIndex ix;
    uint8_t *fclass;               // [n_reads / 2] (zeroed ahead of the launch)
    uint4 *log;                    // [log_cap] (slot-owned)
    uint32_t *n_log;               // [1] entries, logged or not (slot-owned, zeroed ahead of the launch)
    uint32_t log_cap;

    __device__ __forceinline__ void entry(uint32_t row, uint32_t p, uint32_t pos, uint32_t last) const
    {
        const uint32_t at = atomicAdd(n_log, 1u);           // (fragments on bitmaps are rare: one atomic per record)
        if (at < log_cap) log[at] = make_uint4(row, p, pos, last);
    }
    __device__ __forceinline__ void mate(const RescuePairArgs &a, const PairMate &m, uint32_t row) const
    {
        if (m.rescued) {
            const uint32_t len = (uint32_t)(a.e.r.seq_off[m.r + 1] - a.e.r.seq_off[m.r]);
            rescue_each_kept(a.e.r, m.r, m.d, [&](uint32_t p, uint32_t to) {
                if (p >= a.e.s.n_paths) return;
                const uint32_t x = rescue_acov_x(a.e.r, p, to);
                entry(row, p, x, x + len - 1u);
            });
        } else if (m.exact) {
            rap_each_record(a.e.s, ix, a.e.r.seq_off, m.r, m.t0, m.t1, [&](uint32_t, uint32_t, uint32_t gp, uint32_t pos, uint32_t last) { entry(row | kRapLogExact, gp, pos, last); });
        }
    }
    __device__ __forceinline__ void rows(uint32_t f, bool joined) const { fclass[f] = joined ? kRapJoined : kRapOwn; }
    // (apart: two mates, not joined -- the second mate's unit is the bitmap behind the first's)
    __device__ __forceinline__ void bitmaps(const RescuePairArgs &a, uint32_t f, const PairMate &x, const PairMate &y, uint32_t row, bool apart) const
    {
        fclass[f] = kRapBitmap;
        if (x.any()) mate(a, x, row);
        if (y.any()) mate(a, y, x.any() && apart ? row + 1u : row);
    }
};

__global__ __launch_bounds__(kBlock) void rescue_acov_pair_kernel(RescuePairArgs a, RescueAcovPairSink sink) { rescue_pair_body(a, sink); }

__global__ __launch_bounds__(kBlock) void rescue_acov_pair_insert_kernel(RescuePairArgs a, const uint32_t *n_log, uint32_t log_cap)
{
    if (!shared_live(a.e.s)) return;
    rescue_pair_insert_body(a, *a.e.n_slow > a.e.rows || *n_log > log_cap);
}

struct RescueAcovPairsArgs {
    RescueAcovArgs a;              // a.e: the candidates, the rows, the per-batch table; tab_ser, cand_ser, fill; stats = the rule's + kRapRescued; the slot's log
    RapIndex ix;
    const uint8_t *fclass;         // [n_reads / 2] (rescue_acov_pair_kernel)
    uint32_t *read_ser;            // [n_reads] AcovArgs::read_ser of the slot
    unsigned long long *stats;     // [kRescueAcovPairStats]
};

// the batch counts nothing: rescue_acov_pair_insert_kernel has cleared the table
__device__ __forceinline__ bool rap_live(const RescueAcovArgs &a) { return shared_live(a.e.s) && *a.e.n_slow <= a.e.rows && *a.n_log <= a.log_cap; }

// the unit row of rescued mate r, which is in a unit with a row (fclass kRapJoined or kRapOwn)
__device__ __forceinline__ uint32_t rap_unit_row(const uint8_t *fclass, uint32_t r) { return fclass[r >> 1] == kRapJoined ? r & ~1u : r; }

__global__ __launch_bounds__(kBlock) void rescue_acov_pairs_serial_kernel(RescueAcovPairsArgs p)
{
    const RescueAcovArgs &a = p.a;
    if (!rap_live(a)) return;
    const uint32_t n = min(*a.e.r.n_cand, a.e.r.n_reads), n_frag = a.e.r.n_reads >> 1;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        uint32_t ser = kAcovNone;
        const uint32_t r = a.e.r.cand[i];
        if (rescue_ec_rescued(a.e, i) && (r >> 1) < n_frag) {
            const uint8_t cls = p.fclass[r >> 1];
            if (cls == kRapJoined || cls == kRapOwn) ser = acov_row_serial(a.e.s, a.tab_ser, rap_unit_row(p.fclass, r));
        }
        a.cand_ser[i] = ser;
    }
}

__global__ __launch_bounds__(kBlock) void rescue_acov_pairs_exact_kernel(RescueAcovPairsArgs p, AcovTable t)
{
    const RescueAcovArgs &a = p.a;
    if (!rap_live(a)) return;
    const SharedArgs &s = a.e.s;
    const uint32_t n = min(s.ctr->n_trav, s.cap), n_reads = a.e.r.n_reads, n_frag = n_reads >> 1;
    uint32_t added = 0, left = 0, dropped = 0;
    for (uint32_t f0 = blockIdx.x * kBlock; f0 < n_frag; f0 += gridDim.x * kBlock) {      // (uniform per wavefront: the shuffles of the stats)
        const uint32_t f = f0 + threadIdx.x;
        if (f >= n_frag) continue;
        const uint8_t cls = p.fclass[f];
        if (cls != kRapJoined && cls != kRapBitmap) continue;
        const uint32_t row = 2u * f;
        uint32_t ser = kAcovNone;
        bool probed = false;
        for (uint32_t r = row; r < row + 2u; r++) {
            const uint32_t t0 = min(a.e.r.trav_off[r], n), t1 = r + 1 < n_reads ? min(a.e.r.trav_off[r + 1], n) : n;
            if (t1 <= t0) continue;
            p.read_ser[r] = kAcovNone;
            if (cls == kRapBitmap) continue;               // (its records are in the log)
            if (!probed) { ser = acov_row_serial(s, a.tab_ser, row); probed = true; }
            rap_each_record(s, p.ix, a.e.r.seq_off, r, t0, t1, [&](uint32_t g, uint32_t bit, uint32_t gp, uint32_t pos, uint32_t last) {
                const bool in = rap_in_row(s, row, g, bit);
                uint32_t slot = kAcovNone;
                if (in && ser != kAcovNone) slot = acov_claim(t, ((unsigned long long)(ser + 1u) << 32) | gp, ((unsigned long long)pos << 32) | last, a.fill, ~0u);
                const bool room = slot != kAcovNone;
                left += !in;
                added += room;
                dropped += in && !room;
                if (room) atomicAdd(t.cnt + slot, 1ull);
            });
        }
    }
    const uint32_t st[3] = {added, left, dropped}, where[3] = {kRapExact, kRapExactLeft, kRapDropped};
    rescue_add_stats(p.stats, st, where);
}

struct RescueAcovUnit {
    static constexpr bool kFilter = true;
    const uint8_t *fclass;
    __device__ __forceinline__ uint32_t row(uint32_t r) const { return rap_unit_row(fclass, r); }
    __device__ __forceinline__ bool has(const RescueEcArgs &e, uint32_t row, uint32_t p) const
    {
        const uint2 pb = e.r.path_bit[p];
        return rap_in_row(e.s, row, pb.x, pb.y);
    }
};

__global__ __launch_bounds__(kBlock) void rescue_acov_pairs_kernel(RescueAcovPairsArgs p, AcovTable t)
{
    if (!rap_live(p.a)) return;
    rescue_acov_body(p.a, t, RescueAcovUnit{p.fclass}, p.stats + kRapRescuedLeft);
}

} // namespace groot
