// kernels_rescue_pairs.hpp -- rescued mates in their fragment's unit (groot_hip_rescue_pairs_*; the rule is in include/groot_hip.h,
// "rescued mates in paired-end units"): with pairing and the rescued reads in the classes both on, a fragment's unit is made of
// A = S+(r_2i) and B = S+(r_2i+1) -- a mate's records when it has some, R(r) when mismatch rescue places it, nothing otherwise.
//
// The obstacle is launch order: the gather of kernels_shared.hpp runs ahead of rescue, so a fragment with records on one mate only would
// be merged as a single unit before R of the other mate exists.  With the rule on, shared_gather_paired_kernel<true> DEFERS those
// fragments (no unit, no count; the mate's row starts with kSharedEmpty, which shared_insert_kernel skips), fragments with records on
// both mates are gathered and inserted into the per-batch table as ever, and ec_merge_kernel<true> and shared_expand_kernel<true> wait until
// rescue is through (counters_launch): behind rescue_count_ec_kernel three kernels on the tail stream, launched only while the rule is on,
// take the place of rescue_ec_slow_kernel, rescue_ec_insert_kernel and rescue_ec_merge_kernel, and ONE merge folds every unit of the batch:
//
// rescue_pair_mark_kernel    one thread per candidate: d* of candidate i to state[cand[i]] -- "is mate r rescued", by READ.  The host sets
//                            state[] to kRescueUnplaced ahead of it, so a read that is no candidate, or is one and stayed unplaced, says so;
//                            its row in set_graph / set_mask is stale and is never read.
// rescue_pair_kernel         one thread per fragment of the batch (not per traversal start: two rescued mates have no traversal).  "Has
//                            records" comes from trav_off, as in rescue_pack_kernel, never from a row.  A fragment with records on both
//                            mates is skipped.  Otherwise an exact mate's row is written from its records, the two rows' ascending
//                            segment lists are merged -- graphs in common only, masks ANDed word by word, all-zero segments dropped: the
//                            canonical key of kernels_shared.hpp -- and the outcome is left in state[]: kRescuePairUnit for a row that
//                            holds a unit.  Joined: the unit in the even mate's row; split: both rows; single: one.  The thread owns both
//                            rows and both state bytes: plain loads and stores.
//                            A fragment with a mate that fits no row (records in more than max_segs graphs, or a slow rescued row) takes one
//                            bitmap of n_paths bits per non-empty mate in the slot's pool (RescueEcArgs::bits, counted at n_slow): an exact
//                            mate's bits from its records at graph_path_off[g] + bit, a rescued mate's from its row or from
//                            rescue_each_kept; with two mates the bitmaps are ANDed, and a joined fragment keeps the AND in the first and
//                            zeroes the second.  The host folds every non-empty bitmap as one unit at collect (rec_collect), and fails the
//                            batch when the pool is too small: no unit is dropped silently.  Its counts go to the batch's own words.
// rescue_pair_insert_kernel  one thread per read: a row marked kRescuePairUnit goes into the per-batch table (shared_insert_row), beside the
//                            exact + exact fragments' units.  A batch whose fragments need more bitmaps than the pool has counts nothing:
//                            the kernel clears the table and the batch's counts instead, and the merge behind it finds nothing.
// ec_merge_kernel<true> and shared_expand_kernel<true> (counters.hip) then fold the table into the run-wide one and the counts into the totals.
// Integer sums only, and every kernel reads the pass's status word first: a pass collect redoes, or a batch that fails, adds nothing.
#pragma once

#include "kernels_rescue_ec.hpp"

namespace groot {

// stats[]: fragments exact + rescued joined / split, rescued + rescued joined / split, one mate alone with records / rescued, rescued mates
// in a unit, units that took a bitmap, rescued mates in those
constexpr uint32_t kRescuePairStats = 9;
constexpr uint8_t kRescuePairUnit = 0xFEu;      // state[r] behind rescue_pair_kernel: row r holds a unit (kRescueUnplaced: it does not)

struct RescuePairArgs {
    RescueEcArgs e;                // e.r: the candidates, d*, trav_off; e.s: the records, the rows and the per-batch table; the slot's bitmaps
    uint8_t *state;                // [n_reads] d* of a rescued mate / kRescueUnplaced; behind rescue_pair_kernel kRescuePairUnit / kRescueUnplaced
    unsigned long long *stats;     // [kRescuePairStats] of this batch (zeroed ahead of the launch)
    unsigned long long *total;     // [kRescuePairStats] since the rule came on / groot_hip_ec_reset: the batches whose bitmaps found room
    uint32_t tab_size;             // slots of this batch's part of the per-batch table
};

__global__ __launch_bounds__(kBlock) void rescue_pair_mark_kernel(RescuePairArgs a)
{
    if (!shared_live(a.e.s)) return;
    const uint32_t n = min(*a.e.r.n_cand, a.e.r.n_reads);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t r = a.e.r.cand[i];
        if (r < a.e.r.n_reads) a.state[r] = a.e.r.dstar[i];
    }
}

// one mate of a fragment as rescue_pair_kernel sees it
struct PairMate {
    uint32_t r, t0, t1;            // the read, its records [t0, t1)
    uint32_t d;                    // d* when it is rescued
    bool exact, rescued, big;      // has records / is rescued / fits no row
    __device__ __forceinline__ bool any() const { return exact || rescued; }
};

__device__ __forceinline__ PairMate pair_mate(const RescuePairArgs &a, uint32_t r, uint32_t n)
{
    PairMate m;
    m.r = r;
    m.t0 = min(a.e.r.trav_off[r], n);
    m.t1 = r + 1 < a.e.r.n_reads ? min(a.e.r.trav_off[r + 1], n) : n;
    m.exact = m.t1 > m.t0;
    m.d = a.state[r];
    m.rescued = !m.exact && m.d != kRescueUnplaced;
    m.big = false;
    return m;
}

// mate m fits no row: records in more than max_segs graphs, or a slow rescued row (looked at only for the fragments the kernel handles)
__device__ __forceinline__ bool pair_big(const RescuePairArgs &a, const PairMate &m)
{
    if (m.exact) {
        uint32_t segs = 0;
        for (uint32_t s = m.t0; s < m.t1; s = seg_end(a.e.s, s, m.t1)) segs++;
        return segs > a.e.s.max_segs;
    }
    return m.rescued && a.e.s.set_graph[(size_t)m.r * kSharedSegs] == kSharedEmpty;
}

// an exact mate's row from its records (at most max_segs graphs: checked by the caller), as gather_read writes it
__device__ __forceinline__ void pair_write_row(const SharedArgs &a, const PairMate &m)
{
    uint32_t *sg = a.set_graph + (size_t)m.r * kSharedSegs;
    uint32_t k = 0;
    for (uint32_t s = m.t0; s < m.t1 && k < kSharedSegs; k++) {
        const uint32_t e = seg_end(a, s, m.t1);
        sg[k] = a.trav[s].graph_id;
        for (uint32_t w = 0; w < a.pw; w++) a.set_mask[((size_t)m.r * kSharedSegs + k) * a.pw + w] = seg_or(a, s, e, w);
        s = e;
    }
    for (; k < kSharedSegs; k++) sg[k] = kSharedEmpty;
}

// The rows of reads x and y merged: graphs in common only, masks ANDed, all-zero segments dropped.  kWrite: into row x (segment k of the
// result is written behind the reads of segment >= k of x: in place); else nothing is written.  -> segments of the result
template <bool kWrite> __device__ __forceinline__ uint32_t pair_merge_rows(const SharedArgs &a, uint32_t x, uint32_t y)
{
    uint32_t *gx = a.set_graph + (size_t)x * kSharedSegs;
    const uint32_t *gy = a.set_graph + (size_t)y * kSharedSegs;
    uint64_t *mx = a.set_mask + (size_t)x * kSharedSegs * a.pw;
    const uint64_t *my = a.set_mask + (size_t)y * kSharedSegs * a.pw;
    uint32_t k = 0;
    for (uint32_t i = 0, j = 0; i < kSharedSegs && j < kSharedSegs && gx[i] != kSharedEmpty && gy[j] != kSharedEmpty;) {
        const uint32_t ga = gx[i], gb = gy[j];
        if (ga < gb) { i++; continue; }
        if (gb < ga) { j++; continue; }
        uint64_t any = 0;
        for (uint32_t w = 0; w < a.pw; w++) {
            const uint64_t m = mx[i * a.pw + w] & my[j * a.pw + w];
            any |= m;
            if (kWrite) mx[k * a.pw + w] = m;      // (k <= i; kept only if any: else segment k is written again)
        }
        if (any) {
            if (kWrite) gx[k] = ga;
            k++;
        }
        i++; j++;
    }
    if (kWrite)
        for (uint32_t q = k; q < kSharedSegs; q++) gx[q] = kSharedEmpty;
    return k;
}

// the set of mate m as a bitmap of n_paths bits (zeroed by the caller)
__device__ __forceinline__ void pair_mate_bits(const RescuePairArgs &a, const PairMate &m, unsigned long long *b)
{
    const SharedArgs &s = a.e.s;
    auto set = [&](uint64_t p) {
        if (p < s.n_paths) b[p >> 6] |= 1ull << (p & 63u);
    };
    if (m.exact) {
        for (uint32_t t = m.t0; t < m.t1; t++) {
            const uint64_t g0 = s.graph_path_off[s.trav[t].graph_id];
            for (uint32_t w = 0; w < s.pw; w++)
                for (uint64_t x = s.mask[(size_t)t * s.pw + w]; x; x &= x - 1) set(g0 + w * 64 + (uint32_t)__builtin_ctzll(x));
        }
    } else if (!m.big) {
        const uint32_t *sg = s.set_graph + (size_t)m.r * kSharedSegs;
        for (uint32_t k = 0; k < kSharedSegs && sg[k] != kSharedEmpty; k++) {
            const uint64_t g0 = s.graph_path_off[sg[k]];
            for (uint32_t w = 0; w < s.pw; w++)
                for (uint64_t x = s.set_mask[((size_t)m.r * kSharedSegs + k) * s.pw + w]; x; x &= x - 1) set(g0 + w * 64 + (uint32_t)__builtin_ctzll(x));
        }
    } else {
        rescue_each_kept(a.e.r, m.r, m.d, [&](uint32_t p, uint32_t) { set(p); });
    }
}

// what rescue_pair_body tells of every fragment it makes a unit of: nothing here; the fragment's class, and the records of a fragment on
// bitmaps, to the slot's log in kernels_rescue_acov_pairs.hpp (RescueAcovPairSink)
struct RescuePairNoSink {
    __device__ __forceinline__ void rows(uint32_t, bool) const {}
    __device__ __forceinline__ void bitmaps(const RescuePairArgs &, uint32_t, const PairMate &, const PairMate &, uint32_t, bool) const {}
};

template <class Sink> __device__ __forceinline__ void rescue_pair_body(const RescuePairArgs &a, const Sink &sink)
{
    const SharedArgs &s = a.e.s;
    if (!shared_live(s)) return;
    const uint32_t n = min(s.ctr->n_trav, s.cap), n_frag = a.e.r.n_reads >> 1;
    // (scalars, added up under constant indices below: a per-thread array indexed by the kind would live in scratch)
    uint32_t er_j = 0, er_s = 0, rr_j = 0, rr_s = 0, one_e = 0, one_r = 0, mates = 0, bm_units = 0, bm_mates = 0;
    for (uint32_t f = blockIdx.x * kBlock + threadIdx.x; f < n_frag; f += gridDim.x * kBlock) {
        PairMate x = pair_mate(a, 2u * f, n), y = pair_mate(a, 2u * f + 1u, n);
        if (x.exact && y.exact) continue;                  // a unit of shared_gather_paired_kernel already
        x.big = pair_big(a, x);
        y.big = pair_big(a, y);
        a.state[x.r] = kRescueUnplaced;
        a.state[y.r] = kRescueUnplaced;
        if (!x.any() && !y.any()) continue;                // none
        const bool two = x.any() && y.any();
        const uint32_t n_resc = (uint32_t)x.rescued + (uint32_t)y.rescued;
        bool joined = false;
        if (x.big || y.big) {
            const uint32_t want = two ? 2u : 1u, row = atomicAdd(a.e.n_slow, want);      // (rare: one atomic each)
            if (row + want > a.e.rows) continue;           // no bitmaps left: the count tells the host, which fails the batch
            unsigned long long *b0 = a.e.bits + (size_t)row * a.e.bw, *b1 = b0 + a.e.bw;
            for (uint32_t w = 0; w < want * a.e.bw; w++) b0[w] = 0;
            pair_mate_bits(a, x.any() ? x : y, b0);
            if (two) {
                pair_mate_bits(a, y, b1);
                unsigned long long any = 0;
                for (uint32_t w = 0; w < a.e.bw; w++) any |= b0[w] & b1[w];
                joined = any != 0;
                for (uint32_t w = 0; joined && w < a.e.bw; w++) { b0[w] &= b1[w]; b1[w] = 0; }
            }
            bm_units += two && !joined ? 2u : 1u;
            bm_mates += n_resc;
            sink.bitmaps(a, f, x, y, row, two && !joined);
        } else {
            if (x.exact) pair_write_row(s, x);
            if (y.exact) pair_write_row(s, y);
            if (two) joined = pair_merge_rows<false>(s, x.r, y.r) != 0;
            if (joined) {
                pair_merge_rows<true>(s, x.r, y.r);
                s.set_graph[(size_t)y.r * kSharedSegs] = kSharedEmpty;
                a.state[x.r] = kRescuePairUnit;
            } else {
                if (x.any()) a.state[x.r] = kRescuePairUnit;
                if (y.any()) a.state[y.r] = kRescuePairUnit;
            }
            sink.rows(f, joined);
        }
        er_j += two && n_resc == 1u && joined;  er_s += two && n_resc == 1u && !joined;
        rr_j += two && n_resc == 2u && joined;  rr_s += two && n_resc == 2u && !joined;
        one_e += !two && !n_resc;               one_r += !two && n_resc;
        mates += n_resc;
    }
    const uint32_t st[kRescuePairStats] = {er_j, er_s, rr_j, rr_s, one_e, one_r, mates, bm_units, bm_mates};
    const uint32_t where[kRescuePairStats] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    rescue_add_stats(a.stats, st, where);
    // into the batch's own pairing counts, beside those of the fragments with records on both mates: shared_expand_kernel<true> adds them to the totals
    block_add(er_j + rr_j + 2u * (er_s + rr_s) + one_e + one_r, &s.batch[0]);      // units
    block_add(er_j + rr_j, &s.batch[3]);
    block_add(er_s + rr_s, &s.batch[4]);
    block_add(one_e + one_r, &s.batch[5]);
}

__global__ __launch_bounds__(kBlock) void rescue_pair_kernel(RescuePairArgs a) { rescue_pair_body(a, RescuePairNoSink{}); }

// The bitmap demand of the batch is known here (rescue_pair_kernel has ended).  It fits: the rows marked kRescuePairUnit join the units
// of the exact + exact fragments in the per-batch table, and the batch's counts of the rule go to the totals.  It does not fit: the batch
// counts NOTHING -- the table (the exact + exact fragments' units, not merged yet), the batch's pairing counts and its slow lists are
// cleared, so ec_merge_kernel<true> and shared_expand_kernel<true> behind this launch find nothing, and the host fails the batch at collect.
// (no_room: the batch needs more than the slot holds -- bitmaps here, bitmaps or log entries in kernels_rescue_acov_pairs.hpp)
__device__ __forceinline__ void rescue_pair_insert_body(const RescuePairArgs &a, bool no_room)
{
    const SharedArgs &s = a.e.s;
    if (no_room) {
        for (uint32_t slot = blockIdx.x * kBlock + threadIdx.x; slot < a.tab_size; slot += gridDim.x * kBlock) {
            s.tab_rep[slot] = kSharedEmpty;
            s.tab_cnt[slot] = 0;
        }
        if (blockIdx.x == 0 && threadIdx.x < kSharedBatch) s.batch[threadIdx.x] = 0;
        return;
    }
    for (uint32_t r = blockIdx.x * kBlock + threadIdx.x; r < a.e.r.n_reads; r += gridDim.x * kBlock)
        if (a.state[r] == kRescuePairUnit) shared_insert_row(s, r);
    if (blockIdx.x == 0 && threadIdx.x < kRescuePairStats) a.total[threadIdx.x] += a.stats[threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void rescue_pair_insert_kernel(RescuePairArgs a)
{
    if (!shared_live(a.e.s)) return;
    rescue_pair_insert_body(a, *a.e.n_slow > a.e.rows);
}

} // namespace groot
