// kernels_rescue_ec.hpp -- rescued reads in the equivalence classes (groot_hip_rescue_ec_*; the definition is in include/groot_hip.h,
// "rescued reads in the equivalence classes"): R(r), the global paths a rescued read has a kept placement on, becomes a unit of the
// run-wide table of kernels_ec.hpp, as S(r) of a read with a record is.  Four kernels per batch on the tail stream, launched only while
// the feature is on; rescue_count_ec_kernel takes the place of rescue_count_kernel, the other three run behind it:
//
// rescue_count_ec_kernel   rescue_count_kernel, whose second sweep also writes the candidate's set in the row format of
//                          kernels_shared.hpp -- up to max_segs segments (graph ascending, pw mask words each) in set_graph / set_mask
//                          row r.  A read without a record has no row of its own there, and behind shared_expand_kernel the batch's rows
//                          and the per-batch table are free.  The thread owns its row: plain loads and stores, no atomics.  A key's
//                          occurrences ascend by path, so consecutive placements mostly hit the same (segment, word): it is kept in
//                          registers and written back when it changes.  Occurrences arrive per block and per strand, not per graph:
//                          a new graph is inserted in order (the segments above it move up).  A set in more than max_segs graphs marks
//                          the row slow (first graph kSharedEmpty), as shared_gather_kernel does.  d* of every candidate is kept, one byte.
// rescue_ec_slow_kernel    one thread per candidate; a rescued one with a slow row takes a bitmap of n_paths bits in a buffer the slot
//                          owns, walks its placements at the stored d* again and ORs bit p in.  The bitmap deduplicates by construction
//                          and its size does not depend on the number of placements; the host reads it at collect.  The batch's slow
//                          rescued reads are counted whether they found a bitmap or not: more than `rows` of them fail the batch at collect.
// rescue_ec_insert_kernel  one thread per candidate; a rescued one with a fast row goes into the per-batch table (shared_insert_row).
// rescue_ec_merge_kernel   one thread per slot of that table: the owner's set into the run-wide table (ec_add, under an epoch of its
//                          own: the batch's rescued sets are distinct within the launch, as ec_merge_kernel's are), then the slot is
//                          cleared.  It writes neither the slot's list of exact slow reads nor assigned coverage's serials.
// rescue_ec_slow_kernel and rescue_ec_merge_kernel are bodies with a sink / a switch that does nothing here; kernels_rescue_acov.hpp (rescued
// reads in assigned coverage) instantiates them with a placement log and with the serials kept.
// Integer sums only, and every kernel reads the pass's status word first: a pass collect redoes, or a batch that fails, adds nothing.
#pragma once

#include "kernels_ec.hpp"
#include "kernels_rescue.hpp"

namespace groot {

// stats[]: rescued reads that went through the per-batch table (the slow ones are counted at collect)
constexpr uint32_t kRescueEcStats = 1;

// the set row of one candidate while rescue_place's second sweep runs: the (segment, word) in hand, its value, the segments so far
struct RescueRow {
    uint32_t nseg, k, w, g;
    uint64_t val;
    bool open, slow;

    __device__ __forceinline__ void kept(const RescueArgs &a, uint32_t r, uint32_t p)
    {
        if (slow) return;
        const uint2 pb = a.path_bit[p];
        const uint32_t word = pb.y >> 6;
        const uint64_t bit = 1ull << (pb.y & 63u);
        if (open && g == pb.x && w == word) { val |= bit; return; }
        uint32_t *sg = a.set_graph + (size_t)r * kSharedSegs;
        uint64_t *sm = a.set_mask + (size_t)r * kSharedSegs * a.pw;
        if (open) sm[k * a.pw + w] = val;
        uint32_t at = 0;
        while (at < nseg && sg[at] < pb.x) at++;
        if (at == nseg || sg[at] != pb.x) {
            if (nseg >= a.max_segs) { slow = true; open = false; return; }     // (max_segs <= kSharedSegs: the row never overflows)
            for (uint32_t j = nseg; j > at; j--) {
                sg[j] = sg[j - 1];
                for (uint32_t x = 0; x < a.pw; x++) sm[j * a.pw + x] = sm[(j - 1) * a.pw + x];
            }
            sg[at] = pb.x;
            for (uint32_t x = 0; x < a.pw; x++) sm[at * a.pw + x] = 0;
            nseg++;
        }
        open = true; g = pb.x; k = at; w = word;
        val = sm[at * a.pw + word] | bit;
    }

    // behind the sweeps of read r: the word in hand written back, the row ended
    __device__ __forceinline__ void end(const RescueArgs &a, uint32_t r)
    {
        uint32_t *sg = a.set_graph + (size_t)r * kSharedSegs;
        if (open) a.set_mask[((size_t)r * kSharedSegs + k) * a.pw + w] = val;
        if (slow || !nseg) sg[0] = kSharedEmpty;
        else for (uint32_t j = nseg; j < kSharedSegs; j++) sg[j] = kSharedEmpty;
    }

    // behind the sweeps of candidate i (read r): the row ended, d* kept
    __device__ __forceinline__ void done(const RescueArgs &a, uint32_t r, uint32_t i, uint32_t best)
    {
        end(a, r);
        a.dstar[i] = best <= a.max_mismatch ? (uint8_t)best : kRescueUnplaced;
    }
};

template <bool kGap> __global__ __launch_bounds__(kBlock) void rescue_count_ec_kernel(RescueArgs a) { rescue_count_body<kGap, RescueRow>(a); }

struct RescueEcArgs {
    RescueArgs r;
    SharedArgs s;                  // the rows and the per-batch table (trav, mask, slow, batch, tri and stats stay unused)
    unsigned long long *bits;      // [rows][bw] the bitmaps of the batch's slow rescued reads (slot-owned)
    uint32_t *n_slow;              // [1] the batch's slow rescued reads, with or without a bitmap (slot-owned, zeroed ahead of the launch)
    unsigned long long *stats;     // [kRescueEcStats]
    uint32_t rows, bw;             // bitmaps, words each: ceil(n_paths / 64)
};

// the kept placements of candidate read r at distance d = d*(r): f(global path, text offset of the read's first base) once per placement
// (rescue_place's second sweep without the tables).  rescue_each_kept_strand tells f the strand as well (kernels_rescue_rec.hpp)
template <class F> __device__ __forceinline__ void rescue_each_kept_strand(const RescueArgs &a, uint32_t r, uint32_t d, F &&f)
{
    const uint64_t o = a.seq_off[r];
    const uint32_t len = (uint32_t)(a.seq_off[r + 1] - o), nb = len / kRescueAnchor;
    const uint64_t w0 = ((o - a.seq_off[0]) >> 5) + r;
    for (uint32_t strand = 0; strand < 2u; strand++) {
        const unsigned long long *rd = a.rbuf + strand * a.rcap + w0;
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t key = (uint32_t)(rd[j >> 1] >> (32u * (j & 1u)));
            uint32_t slot = rescue_hash(key) & a.tab_mask;
            uint4 e = a.tab[slot];
            while (e.z && e.x != key) { slot = (slot + 1u) & a.tab_mask; e = a.tab[slot]; }
            for (uint32_t q = e.y; q < e.y + e.z; q++) {
                const uint2 oc = a.occ[q];
                const uint4 pi = a.path[oc.x];
                const uint32_t rel = oc.y - pi.x;
                if (rel < kRescueAnchor * j || rel - kRescueAnchor * j + len > pi.y) continue;
                if (rescue_distance(a, rd, len, pi.x + rel - kRescueAnchor * j, j, d) == d) f(oc.x, rel - kRescueAnchor * j, strand);
            }
        }
    }
}

template <class F> __device__ __forceinline__ void rescue_each_kept(const RescueArgs &a, uint32_t r, uint32_t d, F &&f)
{
    rescue_each_kept_strand(a, r, d, [&](uint32_t p, uint32_t to, uint32_t) { f(p, to); });
}

// candidate i of the batch is rescued: its row is written and dstar[i] holds d*
__device__ __forceinline__ bool rescue_ec_rescued(const RescueEcArgs &a, uint32_t i) { return a.r.dstar[i] != kRescueUnplaced; }

// what rescue_ec_slow_body tells of every kept placement beyond the bitmap: nothing here, the placement to the slot's log in
// kernels_rescue_acov.hpp (RescueAcovLog)
struct RescueNoLog {
    __device__ __forceinline__ void kept(const RescueEcArgs &, uint32_t, uint32_t, uint32_t, uint32_t) const {}
};

template <class Log> __device__ __forceinline__ void rescue_ec_slow_body(const RescueEcArgs &a, const Log &log)
{
    if (!shared_live(a.s)) return;
    const uint32_t n = min(*a.r.n_cand, a.r.n_reads);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t r = a.r.cand[i];
        if (!rescue_ec_rescued(a, i) || a.s.set_graph[(size_t)r * kSharedSegs] != kSharedEmpty) continue;
        const uint32_t row = atomicAdd(a.n_slow, 1u);      // (slow rescued reads are rare: one atomic each)
        if (row >= a.rows) continue;                        // no bitmap left: the count tells the host, which fails the batch
        unsigned long long *b = a.bits + (size_t)row * a.bw;
        for (uint32_t w = 0; w < a.bw; w++) b[w] = 0;
        rescue_each_kept(a.r, r, a.r.dstar[i], [&](uint32_t p, uint32_t to) {
            if (p >= a.s.n_paths) return;
            b[p >> 6] |= 1ull << (p & 63u);
            log.kept(a, r, row, p, to);
        });
    }
}

__global__ __launch_bounds__(kBlock) void rescue_ec_slow_kernel(RescueEcArgs a) { rescue_ec_slow_body(a, RescueNoLog{}); }

__global__ __launch_bounds__(kBlock) void rescue_ec_insert_kernel(RescueEcArgs a)
{
    if (!shared_live(a.s)) return;
    const uint32_t n = min(*a.r.n_cand, a.r.n_reads);
    uint32_t st[1] = {0};
    for (uint32_t i0 = blockIdx.x * kBlock; i0 < n; i0 += gridDim.x * kBlock) {      // (uniform per wavefront: the shuffles of the stats)
        const uint32_t i = i0 + threadIdx.x;
        if (i >= n || !rescue_ec_rescued(a, i)) continue;
        const uint32_t r = a.r.cand[i];
        if (a.s.set_graph[(size_t)r * kSharedSegs] == kSharedEmpty) continue;
        shared_insert_row(a.s, r);
        st[0]++;
    }
    const uint32_t where[1] = {0};
    rescue_add_stats(a.stats, st, where);
}

// one thread per slot of the batch's table (tab_size slots).  tab_ser (rescued reads in assigned coverage: kernels_rescue_acov.hpp) gets
// the serial of every occupied slot's EC, and the slots then stay as they are for the probe behind this launch, which clears them
template <bool kKeep>
__device__ __forceinline__ void rescue_ec_merge_body(const SharedArgs &a, const EcTable &t, uint32_t tab_size, uint32_t epoch, uint32_t *fill, uint32_t *tab_ser)
{
    if (!shared_live(a)) return;
    for (uint32_t slot = blockIdx.x * kBlock + threadIdx.x; slot < tab_size; slot += gridDim.x * kBlock) {
        const uint32_t r = a.tab_rep[slot];
        if (r == kSharedEmpty) continue;
        const uint32_t ser = ec_add(t, a.set_graph + (size_t)r * kSharedSegs, a.set_mask + (size_t)r * kSharedSegs * a.pw, a.pw, a.tab_cnt[slot], epoch, true, fill, 0);
        if (kKeep) { tab_ser[slot] = ser; continue; }
        a.tab_rep[slot] = kSharedEmpty;
        a.tab_cnt[slot] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void rescue_ec_merge_kernel(SharedArgs a, EcTable t, uint32_t tab_size, uint32_t epoch, uint32_t *fill)
{
    rescue_ec_merge_body<false>(a, t, tab_size, epoch, fill, nullptr);
}

} // namespace groot
