// kernels_rescue.hpp -- mismatch rescue of unaligned reads on the device (groot_hip_rescue_*; the definition is in include/groot_hip.h,
// "mismatch rescue").  Two kernels per batch on the tail stream, behind the order stage:
//
// rescue_pack_kernel   one thread per read of the batch.  A read without a record (trav_off[r + 1] == trav_off[r]: the order stage's
//                      exclusive scan of the per-read record counts, still in place on the tail stream) is scanned once: a byte other than
//                      A/C/G/T leaves it out (the exception list is already patched into the bases), so does a length below A (M + 1).  A
//                      candidate is written at 2 bits per base, forward and reverse-complemented, 32 bases to a 64-bit word, to words of
//                      its own (word (seq_off[r] - seq_off[0]) / 32 + r of either strand: no two reads share a word), and joins the
//                      candidate list: one ballot and one atomic per wavefront, as the first pass builds its list.
// rescue_count_kernel  one thread per candidate, two sweeps.  Either sweep probes the floor(len / 16) disjoint blocks of both orientations
//                      in the 16-mer table and verifies every occurrence as a whole-read XOR / popcount against the 2-bit text (64-bit
//                      words, a funnel shift for the text's bit offset, the tag for 'N', the last word masked).  A placement reached
//                      through block j is dropped when a block i < j is mismatch-free there too: it was, or will be, reached through i,
//                      so every placement counts once without a sort.  Sweep 1 keeps the smallest distance d*, sweep 2 adds the placements
//                      at d* to the dense tables with plain atomicAdd: starts / ends in report coverage's layout (path_len + 1 slots per
//                      path), alt as four counters (A, C, G, T) per slot.
//                      rescue_count_kernel<true> (gapped rescue on: kernels_gap.hpp) also hands on the candidates it leaves unplaced;
//                      <false> is the kernel without that, and the only one launched while gapped rescue is off.
//                      Both are rescue_count_body with a sink that does nothing; rescue_count_ec_kernel (kernels_rescue_ec.hpp: rescued
//                      reads in the equivalence classes) is the same body with a sink that keeps the paths of the kept placements, and
//                      rescue_count_rec_kernel (kernels_rescue_rec.hpp: rescued records) with one that also counts them per read.
// Integer sums only: the tables do not depend on the order of the candidates, of the wavefronts or of the batches.
#pragma once

#include "kernels_common.hpp"
#include "kernels_cov.hpp"   // kCovSkipFlags

namespace groot {

// stats[]: candidates, rescued, rescued at d* = 0, kept placements, too short, non-ACGT, reads whose words did not fit rbuf (never, when
// the batch keeps to max_batch_bases)
constexpr uint32_t kRescueStats = 8;
constexpr uint32_t kRescueNone = 0xFFFFFFFFu;
constexpr uint8_t kRescueUnplaced = 0xFFu;      // RescueArgs::dstar of a candidate that is not rescued
constexpr unsigned long long kRescueOdd = 0x5555555555555555ull;

struct RescueArgs {
    const uint8_t *seq;            // the batch's bases (ASCII, exceptions patched in)
    const uint64_t *seq_off;       // [n_reads + 1]
    const DeviceCounters *ctr;     // n_trav + flags of the pass
    const uint32_t *trav_off;      // [n_reads] first record of every read (the order stage's scan)
    unsigned long long *rbuf;      // [2][rcap] the candidates at 2 bits per base: forward, reverse complement
    uint64_t rcap;
    uint32_t *cand, *n_cand;       // [n_reads] the candidates, their number
    const uint32_t *text, *tag;    // RescueTables (index_tables.hpp)
    const uint4 *path, *tab;
    const uint2 *occ;
    const uint64_t *slot_base;     // [n_paths] first slot of global path p: sum_{q<p} (path_len[q] + 1)
    unsigned long long *starts, *ends, *alt, *stats;
    uint32_t tab_mask, n_reads, max_mismatch;
    // gapped rescue (kernels_gap.hpp; rescue_count_kernel<true> only): the candidates left unplaced that are long enough for a gap
    uint32_t *gcand, *n_gcand;     // [n_reads] the gap candidates handed on, their number
    unsigned long long *gstats;    // GapArgs::stats
    // rescued reads in the equivalence classes (kernels_rescue_ec.hpp; rescue_count_ec_kernel and the kernels behind it only)
    const uint2 *path_bit;         // [n_paths] {graph of global path p, p's bit in that graph's path sets}
    uint32_t *set_graph;           // SharedArgs::set_graph / set_mask: row r is free behind shared_expand_kernel
    uint64_t *set_mask;
    uint8_t *dstar;                // [n_reads] d* of candidate i, kRescueUnplaced when it is not rescued
    uint32_t pw, max_segs;         // SharedArgs::pw, max_segs
    // rescued records (kernels_rescue_rec.hpp; the rescue_count_rec kernels and rescue_rec_emit_kernel only)
    uint32_t *n_kept;              // [n_reads + 1] kept placements of read r (zeroed ahead of the launch), then their exclusive scan in rec_off
    uint8_t *rec_d;                // [n_reads] d* of candidate i, kRescueUnplaced when it is not rescued (a copy of its own: dstar is there only beside the classes)
};

// what rescue_place tells of every kept placement beyond the dense tables: nothing here, the path to the read's set row in
// kernels_rescue_ec.hpp (RescueRow)
struct RescueNoSink {
    __device__ __forceinline__ void kept(const RescueArgs &, uint32_t, uint32_t) {}
    __device__ __forceinline__ void done(const RescueArgs &, uint32_t, uint32_t, uint32_t) {}
};

// the workgroup's sums of up to kRescueStats per-thread counts, one atomic each per wavefront
template <uint32_t N> __device__ __forceinline__ void rescue_add_stats(unsigned long long *stats, const uint32_t (&st)[N], const uint32_t (&where)[N])
{
    for (uint32_t i = 0; i < N; i++) {
        uint32_t v = st[i];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(stats + where[i], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kBlock) void rescue_pack_kernel(RescueArgs a)
{
    if (a.ctr->flags & kCovSkipFlags) return;
    const uint32_t n_trav = a.ctr->n_trav, min_len = kRescueAnchor * (a.max_mismatch + 1u);
    const uint64_t off0 = a.seq_off[0];
    uint32_t st[3] = {0, 0, 0};            // too short, non-ACGT, no room
    for (uint32_t r0 = blockIdx.x * kBlock; r0 < a.n_reads; r0 += gridDim.x * kBlock) {      // (uniform per wavefront: the ballot below)
        const uint32_t r = r0 + threadIdx.x;
        bool is_cand = false;
        if (r < a.n_reads && (r + 1 < a.n_reads ? a.trav_off[r + 1] : n_trav) == a.trav_off[r]) {
            const uint64_t o = a.seq_off[r];
            const uint32_t len = (uint32_t)(a.seq_off[r + 1] - o), nw = (len + 31u) >> 5;
            const uint64_t w0 = ((o - off0) >> 5) + r;
            const uint8_t *s = a.seq + o;
            if (w0 + nw > a.rcap) st[2]++;
            else {
                bool acgt = true;
                unsigned long long w = 0;
                for (uint32_t i = 0; i < len; i++) {
                    const uint8_t b = s[i];
                    acgt &= b == 'A' || b == 'C' || b == 'G' || b == 'T';
                    w |= (unsigned long long)((b >> 1) & 3u) << (2 * (i & 31u));
                    if ((i & 31u) == 31u || i + 1 == len) {
                        if (len >= min_len) a.rbuf[w0 + (i >> 5)] = w;      // (a read that is too short is only scanned, for the stats)
                        w = 0;
                    }
                }
                if (!acgt) st[1]++;
                else if (len < min_len) st[0]++;
                else {
                    is_cand = true;
                    for (uint32_t i = 0; i < len; i++) {                  // the reverse complement: A <-> T is 0 <-> 2, C <-> G is 1 <-> 3
                        w |= (unsigned long long)((((uint32_t)s[len - 1 - i] >> 1) & 3u) ^ 2u) << (2 * (i & 31u));
                        if ((i & 31u) == 31u || i + 1 == len) { a.rbuf[a.rcap + w0 + (i >> 5)] = w; w = 0; }
                    }
                }
            }
        }
        const unsigned long long cb = __ballot(is_cand);
        if (cb) {
            const unsigned lane = threadIdx.x & 63u;
            const int first = __ffsll(cb) - 1;
            uint32_t at = 0;
            if ((int)lane == first) at = atomicAdd(a.n_cand, (uint32_t)__popcll(cb));
            at = __shfl(at, first);
            if (is_cand) a.cand[at + (uint32_t)__popcll(cb & ((1ull << lane) - 1ull))] = r;
        }
    }
    const uint32_t where[3] = {4, 5, 6};
    rescue_add_stats(a.stats, st, where);
}

// the 32 bases from base g of a 2-bit text as one word (the texts carry slack for the three dwords)
__device__ __forceinline__ unsigned long long rescue_text64(const uint32_t *t, uint32_t g)
{
    const uint32_t d = g >> 4, sh = 2u * (g & 15u);
    const unsigned long long lo = (unsigned long long)t[d] | ((unsigned long long)t[d + 1] << 32), hi = t[d + 2];
    return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

// word k of the oriented read rd (len bases) against the text at base g: its mismatching bases as bits of kRescueOdd; kRescueNone in
// `n` when the window holds an 'N' there
__device__ __forceinline__ unsigned long long rescue_diff(const RescueArgs &a, const unsigned long long *rd, uint32_t len, uint32_t g, uint32_t k, bool &n)
{
    const unsigned long long keep = (k + 1u == ((len + 31u) >> 5) && (len & 31u)) ? (1ull << (2u * (len & 31u))) - 1ull : ~0ull;
    const unsigned long long x = rd[k] ^ rescue_text64(a.text, g + 32u * k);
    n = (rescue_text64(a.tag, g + 32u * k) & kRescueOdd & keep) != 0;
    return (x | (x >> 1)) & kRescueOdd & keep;
}

// Hamming distance of the placement at text base g, reached through block j; kRescueNone when it is above maxd, when the window holds
// an 'N', or when an earlier block is mismatch-free there as well (then that block counts it)
__device__ __forceinline__ uint32_t rescue_distance(const RescueArgs &a, const unsigned long long *rd, uint32_t len, uint32_t g, uint32_t j, uint32_t maxd)
{
    uint32_t d = 0;
    const uint32_t nw = (len + 31u) >> 5;
    for (uint32_t k = 0; k < nw; k++) {
        bool n;
        const unsigned long long m = rescue_diff(a, rd, len, g, k, n);
        if (n) return kRescueNone;
        if (2u * k < j && !(uint32_t)m) return kRescueNone;
        if (2u * k + 1u < j && !(uint32_t)(m >> 32)) return kRescueNone;
        d += (uint32_t)__popcll(m);
        if (d > maxd) return kRescueNone;
    }
    return d;
}

// the placements of candidate r: sweep 1 keeps the smallest distance, sweep 2 adds the placements at it to the tables.  -> d*, M + 1 when
// there is no placement; hit: one of its blocks is in the table at all
template <class Sink>
__device__ __forceinline__ uint32_t rescue_place(const RescueArgs &a, uint32_t r, uint32_t &len, uint32_t (&st)[4], bool &hit, Sink &sink)
{
    const uint32_t M = a.max_mismatch;
    const uint64_t off0 = a.seq_off[0];
    const uint64_t o = a.seq_off[r];
    len = (uint32_t)(a.seq_off[r + 1] - o);
    const uint32_t nb = len / kRescueAnchor;
    const uint64_t w0 = ((o - off0) >> 5) + r;
    st[0]++;
    uint32_t best = M + 1u;
    for (uint32_t sweep = 0; sweep < 2u && (sweep == 0 || best <= M); sweep++)
        for (uint32_t strand = 0; strand < 2u; strand++) {
            const unsigned long long *rd = a.rbuf + strand * a.rcap + w0;
            for (uint32_t j = 0; j < nb; j++) {
                const uint32_t key = (uint32_t)(rd[j >> 1] >> (32u * (j & 1u)));
                uint32_t slot = rescue_hash(key) & a.tab_mask;
                uint4 e = a.tab[slot];
                while (e.z && e.x != key) { slot = (slot + 1u) & a.tab_mask; e = a.tab[slot]; }
                hit |= e.z != 0;
                for (uint32_t q = e.y; q < e.y + e.z; q++) {
                    const uint2 oc = a.occ[q];
                    const uint4 pi = a.path[oc.x];                  // {text start, bases inside path_len, first Position, 0}
                    const uint32_t rel = oc.y - pi.x;
                    if (rel < kRescueAnchor * j || rel - kRescueAnchor * j + len > pi.y) continue;      // the read would hang over an end of the path
                    const uint32_t to = rel - kRescueAnchor * j, g = pi.x + to;
                    const uint32_t d = rescue_distance(a, rd, len, g, j, sweep ? best : min(best, M));
                    if (sweep == 0) { best = min(best, d); continue; }
                    if (d != best) continue;
                    st[3]++;
                    sink.kept(a, r, oc.x);
                    const uint64_t at = a.slot_base[oc.x] + pi.z + to;
                    atomicAdd(a.starts + at, 1ull);
                    atomicAdd(a.ends + at + len, 1ull);
                    for (uint32_t k = 0; d && k < ((len + 31u) >> 5); k++) {
                        bool nn;
                        for (unsigned long long m = rescue_diff(a, rd, len, g, k, nn); m; m &= m - 1) {
                            const uint32_t bit = (uint32_t)__ffsll(m) - 1u, code = (uint32_t)(rd[k] >> bit) & 3u;
                            atomicAdd(a.alt + 4u * (at + 32u * k + (bit >> 1)) + (code ^ (code >> 1)), 1ull);      // A C T G -> A C G T
                        }
                    }
                }
            }
        }
    return best;
}

// kGap: a candidate that stays unplaced and has len >= A (M + 3) joins the gap candidates (one ballot and one atomic per wavefront), if
// one of its blocks had a table hit at all: a gapped placement needs an occurrence of a block.  The gap stats count by the definition.
// Sink: RescueNoSink, or RescueRow (kernels_rescue_ec.hpp), which also gets d* of every candidate
template <bool kGap, class Sink> __device__ __forceinline__ void rescue_count_body(const RescueArgs &a)
{
    if (a.ctr->flags & kCovSkipFlags) return;
    const uint32_t n = min(*a.n_cand, a.n_reads), M = a.max_mismatch;
    uint32_t st[4] = {0, 0, 0, 0};         // candidates, rescued, rescued at 0, kept placements
    uint32_t gst[2] = {0, 0};              // gap candidates, too short for a gap
    for (uint32_t i0 = blockIdx.x * kBlock; i0 < n; i0 += gridDim.x * kBlock) {      // (uniform per wavefront: the ballot below)
        const uint32_t i = i0 + threadIdx.x, r = i < n ? a.cand[i] : 0u;
        bool hand_on = false;
        if (i < n) {
            uint32_t len;
            bool hit = false;
            Sink sink{};
            const uint32_t best = rescue_place(a, r, len, st, hit, sink);
            sink.done(a, r, i, best);
            if (best <= M) st[1]++;
            if (best == 0) st[2]++;
            if (kGap && best > M) {
                const bool long_enough = len >= kRescueAnchor * (M + 3u);
                gst[0] += long_enough;
                gst[1] += !long_enough;
                hand_on = hit && long_enough;
            }
        }
        if (kGap) {
            const unsigned long long cb = __ballot(hand_on);
            if (cb) {
                const unsigned lane = threadIdx.x & 63u;
                const int first = __ffsll(cb) - 1;
                uint32_t at = 0;
                if ((int)lane == first) at = atomicAdd(a.n_gcand, (uint32_t)__popcll(cb));
                at = __shfl(at, first);
                if (hand_on) a.gcand[at + (uint32_t)__popcll(cb & ((1ull << lane) - 1ull))] = r;
            }
        }
    }
    const uint32_t where[4] = {0, 1, 2, 3};
    rescue_add_stats(a.stats, st, where);
    if (kGap) {
        const uint32_t gwhere[2] = {0, 5};
        rescue_add_stats(a.gstats, gst, gwhere);
    }
}

template <bool kGap> __global__ __launch_bounds__(kBlock) void rescue_count_kernel(RescueArgs a) { rescue_count_body<kGap, RescueNoSink>(a); }

} // namespace groot
