// kernels_gap.hpp -- gapped rescue of the reads mismatch rescue leaves (groot_hip_gap_*; the definition is in include/groot_hip.h,
// "gapped rescue").  One kernel per batch on the tail stream, behind the two rescue kernels:
//
// rescue_count_kernel<true> (kernels_rescue.hpp) hands on the candidates it could not place ungapped and that are long enough for a gap
//                      (len >= A (M + 3)) in a list of their own, one ballot and one atomic per wavefront; only those for which a block had
//                      a table hit at all, since a gapped placement needs an occurrence of one of the read's blocks.
// rescue_gap_kernel    one thread per gap candidate, two sweeps.  Either sweep takes every occurrence t of every 16-base block j of both
//                      orientations and both hypotheses for it: the block lies in the part in front of the gap (x = t - 16 j) or behind it
//                      (x = t - 16 j - g for a DEL, + g for an INS), for both types and every g in 1..G.  A tuple (p, strand, x, type, g) is
//                      two streams of mismatch bits indexed by the cut k: P(k) = R[k] != T[x + k] in front of the gap, S(k) = R[k] != T[x + g + k]
//                      (DEL) or R[k + g] != T[x + k] (INS: the READ is shifted, so no text in front of x is touched) behind it, both over
//                      Ls = len (DEL) or len - g (INS) positions, and d(k) = |P[0, k)| + |S[k, Ls)| for A <= k <= Ls - A.  The streams
//                      are 64-bit XOR words as in rescue_diff; d(k + 1) - d(k) = P(k) - S(k) is non-zero at set bits only, so the walk
//                      for (d, k*) visits set bits, in ascending order, and a strict `<` keeps the smallest k.  Sweep 1 keeps the smallest
//                      e = d + g, sweep 2 adds the tuples at e*.  A tuple is reached through (block i, hypothesis h) exactly when block i
//                      equals the text on h's diagonal and lies in the window W; sweep 2 counts it only through the lowest such (i, h), so
//                      every tuple counts once without a sort (gap_sweep: the walk of either sweep, which the emit kernel of the
//                      gapped records, kernels_gap_rec.hpp, takes a third time at e*; rescue_gap_body: the kernel with a sink).  gdepth: starts / ends in report coverage's layout with plain atomicAdd (a
//                      DEL adds two intervals).  Events: an open-addressing table, key claimed with atomicCAS, count with atomicAdd.
// Integer sums only: the tables do not depend on the order of the candidates, of the wavefronts or of the batches; the table's slot
// order does, the export sorts.
#pragma once

#include "kernels_rescue.hpp"

namespace groot {

// stats[]: gap candidates, gap-rescued, kept placements, kept DEL, kept INS, too short for a gap, distinct events, events dropped
constexpr uint32_t kGapStats = 8;
constexpr uint32_t kGapMax = 8;

struct GapArgs {
    RescueArgs r;                          // the candidates' words, the texts and the 16-mer table: rescue's
    const uint32_t *gcand, *n_gcand;       // the gap candidates of the batch (rescue_count_kernel<true>), their number
    unsigned long long *starts, *ends;     // gdepth in report coverage's layout
    unsigned long long *ev_key, *ev_cnt;   // [ev_mask + 1] the event table; key 0 = free (an event's pos is at least A - 1, so no key is 0)
    unsigned long long *stats;             // [kGapStats]
    uint64_t ev_mask;
    uint32_t max_gap;
};

// key = slot_base[p] + pos (40 bits) | type (1) | g - 1 (3) | seq (16)
__host__ __device__ __forceinline__ unsigned long long gap_event_key(uint64_t slot, uint32_t type, uint32_t g, uint32_t seq)
{
    return (unsigned long long)slot | (unsigned long long)type << 40 | (unsigned long long)(g - 1u) << 41 | (unsigned long long)seq << 44;
}
__host__ __device__ __forceinline__ uint64_t gap_event_hash(unsigned long long k)
{
    k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
    k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
    return k ^ (k >> 31);
}

// += 1 for the event; a key that finds no slot after probing the whole table is counted as dropped
__device__ __forceinline__ void gap_event_add(const GapArgs &a, unsigned long long key)
{
    uint64_t slot = gap_event_hash(key) & a.ev_mask;
    for (uint64_t probe = 0; probe <= a.ev_mask; probe++, slot = (slot + 1) & a.ev_mask) {
        const unsigned long long was = atomicCAS(a.ev_key + slot, 0ull, key);
        if (was == 0ull) atomicAdd(a.stats + 6, 1ull);
        if (was == 0ull || was == key) { atomicAdd(a.ev_cnt + slot, 1ull); return; }
    }
    atomicAdd(a.stats + 7, 1ull);
}

// the mismatching bases of two words of bases as bits of kRescueOdd
__device__ __forceinline__ unsigned long long gap_mis(unsigned long long x) { return (x | (x >> 1)) & kRescueOdd; }

// word w of the oriented read rd (nw words) from base g on: the read shifted down by g bases (0 <= g <= 8)
__device__ __forceinline__ unsigned long long gap_read_from(const unsigned long long *rd, uint32_t nw, uint32_t w, uint32_t g)
{
    const unsigned long long lo = rd[w], hi = w + 1u < nw ? rd[w + 1u] : 0ull;
    return g ? (lo >> (2u * g)) | (hi << (64u - 2u * g)) : lo;
}

// (d, k*) of the tuple (text base tg of x, type, g) of the oriented read rd (len bases): d = kRescueNone when the window holds an 'N'
// or when d is above maxd
__device__ __forceinline__ uint32_t gap_fit(const RescueArgs &a, const unsigned long long *rd, uint32_t len, uint32_t tg, uint32_t ins, uint32_t g, uint32_t maxd, uint32_t &kstar)
{
    const uint32_t nw = (len + 31u) >> 5, ls = ins ? len - g : len, nws = (ls + 31u) >> 5, kmax = ls - kRescueAnchor;
    int v = 0, best = 0;                   // v(k) = |P[0, k)| - |S[0, k)|: d(k) = v(k) + |S|
    uint32_t tot = 0;
    kstar = kRescueAnchor;
    for (uint32_t w = 0; w < nws; w++) {
        const unsigned long long keep = (w + 1u == nws && (ls & 31u)) ? (1ull << (2u * (ls & 31u))) - 1ull : ~0ull;
        const unsigned long long tp = rescue_text64(a.text, tg + 32u * w);
        unsigned long long tags = rescue_text64(a.tag, tg + 32u * w), sx;
        if (ins) sx = gap_read_from(rd, nw, w, g) ^ tp;
        else {
            sx = rd[w] ^ rescue_text64(a.text, tg + g + 32u * w);
            tags |= rescue_text64(a.tag, tg + g + 32u * w);
        }
        if (tags & kRescueOdd & keep) return kRescueNone;
        const unsigned long long P = gap_mis(rd[w] ^ tp) & keep, S = gap_mis(sx) & keep;
        tot += (uint32_t)__popcll(S);
        unsigned long long m = P | S;
        if (w == 0) {                      // v(A), the first allowed cut
            v = __popcll(P & 0xFFFFFFFFull) - __popcll(S & 0xFFFFFFFFull);
            if ((uint32_t)__popcll(P & 0xFFFFFFFFull) > maxd) return kRescueNone;      // d(k) >= |P[0, A)|
            best = v;
            m &= ~0xFFFFFFFFull;
        }
        // the steps k -> k + 1 with A <= k < kmax
        if (32u * w >= kmax) m = 0;
        else if (kmax - 32u * w < 32u) m &= (1ull << (2u * (kmax - 32u * w))) - 1ull;
        for (; m; m &= m - 1) {
            const uint32_t bit = (uint32_t)__ffsll(m) - 1u;
            v += (int)((P >> bit) & 1ull) - (int)((S >> bit) & 1ull);
            if (v < best) { best = v; kstar = 32u * w + (bit >> 1) + 1u; }
        }
    }
    const uint32_t d = (uint32_t)(best + (int)tot);
    return d <= maxd ? d : kRescueNone;
}

// block i of the read equals the text from base t on
__device__ __forceinline__ bool gap_block_at(const RescueArgs &a, const unsigned long long *rd, uint32_t i, uint32_t t)
{
    return (uint32_t)rescue_text64(a.text, t) == (uint32_t)(rd[i >> 1] >> (32u * (i & 1u)));
}

// block i under hypothesis h (0: in front of the gap, 1: behind it) lies in the window of a tuple of this type and g
__device__ __forceinline__ bool gap_block_in(uint32_t i, uint32_t h, uint32_t ins, uint32_t g, uint32_t len)
{
    return !ins || (h ? i >= 1u : kRescueAnchor * i + kRescueAnchor + g <= len);
}

// what a sweep-2 walk tells of every kept tuple (of read r, on path p) beyond the tables: nothing here, their number per read for the
// gapped records (kernels_gap_rec.hpp), the path to the read's set row for the gap-placed reads in the classes (kernels_gap_ec.hpp)
struct GapNoSink {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void kept(const RescueArgs &, uint32_t, uint32_t) {}
    __device__ __forceinline__ void done(const RescueArgs &, uint32_t, uint32_t, uint32_t, bool) {}
};

// One sweep over the tuples of the oriented reads at w0 (len bases): occurrence x hypothesis x type x g.  Sweep 0 lowers `best` to the
// smallest e = d + g.  Sweep 1 calls f(path, its res_path entry, strand, x, ins, g, k*, d, the oriented read) for every tuple at
// e = best, each once: only through the lowest (block, hypothesis) that reaches it.  rescue_gap_kernel's second sweep and
// gap_rec_emit_kernel (kernels_gap_rec.hpp) are this one walk: the same tuples in the same order.
template <class F> __device__ __forceinline__ void gap_sweep(const RescueArgs &a, uint32_t G, uint64_t w0, uint32_t len, uint32_t sweep, uint32_t &best, F &&f)
{
    const uint32_t M = a.max_mismatch, nb = len / kRescueAnchor;
    for (uint32_t strand = 0; strand < 2u; strand++) {
        const unsigned long long *rd = a.rbuf + strand * a.rcap + w0;
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t key = (uint32_t)(rd[j >> 1] >> (32u * (j & 1u)));
            uint32_t slot = rescue_hash(key) & a.tab_mask;
            uint4 e = a.tab[slot];
            while (e.z && e.x != key) { slot = (slot + 1u) & a.tab_mask; e = a.tab[slot]; }
            for (uint32_t q = e.y; q < e.y + e.z; q++) {
                const uint2 oc = a.occ[q];
                const uint4 pi = a.path[oc.x];                  // {text start, bases inside path_len, first Position, 0}
                const int t0 = (int)(oc.y - pi.x) - (int)(kRescueAnchor * j);      // x under the hypothesis "in front of the gap"
                for (uint32_t v = 0; v < 4u * G; v++) {         // hypothesis, type, g
                    const uint32_t h = v & 1u, ins = (v >> 1) & 1u, g = (v >> 2) + 1u;
                    if (!gap_block_in(j, h, ins, g, len)) continue;
                    const int x = t0 - (h ? (ins ? -(int)g : (int)g) : 0);
                    if (x < 0 || (uint32_t)x + (ins ? len - g : len + g) > pi.y) continue;      // W would hang over an end of the path
                    if (g > best) continue;                     // e = d + g >= g
                    uint32_t ks;
                    const uint32_t d = gap_fit(a, rd, len, pi.x + (uint32_t)x, ins, g, min(M, best - g), ks);
                    if (d == kRescueNone) continue;
                    if (sweep == 0) { best = min(best, d + g); continue; }
                    if (d + g != best) continue;
                    bool lower = false;                         // a lower (block, hypothesis) reaches the tuple as well: it counts it
                    for (uint32_t i = 0; i <= j && !lower; i++)
                        for (uint32_t hh = 0; hh < (i < j ? 2u : h); hh++)
                            if (gap_block_in(i, hh, ins, g, len) &&
                                gap_block_at(a, rd, i, (uint32_t)((int)(pi.x + (uint32_t)x + kRescueAnchor * i) + (hh ? (ins ? -(int)g : (int)g) : 0))))
                                lower = true;
                    if (lower) continue;
                    f(oc.x, pi, strand, (uint32_t)x, ins, g, ks, d, rd);
                }
            }
        }
    }
}

template <class Sink> __device__ __forceinline__ void rescue_gap_body(const GapArgs &ga, Sink sink)
{
    const RescueArgs &a = ga.r;
    if (a.ctr->flags & kCovSkipFlags) return;
    const uint32_t n = min(*ga.n_gcand, a.n_reads), M = a.max_mismatch, G = ga.max_gap;
    const uint64_t off0 = a.seq_off[0];
    uint32_t st[4] = {0, 0, 0, 0};         // gap-rescued, kept placements, kept DEL, kept INS
    for (uint32_t c = blockIdx.x * kBlock + threadIdx.x; c < n; c += gridDim.x * kBlock) {
        const uint32_t r = ga.gcand[c];
        const uint64_t o = a.seq_off[r];
        const uint32_t len = (uint32_t)(a.seq_off[r + 1] - o);
        const uint64_t w0 = ((o - off0) >> 5) + r;
        uint32_t best = M + G + 1u;        // e*
        sink.begin();
        for (uint32_t sweep = 0; sweep < 2u && (sweep == 0 || best <= M + G); sweep++)
            gap_sweep(a, G, w0, len, sweep, best, [&](uint32_t p, const uint4 &pi, uint32_t, uint32_t x, uint32_t ins, uint32_t g, uint32_t ks, uint32_t, const unsigned long long *rd) {
                st[1]++;
                st[2] += 1u - ins;
                st[3] += ins;
                sink.kept(a, r, p);
                const uint64_t at = a.slot_base[p] + pi.z + x;
                atomicAdd(ga.starts + at, 1ull);
                uint32_t seq = 0;
                if (ins) {
                    atomicAdd(ga.ends + at + len - g, 1ull);
                    for (uint32_t i = 0; i < g; i++) {
                        const uint32_t code = (uint32_t)(rd[(ks + i) >> 5] >> (2u * ((ks + i) & 31u))) & 3u;
                        seq |= (code ^ (code >> 1)) << (2u * i);      // A C T G -> A C G T
                    }
                } else {
                    atomicAdd(ga.ends + at + ks, 1ull);
                    atomicAdd(ga.starts + at + ks + g, 1ull);
                    atomicAdd(ga.ends + at + len + g, 1ull);
                }
                gap_event_add(ga, gap_event_key(at + ks - 1u, ins, g, seq));
            });
        if (best <= M + G) st[0]++;
        sink.done(a, c, r, best, best <= M + G);
    }
    const uint32_t where[4] = {1, 2, 3, 4};
    rescue_add_stats(ga.stats, st, where);
}

// the kernel launched while the gapped records are off; rescue_gap_rec_kernel (kernels_gap_rec.hpp) is the same body with a sink
__global__ __launch_bounds__(kBlock) void rescue_gap_kernel(GapArgs ga)
{
    rescue_gap_body(ga, GapNoSink());
}

} // namespace groot
