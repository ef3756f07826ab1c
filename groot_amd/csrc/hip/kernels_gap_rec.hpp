// kernels_gap_rec.hpp -- gapped records (groot_hip_gap_rec_*; the definition is in include/groot_hip.h, "gapped records"): every kept
// gapped placement of every gap-rescued read of a batch as one 24-byte record (read, path, pos, k, mm[3], strand, d, type, g), in
// ascending (read, path, strand, pos, type, g) order, in a buffer the pipeline slot owns.  Three steps per batch on the tail stream,
// behind rescue_gap_kernel's inputs and launched only while the feature is on:
//
// rescue_gap_rec_kernel    takes the place of rescue_gap_kernel: the same body (rescue_gap_body, kernels_gap.hpp), whose sink also
//                          counts the candidate's kept placements and leaves them at n_gkept[r] -- indexed by READ, zeroed ahead of the
//                          launch, so a read that is no gap candidate or is not gap-rescued holds 0 -- and e* (kGapRecNone: none) at
//                          gap_e[c], indexed by gap candidate.
// the scan                 rocprim::exclusive_scan of n_gkept[0 .. n_reads] (one slot more than reads: the last output is the batch's
//                          total) into 64-bit offsets.  Indexed by read, a segment's start does not depend on the order in which the
//                          wavefronts built the gap-candidate list.
// gap_rec_emit_kernel      one thread per gap candidate with a stored e*: one walk at e* (gap_sweep, sweep 2: the tuples of the count in
//                          the order of the count), placement j to rec[off[r] + j] with the mismatch offsets re-derived from the P and S
//                          mismatch words of the tuple -- P bits below k* at offset = index, S bits from k* on at offset = index (DEL) or
//                          index + g (INS): ascending by construction -- then sorts its own segment by (path, strand, pos, type, g) in
//                          place: an insertion sort over global memory, no other thread touches the segment.  A segment that would end
//                          past `cap` is not written at all; the total tells the host, which fails the batch.
// The record travels as six dwords (the layout of groot_gap_record on a little-endian host): the mismatch offsets are kept in one 64-bit
// register and shifted in, so that no per-thread array is indexed dynamically.  Plain loads and stores only, and every kernel reads the
// pass's status word first: a pass that collect redoes, or a batch that fails, leaves the total at 0.
#pragma once

#include "kernels_gap.hpp"

namespace groot {

constexpr uint32_t kGapRecWords = 6;         // sizeof(groot_gap_record) / 4
constexpr uint8_t kGapRecNone = 0xFF;        // gap_e[c] of a gap candidate that is not gap-rescued

struct GapRecArgs {
    GapArgs g;
    uint32_t *n_gkept;             // [n_reads + 1] kept gapped placements of read r (zeroed ahead of the launch)
    uint8_t *gap_e;                // [n_reads] e* of gap candidate c, kGapRecNone when it is not gap-rescued
    const uint64_t *off;           // [n_reads + 1] first record of read r, the batch's total behind the last read (the emit kernel only)
    uint32_t *rec;                 // [cap][kGapRecWords] (slot-owned; the emit kernel only)
    uint64_t cap;
};

// the sink of rescue_gap_body with the records on
struct GapRecCount {
    uint32_t *n_gkept;
    uint8_t *gap_e;
    uint32_t n;
    __device__ __forceinline__ void begin() { n = 0; }
    __device__ __forceinline__ void kept(const RescueArgs &, uint32_t, uint32_t) { n++; }
    __device__ __forceinline__ void done(const RescueArgs &, uint32_t c, uint32_t r, uint32_t best, bool rescued)
    {
        gap_e[c] = rescued ? (uint8_t)best : kGapRecNone;
        if (rescued) n_gkept[r] = n;
    }
};

__global__ __launch_bounds__(kBlock) void rescue_gap_rec_kernel(GapRecArgs a)
{
    GapRecCount sink{a.n_gkept, a.gap_e, 0};
    rescue_gap_body(a.g, sink);
}

// the P and S mismatch words w of the tuple (text base tg of x, type, g), as gap_fit builds them (no 'N' in a kept tuple's window)
__device__ __forceinline__ void gap_rec_words(const RescueArgs &a, const unsigned long long *rd, uint32_t len, uint32_t tg, uint32_t ins, uint32_t g, uint32_t w,
                                              unsigned long long &P, unsigned long long &S)
{
    const uint32_t nw = (len + 31u) >> 5, ls = ins ? len - g : len, nws = (ls + 31u) >> 5;
    const unsigned long long keep = (w + 1u == nws && (ls & 31u)) ? (1ull << (2u * (ls & 31u))) - 1ull : ~0ull;
    const unsigned long long tp = rescue_text64(a.text, tg + 32u * w);
    const unsigned long long sx = ins ? gap_read_from(rd, nw, w, g) ^ tp : rd[w] ^ rescue_text64(a.text, tg + g + 32u * w);
    P = gap_mis(rd[w] ^ tp) & keep;
    S = gap_mis(sx) & keep;
}

// the bits of word w (odd bits, base 32 w + bit / 2) at bases below k / from k on
__device__ __forceinline__ unsigned long long gap_rec_below(uint32_t w, uint32_t k)
{
    return k <= 32u * w ? 0ull : k - 32u * w >= 32u ? ~0ull : (1ull << (2u * (k - 32u * w))) - 1ull;
}

// (path, strand, pos, type, g) of record x before that of record y; w1 = path, w2 = pos, w5 = strand | d << 8 | type << 16 | g << 24
__device__ __forceinline__ bool gap_rec_before(uint32_t x1, uint32_t x2, uint32_t x5, uint32_t y1, uint32_t y2, uint32_t y5)
{
    if (x1 != y1) return x1 < y1;
    if ((x5 & 0xFFu) != (y5 & 0xFFu)) return (x5 & 0xFFu) < (y5 & 0xFFu);
    if (x2 != y2) return x2 < y2;
    return ((x5 >> 8) & 0xFF00u | x5 >> 24) < ((y5 >> 8) & 0xFF00u | y5 >> 24);      // type, then g
}

__global__ __launch_bounds__(kBlock) void gap_rec_emit_kernel(GapRecArgs ar)
{
    const RescueArgs &a = ar.g.r;
    if (a.ctr->flags & kCovSkipFlags) return;
    const uint32_t n = min(*ar.g.n_gcand, a.n_reads), G = ar.g.max_gap;
    const uint64_t off0 = a.seq_off[0];
    for (uint32_t c = blockIdx.x * kBlock + threadIdx.x; c < n; c += gridDim.x * kBlock) {
        uint32_t best = ar.gap_e[c];
        if (best == kGapRecNone) continue;
        const uint32_t r = ar.g.gcand[c], nk = ar.n_gkept[r];
        const uint64_t first = ar.off[r];
        if (first + nk > ar.cap) continue;                     // no room: nothing of the read is written, the total fails the batch at collect
        const uint64_t o = a.seq_off[r];
        const uint32_t len = (uint32_t)(a.seq_off[r + 1] - o);
        const uint64_t w0 = ((o - off0) >> 5) + r;
        uint32_t *seg = ar.rec + first * kGapRecWords;
        uint32_t j = 0;
        gap_sweep(a, G, w0, len, 1u, best, [&](uint32_t p, const uint4 &pi, uint32_t strand, uint32_t x, uint32_t ins, uint32_t g, uint32_t ks, uint32_t d, const unsigned long long *rd) {
            if (j >= nk) return;                               // (the walk is the count's: never taken; a segment is never left)
            unsigned long long mm = 0xFFFFFFFFFFFFull;
            uint32_t cnt = 0;
            const uint32_t nws = ((ins ? len - g : len) + 31u) >> 5;
            for (uint32_t part = 0; d && part < 2u; part++)    // the bases in front of the gap, then those behind it
                for (uint32_t w = 0; w < nws; w++) {
                    unsigned long long P, S;
                    gap_rec_words(a, rd, len, pi.x + x, ins, g, w, P, S);
                    const unsigned long long below = gap_rec_below(w, ks);
                    for (unsigned long long m = part ? S & ~below : P & below; m; m &= m - 1) {
                        const unsigned long long at = 32u * w + (((uint32_t)__ffsll(m) - 1u) >> 1) + (part && ins ? g : 0u);
                        if (cnt < 3u) mm = (mm & ~(0xFFFFull << (16u * cnt))) | (at << (16u * cnt));
                        cnt++;
                    }
                }
            uint32_t *y = seg + (size_t)j * kGapRecWords;
            y[0] = r; y[1] = p; y[2] = pi.z + x;
            y[3] = ks | (uint32_t)(mm & 0xFFFFull) << 16;
            y[4] = (uint32_t)(mm >> 16);
            y[5] = strand | d << 8 | ins << 16 | g << 24;
            j++;
        });
        for (uint32_t i = 1; i < nk; i++) {                    // the thread's own segment into (path, strand, pos, type, g) order
            uint32_t *x = seg + (size_t)i * kGapRecWords;
            const uint32_t c1 = x[1], c2 = x[2], c3 = x[3], c4 = x[4], c5 = x[5];
            uint32_t at = i;
            while (at > 0) {
                const uint32_t *y = seg + (size_t)(at - 1) * kGapRecWords;
                const uint32_t y1 = y[1], y2 = y[2], y3 = y[3], y4 = y[4], y5 = y[5];
                if (!gap_rec_before(c1, c2, c5, y1, y2, y5)) break;
                uint32_t *z = seg + (size_t)at * kGapRecWords;
                z[1] = y1; z[2] = y2; z[3] = y3; z[4] = y4; z[5] = y5;      // (word 0, the read, is the same all over the segment)
                at--;
            }
            if (at != i) {
                uint32_t *z = seg + (size_t)at * kGapRecWords;
                z[1] = c1; z[2] = c2; z[3] = c3; z[4] = c4; z[5] = c5;
            }
        }
    }
}

} // namespace groot
