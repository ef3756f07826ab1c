#pragma once

#include "kernels_common.hpp"

namespace groot {

// ---------------------------------------------------------------------------------------------
// K3, first pass against path text (align_path_kernel = first_pass_body<PW, NCH, true>, kernels_lean.hpp).
// An error-free read spells a stretch of one path's linear text.  Inside a path the DFS (dfsRecursive, alignment.go:196-254) is
// deterministic at every node boundary where no two out-neighbours of the node share a first base, none starts with an 'N' and the
// path's next node is one of them: it can only go on into the neighbour whose first base is the read's next base.  So a walk is a chain
// of SEGMENTS, each one comparison of the read against one path's text (built at open: index_tables.hpp, build_path_tables), from a start
// (node, offset) up to the first of: the end of the read, a boundary that is not deterministic (flagged in the text), a mismatch.
//   * a mismatch inside a node ends the branch, as in the DFS;
//   * a mismatch on the first base of the path's next node (an unflagged boundary), a flagged boundary and the end of the path's text
//     end the segment at the end of node `prev`: there the DFS's neighbour loop runs as in the node walk -- the neighbour with the read's
//     next base (the path's next node: the segment goes on in the same text; another one: its own lowest path, "the jump"), the second of
//     two pending on the read's stack, a sink reporting the overhang (:229-236);
//   * the graph's 'N' is masked out of the comparison (the DFS counts it as a match, :212-215);
//   * the path set (processTraversal, :263-317, keeps the paths present in every node of the walk) is the AND over the segments of a
//     range-AND over the path's node index: two entries of a per-path sparse table (AND is idempotent, so overlapping halves do).
// Text: 2 bits per base in two parallel arrays, the code (A=0 C=1 T=2 G=3, 'N' = 0) and a tag: bit 0 = a node starts here, bit 1 = with
// bit 0: the boundary into this node is flagged, without: the base is an 'N'.
// ---------------------------------------------------------------------------------------------

#ifndef GROOT_PATH_WAVES
#define GROOT_PATH_WAVES 4
#endif
constexpr int kPathWaves = GROOT_PATH_WAVES;
constexpr uint32_t kPathHold = 4;          // traversal records with ord >= 1 a read may hold until it finishes (more: left to align_kernel)

struct PathStop {
    uint32_t n;                            // bases compared
    uint32_t e;                            // first event (mismatch that is not an 'N', flagged boundary) at or after base 0, kEmpty: none before n
    uint32_t ns;                           // node starts in (0, min(e, n))
    bool at_start, flagged;                // the event sits on a node's first base / that boundary is flagged
};

__device__ __forceinline__ uint64_t path_funnel(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t sh)
{
    return (uint64_t)__funnelshift_r(x0, x1, sh) | ((uint64_t)__funnelshift_r(x1, x2, sh) << 32);
}
// the read's view from `dist` (view(d) = its 32 bases from dist + d) against n <= 32 * NCH bases of text from global offset t
template <int NCH, typename View>
__device__ __forceinline__ PathStop path_segment(const uint32_t *text, const uint32_t *tag, uint32_t t, uint32_t n, View view)
{
    constexpr uint64_t k55 = 0x5555555555555555ull;
    const uint32_t bit = 2u * t, sh = bit & 31u;
    const uint32_t *cp = text + (bit >> 5), *tp = tag + (bit >> 5);
    uint32_t x[2 * NCH + 1], y[2 * NCH + 1];
#pragma unroll
    for (int c = 0; c < 2 * NCH + 1; c++) { x[c] = cp[c]; y[c] = tp[c]; }
    PathStop ps{n, kEmpty, 0u, false, false};
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        if (ps.e == kEmpty && n > 32u * c) {
            const uint64_t lim = (n >= 32u * (c + 1) ? ~0ull : ((1ull << (2 * (n - 32u * c))) - 1ull)) & (c == 0 ? ~3ull : ~0ull);
            const uint64_t g = path_funnel(x[2 * c], x[2 * c + 1], x[2 * c + 2], sh), tg = path_funnel(y[2 * c], y[2 * c + 1], y[2 * c + 2], sh);
            const uint64_t d = g ^ view(32u * c), lo = tg & k55, hi = (tg >> 1) & k55;
            // mismatches (base 0 included: it cannot be one) that are not an 'N'; flagged boundaries after base 0
            const uint64_t mis = (d | (d >> 1)) & k55 & ~(hi & ~lo) & (n >= 32u * (c + 1) ? ~0ull : ((1ull << (2 * (n - 32u * c))) - 1ull));
            const uint64_t ev = mis | (hi & lo & lim);
            const uint64_t starts = lo & lim;
            if (ev) {
                const uint32_t j = (uint32_t)__builtin_ctzll(ev) >> 1;
                ps.e = 32u * c + j;
                ps.at_start = (lo >> (2 * j)) & 1u;
                ps.flagged = (hi >> (2 * j)) & ps.at_start;
                ps.ns += (uint32_t)__popcll(starts & ((1ull << (2 * j)) - 1ull));
            } else ps.ns += (uint32_t)__popcll(starts);
        }
    }
    return ps;
}
// ptab: per path, levels k = 0.. of [n] entries of PW words: entry (k, i) = AND of the path sets of nodes [i, i + 2^k)
template <int PW>
__device__ __forceinline__ void path_range_and(const uint64_t *ptab, uint32_t tbase, uint32_t n, uint32_t lo, uint32_t hi, uint64_t &r0, uint64_t &r1, uint64_t &r2)
{
    const uint32_t lv = 31u - __builtin_clz(hi - lo + 1u);
    const uint64_t *pa = ptab + (size_t)PW * (tbase + (size_t)lv * n + lo), *pb = ptab + (size_t)PW * (tbase + (size_t)lv * n + hi + 1u - (1u << lv));
    r0 = pa[0] & pb[0]; r1 = pa[1] & pb[1]; r2 = pa[2] & pb[2];
}

} // namespace groot
