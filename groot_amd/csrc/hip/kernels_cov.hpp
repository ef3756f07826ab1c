// kernels_cov.hpp -- report coverage on the device (groot_hip_coverage_*): what `groot report` reads back from the BAM
// (src/reporting/reporting.go:100-127), accumulated batch by batch behind the order stage.
//
// Every record of a traversal (one per path p of its path set, alignment.go:113-156) sits at Pos = Position[p] of the first node +
// offset with an M op of M = read length - clips bases and covers [Pos, min(Pos + M, path_len - 1)] of p, both ends included.  Per
// path the ctx keeps path_len + 1 slots of two u64 counters: starts[Pos] += 1 and ends[last + 1] += 1.  At export, records[p] = the
// sum of p's starts and depth[i] = the prefix sum of starts - ends.  A record whose Pos lies past the path (never met) only counts
// in starts[path_len], outside the pileup.  u64 counters: nothing wraps.
#pragma once

#include "kernels_common.hpp"

namespace groot {

struct CovArgs {
    const groot_trav *trav;        // the batch's records in (read, ord) order
    const uint64_t *mask;          // their path sets, pw words each
    const uint64_t *seq_off;       // read offsets of the batch: read length = seq_off[r + 1] - seq_off[r]
    const DeviceCounters *ctr;     // n_trav + flags of the pass
    const uint32_t *node_np_off;   // [n_nodes + 1] into np
    const uint2 *np;               // (local path id, Position) of every path through a node, PathIDs order
    const uint32_t *graph_path_off;
    const uint32_t *path_len;      // [n_paths]
    const uint64_t *slot_base;     // [n_paths] first slot of global path p: sum_{q<p} (path_len[q] + 1)
    unsigned long long *starts, *ends;
    uint32_t cap, pw, first_read_id;
};

// Flags after which a pass's records are not counted: the batch is redone at collect (finish_counters; the redo pass counts), or it
// fails (a read longer than max_read_len, a read with more than 65535 traversals) and a host runs it again elsewhere.
constexpr uint32_t kCovSkipFlags = kFlagSeedOverflow | kFlagTravOverflow | kFlagOvfOverflow | kFlagQOverflow | kFlagLongRead | kFlagOrdOverflow;

__global__ __launch_bounds__(kBlock) void cov_count_kernel(CovArgs a)
{
    if (a.ctr->flags & kCovSkipFlags) return;
    const uint32_t n = min(a.ctr->n_trav, a.cap);
    for (uint32_t t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
        const groot_trav tr = a.trav[t];
        const uint32_t r = tr.read_id - a.first_read_id;
        const uint64_t m = (a.seq_off[r + 1] - a.seq_off[r]) - ((tr.flags & GROOT_TRAV_START_CLIP) ? 1u : 0u) - ((tr.flags & GROOT_TRAV_END_CLIP) ? 1u : 0u);
        const uint32_t g0 = a.graph_path_off[tr.graph_id];
        const uint64_t *mk = a.mask + (size_t)t * a.pw;
        const uint32_t j1 = a.node_np_off[tr.node + 1];
        for (uint32_t j = a.node_np_off[tr.node]; j < j1; j++) {
            const uint2 e = a.np[j];
            if (!((mk[e.x >> 6] >> (e.x & 63)) & 1ull)) continue;
            const uint32_t gp = g0 + e.x;
            const uint64_t len = a.path_len[gp], base = a.slot_base[gp];
            const uint64_t pos = (uint64_t)e.y + tr.offset;
            if (pos >= len) { atomicAdd(a.starts + base + len, 1ull); continue; }
            const uint64_t last = min(pos + m, len - 1);
            atomicAdd(a.starts + base + pos, 1ull);
            atomicAdd(a.ends + base + last + 1, 1ull);
        }
    }
}

} // namespace groot
