// kernels_acov.hpp -- the assigned-coverage table on the device (groot_hip_acov_*): the records of a run grouped by
// (e = EC of S(r), p, Pos, last), integers only.  The definition (include/groot_hip.h quotes it in full):
//   A record of read r on path p with an M op of M bases at Pos covers [Pos, last], last = min(Pos + M, path_len(p) - 1), both ends
//   included: the interval `report` piles up.  EVERY record counts (both strands, primary and secondary), as in the report.
//   The assigned-coverage table of a run is the multiset of records grouped by (e = EC of S(r), p, Pos, last):  n(e,p,Pos,last).
// The weights w(e,p), the depth D_p and everything else in floating point is the host's (groot_host_calls_from_table).
//
// e on the device is the serial number of the EC's slot in the run-wide EC table (kernels_ec.hpp): the value the table's fill counter
// had when the slot was claimed, kept beside the key and carried through ec_rehash_kernel.  ec_merge_kernel leaves the serial of
// every slot of the per-batch set table in tab_ser[]; acov_serial_kernel (a thread per read start: shared_insert_kernel's probe
// without the add) finds each read's owner slot and writes the serial into read_ser[], which the batch's pipeline slot owns.  From
// there on a batch needs nothing but what its slot owns, so collect can repeat the count while the slot still holds its records.
//
// The table: open addressing, linear probing, a slot = two key words and a u64 count,
//   k0 = (serial + 1) << 32 | path   (0 = free),   k1 = Pos << 32 | last   (all ones = not yet written),
// claimed by two CAS: k0 from 0, then k1 from all ones.  Whoever loses either CAS looks at what won: a slot is (k0, k1) of the
// winners for good, every thread decides about a slot from that final pair alone, so equal keys of one launch end in one slot and no
// lane ever waits for another.  (A slot between its two CAS is owned by a thread that does the second one next.)
//
// Exactly once, also when the table fills -- two launches of acov_count_kernel per batch:
//   <false> claim: inserts the keys, adds nothing; idempotent.  A key that finds neither itself nor room within kAcovProbe probes
//           sets state[0], and the wavefronts that see the word set stop claiming: a table far too small costs a batch little.
//   <true>  add:   returns at once when state[0] is set; else every key is there, and the add cannot fail.
// The host reads state[0] at collect: when it is set it grows the table fourfold (acov_rehash_kernel), clears the word and runs both
// again, until the claim goes through.  It also doubles a table that is more than half full, so probe runs stay short; a run past
// kAcovProbe in a table that has room only costs one more growth, never a count.
//
// Equal keys are combined before the global atomic: neighbouring traversals of a read share (serial, path) and often the interval,
// and so do neighbouring reads of one EC at one place.  The k-th record of lane l is compared with the k-th record of lane l - 1; a
// run of equal keys adds its length once, from its first lane (one ballot and four shuffles per step, no LDS).
// Every kernel reads the pass's status word first, as the other counters do: a pass collect redoes is not counted.
//
// Over fragments (groot_hip_acov_pairs_enable; the rule is in groot_hip.h): the rows are units (shared_gather_paired_kernel), so
// acov_serial_paired_kernel (a thread per fragment start) gives both mates of a joined fragment the serial of the unit row and leaves
// each of them the span of its mate's records in read_mate[], which the slot owns as it owns read_ser[].  acov_count_kernel<.., true>
// counts a record of such a read on path p only when p is in a record of the mate in the same graph (the record's own bit ANDed with
// the OR of the mate's path sets there, a word at a time); the others are left out and counted in pstats[0] by the add phase, which runs
// to its end exactly once.  It reads the records, their masks, read_ser[] and read_mate[] and no row of the batch's set table: by the
// time collect repeats the count, the next batch has overwritten those rows.  kPaired = false drops every branch.
#pragma once

#include "kernels_shared.hpp"

namespace groot {

constexpr uint32_t kAcovNone = 0xFFFFFFFFu;                 // read_ser: the read is on the slow path (the host counts its records)
constexpr unsigned long long kAcovUnset = ~0ull;            // k1 of a slot whose second word is not written
constexpr uint32_t kAcovProbe = 128;                        // slots a batch's claim looks at before it reports the table full

struct AcovTable {
    unsigned long long *k0, *k1, *cnt;                      // [cap] each
    uint32_t cap_mask;                                      // cap - 1 (cap a power of two)
};

struct AcovArgs {
    const groot_trav *trav;        // the batch's records in (read, ord) order
    const uint64_t *mask;          // their path sets, pw words each
    const uint64_t *seq_off;       // read offsets of the batch
    const DeviceCounters *ctr;     // n_trav + flags of the pass
    const uint32_t *node_np_off;   // [n_nodes + 1] into np
    const uint2 *np;               // (local path id, Position) of every path through a node
    const uint32_t *graph_path_off;
    const uint32_t *path_len;      // [n_paths]
    const uint32_t *read_ser;      // [n_reads] EC serial of every read with records (acov_serial_kernel)
    uint32_t *state;               // [0] of this batch: 1 = the claim ran out of room, 2 = the add missed a key (never met)
    uint32_t *fill;                // claimed slots of the table
    uint32_t cap, pw, first_read_id, n_paths;
    const uint2 *read_mate;        // kPaired: [n_reads] (first, end) of the mate's records for a read of a joined fragment, (0, 0) for any other
    unsigned long long *pstats;    // kPaired: [0] records left out, [1] reads of joined fragments (acov_serial_paired_kernel)
};

constexpr uint32_t kAcovPairStats = 2;

__device__ __forceinline__ uint32_t acov_hash(unsigned long long k0, unsigned long long k1)
{
    uint64_t h = k0 * 0x9E3779B97F4A7C15ull ^ (k1 + 0x7F4A7C159E3779B9ull) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29; h *= 0x94D049BB133111EBull; h ^= h >> 32;
    return (uint32_t)h;
}

// the slot of key (k0, k1), claimed if the key is new; kAcovNone when `limit` probes (at most the whole table) found neither the key
// nor room
__device__ __forceinline__ uint32_t acov_claim(const AcovTable &t, unsigned long long k0, unsigned long long k1, uint32_t *fill, uint32_t limit)
{
    uint32_t s = acov_hash(k0, k1) & t.cap_mask;
    for (uint32_t i = 0; i <= t.cap_mask && i < limit; i++, s = (s + 1) & t.cap_mask) {
        unsigned long long c0 = __hip_atomic_load(t.k0 + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c0 == 0) {
            c0 = atomicCAS(t.k0 + s, 0ull, k0);
            if (c0 == 0) { if (fill) atomicAdd(fill, 1u); c0 = k0; }
        }
        if (c0 != k0) continue;
        unsigned long long c1 = __hip_atomic_load(t.k1 + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c1 == kAcovUnset) {
            c1 = atomicCAS(t.k1 + s, kAcovUnset, k1);
            if (c1 == kAcovUnset) c1 = k1;
        }
        if (c1 == k1) return s;
    }
    return kAcovNone;
}

// the slot of a key the claim phase has put there
__device__ __forceinline__ uint32_t acov_find(const AcovTable &t, unsigned long long k0, unsigned long long k1)
{
    uint32_t s = acov_hash(k0, k1) & t.cap_mask;
    for (uint32_t i = 0; i <= t.cap_mask; i++, s = (s + 1) & t.cap_mask)
        if (t.k0[s] == k0 && t.k1[s] == k1) return s;
    return kAcovNone;
}

// the serial of the EC of row r of the batch's set table (tab_ser: ec_merge_kernel); kAcovNone for a slow-path unit
__device__ __forceinline__ uint32_t acov_row_serial(const SharedArgs &a, const uint32_t *tab_ser, uint32_t r)
{
    if (a.set_graph[(size_t)r * kSharedSegs] == kSharedEmpty) return kAcovNone;
    uint32_t slot = (uint32_t)shared_hash(a, r) & a.tab_mask;
    for (uint32_t i = 0; i <= a.tab_mask; i++, slot = (slot + 1) & a.tab_mask) {
        const uint32_t cur = a.tab_rep[slot];
        if (cur == kSharedEmpty) break;        // (insert put every row in: never met)
        if (cur == r || same_set(a, cur, r)) return tab_ser[slot];
    }
    return kAcovNone;
}

// one thread per read start: the serial of the read's EC from the owner slot of its set row
__global__ __launch_bounds__(kBlock) void acov_serial_kernel(SharedArgs a, const uint32_t *tab_ser, uint32_t *read_ser)
{
    if (!shared_live(a)) return;
    const uint32_t n = min(a.ctr->n_trav, a.cap);
    for (uint32_t t0 = blockIdx.x * kBlock + threadIdx.x; t0 < n; t0 += gridDim.x * kBlock) {
        if (!read_start(a, t0)) continue;
        const uint32_t r = a.trav[t0].read_id - a.first_read_id;
        read_ser[r] = acov_row_serial(a, tab_ser, r);
    }
}

// the mates' sets intersect: some graph both have records in, with a path in both ORs (what shared_gather_paired_kernel calls joined)
__device__ __forceinline__ bool frag_joined(const SharedArgs &a, uint32_t t0, uint32_t tm, uint32_t t1)
{
    for (uint32_t sa = t0, sb = tm; sa < tm && sb < t1;) {
        const uint32_t ga = a.trav[sa].graph_id, gb = a.trav[sb].graph_id;
        if (ga < gb) { sa = seg_end(a, sa, tm); continue; }
        if (gb < ga) { sb = seg_end(a, sb, t1); continue; }
        const uint32_t ea = seg_end(a, sa, tm), eb = seg_end(a, sb, t1);
        for (uint32_t w = 0; w < a.pw; w++)
            if (seg_or(a, sa, ea, w) & seg_or(a, sb, eb, w)) return true;
        sa = ea; sb = eb;
    }
    return false;
}

// one thread per fragment start.  Joined: both mates get the serial of the unit row (the even mate's) and the span of the other's
// records; a joined unit on the slow path leaves kAcovNone to both, and the host counts the fragment.  Split or single: every mate with
// records as acov_serial_kernel has it, its row being its own.
__global__ __launch_bounds__(kBlock) void acov_serial_paired_kernel(SharedArgs a, const uint32_t *tab_ser, uint32_t *read_ser, uint2 *read_mate,
                                                                    unsigned long long *pstats)
{
    if (!shared_live(a)) return;
    const uint32_t n = min(a.ctr->n_trav, a.cap);
    uint32_t joined = 0;
    for (uint32_t t0 = blockIdx.x * kBlock + threadIdx.x; t0 < n; t0 += gridDim.x * kBlock) {
        if (!frag_start(a, t0)) continue;
        uint32_t tm, t1;
        frag_span(a, t0, n, tm, t1);
        const uint32_t r0 = (a.trav[t0].read_id - a.first_read_id) & ~1u;
        if (tm > t0 && t1 > tm && frag_joined(a, t0, tm, t1)) {
            read_ser[r0] = read_ser[r0 + 1] = acov_row_serial(a, tab_ser, r0);
            read_mate[r0] = make_uint2(tm, t1);
            read_mate[r0 + 1] = make_uint2(t0, tm);
            joined += 2;
            continue;
        }
        if (tm > t0) { read_ser[r0] = acov_row_serial(a, tab_ser, r0); read_mate[r0] = make_uint2(0, 0); }
        if (t1 > tm) { read_ser[r0 + 1] = acov_row_serial(a, tab_ser, r0 + 1); read_mate[r0 + 1] = make_uint2(0, 0); }
    }
    for (int o = 32; o > 0; o >>= 1) joined += __shfl_down(joined, o, 64);
    if ((threadIdx.x & 63) == 0 && joined) atomicAdd(pstats + 1, (unsigned long long)joined);
}

// one lane per traversal, a wavefront over 64 neighbouring ones; step k handles the k-th record (path of the path set, in the
// order of the first node's list) of every lane that has one
template <bool kAdd, bool kPaired>
__global__ __launch_bounds__(kBlock) void acov_count_kernel(AcovArgs a, AcovTable t)
{
    if (a.ctr->flags & kCovSkipFlags) return;
    if (kAdd && a.state[0]) return;
    const uint32_t n = min(a.ctr->n_trav, a.cap), lane = threadIdx.x & 63;
    uint32_t left = 0;                             // kPaired: records this lane left out
    for (uint32_t tb = blockIdx.x * kBlock + (threadIdx.x & ~63u); tb < n; tb += gridDim.x * kBlock) {
        if (!kAdd && __hip_atomic_load(a.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;     // the table is full: collect grows it and claims again
        const uint32_t tv = tb + lane;
        groot_trav tr{};
        uint32_t ser = kAcovNone, j = 0, j1 = 0, g0 = 0;
        uint32_t mf = 0, me = 0, fword = ~0u;      // kPaired: the mate's records [mf, me) of a joined read; the word of their OR in `fw`
        uint64_t m = 0, fw = 0;
        if (tv < n) {
            tr = a.trav[tv];
            const uint32_t r = tr.read_id - a.first_read_id;
            ser = a.read_ser[r];
            if (ser != kAcovNone) {
                m = (a.seq_off[r + 1] - a.seq_off[r]) - ((tr.flags & GROOT_TRAV_START_CLIP) ? 1u : 0u) - ((tr.flags & GROOT_TRAV_END_CLIP) ? 1u : 0u);
                g0 = a.graph_path_off[tr.graph_id];
                j = a.node_np_off[tr.node];
                j1 = a.node_np_off[tr.node + 1];
                if (kPaired) { const uint2 mt = a.read_mate[r]; mf = mt.x; me = mt.y; }
            }
        }
        const uint64_t *mk = a.mask + (size_t)tv * a.pw;
        for (;;) {
            bool have = false;
            unsigned long long k0 = 0, k1 = 0;
            while (j < j1) {
                const uint2 e = a.np[j++];
                if (!((mk[e.x >> 6] >> (e.x & 63)) & 1ull)) continue;
                const uint32_t gp = g0 + e.x;
                if (gp >= a.n_paths) continue;
                const uint64_t len = a.path_len[gp], pos = (uint64_t)e.y + tr.offset;
                if (len == 0 || pos > 0xFFFFFFFEull) continue;      // (no such path / Pos: never met; nothing a u32 pair could hold)
                if (kPaired && me > mf) {          // a joined read: the path must be in the mate's set too
                    if (fword != (e.x >> 6)) {
                        fword = e.x >> 6;
                        fw = 0;
                        for (uint32_t u = mf; u < me; u++)
                            if (a.trav[u].graph_id == tr.graph_id) fw |= a.mask[(size_t)u * a.pw + fword];
                    }
                    if (!((fw >> (e.x & 63)) & 1ull)) { left += kAdd; continue; }
                }
                const uint64_t last = min(pos + m, len - 1);
                k0 = ((unsigned long long)(ser + 1u) << 32) | gp;
                k1 = ((unsigned long long)pos << 32) | last;
                have = true;
                break;
            }
            if (!__ballot(have)) break;
            const unsigned long long p0 = __shfl_up(k0, 1, 64), p1 = __shfl_up(k1, 1, 64);
            const int ph = __shfl_up((int)have, 1, 64);
            const bool head = have && !(lane > 0 && ph && p0 == k0 && p1 == k1);
            const unsigned long long stops = __ballot(head || !have);
            if (head) {
                if (!kAdd) {
                    if (acov_claim(t, k0, k1, a.fill, kAcovProbe) == kAcovNone) a.state[0] = 1;
                } else {
                    const unsigned long long rest = lane == 63 ? 0ull : stops >> (lane + 1);
                    const unsigned long long run = rest ? (unsigned long long)__builtin_ctzll(rest) + 1ull : 64ull - lane;
                    const uint32_t s = acov_find(t, k0, k1);
                    if (s == kAcovNone) a.state[0] = 2;
                    else atomicAdd(t.cnt + s, run);
                }
            }
        }
    }
    if (kAdd && kPaired) {
        for (int o = 32; o > 0; o >>= 1) left += __shfl_down(left, o, 64);
        if (lane == 0 && left) atomicAdd(a.pstats, (unsigned long long)left);
    }
}

// every key of `from` with its count into the (empty, at least as large) table `to`: keys are distinct
__global__ __launch_bounds__(kBlock) void acov_rehash_kernel(AcovTable from, uint32_t from_cap, AcovTable to, uint32_t *state)
{
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < from_cap; s += gridDim.x * kBlock) {
        const unsigned long long k0 = from.k0[s];
        if (!k0) continue;
        const uint32_t d = acov_claim(to, k0, from.k1[s], nullptr, ~0u);
        if (d == kAcovNone) state[0] = 2;
        else to.cnt[d] = from.cnt[s];
    }
}

// the slots with a count, compacted (in no particular order) into out_key (k0, k1 per tuple) / out_cnt; *n_out counts them
__global__ __launch_bounds__(kBlock) void acov_export_kernel(AcovTable t, uint32_t cap, unsigned long long *out_key, unsigned long long *out_cnt, uint32_t *n_out,
                                                             uint32_t cap_out)
{
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < cap; s += gridDim.x * kBlock) {
        if (!t.k0[s] || !t.cnt[s]) continue;
        const uint32_t i = atomicAdd(n_out, 1u);
        if (i >= cap_out) continue;
        out_key[2 * (size_t)i] = t.k0[s];
        out_key[2 * (size_t)i + 1] = t.k1[s];
        out_cnt[i] = t.cnt[s];
    }
}

} // namespace groot
