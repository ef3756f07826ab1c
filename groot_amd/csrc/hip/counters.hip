// counters.hip -- the counters that run behind every batch's order stage, and their C ABI (include/groot_hip.h): report coverage
// (kernels_cov.hpp), shared reads (kernels_shared.hpp), equivalence classes (kernels_ec.hpp), assigned coverage (kernels_acov.hpp),
// paired-end units, the bootstrap replicates of the abundance EM (kernels_boot.hpp) and of the calls (kernels_csup.hpp), the rarefaction
// draws (kernels_rare.hpp).  One of the seven translation units of libgroot_hip.so (launch.hpp); the pipeline calls the hooks of
// counters.hpp, the rescue family (rescue.hip) is reached through those of rescue.hpp, everything else here is internal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <tuple>
#include <vector>

#include "counters.hpp"
#include "ctx.hpp"
#include "kernels_acov.hpp"
#include "kernels_assign.hpp"
#include "kernels_boot.hpp"
#include "kernels_cov.hpp"
#include "kernels_csup.hpp"
#include "kernels_ec.hpp"
#include "kernels_rare.hpp"
#include "kernels_shared.hpp"
#include "rescue.hpp"

using namespace groot;

// ---- the position tables' one device copy (Counters::d_*) ----
static bool pos_wanted(const Counters &k) { return k.cov_on || k.sh_on || k.ec_on || k.acov_on; }

static void pos_release(Counters &k)
{
    for (auto *b : {&k.d_np_off, &k.d_gpo, &k.d_len}) b->release();
    k.d_np.release();
}

// for a counter that comes on: there already when another one is on
static hipError_t pos_acquire(Counters &k)
{
    if (pos_wanted(k)) return hipSuccess;
    hipError_t e = upload(k.d_np_off, k.h_np_off.data(), k.h_np_off.size());
    if (e == hipSuccess) e = upload(k.d_gpo, k.h_gpo.data(), k.h_gpo.size());
    if (e == hipSuccess) e = upload(k.d_len, k.h_len.data(), k.h_len.size());
    if (e == hipSuccess) e = upload(k.d_np, k.h_np.data(), k.h_np.size());
    if (e != hipSuccess) pos_release(k);
    return e;
}

// ---- equivalence classes (kernels_ec.hpp) ----
hipError_t EcBufs::alloc(uint32_t slots, uint32_t pw, hipStream_t st)
{
    cap = slots;
    hipError_t e = claim.alloc(cap);
    if (e == hipSuccess) e = graph.alloc((size_t)cap * kSharedSegs);
    if (e == hipSuccess) e = mask.alloc((size_t)cap * kSharedSegs * pw);
    if (e == hipSuccess) e = cnt.alloc(cap);
    if (e == hipSuccess) e = serial.alloc(cap);
    if (e == hipSuccess) e = hipMemsetAsync(claim.p, 0, (size_t)cap * sizeof(uint32_t), st);
    return e;
}
EcTable EcBufs::table() const { return EcTable{claim.p, graph.p, mask.p, cnt.p, serial.p, cap - 1}; }
void EcBufs::swap(EcBufs &o)
{
    std::swap(cap, o.cap);
    claim.swap(o.claim); graph.swap(o.graph); mask.swap(o.mask); cnt.swap(o.cnt); serial.swap(o.serial);
}
void EcBufs::release()
{
    for (auto *b : {&claim, &graph, &serial}) b->release();
    mask.release(); cnt.release();
    cap = 0;
}

// Before a batch's merge: each batch adds at most n_reads keys, so the table must keep >= 2 x (the fill read back at the newest
// collect + n_reads of every batch launched and not collected, this one included) slots -- else it doubles, rehashed in tail-stream
// order.  (Growth is rare -- a handful of times per run -- so the old buffers are freed behind a wait for the tail stream.)
// With rescued reads in the ECs (kernels_rescue_ec.hpp) a batch has a second merge, and the bound holds for both together: a rescued
// read has no record, so the reads with a record and the rescued ones are at most n_reads, and so are their distinct sets.  The
// gap-placed reads (kernels_gap_ec.hpp) go through that second merge and change nothing: a gap candidate is a candidate that ended
// unplaced, so a read is exact, rescued or gap-rescued and never two of them: exact + rescued + gap-rescued <= n_reads.
static int ec_reserve(groot_ctx *c, Slot *s)
{
    Counters &k = c->ct;
    uint64_t pending = s->n_reads;
    for (Slot *x : c->inflight)
        if (x != s && x->state == Slot::IN_FLIGHT) pending += x->n_reads;
    const uint64_t need = 2 * (k.ec_fill_known + pending);
    if (k.ec.cap >= need) return GROOT_OK;
    uint64_t cap = k.ec.cap;
    while (cap < need) cap *= 2;
    if (cap > (1ull << 31)) return fail(c, GROOT_E_NOSPACE, "equivalence classes: the table would need %llu slots", (unsigned long long)cap);
    const uint32_t pw = std::max<uint32_t>(c->pw_view, 1u);
    EcBufs grown;
    hipError_t e = grown.alloc((uint32_t)cap, pw, c->tstream);
    if (e != hipSuccess) return fail(c, GROOT_E_DEVICE, "equivalence classes: growing the table to %llu slots: %s", (unsigned long long)cap, hipGetErrorString(e));
    hipLaunchKernelGGL(ec_rehash_kernel, dim3(grid_for(k.ec.cap)), dim3(kBlock), 0, c->tstream, k.ec.table(), k.ec.cap, grown.table(), pw, ++k.ec_epoch);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->tstream));
    k.ec.swap(grown);
    k.ec_grows++;
    return GROOT_OK;
}

// S(r) of the records trav[0..n) (one read): global path IDs, ascending, each once
static void ec_set_of(const groot_ctx *c, const groot_trav *trav, const uint64_t *mask, size_t n, std::vector<uint32_t> &ids)
{
    const uint32_t pw = c->pw_view, n_paths = (uint32_t)c->ct.h_len.size();
    ids.clear();
    for (size_t t = 0; t < n; t++)
        for (uint32_t w = 0; w < pw; w++)
            for (uint64_t m = mask[t * pw + w]; m; m &= m - 1) {
                const uint64_t id = (uint64_t)c->ct.h_gpo[trav[t].graph_id] + w * 64 + (uint32_t)__builtin_ctzll(m);
                if (id < n_paths) ids.push_back((uint32_t)id);
            }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
}

// ---- assigned coverage (kernels_acov.hpp) ----
hipError_t AcovBufs::alloc(uint32_t slots, hipStream_t st)
{
    cap = slots;
    hipError_t e = k0.alloc(cap);
    if (e == hipSuccess) e = k1.alloc(cap);
    if (e == hipSuccess) e = cnt.alloc(cap);
    if (e == hipSuccess) e = hipMemsetAsync(k0.p, 0, (size_t)cap * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(k1.p, 0xFF, (size_t)cap * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(cnt.p, 0, (size_t)cap * sizeof(unsigned long long), st);
    return e;
}
AcovTable AcovBufs::table() const { return AcovTable{k0.p, k1.p, cnt.p, cap - 1}; }
void AcovBufs::swap(AcovBufs &o)
{
    std::swap(cap, o.cap);
    k0.swap(o.k0); k1.swap(o.k1); cnt.swap(o.cnt);
}
void AcovBufs::release()
{
    for (auto *b : {&k0, &k1, &cnt}) b->release();
    cap = 0;
}

// the claim and the add phase of slot s's batch on the tail stream; both read nothing but what the slot owns and the ctx's tables
static int acov_count(groot_ctx *c, Slot *s)
{
    Counters &k = c->ct;
    AcovArgs a{};
    a.trav = s->d_trav.p; a.mask = s->d_mask.p; a.seq_off = s->off(); a.ctr = s->d_ctr.p;
    a.node_np_off = k.d_np_off.p; a.np = k.d_np.p; a.graph_path_off = k.d_gpo.p; a.path_len = k.d_len.p;
    a.read_ser = s->ct.d_acov_ser.p; a.state = s->ct.d_acov_state.p; a.fill = k.acov_fill.p;
    a.cap = s->trav_cap; a.pw = c->pw_view; a.first_read_id = s->first_read_id; a.n_paths = (uint32_t)k.h_len.size();
    a.read_mate = s->ct.d_acov_mate.p; a.pstats = k.acp_stats.p;
    const dim3 g(grid_for(s->trav_cap));
    if (k.acp_on) {
        hipLaunchKernelGGL((acov_count_kernel<false, true>), g, dim3(kBlock), 0, c->tstream, a, k.acov.table());
        hipLaunchKernelGGL((acov_count_kernel<true, true>), g, dim3(kBlock), 0, c->tstream, a, k.acov.table());
    } else {
        hipLaunchKernelGGL((acov_count_kernel<false, false>), g, dim3(kBlock), 0, c->tstream, a, k.acov.table());
        hipLaunchKernelGGL((acov_count_kernel<true, false>), g, dim3(kBlock), 0, c->tstream, a, k.acov.table());
    }
    k.acov_launches += 2;
    HIP_TRY(c, hipGetLastError());
    return GROOT_OK;
}

// behind the batch's ec_merge_kernel and before shared_expand_kernel clears the per-batch table (tail stream)
static int acov_launch(groot_ctx *c, Slot *s, const SharedArgs &sa)
{
    HIP_TRY(c, s->ct.d_acov_ser.reserve(std::max<uint32_t>(c->prm.max_batch_reads, 1u)));
    HIP_TRY(c, s->ct.d_acov_state.reserve(1));
    HIP_TRY(c, hipMemsetAsync(s->ct.d_acov_state.p, 0, sizeof(uint32_t), c->tstream));
    if (c->ct.acp_on) {
        HIP_TRY(c, s->ct.d_acov_mate.reserve(std::max<uint32_t>(c->prm.max_batch_reads, 1u)));
        hipLaunchKernelGGL(acov_serial_paired_kernel, dim3(grid_for(s->trav_cap)), dim3(kBlock), 0, c->tstream, sa, c->ct.acov_tab_ser.p, s->ct.d_acov_ser.p,
                           s->ct.d_acov_mate.p, c->ct.acp_stats.p);
    } else {
        hipLaunchKernelGGL(acov_serial_kernel, dim3(grid_for(s->trav_cap)), dim3(kBlock), 0, c->tstream, sa, c->ct.acov_tab_ser.p, s->ct.d_acov_ser.p);
    }
    c->ct.acov_launches++;
    if (int rc = rescue_acov_pairs_launch(c, s, sa)) return rc;     // (rescued mates in assigned coverage over fragments: while the unit rows are live)
    return acov_count(c, s);
}

// `factor` times the slots, every key and count moved over; everything launched on the tail stream has ended when this returns
int groot::acov_grow(groot_ctx *c, uint32_t factor)
{
    Counters &k = c->ct;
    HIP_TRY(c, hipStreamSynchronize(c->tstream));
    const uint64_t cap = (uint64_t)factor * k.acov.cap;
    if (cap > (1ull << 31)) return fail(c, GROOT_E_NOSPACE, "assigned coverage: the table would need %llu slots", (unsigned long long)cap);
    AcovBufs grown;
    hipError_t e = grown.alloc((uint32_t)cap, c->tstream);
    if (e != hipSuccess) return fail(c, GROOT_E_DEVICE, "assigned coverage: growing the table to %llu slots: %s", (unsigned long long)cap, hipGetErrorString(e));
    hipLaunchKernelGGL(acov_rehash_kernel, dim3(grid_for(k.acov.cap)), dim3(kBlock), 0, c->tstream, k.acov.table(), k.acov.cap, grown.table(), k.acov_err.p);
    k.acov_launches++;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->tstream));
    uint32_t err = 0;
    HIP_TRY(c, hipMemcpy(&err, k.acov_err.p, sizeof err, hipMemcpyDeviceToHost));
    if (err) return fail(c, GROOT_E_DEVICE, "assigned coverage: a key did not fit the grown table");
    k.acov.swap(grown);
    k.acov_grows++;
    return GROOT_OK;
}

// At collect, while slot s still owns its records and its reads' serials: a batch whose claim phase ran out of room added nothing;
// the table grows fourfold and both phases run again until the claim goes through.  A table more than half full is doubled.
// refetch: the copies enqueue made are stale (the batch was redone).
static int acov_collect(groot_ctx *c, Slot *s, bool refetch)
{
    auto fetch = [&]() -> int {
        HIP_TRY(c, hipMemcpy(&s->ct.h_status.p->acov_state, s->ct.d_acov_state.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(&s->ct.h_status.p->acov_fill, c->ct.acov_fill.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
        return GROOT_OK;
    };
    if (refetch)
        if (int rc = fetch()) return rc;
    for (;;) {
        const uint32_t st = s->ct.h_status.p->acov_state, fill = s->ct.h_status.p->acov_fill;
        if (st > 1) return fail(c, GROOT_E_DEVICE, "assigned coverage: a claimed key was not found in the table");
        if (!st && 2ull * fill <= c->ct.acov.cap) return GROOT_OK;
        if (int rc = acov_grow(c, st ? 4u : 2u)) return rc;
        if (!st) continue;
        HIP_TRY(c, hipMemsetAsync(s->ct.d_acov_state.p, 0, sizeof(uint32_t), c->tstream));
        if (int rc = acov_count(c, s)) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->tstream));
        c->ct.acov_redone++;
        if (int rc = fetch()) return rc;
    }
}

// the records of one slow-path unit (trav[0..n), their path sets, the unit's set = ids) into acov_host; offs = the batch's read offsets
// (a record's M op is its own read's length less its clips).  in_ids: the unit is a joined fragment, and only the records on a path of
// ids count (the others are left out); else every path of the records is in ids, and nothing is looked up.
static void acov_fold_host(groot_ctx *c, const Slot *s, const groot_trav *trav, const uint64_t *mask, size_t n, const std::vector<uint32_t> &ids,
                           const std::vector<uint64_t> &offs, bool in_ids)
{
    const uint32_t pw = c->pw_view, n_paths = (uint32_t)c->ct.h_len.size();
    auto &tab = c->ct.acov_host[ids];
    for (size_t t = 0; t < n; t++) {
        const groot_trav &tr = trav[t];
        const uint32_t r = tr.read_id - s->first_read_id;
        const uint64_t m = (offs[r + 1] - offs[r]) - ((tr.flags & GROOT_TRAV_START_CLIP) ? 1u : 0u) - ((tr.flags & GROOT_TRAV_END_CLIP) ? 1u : 0u);
        const uint32_t g0 = c->ct.h_gpo[tr.graph_id];
        for (uint32_t j = c->ct.h_np_off[tr.node]; j < c->ct.h_np_off[tr.node + 1]; j++) {
            const uint2 e = c->ct.h_np[j];
            if (!((mask[t * pw + (e.x >> 6)] >> (e.x & 63)) & 1ull)) continue;
            const uint32_t gp = g0 + e.x;
            if (gp >= n_paths) continue;
            const uint64_t len = c->ct.h_len[gp], pos = (uint64_t)e.y + tr.offset;
            if (len == 0 || pos > 0xFFFFFFFEull) continue;
            if (in_ids && !std::binary_search(ids.begin(), ids.end(), gp)) { c->ct.acp_host_left++; continue; }
            const uint64_t last = std::min<uint64_t>(pos + m, len - 1);
            tab[{gp, (uint32_t)pos, (uint32_t)last}]++;
            c->ct.acov_slow_records++;
        }
    }
}

// At collect, while slot s still owns its records: the table's fill, and the exact S(r) of the batch's slow-path reads into ec_host.
// refetch: the copies enqueue made are stale (the batch was redone).
static int ec_collect(groot_ctx *c, Slot *s, bool refetch)
{
    if (refetch) {
        HIP_TRY(c, hipMemcpy(&s->ct.h_status.p->ec_slow, s->ct.d_ec_slow.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(&s->ct.h_status.p->ec_fill, c->ct.ec_fill.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    const uint32_t n_slow = s->ct.h_status.p->ec_slow;
    c->ct.ec_fill_known = std::max<uint64_t>(c->ct.ec_fill_known, s->ct.h_status.p->ec_fill);
    if (!n_slow) return GROOT_OK;
    // per unit (first, end) traversal; in paired mode (first, end of the even mate's records, end): the unit is a fragment, and its
    // set the intersection of the two mates' sets, when the middle differs from the end
    const size_t sw = c->ct.pairs_on ? 3 : 2;
    std::vector<uint32_t> span(sw * (size_t)n_slow);
    HIP_TRY(c, hipMemcpy(span.data(), s->ct.d_ec_slow.p + 1, span.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t pw = c->pw_view;
    // few reads: their records one by one; many (GROOT_TEST_SHARED_SLOW): the range that holds them all in one copy
    uint32_t lo = ~0u, hi = 0;
    for (uint32_t i = 0; i < n_slow; i++) { lo = std::min(lo, span[sw * i]); hi = std::max(hi, span[sw * i + sw - 1]); }
    const bool whole = n_slow > 32;
    std::vector<groot_trav> tr;
    std::vector<uint64_t> mk;
    if (whole) {
        tr.resize(hi - lo); mk.resize((size_t)(hi - lo) * pw);
        HIP_TRY(c, hipMemcpy(tr.data(), s->d_trav.p + lo, tr.size() * sizeof(groot_trav), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(mk.data(), s->d_mask.p + (size_t)lo * pw, mk.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    std::vector<uint32_t> ids, ids_a, ids_b;
    std::vector<uint64_t> offs;            // assigned coverage: the batch's read offsets (a record's M op is the read's length less its clips)
    if (c->ct.acov_on) {
        offs.resize((size_t)s->n_reads + 1);
        HIP_TRY(c, hipMemcpy(offs.data(), s->off(), offs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    for (uint32_t i = 0; i < n_slow; i++) {
        const uint32_t t0 = span[sw * i], tm = span[sw * i + sw - 2], t1 = span[sw * i + sw - 1];
        if (!whole) {
            tr.resize(t1 - t0); mk.resize((size_t)(t1 - t0) * pw);
            HIP_TRY(c, hipMemcpy(tr.data(), s->d_trav.p + t0, tr.size() * sizeof(groot_trav), hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(mk.data(), s->d_mask.p + (size_t)t0 * pw, mk.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        }
        const size_t o = whole ? t0 - lo : 0;
        if (c->ct.pairs_on && tm != t1) {
            ec_set_of(c, tr.data() + o, mk.data() + o * pw, tm - t0, ids_a);
            ec_set_of(c, tr.data() + o + (tm - t0), mk.data() + (o + (tm - t0)) * pw, t1 - tm, ids_b);
            ids.clear();
            std::set_intersection(ids_a.begin(), ids_a.end(), ids_b.begin(), ids_b.end(), std::back_inserter(ids));
        } else {
            ec_set_of(c, tr.data() + o, mk.data() + o * pw, t1 - t0, ids);
        }
        if (c->ct.acov_on && !ids.empty() && t1 > t0) {
            const bool fragment = c->ct.pairs_on && tm != t1;
            acov_fold_host(c, s, tr.data() + o, mk.data() + o * pw, t1 - t0, ids, offs, fragment);
            c->ct.acp_slow_frags += fragment;
        }
        if (!ids.empty()) c->ct.ec_host[ids]++;
    }
    c->ct.ec_slow_reads += n_slow;
    return GROOT_OK;
}

// ---- the pipeline's hooks (counters.hpp) ---------------------------------------------------------------------------
namespace groot {

void counters_init(groot_ctx *c, const groot_index_view *v)
{
    Counters &k = c->ct;
    // (a view without graphs -- the sketch engine of `index --gpu` -- may carry no offset arrays at all)
    if (v->node_np_off) k.h_np_off.assign(v->node_np_off, v->node_np_off + v->n_nodes + 1); else k.h_np_off.assign(v->n_nodes + 1, 0);
    if (v->graph_path_off) k.h_gpo.assign(v->graph_path_off, v->graph_path_off + v->n_graphs + 1); else k.h_gpo.assign(v->n_graphs + 1, 0);
    k.h_len.assign(v->path_len, v->path_len + v->n_paths);
    k.h_np.resize(v->n_np);
    for (uint64_t j = 0; j < v->n_np; j++) k.h_np[j] = make_uint2(v->np_path[j], v->np_pos[j]);
    k.h_cov_base.assign(v->n_paths + 1, 0);
    for (uint32_t p = 0; p < v->n_paths; p++) k.h_cov_base[p + 1] = k.h_cov_base[p] + v->path_len[p] + 1;
}

int counters_assign(groot_ctx *c, Slot *s)
{
    Counters &k = c->ct;
    if (!k.asg_on) return GROOT_OK;
    const size_t R = std::max<uint32_t>(c->prm.max_batch_reads, 1u);
    HIP_TRY(c, s->ct.d_best.reserve(R));
    HIP_TRY(c, s->ct.d_mapq.reserve(R));
    HIP_TRY(c, s->ct.h_best.reserve(R));
    HIP_TRY(c, s->ct.h_mapq.reserve(R));
    if (!s->n_reads) return GROOT_OK;
    const WorkSet &w = c->ws[s->set];
    AssignArgs a{};
    a.trav = s->d_trav.p; a.mask = s->d_mask.p; a.ctr = s->d_ctr.p; a.off = c->trav_off.p; a.cnt = w.trav_cnt.p;
    a.graph_path_off = k.asg_gpo.p; a.alpha = k.asg_alpha.p; a.best = s->ct.d_best.p; a.mapq = s->ct.d_mapq.p; a.stats = k.asg_stats.p;
    a.min_post = k.asg_min_post;
    a.n_reads = s->n_reads; a.cap = s->trav_cap; a.pw = c->pw_view; a.n_paths = (uint32_t)k.h_len.size(); a.n_graphs = (uint32_t)k.h_gpo.size() - 1;
    // Once per pass, on records the order stage has just written: the filter is not idempotent (a second application would see
    // S(r) = {best} and give MAPQ 60).  A redo pass rewrites the records first and is filtered here again; the skipped pass was not.
    const dim3 g(grid_for(s->n_reads));
    if (a.n_paths <= kAssignLdsPaths && !c->kn.assign_global)
        hipLaunchKernelGGL(assign_kernel<true>, g, dim3(kBlock), (size_t)a.n_paths * sizeof(double), c->tstream, a);
    else hipLaunchKernelGGL(assign_kernel<false>, g, dim3(kBlock), 0, c->tstream, a);
    HIP_TRY(c, hipGetLastError());
    k.asg_launches++;
    return GROOT_OK;
}

int counters_launch(groot_ctx *c, Slot *s)
{
    Counters &k = c->ct;
    const dim3 g(grid_for(s->trav_cap));
    if (k.cov_on) {   // (reads the slot's records and read offsets only: the next batch's seed stage need not wait for it)
        CovArgs ca{};
        ca.trav = s->d_trav.p; ca.mask = s->d_mask.p; ca.seq_off = s->off(); ca.ctr = s->d_ctr.p;
        ca.node_np_off = k.d_np_off.p; ca.np = k.d_np.p; ca.graph_path_off = k.d_gpo.p; ca.path_len = k.d_len.p; ca.slot_base = k.cov_base.p;
        ca.starts = k.cov_starts.p; ca.ends = k.cov_ends.p;
        ca.cap = s->trav_cap; ca.pw = c->pw_view; ca.first_read_id = s->first_read_id;
        hipLaunchKernelGGL(cov_count_kernel, g, dim3(kBlock), 0, c->tstream, ca);
        HIP_TRY(c, hipGetLastError());
    }
    SharedArgs sa{};
    uint32_t tab = 1;                      // this batch's part of the table: >= 2 n_reads slots
    if (k.sh_on || k.ec_on) {    // (the same: slot data and the ctx's own buffers, in tail-stream order)
        sa.trav = s->d_trav.p; sa.mask = s->d_mask.p; sa.ctr = s->d_ctr.p; sa.graph_path_off = k.d_gpo.p;
        sa.set_graph = k.sh_set_graph.p; sa.set_mask = k.sh_set_mask.p; sa.tab_rep = k.sh_tab_rep.p; sa.tab_cnt = k.sh_tab_cnt.p;
        sa.slow = k.sh_slow.p; sa.batch = k.sh_batch.p; sa.tri = k.sh_tri.p; sa.stats = k.sh_stats.p;
        sa.cap = s->trav_cap; sa.pw = c->pw_view; sa.first_read_id = s->first_read_id; sa.n_paths = (uint32_t)k.h_len.size();
        sa.max_segs = c->kn.shared_slow ? 1u : kSharedSegs;
        sa.pairs = k.sh_on;
        sa.slow_cap = std::max<uint32_t>(c->prm.max_batch_reads, 1u);
        while (tab < 2u * std::max<uint32_t>(s->n_reads, 1u)) tab <<= 1;
        sa.tab_mask = tab - 1;
        const dim3 gt(grid_for(tab));      // the merge and the expansion: one item per slot of that part
        const bool paired = k.pairs_on;
        if (paired && k.rp_on) hipLaunchKernelGGL(shared_gather_paired_kernel<true>, g, dim3(kBlock), 0, c->tstream, sa);     // (rescue_launch makes the units it defers)
        else if (paired) hipLaunchKernelGGL(shared_gather_paired_kernel<false>, g, dim3(kBlock), 0, c->tstream, sa);
        else hipLaunchKernelGGL(shared_gather_kernel, g, dim3(kBlock), 0, c->tstream, sa);
        hipLaunchKernelGGL(shared_insert_kernel, g, dim3(kBlock), 0, c->tstream, sa);
        if (k.sh_on && paired) hipLaunchKernelGGL(shared_slow_kernel<true>, dim3(256), dim3(kBlock), 0, c->tstream, sa);
        else if (k.sh_on) hipLaunchKernelGGL(shared_slow_kernel<false>, dim3(256), dim3(kBlock), 0, c->tstream, sa);
        if (k.ec_on) {
            if (int rc = ec_reserve(c, s)) return rc;
            HIP_TRY(c, s->ct.d_ec_slow.reserve(1 + (paired ? 3 : 2) * (size_t)c->prm.max_batch_reads));
            HIP_TRY(c, s->ct.h_status.reserve(1));
        }
        if (k.rp_on) {           // rescued mates in paired-end units: the merge and the expansion wait for the units rescue_launch makes -- all of a batch or none
            HIP_TRY(c, hipGetLastError());
            if (int rc = rescue_launch(c, s, sa, tab)) return rc;
            // (with the rescued mates in assigned coverage over fragments: the units' serials, and the pileup behind that one merge)
            hipLaunchKernelGGL(ec_merge_kernel<true>, gt, dim3(kBlock), 0, c->tstream, sa, k.ec.table(), tab, ++k.ec_epoch, k.ec_fill.p, s->ct.d_ec_slow.p,
                               k.rap_on ? k.acov_tab_ser.p : (uint32_t *)nullptr);
            if (k.rap_on)
                if (int rc = acov_launch(c, s, sa)) return rc;
            hipLaunchKernelGGL(shared_expand_kernel<true>, gt, dim3(kBlock), 0, c->tstream, sa, tab);
            HIP_TRY(c, hipGetLastError());
            return GROOT_OK;
        }
        if (k.ec_on) {
            uint32_t *tab_ser = k.acov_on ? k.acov_tab_ser.p : nullptr;     // (with pairing on: assigned coverage over fragments, the units' serials)
            if (paired) hipLaunchKernelGGL(ec_merge_kernel<true>, gt, dim3(kBlock), 0, c->tstream, sa, k.ec.table(), tab, ++k.ec_epoch, k.ec_fill.p, s->ct.d_ec_slow.p, tab_ser);
            else hipLaunchKernelGGL(ec_merge_kernel<false>, gt, dim3(kBlock), 0, c->tstream, sa, k.ec.table(), tab, ++k.ec_epoch, k.ec_fill.p, s->ct.d_ec_slow.p, tab_ser);
            if (k.acov_on)
                if (int rc = acov_launch(c, s, sa)) return rc;
        }
        if (paired) hipLaunchKernelGGL(shared_expand_kernel<true>, gt, dim3(kBlock), 0, c->tstream, sa, tab);
        else hipLaunchKernelGGL(shared_expand_kernel<false>, gt, dim3(kBlock), 0, c->tstream, sa, tab);
        HIP_TRY(c, hipGetLastError());
    }
    // the rescue family (rescue.hip); the rows and the per-batch table it writes the rescued reads' sets into are free: shared_expand_kernel,
    // above on this stream, has cleared them
    return rescue_launch(c, s, sa, tab);
}

int counters_fetch(groot_ctx *c, Slot *s)
{
    if (s->ct.assigned && s->n_reads) {   // 5 bytes per read
        HIP_TRY(c, hipMemcpyAsync(s->ct.h_best.p, s->ct.d_best.p, (size_t)s->n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
        HIP_TRY(c, hipMemcpyAsync(s->ct.h_mapq.p, s->ct.d_mapq.p, (size_t)s->n_reads, hipMemcpyDeviceToHost, c->d2h_stream));
    }
    if (c->ct.ec_on) {
        CounterStatus *h = s->ct.h_status.p;
        HIP_TRY(c, hipMemcpyAsync(&h->ec_slow, s->ct.d_ec_slow.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
        HIP_TRY(c, hipMemcpyAsync(&h->ec_fill, c->ct.ec_fill.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
        if (c->ct.acov_on) {
            HIP_TRY(c, hipMemcpyAsync(&h->acov_state, s->ct.d_acov_state.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
            HIP_TRY(c, hipMemcpyAsync(&h->acov_fill, c->ct.acov_fill.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
        }
    }
    return rescue_fetch(c, s);
}

int counters_collect(groot_ctx *c, Slot *s, bool redone)
{
    if (s->ct.assigned && s->n_reads && s->ct.h_best.p) {
        if (s->h_ctr.p->flags & kCovSkipFlags) {           // the batch fails: assign_kernel left its records as they were
            std::fill(s->ct.h_best.p, s->ct.h_best.p + s->n_reads, kAssignNone);
            memset(s->ct.h_mapq.p, 0, s->n_reads);
        } else if (redone) {                               // fetch's copies are those of the skipped pass
            HIP_TRY(c, hipMemcpy(s->ct.h_best.p, s->ct.d_best.p, (size_t)s->n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(s->ct.h_mapq.p, s->ct.d_mapq.p, (size_t)s->n_reads, hipMemcpyDeviceToHost));
        }
    }
    if (int rc = rescue_collect_records(c, s, redone)) return rc;
    if (!c->ct.ec_on || !s->n_reads) return GROOT_OK;
    if (int rc = ec_collect(c, s, redone)) return rc;
    if (int rc = rescue_collect_classes(c, s, redone)) return rc;
    return c->ct.acov_on ? acov_collect(c, s, redone) : GROOT_OK;
}

} // namespace groot

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

// ---- report coverage (kernels_cov.hpp) ------------------------------------------------------------------------------
int groot_hip_coverage_enable(groot_ctx *c, int on)
{
    if (!c) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "coverage can only be switched while nothing is in flight");
    HIP_TRY(c, hipSetDevice(c->device));
    Counters &k = c->ct;
    if (!on) {
        k.cov_base.release(); k.cov_starts.release(); k.cov_ends.release();
        k.cov_on = false;
        if (!pos_wanted(k)) pos_release(k);
        return GROOT_OK;
    }
    if (k.cov_on) return GROOT_OK;
    const uint64_t slots = k.h_cov_base.back();
    auto undo = [&](int rc) { k.cov_on = true; groot_hip_coverage_enable(c, 0); return rc; };
    hipError_t e = pos_acquire(k);
    if (e == hipSuccess) e = upload(k.cov_base, k.h_cov_base.data(), k.h_cov_base.size());
    if (e == hipSuccess) e = k.cov_starts.alloc(slots);
    if (e == hipSuccess) e = k.cov_ends.alloc(slots);
    if (e == hipSuccess) e = hipMemset(k.cov_starts.p, 0, std::max<uint64_t>(slots, 1) * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(k.cov_ends.p, 0, std::max<uint64_t>(slots, 1) * sizeof(unsigned long long));
    if (e != hipSuccess) return undo(fail(c, GROOT_E_DEVICE, "coverage: %s", hipGetErrorString(e)));
    k.cov_on = true;
    return GROOT_OK;
}

int groot_hip_coverage_export(groot_ctx *c, uint64_t *records, uint64_t *depth)
{
    if (!c || (!c->ct.h_len.empty() && (!records || !depth))) return GROOT_E_INVALID;
    if (!c->ct.cov_on) return fail(c, GROOT_E_STATE, "coverage is not enabled (groot_hip_coverage_enable)");
    if (int rc = drain(c)) return rc;     // (the batches in flight through their redo, if they need one)
    const uint64_t slots = c->ct.h_cov_base.back();
    std::vector<uint64_t> st(slots), en(slots);
    if (slots) {
        HIP_TRY(c, hipMemcpy(st.data(), c->ct.cov_starts.p, slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(en.data(), c->ct.cov_ends.p, slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    uint64_t at = 0;
    for (size_t p = 0; p < c->ct.h_len.size(); p++) {
        const uint64_t b = c->ct.h_cov_base[p], len = c->ct.h_len[p];
        uint64_t n = 0, d = 0;
        for (uint64_t i = 0; i < len; i++) {
            n += st[b + i];
            d += st[b + i] - en[b + i];
            depth[at++] = d;
        }
        records[p] = n + st[b + len];
    }
    return GROOT_OK;
}

int groot_hip_coverage_reset(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.cov_on) return GROOT_OK;
    if (int rc = drain(c)) return rc;
    const uint64_t slots = std::max<uint64_t>(c->ct.h_cov_base.back(), 1);
    HIP_TRY(c, hipMemset(c->ct.cov_starts.p, 0, slots * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(c->ct.cov_ends.p, 0, slots * sizeof(unsigned long long)));
    return GROOT_OK;
}

// ---- shared reads (kernels_shared.hpp) -------------------------------------------------------------------------------
static uint64_t shared_tri_size(uint64_t n_paths) { return n_paths * (n_paths + 1) / 2; }

// the per-batch buffers shared reads and equivalence classes both use (allocated while either is on)
static void sh_common_release(groot_ctx *c)
{
    for (auto *b : {&c->ct.sh_set_graph, &c->ct.sh_tab_rep, &c->ct.sh_tab_cnt, &c->ct.sh_slow, &c->ct.sh_batch}) b->release();
    c->ct.sh_set_mask.release(); c->ct.sh_stats.release();
    if (!pos_wanted(c->ct)) pos_release(c->ct);
}

static hipError_t sh_common_alloc(groot_ctx *c)
{
    if (c->ct.sh_on || c->ct.ec_on) return hipSuccess;
    const uint32_t R = std::max<uint32_t>(c->prm.max_batch_reads, 1u);
    const uint64_t tab = c->ct.sh_tab_cap;
    hipError_t e = pos_acquire(c->ct);
    if (e == hipSuccess) e = c->ct.sh_set_graph.alloc((size_t)R * kSharedSegs);
    if (e == hipSuccess) e = c->ct.sh_set_mask.alloc((size_t)R * kSharedSegs * std::max<uint32_t>(c->pw_view, 1u));
    if (e == hipSuccess) e = c->ct.sh_tab_rep.alloc(tab);
    if (e == hipSuccess) e = c->ct.sh_tab_cnt.alloc(tab);
    if (e == hipSuccess) e = c->ct.sh_slow.alloc(R);
    if (e == hipSuccess) e = c->ct.sh_batch.alloc(kSharedBatch);
    if (e == hipSuccess) e = c->ct.sh_stats.alloc(kSharedStats);
    if (e == hipSuccess) e = hipMemset(c->ct.sh_tab_rep.p, 0xFF, tab * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(c->ct.sh_tab_cnt.p, 0, tab * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(c->ct.sh_batch.p, 0, kSharedBatch * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(c->ct.sh_stats.p, 0, kSharedStats * sizeof(unsigned long long));
    return e;
}

static int sh_table_size(groot_ctx *c, const char *what)
{
    const uint32_t R = std::max<uint32_t>(c->prm.max_batch_reads, 1u);
    uint64_t tab = 1;
    while (tab < 2ull * R) tab <<= 1;
    if (tab > (1ull << 31)) return fail(c, GROOT_E_UNSUPPORTED, "%s: max_batch_reads=%u is above 2^30", what, R);
    c->ct.sh_tab_cap = (uint32_t)tab;
    return GROOT_OK;
}

int groot_hip_shared_enable(groot_ctx *c, int on)
{
    if (!c) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "shared reads can only be switched while nothing is in flight");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!on) {
        c->ct.sh_tri.release();
        c->ct.sh_on = false;
        if (!c->ct.ec_on) sh_common_release(c);
        return GROOT_OK;
    }
    if (c->ct.sh_on) return GROOT_OK;
    if (c->ct.asg_on) return fail(c, GROOT_E_UNSUPPORTED, "shared reads count S(r), which assignment collapses (groot_hip_assign_enable)");
    if (c->ct.rp_on)
        return fail(c, GROOT_E_UNSUPPORTED, "shared reads with rescued mates in paired-end units are not supported: the triangle has no rescued reads, and the "
                    "fragments left to rescue would be missing from it (groot_hip_rescue_pairs_enable)");
    const uint64_t n_paths = c->ct.h_len.size(), tri = shared_tri_size(n_paths);
    if (tri * sizeof(uint64_t) > GROOT_SHARED_MAX_BYTES)
        return fail(c, GROOT_E_UNSUPPORTED, "shared reads: %llu paths need a %llu MiB pair table, above the bound of %llu MiB", (unsigned long long)n_paths,
                    (unsigned long long)(tri * sizeof(uint64_t) >> 20), (unsigned long long)(GROOT_SHARED_MAX_BYTES >> 20));
    if (!c->ct.ec_on)
        if (int rc = sh_table_size(c, "shared reads")) return rc;
    auto undo = [&](int rc) { c->ct.sh_on = true; groot_hip_shared_enable(c, 0); return rc; };
    hipError_t e = sh_common_alloc(c);
    if (e == hipSuccess) e = c->ct.sh_tri.alloc(tri);
    if (e == hipSuccess) e = hipMemset(c->ct.sh_tri.p, 0, std::max<uint64_t>(tri, 1) * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(c->ct.sh_stats.p, 0, kSharedStats * sizeof(unsigned long long));
    if (e != hipSuccess) return undo(fail(c, GROOT_E_DEVICE, "shared reads: %s", hipGetErrorString(e)));
    c->ct.sh_on = true;
    return GROOT_OK;
}

int groot_hip_shared_export(groot_ctx *c, uint32_t *pa, uint32_t *pb, uint64_t *count, uint64_t cap, uint64_t *n_pairs)
{
    if (!c || !n_pairs || (cap && (!pa || !pb || !count))) return GROOT_E_INVALID;
    if (!c->ct.sh_on) return fail(c, GROOT_E_STATE, "shared reads are not enabled (groot_hip_shared_enable)");
    if (int rc = drain(c)) return rc;     // (the batches in flight through their redo, if they need one)
    const uint64_t P = c->ct.h_len.size(), tri = shared_tri_size(P);
    std::vector<uint64_t> t(tri);
    if (tri) HIP_TRY(c, hipMemcpy(t.data(), c->ct.sh_tri.p, tri * sizeof(uint64_t), hipMemcpyDeviceToHost));
    uint64_t n = 0, i = 0;
    for (uint64_t x = 0; x < P; x++)
        for (uint64_t y = x; y < P; y++, i++) {
            if (!t[i]) continue;
            if (n < cap) { pa[n] = (uint32_t)x; pb[n] = (uint32_t)y; count[n] = t[i]; }
            n++;
        }
    *n_pairs = n;
    return GROOT_OK;
}

int groot_hip_shared_stats(groot_ctx *c, uint64_t *reads, uint64_t *distinct_sets, uint64_t *slow_reads)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.sh_on) return fail(c, GROOT_E_STATE, "shared reads are not enabled (groot_hip_shared_enable)");
    if (int rc = drain(c)) return rc;
    uint64_t st[kSharedPairStats];
    HIP_TRY(c, hipMemcpy(st, c->ct.sh_stats.p, sizeof(st), hipMemcpyDeviceToHost));
    if (reads) *reads = st[0];
    if (distinct_sets) *distinct_sets = st[1];
    if (slow_reads) *slow_reads = st[2];
    return GROOT_OK;
}

int groot_hip_shared_reset(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.sh_on) return GROOT_OK;
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemset(c->ct.sh_tri.p, 0, std::max<uint64_t>(shared_tri_size(c->ct.h_len.size()), 1) * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(c->ct.sh_stats.p, 0, kSharedStats * sizeof(unsigned long long)));
    return GROOT_OK;
}

// ---- equivalence classes (kernels_ec.hpp) ---------------------------------------------------------------------------
int groot_hip_ec_enable(groot_ctx *c, int on)
{
    if (!c) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "equivalence classes can only be switched while nothing is in flight");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!on) {
        if (c->ct.acov_on)
            if (int rc = groot_hip_acov_enable(c, 0)) return rc;     // (its tuples are keyed by this table's serials)
        rescue_ec_release(c->ct);                                    // (the rescued reads' sets have no table to go to)
        c->ct.ec.release(); c->ct.ec_fill.release();
        c->ct.ec_host.clear();
        c->ct.ec_on = false;
        if (!c->ct.sh_on) sh_common_release(c);
        return GROOT_OK;
    }
    if (c->ct.ec_on) return GROOT_OK;
    if (c->ct.asg_on) return fail(c, GROOT_E_UNSUPPORTED, "equivalence classes count S(r), which assignment collapses (groot_hip_assign_enable)");
    if (!c->ct.sh_on)
        if (int rc = sh_table_size(c, "equivalence classes")) return rc;
    uint32_t cap = 1;
    while (cap < (c->kn.ec_slots ? std::max<uint32_t>(c->kn.ec_slots, 2u) : (1u << 16))) cap <<= 1;
    auto undo = [&](int rc) { c->ct.ec_on = true; groot_hip_ec_enable(c, 0); return rc; };
    hipError_t e = sh_common_alloc(c);
    if (e == hipSuccess) e = c->ct.ec.alloc(cap, std::max<uint32_t>(c->pw_view, 1u), c->tstream);
    if (e == hipSuccess) e = c->ct.ec_fill.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(c->ct.ec_fill.p, 0, sizeof(uint32_t), c->tstream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->tstream);
    if (e != hipSuccess) return undo(fail(c, GROOT_E_DEVICE, "equivalence classes: %s", hipGetErrorString(e)));
    c->ct.ec_fill_known = c->ct.ec_grows = c->ct.ec_slow_reads = 0;
    c->ct.ec_host.clear();
    c->ct.ec_on = true;
    return GROOT_OK;
}

// the device table and the host map merged: S -> reads, in canonical order (lexicographic on the ascending ID lists)
// by_serial (optional): the ID list of every slot of the device table, by the slot's serial
static int ec_gather(groot_ctx *c, std::map<std::vector<uint32_t>, uint64_t> &out, std::vector<std::vector<uint32_t>> *by_serial = nullptr)
{
    if (int rc = drain(c)) return rc;     // (the batches in flight through their redo and their slow-path reads)
    uint32_t fill = 0;
    HIP_TRY(c, hipMemcpy(&fill, c->ct.ec_fill.p, sizeof fill, hipMemcpyDeviceToHost));
    out = c->ct.ec_host;
    if (!fill) return GROOT_OK;
    const uint32_t pw = std::max<uint32_t>(c->pw_view, 1u);
    DevBuf<uint32_t> g, n, ser;
    DevBuf<uint64_t> m;
    DevBuf<unsigned long long> cnt;
    HIP_TRY(c, ser.alloc(fill));
    HIP_TRY(c, g.alloc((size_t)fill * kSharedSegs));
    HIP_TRY(c, m.alloc((size_t)fill * kSharedSegs * pw));
    HIP_TRY(c, cnt.alloc(fill));
    HIP_TRY(c, n.alloc(1));
    HIP_TRY(c, hipMemsetAsync(n.p, 0, sizeof(uint32_t), c->tstream));
    hipLaunchKernelGGL(ec_export_kernel, dim3(grid_for(c->ct.ec.cap)), dim3(kBlock), 0, c->tstream, c->ct.ec.table(), c->ct.ec.cap, pw, g.p, m.p, cnt.p, ser.p, n.p, fill);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->tstream));
    uint32_t got = 0;
    HIP_TRY(c, hipMemcpy(&got, n.p, sizeof got, hipMemcpyDeviceToHost));
    if (got != fill) return fail(c, GROOT_E_DEVICE, "equivalence classes: %u keys in a table that counted %u", got, fill);
    std::vector<uint32_t> hg((size_t)fill * kSharedSegs);
    std::vector<uint64_t> hm((size_t)fill * kSharedSegs * pw), hc(fill);
    HIP_TRY(c, hipMemcpy(hg.data(), g.p, hg.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hm.data(), m.p, hm.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hc.data(), cnt.p, hc.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    std::vector<uint32_t> hs(fill);
    HIP_TRY(c, hipMemcpy(hs.data(), ser.p, hs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (by_serial) by_serial->assign(fill, {});
    std::vector<groot_trav> tr;
    std::vector<uint64_t> mk;
    std::vector<uint32_t> ids;
    for (uint32_t i = 0; i < fill; i++) {
        // a key = one pseudo-record per segment: (graph, OR of its path sets)
        tr.clear(); mk.clear();
        for (uint32_t k = 0; k < kSharedSegs && hg[(size_t)i * kSharedSegs + k] != kSharedEmpty; k++) {
            groot_trav t{};
            t.graph_id = hg[(size_t)i * kSharedSegs + k];
            tr.push_back(t);
            for (uint32_t w = 0; w < pw; w++) mk.push_back(hm[((size_t)i * kSharedSegs + k) * pw + w]);
        }
        ec_set_of(c, tr.data(), mk.data(), tr.size(), ids);
        if (!ids.empty() && hc[i]) out[ids] += hc[i];
        if (by_serial && hs[i] < fill) (*by_serial)[hs[i]] = ids;
    }
    return GROOT_OK;
}

// the classes of m as a CSR: off[e] .. off[e + 1] of ids are the path IDs of class e, count[e] its reads (the caller has checked the room)
static void write_ecs(const std::map<std::vector<uint32_t>, uint64_t> &m, uint64_t *off, uint32_t *ids, uint64_t *count)
{
    uint64_t e = 0, at = 0;
    if (off) off[0] = 0;
    for (const auto &kv : m) {
        for (uint32_t x : kv.first) ids[at++] = x;
        count[e] = kv.second;
        off[++e] = at;
    }
}

int groot_hip_ec_export(groot_ctx *c, uint64_t *off, uint32_t *ids, uint64_t *count, uint64_t cap_ec, uint64_t cap_ids, uint64_t *n_ec, uint64_t *n_ids)
{
    if (!c || !n_ec || !n_ids || (cap_ec && (!off || !count)) || (cap_ids && !ids)) return GROOT_E_INVALID;
    if (!c->ct.ec_on) return fail(c, GROOT_E_STATE, "equivalence classes are not enabled (groot_hip_ec_enable)");
    std::map<std::vector<uint32_t>, uint64_t> m;
    if (int rc = ec_gather(c, m)) return rc;
    uint64_t ni = 0;
    for (const auto &kv : m) ni += kv.first.size();
    *n_ec = m.size();
    *n_ids = ni;
    if (!cap_ec && !cap_ids) return GROOT_OK;
    if (cap_ec < m.size() || cap_ids < ni)
        return fail(c, GROOT_E_NOSPACE, "equivalence classes: room for %llu classes / %llu IDs, %llu / %llu needed", (unsigned long long)cap_ec,
                    (unsigned long long)cap_ids, (unsigned long long)m.size(), (unsigned long long)ni);
    write_ecs(m, off, ids, count);
    return GROOT_OK;
}

int groot_hip_ec_stats(groot_ctx *c, uint64_t *reads, uint64_t *distinct, uint64_t *slow_reads, uint64_t *grows)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.ec_on) return fail(c, GROOT_E_STATE, "equivalence classes are not enabled (groot_hip_ec_enable)");
    std::map<std::vector<uint32_t>, uint64_t> m;
    if (int rc = ec_gather(c, m)) return rc;
    uint64_t r = 0;
    for (const auto &kv : m) r += kv.second;
    if (reads) *reads = r;
    if (distinct) *distinct = m.size();
    if (slow_reads) *slow_reads = c->ct.ec_slow_reads;
    if (grows) *grows = c->ct.ec_grows;
    return GROOT_OK;
}

int groot_hip_ec_reset(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.ec_on) return GROOT_OK;
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemset(c->ct.ec.claim.p, 0, (size_t)c->ct.ec.cap * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(c->ct.ec_fill.p, 0, sizeof(uint32_t)));
    c->ct.ec_fill_known = c->ct.ec_grows = c->ct.ec_slow_reads = 0;
    c->ct.ec_host.clear();
    if (int rc = rescue_ec_reset(c)) return rc;     // (the rescued and the gap-placed reads are counted with the classes they are in)
    if (c->ct.pairs_on) HIP_TRY(c, hipMemset(c->ct.sh_stats.p + kSharedPairStats, 0, (kSharedStats - kSharedPairStats) * sizeof(unsigned long long)));
    return groot_hip_acov_reset(c);     // (the serials start again: its tuples would name other classes)
}

// ---- assigned coverage (kernels_acov.hpp; the definition is in groot_hip.h) ------------------------------------------------
int groot_hip_acov_enable(groot_ctx *c, int on)
{
    if (!c) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "assigned coverage can only be switched while nothing is in flight");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!on) {
        if (c->ct.rac_on) rescue_ec_release(c->ct);     // (the rescued reads in it go, and the rescued classes that came on with them)
        rescue_acov_pairs_release(c->ct);               // (the rescued mates leave it; their rule in the classes stays)
        c->ct.acp_stats.release();                      // (the rule over fragments goes with it; pairing stays)
        c->ct.acp_on = false;
        c->ct.acov.release();
        for (auto *b : {&c->ct.acov_fill, &c->ct.acov_err, &c->ct.acov_tab_ser}) b->release();
        c->ct.acov_host.clear();
        c->ct.acov_on = false;
        return GROOT_OK;
    }
    if (c->ct.acov_on) return GROOT_OK;
    if (c->ct.pairs_on) return fail(c, GROOT_E_UNSUPPORTED, "assigned coverage with paired-end units is not supported");
    if (c->ct.rec_on) return fail(c, GROOT_E_UNSUPPORTED, "assigned coverage weighs records, and a rescued read in the equivalence classes has none (groot_hip_rescue_ec_enable)");
    if (int rc = groot_hip_ec_enable(c, 1)) return rc;
    uint32_t cap = 1;
    while (cap < (c->kn.acov_slots ? std::max<uint32_t>(c->kn.acov_slots, 2u) : (1u << 20))) cap <<= 1;
    auto undo = [&](int rc) { c->ct.acov_on = true; groot_hip_acov_enable(c, 0); return rc; };
    hipError_t e = c->ct.acov.alloc(cap, c->tstream);
    if (e == hipSuccess) e = c->ct.acov_fill.alloc(1);
    if (e == hipSuccess) e = c->ct.acov_err.alloc(1);
    if (e == hipSuccess) e = c->ct.acov_tab_ser.alloc(c->ct.sh_tab_cap);
    if (e == hipSuccess) e = hipMemsetAsync(c->ct.acov_fill.p, 0, sizeof(uint32_t), c->tstream);
    if (e == hipSuccess) e = hipMemsetAsync(c->ct.acov_err.p, 0, sizeof(uint32_t), c->tstream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->tstream);
    if (e != hipSuccess) return undo(fail(c, GROOT_E_DEVICE, "assigned coverage: %s", hipGetErrorString(e)));
    c->ct.acov_grows = c->ct.acov_slow_records = c->ct.acov_redone = 0;
    c->ct.acov_host.clear();
    c->ct.acov_on = true;
    return GROOT_OK;
}

namespace {
struct AcovTuple {
    uint32_t ec, path, pos, last;
    uint64_t n;
    bool operator<(const AcovTuple &o) const { return std::tie(ec, path, pos, last) < std::tie(o.ec, o.path, o.pos, o.last); }
    bool same_key(const AcovTuple &o) const { return ec == o.ec && path == o.path && pos == o.pos && last == o.last; }
};
}

// the ctx's ECs in canonical order and its tuples, EC = index into that list, ascending, equal keys of the device table and the host
// map summed
static int acov_gather(groot_ctx *c, std::map<std::vector<uint32_t>, uint64_t> &ecs, std::vector<AcovTuple> &out)
{
    std::vector<std::vector<uint32_t>> by_serial;
    if (int rc = ec_gather(c, ecs, &by_serial)) return rc;
    out.clear();
    std::map<std::vector<uint32_t>, uint32_t> index;
    for (const auto &kv : ecs) { const uint32_t i = (uint32_t)index.size(); index[kv.first] = i; }
    uint32_t fill = 0;
    HIP_TRY(c, hipMemcpy(&fill, c->ct.acov_fill.p, sizeof fill, hipMemcpyDeviceToHost));
    if (fill) {
        std::vector<uint32_t> ser_idx(by_serial.size(), ~0u);
        for (size_t i = 0; i < by_serial.size(); i++) {
            auto it = index.find(by_serial[i]);
            if (it != index.end()) ser_idx[i] = it->second;
        }
        DevBuf<unsigned long long> key, cnt;
        DevBuf<uint32_t> n;
        HIP_TRY(c, key.alloc(2 * (size_t)fill));
        HIP_TRY(c, cnt.alloc(fill));
        HIP_TRY(c, n.alloc(1));
        HIP_TRY(c, hipMemsetAsync(n.p, 0, sizeof(uint32_t), c->tstream));
        hipLaunchKernelGGL(acov_export_kernel, dim3(grid_for(c->ct.acov.cap)), dim3(kBlock), 0, c->tstream, c->ct.acov.table(), c->ct.acov.cap, key.p, cnt.p, n.p, fill);
        c->ct.acov_launches++;
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->tstream));
        uint32_t got = 0;
        HIP_TRY(c, hipMemcpy(&got, n.p, sizeof got, hipMemcpyDeviceToHost));
        if (got > fill) return fail(c, GROOT_E_DEVICE, "assigned coverage: %u tuples in a table that counted %u", got, fill);
        std::vector<uint64_t> hk(2 * (size_t)got), hc(got);
        if (got) {
            HIP_TRY(c, hipMemcpy(hk.data(), key.p, hk.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(hc.data(), cnt.p, hc.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        }
        out.reserve(got);
        for (uint32_t i = 0; i < got; i++) {
            const uint64_t ser = (hk[2 * (size_t)i] >> 32) - 1;
            if (ser >= ser_idx.size() || ser_idx[ser] == ~0u) return fail(c, GROOT_E_DEVICE, "assigned coverage: a tuple names class %llu, which the table of classes does not hold", (unsigned long long)ser);
            out.push_back(AcovTuple{ser_idx[ser], (uint32_t)hk[2 * (size_t)i], (uint32_t)(hk[2 * (size_t)i + 1] >> 32), (uint32_t)hk[2 * (size_t)i + 1], hc[i]});
        }
    }
    for (const auto &kv : c->ct.acov_host) {
        auto it = index.find(kv.first);
        if (it == index.end()) return fail(c, GROOT_E_DEVICE, "assigned coverage: the host map holds a class the table of classes does not");
        for (const auto &t : kv.second) out.push_back(AcovTuple{it->second, t.first[0], t.first[1], t.first[2], t.second});
    }
    std::sort(out.begin(), out.end());
    size_t w = 0;
    for (size_t i = 0; i < out.size(); i++) {
        if (w && out[w - 1].same_key(out[i])) out[w - 1].n += out[i].n;
        else out[w++] = out[i];
    }
    out.resize(w);
    return GROOT_OK;
}

int groot_hip_acov_export(groot_ctx *c, uint64_t *ec_off, uint32_t *ec_ids, uint64_t *ec_count, uint32_t *tuples, uint64_t *n, uint64_t cap_ec, uint64_t cap_ids,
                          uint64_t cap_tuples, uint64_t *n_ec, uint64_t *n_ids, uint64_t *n_tuples)
{
    if (!c || !n_ec || !n_ids || !n_tuples || (cap_ec && (!ec_off || !ec_count)) || (cap_ids && !ec_ids) || (cap_tuples && (!tuples || !n))) return GROOT_E_INVALID;
    if (!c->ct.acov_on) return fail(c, GROOT_E_STATE, "assigned coverage is not enabled (groot_hip_acov_enable)");
    std::map<std::vector<uint32_t>, uint64_t> m;
    std::vector<AcovTuple> tp;
    if (int rc = acov_gather(c, m, tp)) return rc;
    if (int rc = rescue_acov_dropped(c)) return rc;      // (behind the drain of acov_gather)
    uint64_t ni = 0;
    for (const auto &kv : m) ni += kv.first.size();
    *n_ec = m.size();
    *n_ids = ni;
    *n_tuples = tp.size();
    if (!cap_ec && !cap_ids && !cap_tuples) return GROOT_OK;
    if (cap_ec < m.size() || cap_ids < ni || cap_tuples < tp.size())
        return fail(c, GROOT_E_NOSPACE, "assigned coverage: room for %llu classes / %llu IDs / %llu tuples, %llu / %llu / %llu needed", (unsigned long long)cap_ec,
                    (unsigned long long)cap_ids, (unsigned long long)cap_tuples, (unsigned long long)m.size(), (unsigned long long)ni, (unsigned long long)tp.size());
    write_ecs(m, ec_off, ec_ids, ec_count);
    for (size_t i = 0; i < tp.size(); i++) {
        tuples[4 * i] = tp[i].ec; tuples[4 * i + 1] = tp[i].path; tuples[4 * i + 2] = tp[i].pos; tuples[4 * i + 3] = tp[i].last;
        n[i] = tp[i].n;
    }
    return GROOT_OK;
}

int groot_hip_acov_stats(groot_ctx *c, uint64_t *records, uint64_t *tuples, uint64_t *slots, uint64_t *grows, uint64_t *slow_records, uint64_t *launches)
{
    if (!c) return GROOT_E_INVALID;
    uint64_t r = 0, nt = 0;
    if (c->ct.acov_on) {
        std::map<std::vector<uint32_t>, uint64_t> m;
        std::vector<AcovTuple> tp;
        if (int rc = acov_gather(c, m, tp)) return rc;
        for (const auto &t : tp) r += t.n;
        nt = tp.size();
    }
    if (records) *records = r;
    if (tuples) *tuples = nt;
    if (slots) *slots = c->ct.acov_on ? c->ct.acov.cap : 0;
    if (grows) *grows = c->ct.acov_on ? c->ct.acov_grows : 0;
    if (slow_records) *slow_records = c->ct.acov_on ? c->ct.acov_slow_records : 0;
    if (launches) *launches = c->ct.acov_launches;
    return GROOT_OK;
}

int groot_hip_acov_reset(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.acov_on) return GROOT_OK;
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemset(c->ct.acov.k0.p, 0, (size_t)c->ct.acov.cap * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(c->ct.acov.k1.p, 0xFF, (size_t)c->ct.acov.cap * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(c->ct.acov.cnt.p, 0, (size_t)c->ct.acov.cap * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(c->ct.acov_fill.p, 0, sizeof(uint32_t)));
    c->ct.acov_grows = c->ct.acov_slow_records = c->ct.acov_redone = 0;
    c->ct.acov_host.clear();
    if (c->ct.acp_on) HIP_TRY(c, hipMemset(c->ct.acp_stats.p, 0, kAcovPairStats * sizeof(unsigned long long)));
    c->ct.acp_host_left = c->ct.acp_slow_frags = 0;
    return rescue_acov_reset(c);
}

// ---- assignment (kernels_assign.hpp) ---------------------------------------------------------------------------------
int groot_hip_assign_enable(groot_ctx *c, const double *alpha, uint32_t n_paths, double min_posterior)
{
    if (!c) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "assignment can only be switched while nothing is in flight");
    HIP_TRY(c, hipSetDevice(c->device));
    Counters &k = c->ct;
    if (!alpha) {
        k.asg_alpha.release(); k.asg_gpo.release(); k.asg_stats.release();
        k.asg_on = false;
        return GROOT_OK;
    }
    if (k.sh_on || k.ec_on || k.acov_on || k.pairs_on)
        return fail(c, GROOT_E_UNSUPPORTED, "assignment collapses S(r): not with shared reads, equivalence classes, assigned coverage or pairing on");
    if (rescue_on(c)) return fail(c, GROOT_E_UNSUPPORTED, "assignment rewrites the records mismatch rescue tells the unaligned reads by (groot_hip_rescue_enable)");
    if (n_paths != k.h_len.size()) return fail(c, GROOT_E_INVALID, "assignment: alpha has %u values, the index %zu paths", n_paths, k.h_len.size());
    if (!(min_posterior >= 0.0 && min_posterior <= 1.0)) return fail(c, GROOT_E_INVALID, "assignment: min_posterior %g is not in [0, 1]", min_posterior);
    for (uint32_t p = 0; p < n_paths; p++)
        if (!(alpha[p] >= 0.0 && alpha[p] <= 1e300)) return fail(c, GROOT_E_INVALID, "assignment: alpha[%u] = %g is not a finite value in [0, 1e300]", p, alpha[p]);
    const bool was_on = k.asg_on;
    auto undo = [&](int rc) { groot_hip_assign_enable(c, nullptr, 0, 0.0); return rc; };
    hipError_t e = upload(k.asg_alpha, alpha, n_paths);
    if (e == hipSuccess && !was_on) {
        e = upload(k.asg_gpo, k.h_gpo.data(), k.h_gpo.size());
        if (e == hipSuccess) e = k.asg_stats.alloc(kAssignStats);
        if (e == hipSuccess) e = hipMemset(k.asg_stats.p, 0, kAssignStats * sizeof(unsigned long long));
    }
    if (e != hipSuccess) return undo(fail(c, GROOT_E_DEVICE, "assignment: %s", hipGetErrorString(e)));
    k.asg_min_post = min_posterior;
    k.asg_on = true;
    return GROOT_OK;
}

int groot_hip_assign_stats(groot_ctx *c, groot_assign_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    uint64_t st[kAssignStats] = {};
    if (c->ct.asg_on) {
        if (int rc = drain(c)) return rc;
        HIP_TRY(c, hipMemcpy(st, c->ct.asg_stats.p, sizeof(st), hipMemcpyDeviceToHost));
    }
    out->reads = st[0]; out->assigned = st[1]; out->unassigned = st[2]; out->below = st[3]; out->ties = st[4];
    out->records_in = st[5]; out->records_kept = st[6]; out->travs_emptied = st[7];
    out->launches = c->ct.asg_launches;
    return GROOT_OK;
}

int groot_hip_assign_reset(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.asg_on) return GROOT_OK;
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemset(c->ct.asg_stats.p, 0, kAssignStats * sizeof(unsigned long long)));
    return GROOT_OK;
}

// ---- paired-end reads (the kPaired kernels of kernels_shared.hpp; the definition is in groot_hip.h) -------------------------
int groot_hip_pairs_enable(groot_ctx *c, int on)
{
    if (!c) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "pairing can only be switched while nothing is in flight");
    if (on && c->ct.acov_on && !c->ct.acp_on) return fail(c, GROOT_E_UNSUPPORTED, "paired-end units with assigned coverage are not supported");
    if (on && c->ct.asg_on) return fail(c, GROOT_E_UNSUPPORTED, "paired-end units with assignment are not supported (groot_hip_assign_enable)");
    if (on && c->ct.rec_on && !c->ct.rp_on) return fail(c, GROOT_E_UNSUPPORTED, "paired-end units with rescued reads in the equivalence classes are not supported: mates are rescued one by one (groot_hip_rescue_ec_enable)");
    if (!on && c->ct.acp_on)              // (assigned coverage over fragments has no meaning without them: the rule and the table go)
        if (int rc = groot_hip_acov_enable(c, 0)) return rc;
    if (!on && c->ct.rp_on) rescue_ec_release(c->ct);     // (the rescued mates' rule has no meaning without fragments: it and the rescued classes go)
    c->ct.pairs_on = on != 0;
    if (c->ct.sh_on || c->ct.ec_on) {     // (else there is nothing to zero: sh_common_alloc zeroes the counts when either comes on)
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipMemset(c->ct.sh_stats.p + kSharedPairStats, 0, (kSharedStats - kSharedPairStats) * sizeof(unsigned long long)));
    }
    return GROOT_OK;
}

int groot_hip_pairs_stats(groot_ctx *c, uint64_t *joined, uint64_t *split, uint64_t *single)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.pairs_on) return fail(c, GROOT_E_STATE, "pairing is not enabled (groot_hip_pairs_enable)");
    if (int rc = drain(c)) return rc;
    uint64_t st[kSharedStats] = {};
    if (c->ct.sh_on || c->ct.ec_on) HIP_TRY(c, hipMemcpy(st, c->ct.sh_stats.p, sizeof(st), hipMemcpyDeviceToHost));
    if (joined) *joined = st[kSharedPairStats];
    if (split) *split = st[kSharedPairStats + 1];
    if (single) *single = st[kSharedPairStats + 2];
    return GROOT_OK;
}

// ---- assigned coverage over fragments (the kPaired kernels of kernels_acov.hpp; the rule is in groot_hip.h) -----------------
int groot_hip_acov_pairs_enable(groot_ctx *c, int on)
{
    if (!c) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "assigned coverage over fragments can only be switched while nothing is in flight");
    Counters &k = c->ct;
    if (!on) return k.acp_on ? groot_hip_acov_enable(c, 0) : GROOT_OK;     // (equivalence classes and pairing stay)
    if (k.acp_on) return GROOT_OK;
    if (k.asg_on) return fail(c, GROOT_E_UNSUPPORTED, "assigned coverage over fragments counts S(r), which assignment collapses (groot_hip_assign_enable)");
    if (k.rec_on)
        return fail(c, GROOT_E_UNSUPPORTED, "assigned coverage over fragments with rescued reads in the equivalence classes is not supported: mates are rescued one by one (groot_hip_rescue_ec_enable)");
    HIP_TRY(c, hipSetDevice(c->device));
    // the two enables refuse each other: each is made with the other one off
    const bool was_acov = k.acov_on, was_pairs = k.pairs_on;
    k.pairs_on = false;
    int rc = groot_hip_acov_enable(c, 1);
    k.pairs_on = was_pairs;
    if (rc) return rc;
    hipError_t e = k.acp_stats.alloc(kAcovPairStats);
    if (e == hipSuccess) e = hipMemset(k.acp_stats.p, 0, kAcovPairStats * sizeof(unsigned long long));
    if (e != hipSuccess) {
        k.acp_stats.release();
        if (!was_acov) groot_hip_acov_enable(c, 0);
        return fail(c, GROOT_E_DEVICE, "assigned coverage over fragments: %s", hipGetErrorString(e));
    }
    k.acp_host_left = k.acp_slow_frags = 0;
    k.acp_on = true;
    return was_pairs ? GROOT_OK : groot_hip_pairs_enable(c, 1);
}

int groot_hip_acov_pairs_stats(groot_ctx *c, groot_acov_pairs_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    *out = groot_acov_pairs_stats{};
    if (!c->ct.acp_on) return GROOT_OK;
    std::map<std::vector<uint32_t>, uint64_t> m;
    std::vector<AcovTuple> tp;
    if (int rc = acov_gather(c, m, tp)) return rc;     // (drains)
    for (const auto &t : tp) out->records += t.n;
    uint64_t st[kAcovPairStats];
    HIP_TRY(c, hipMemcpy(st, c->ct.acp_stats.p, sizeof(st), hipMemcpyDeviceToHost));
    out->left_out = st[0] + c->ct.acp_host_left;
    out->joined_reads = st[1];
    out->slow_fragments = c->ct.acp_slow_frags;
    return GROOT_OK;
}

// ---- bootstrap replicates of the abundance EM (kernels_boot.hpp; the contract is in groot_host.h) ---------------------------
namespace {
struct DeviceGuard {         // the calling thread's current device, put back on return
    int prev = -1;
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
struct StreamGuard {
    hipStream_t s = nullptr;
    ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};
constexpr size_t kBootChunkBytes = 256u << 20;      // device memory of one chunk of replicates (counts + alpha)
constexpr uint32_t kBootDrawGroups = 2048;          // workgroups of one boot_resample_kernel launch, about

// What groot_hip_em_bootstrap and groot_hip_em_rarefy share: the ECs checked and restated for the kernels, the device and a stream of
// the call's own, the uploads, the buffers of one chunk of count vectors, and boot_em_kernel over such a chunk.  (Declared in the
// order the pieces must go in reverse: the buffers are freed before the stream ends and the device is put back.)
struct EmDevice {
    DeviceGuard dg;
    StreamGuard sg;
    hipStream_t st = nullptr;
    uint32_t n_paths = 0, ne = 0;
    uint64_t total = 0;                              // N
    std::vector<uint64_t> cum;
    std::vector<uint32_t> ec_off, path_off, ec_ids, path_ecs;
    DevBuf<uint64_t> d_cum;
    DevBuf<uint32_t> d_ec_off, d_ec_ids, d_path_off, d_path_ecs, d_it;
    DevBuf<unsigned long long> d_cnt;               // [chunk][n_ec]
    DevBuf<double> d_alpha, d_scratch;
    int lds_max = 0, n_cu = 1;
    uint32_t chunk = 0, em_grid = 0;                 // count vectors of one chunk; workgroups of boot_em_kernel
    size_t draw_lds = 0, em_lds = 0;
    bool draw_in_lds = false, em_in_lds = false;

    size_t per_vector() const { return ((size_t)ne + n_paths) * 8; }

    // the EM's own errors, the limits of the device path, and the host side of the uploads
    int check(const char *what, uint32_t paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t min_iter, uint32_t max_iter)
    {
        if (max_iter < min_iter)
            return fail(nullptr, GROOT_E_INVALID, "number of EM iterations (%u) must be greater than minimum iterations (%u)", max_iter, min_iter);
        if (max_iter < 1) return fail(nullptr, GROOT_E_INVALID, "no EM iterations were ran");
        if (n_ec >= 0xFFFFFFFFull || (n_ec && off[n_ec] >= 0xFFFFFFFFull))
            return fail(nullptr, GROOT_E_UNSUPPORTED, "%s on the device: 2^32 ECs or path IDs and more", what);
        n_paths = paths;
        ne = (uint32_t)n_ec;
        cum.assign((size_t)ne + 1, 0);
        ec_off.assign((size_t)ne + 1, 0);
        path_off.assign((size_t)n_paths + 1, 0);
        for (uint32_t e = 0; e < ne; e++) {
            if (off[e + 1] < off[e] || (off[e + 1] > off[e] && !ids)) return fail(nullptr, GROOT_E_INVALID, "EC %u: bad offsets", e);
            for (uint64_t i = off[e]; i < off[e + 1]; i++) {
                if (ids[i] >= n_paths) return fail(nullptr, GROOT_E_INVALID, "EC %u holds path %u of %u", e, ids[i], n_paths);
                path_off[ids[i] + 1]++;
            }
            ec_off[e + 1] = ec_off[e] + (uint32_t)(off[e + 1] - off[e]);
            cum[e + 1] = cum[e] + count[e];
            if (cum[e + 1] < cum[e]) return fail(nullptr, GROOT_E_INVALID, "the EC counts sum to 2^64 or more");
        }
        total = cum[ne];
        // path -> EC, CSR: the ECs are visited in order, so every path's list ascends (an ID an EC names twice is listed twice, as the host adds it twice)
        const uint32_t nnz = ec_off[ne];
        for (uint32_t p = 0; p < n_paths; p++) path_off[p + 1] += path_off[p];
        ec_ids.assign(std::max<uint32_t>(nnz, 1u), 0);
        path_ecs.assign(std::max<uint32_t>(nnz, 1u), 0);
        std::vector<uint32_t> at(path_off.begin(), path_off.end() - 1);
        for (uint32_t e = 0; e < ne; e++)
            for (uint64_t i = off[e]; i < off[e + 1]; i++) {
                ec_ids[ec_off[e] + (i - off[e])] = ids[i];
                path_ecs[at[ids[i]]++] = e;
            }
        return GROOT_OK;
    }

    // the device, the stream, the uploads and the buffers of a chunk: at most n_vec count vectors, a multiple of `group` (a chunk never
    // splits a group of vectors that belong together), within kBootChunkBytes unless one group alone is larger
    int open(int device, size_t n_vec, uint32_t group)
    {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(nullptr, GROOT_E_DEVICE, "no HIP device");
        if (device < 0 || device >= n_dev) return fail(nullptr, GROOT_E_DEVICE, "device %d of %d", device, n_dev);
        if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
        HIP_TRY(nullptr, hipSetDevice(device));
        HIP_TRY(nullptr, hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
        HIP_TRY(nullptr, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
        n_cu = std::max(n_cu, 1);
        HIP_TRY(nullptr, hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
        st = sg.s;

        const size_t fit = std::max<size_t>(1, std::min<size_t>({n_vec, (size_t)65535, kBootChunkBytes / std::max<size_t>(per_vector(), 1)}));
        chunk = (uint32_t)std::max<size_t>(group, fit / group * group);
        HIP_TRY(nullptr, d_cum.alloc(cum.size()));
        HIP_TRY(nullptr, d_ec_off.alloc(ec_off.size()));
        HIP_TRY(nullptr, d_ec_ids.alloc(ec_ids.size()));
        HIP_TRY(nullptr, d_path_off.alloc(path_off.size()));
        HIP_TRY(nullptr, d_path_ecs.alloc(path_ecs.size()));
        HIP_TRY(nullptr, d_cnt.alloc((size_t)chunk * ne));
        HIP_TRY(nullptr, d_alpha.alloc((size_t)chunk * n_paths));
        HIP_TRY(nullptr, d_it.alloc(chunk));
        HIP_TRY(nullptr, hipMemcpyAsync(d_cum.p, cum.data(), cum.size() * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(nullptr, hipMemcpyAsync(d_ec_off.p, ec_off.data(), ec_off.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(nullptr, hipMemcpyAsync(d_ec_ids.p, ec_ids.data(), ec_ids.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(nullptr, hipMemcpyAsync(d_path_off.p, path_off.data(), path_off.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(nullptr, hipMemcpyAsync(d_path_ecs.p, path_ecs.data(), path_ecs.size() * 4, hipMemcpyHostToDevice, st));

        // LDS or global memory: the cumulative table and the histogram of the draws; alpha and norm of the EM
        draw_lds = ((size_t)ne + 1) * 8 + (size_t)ne * 4;
        em_lds = per_vector();
        draw_in_lds = draw_lds <= (size_t)lds_max;
        em_in_lds = em_lds <= (size_t)lds_max;
        if (em_in_lds && em_lds > 48 * 1024)
            HIP_TRY(nullptr, hipFuncSetAttribute((const void *)boot_em_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)em_lds));
        em_grid = std::min<uint32_t>(chunk, (uint32_t)n_cu);
        if (!em_in_lds) HIP_TRY(nullptr, d_scratch.alloc((size_t)em_grid * ((size_t)ne + n_paths)));
        return GROOT_OK;
    }

    // the EM of the chunk's first nv count vectors, and their results to the host arrays' vectors v0 .. v0 + nv; waits for them
    int em_and_fetch(size_t v0, uint32_t nv, uint32_t min_iter, uint32_t max_iter, uint64_t *counts, double *alpha, uint32_t *iterations)
    {
        BootEmArgs ea{d_ec_off.p, d_ec_ids.p, d_path_off.p, d_path_ecs.p, d_cnt.p, d_alpha.p, d_it.p, d_scratch.p, 1.0 / (double)n_paths, n_paths, ne, nv, min_iter, max_iter};
        const dim3 grid(std::min<uint32_t>(nv, em_grid));
        if (em_in_lds) hipLaunchKernelGGL(boot_em_kernel<true>, grid, dim3(kBootEmBlock), em_lds, st, ea);
        else hipLaunchKernelGGL(boot_em_kernel<false>, grid, dim3(kBootEmBlock), 0, st, ea);
        HIP_TRY(nullptr, hipGetLastError());
        if (counts && ne) HIP_TRY(nullptr, hipMemcpyAsync(counts + v0 * ne, d_cnt.p, (size_t)nv * ne * 8, hipMemcpyDeviceToHost, st));
        if (n_paths) HIP_TRY(nullptr, hipMemcpyAsync(alpha + v0 * n_paths, d_alpha.p, (size_t)nv * n_paths * 8, hipMemcpyDeviceToHost, st));
        if (iterations) HIP_TRY(nullptr, hipMemcpyAsync(iterations + v0, d_it.p, (size_t)nv * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(nullptr, hipStreamSynchronize(st));
        return GROOT_OK;
    }
};
} // namespace

int groot_hip_em_bootstrap(int device, uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t n_boot,
                           uint64_t seed, uint64_t n_draws, uint32_t min_iter, uint32_t max_iter, uint64_t *boot_count, double *alpha, uint32_t *iterations)
{
    if ((n_ec && (!off || !count)) || (n_paths && !alpha)) return fail(nullptr, GROOT_E_INVALID, "null argument");
    if (n_boot == 0) return fail(nullptr, GROOT_E_INVALID, "no bootstrap replicates");
    EmDevice em;
    if (int rc = em.check("bootstrap", n_paths, n_ec, off, ids, count, min_iter, max_iter)) return rc;
    const uint32_t ne = em.ne;
    if (ne && em.total == 0) return fail(nullptr, GROOT_E_INVALID, "bootstrap over ECs without reads");
    if (n_draws == 0) n_draws = em.total;
    if (int rc = em.open(device, n_boot, 1)) return rc;
    hipStream_t st = em.st;
    if (em.draw_in_lds && em.draw_lds > 48 * 1024)
        HIP_TRY(nullptr, hipFuncSetAttribute((const void *)boot_resample_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)em.draw_lds));

    constexpr uint64_t kChunkDraws = (uint64_t)kBootDrawBlock * kBootDrawsPerThread;
    const uint64_t draw_chunks = (n_draws + kChunkDraws - 1) / kChunkDraws;
    for (uint32_t b0 = 0; b0 < n_boot; b0 += em.chunk) {
        const uint32_t nb = std::min(em.chunk, n_boot - b0);
        if (ne) {
            HIP_TRY(nullptr, hipMemsetAsync(em.d_cnt.p, 0, (size_t)nb * ne * 8, st));
            if (draw_chunks) {
                BootDrawArgs da{em.d_cum.p, em.d_cnt.p, em.total, n_draws, seed, ne, b0};
                const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(draw_chunks, (kBootDrawGroups + nb - 1) / nb)), nb);
                if (em.draw_in_lds) hipLaunchKernelGGL(boot_resample_kernel<true>, grid, dim3(kBootDrawBlock), em.draw_lds, st, da);
                else hipLaunchKernelGGL(boot_resample_kernel<false>, grid, dim3(kBootDrawBlock), 0, st, da);
                HIP_TRY(nullptr, hipGetLastError());
            }
        }
        if (int rc = em.em_and_fetch(b0, nb, min_iter, max_iter, boot_count, alpha, iterations)) return rc;
    }
    return GROOT_OK;
}

// ---- rarefaction: nested subsamples without replacement, the EM at every depth (kernels_rare.hpp; the contract is in groot_host.h) ----
int groot_hip_em_rarefy(int device, uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t n_rep,
                        uint32_t n_depths, const uint64_t *depths, uint64_t seed, uint32_t min_iter, uint32_t max_iter, uint64_t *rare_count, double *alpha,
                        uint32_t *iterations)
{
    if ((n_ec && (!off || !count)) || (n_paths && !alpha) || (n_depths && !depths)) return fail(nullptr, GROOT_E_INVALID, "null argument");
    if (n_rep == 0) return fail(nullptr, GROOT_E_INVALID, "no rarefaction replicates");
    if (n_depths == 0) return fail(nullptr, GROOT_E_INVALID, "no rarefaction depths");
    EmDevice em;
    if (int rc = em.check("rarefaction", n_paths, n_ec, off, ids, count, min_iter, max_iter)) return rc;
    const uint32_t ne = em.ne;
    if (em.total == 0) return fail(nullptr, GROOT_E_INVALID, "rarefaction over ECs without reads");
    if (em.total >= kRareMaxUnits) return fail(nullptr, GROOT_E_UNSUPPORTED, "rarefaction: 2^62 units and more");
    for (uint32_t d = 0; d < n_depths; d++) {
        if (depths[d] == 0 || depths[d] > em.total)
            return fail(nullptr, GROOT_E_INVALID, "rarefaction depth %u is %llu: not in [1, %llu]", d, (unsigned long long)depths[d], (unsigned long long)em.total);
        if (d && depths[d] < depths[d - 1]) return fail(nullptr, GROOT_E_INVALID, "rarefaction depth %u is below depth %u", d, d - 1);
    }
    // a replicate's depths stay in one chunk (rare_cumsum_kernel adds along them) and in one launch's grid rows
    if (n_depths > 65535 || (uint64_t)n_depths * em.per_vector() > (4ull << 30) || (uint64_t)n_rep * n_depths > 0xFFFFFFFFull)
        return fail(nullptr, GROOT_E_UNSUPPORTED, "rarefaction on the device: %u depths of %zu bytes each", n_depths, em.per_vector());
    if (int rc = em.open(device, (size_t)n_rep * n_depths, n_depths)) return rc;
    hipStream_t st = em.st;
    if (em.draw_in_lds && em.draw_lds > 48 * 1024)
        HIP_TRY(nullptr, hipFuncSetAttribute((const void *)rare_draw_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)em.draw_lds));
    DevBuf<uint64_t> d_depths;
    HIP_TRY(nullptr, d_depths.alloc(n_depths));
    HIP_TRY(nullptr, hipMemcpyAsync(d_depths.p, depths, (size_t)n_depths * 8, hipMemcpyHostToDevice, st));

    // grid.x: the chunks of the longest depth interval, about kBootDrawGroups workgroups a launch (a workgroup past its own interval leaves at once)
    constexpr uint64_t kChunkDraws = (uint64_t)kBootDrawBlock * kBootDrawsPerThread;
    uint64_t longest = depths[0];
    for (uint32_t d = 1; d < n_depths; d++) longest = std::max(longest, depths[d] - depths[d - 1]);
    const uint64_t draw_chunks = (longest + kChunkDraws - 1) / kChunkDraws;
    const uint32_t reps_per_chunk = em.chunk / n_depths, half_bits = rare_half_bits(em.total);
    for (uint32_t b0 = 0; b0 < n_rep; b0 += reps_per_chunk) {
        const uint32_t nb = std::min(reps_per_chunk, n_rep - b0), nv = nb * n_depths;
        HIP_TRY(nullptr, hipMemsetAsync(em.d_cnt.p, 0, (size_t)nv * ne * 8, st));
        RareDrawArgs da{em.d_cum.p, d_depths.p, em.d_cnt.p, em.total, seed, ne, n_depths, b0, half_bits};
        const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(draw_chunks, (kBootDrawGroups + nv - 1) / nv)), nv);
        if (em.draw_in_lds) hipLaunchKernelGGL(rare_draw_kernel<true>, grid, dim3(kBootDrawBlock), em.draw_lds, st, da);
        else hipLaunchKernelGGL(rare_draw_kernel<false>, grid, dim3(kBootDrawBlock), 0, st, da);
        if (n_depths > 1)
            hipLaunchKernelGGL(rare_cumsum_kernel, dim3(grid_for((uint32_t)std::min<uint64_t>((uint64_t)nb * ne, 0xFFFFFFFFull))), dim3(kBlock), 0, st, em.d_cnt.p, nb,
                               n_depths, ne);
        HIP_TRY(nullptr, hipGetLastError());
        if (int rc = em.em_and_fetch((size_t)b0 * n_depths, nv, min_iter, max_iter, rare_count, alpha, iterations)) return rc;
    }
    return GROOT_OK;
}

} // extern "C"

// ---- bootstrap support for the calls (kernels_csup.hpp; the contract is in groot_host.h) -----------------------------------------
namespace {
constexpr uint64_t kCsupBytes = 1ull << 30;          // device memory of one chunk of paths' rows (GROOT_TEST_CSUP_BYTES)
constexpr uint32_t kCsupGroupsPerLaunch = 32;        // groups of kCsupReps replicates in one csup_cover_kernel launch (grid.y)
struct CsupInfo { uint64_t rows = 0; uint32_t width = 0, chunks = 0; };
thread_local CsupInfo tl_csup_info;

template <class T>
int csup_run(hipStream_t st, const std::vector<uint32_t> &chunk_s, const std::vector<uint32_t> &path_row, const std::vector<uint64_t> &row_base,
             const std::vector<uint32_t> &row_t, CsupFillArgs fa, CsupCoverArgs ca, uint32_t nb, size_t max_entries)
{
    DevBuf<T> d;
    HIP_TRY(nullptr, d.alloc(max_entries));
    for (size_t c = 0; c + 1 < chunk_s.size(); c++) {
        const uint32_t s0 = chunk_s[c], s1 = chunk_s[c + 1], r0 = path_row[s0], r1 = path_row[s1];
        const uint64_t base = row_base[r0], entries = row_base[r1] - base;
        if (r1 > r0) {
            HIP_TRY(nullptr, hipMemsetAsync(d.p, 0, entries * sizeof(T), st));
            fa.chunk_base = base; fa.t0 = row_t[r0]; fa.t1 = row_t[r1];
            if (fa.t1 > fa.t0) hipLaunchKernelGGL(csup_fill_kernel<T>, dim3(grid_for(fa.t1 - fa.t0)), dim3(kBlock), 0, st, fa, d.p);
            hipLaunchKernelGGL(csup_scan_kernel<T>, dim3(grid_for(std::min<uint64_t>((uint64_t)(r1 - r0) * 64, 0xFFFFFFFFull))), dim3(kBlock), 0, st, fa.row_base, base,
                               r0, r1, d.p);
        }
        ca.chunk_base = base; ca.s0 = s0;
        const uint32_t groups = (nb + kCsupReps - 1) / kCsupReps;
        for (uint32_t g0 = 0; g0 < groups; g0 += kCsupGroupsPerLaunch) {
            ca.g0 = g0;
            hipLaunchKernelGGL((csup_cover_kernel<T, kCsupReps>), dim3(s1 - s0, std::min(kCsupGroupsPerLaunch, groups - g0)), dim3(kBlock), 0, st, ca, d.p);
        }
        HIP_TRY(nullptr, hipGetLastError());
    }
    return GROOT_OK;
}
} // namespace

extern "C" {

void groot_hip_call_support_info(uint64_t *rows, uint32_t *width, uint32_t *chunks)
{
    if (rows) *rows = tl_csup_info.rows;
    if (width) *width = tl_csup_info.width;
    if (chunks) *chunks = tl_csup_info.chunks;
}

int groot_hip_call_support(int device, uint32_t n_paths, const uint32_t *path_len, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                           uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, uint32_t n_boot, const uint64_t *boot_count, const double *alpha,
                           double call_depth, uint32_t n_sel, const uint32_t *sel_paths, uint32_t *covered_out)
{
    tl_csup_info = CsupInfo{};
    if ((n_paths && !path_len) || (n_ec && (!off || !count || !boot_count)) || (n_paths && !alpha) || (n_tuples && (!tuples || !tn)) ||
        (n_sel && (!sel_paths || !covered_out)))
        return fail(nullptr, GROOT_E_INVALID, "null argument");
    if (n_boot == 0) return fail(nullptr, GROOT_E_INVALID, "no bootstrap replicates");
    if (n_ec >= 0xFFFFFFFFull || (n_ec && off[n_ec] >= 0xFFFFFFFFull) || n_tuples >= 0xFFFFFFFFull)
        return fail(nullptr, GROOT_E_UNSUPPORTED, "call support on the device: 2^32 - 1 ECs, listed IDs or tuples and more");
    const uint32_t ne = (uint32_t)n_ec;
    std::vector<uint32_t> ec_off((size_t)ne + 1, 0);
    for (uint32_t e = 0; e < ne; e++) {
        if (off[e + 1] < off[e] || (off[e + 1] > off[e] && !ids)) return fail(nullptr, GROOT_E_INVALID, "EC %u: bad offsets", e);
        if (count[e] == 0) return fail(nullptr, GROOT_E_INVALID, "EC %u has no reads", e);
        for (uint64_t i = off[e]; i < off[e + 1]; i++)
            if (ids[i] >= n_paths || (i > off[e] && ids[i] <= ids[i - 1])) return fail(nullptr, GROOT_E_INVALID, "EC %u: its IDs do not ascend inside the index", e);
        ec_off[e + 1] = (uint32_t)off[e + 1];
    }
    const uint32_t listed = ne ? ec_off[ne] : 0;
    if (ne && off[0] != 0) return fail(nullptr, GROOT_E_INVALID, "EC 0: bad offsets");
    // the selection: sel_of[p] = the path's place in it (a path named twice gets two places: its rows are made twice)
    for (uint32_t s = 0; s < n_sel; s++)
        if (sel_paths[s] >= n_paths) return fail(nullptr, GROOT_E_INVALID, "selected path %u of %u", sel_paths[s], n_paths);
    // the tuples checked, keyed by their listed-ID index (the pair (e, p)), grouped by it
    struct Rec { uint32_t listed, pos, last; uint64_t n; };
    std::vector<Rec> recs(n_tuples);
    std::vector<uint32_t> per_listed((size_t)listed + 1, 0);
    for (uint64_t i = 0; i < n_tuples; i++) {
        const uint32_t e = tuples[4 * i], p = tuples[4 * i + 1], pos = tuples[4 * i + 2], last = tuples[4 * i + 3];
        if (e >= ne) return fail(nullptr, GROOT_E_INVALID, "tuple %llu names EC %u of %u", (unsigned long long)i, e, ne);
        const uint32_t *lo = ids + off[e], *hi = ids + off[e + 1], *at = std::lower_bound(lo, hi, p);
        if (p >= n_paths || at == hi || *at != p) return fail(nullptr, GROOT_E_INVALID, "tuple %llu: path %u is not in EC %u", (unsigned long long)i, p, e);
        if (last >= path_len[p]) return fail(nullptr, GROOT_E_INVALID, "a tuple of path %u ends at %u, the path has %u bases", p, last, path_len[p]);
        recs[i] = Rec{(uint32_t)(at - ids), pos, last, tn[i]};
        per_listed[recs[i].listed + 1]++;
    }
    for (uint32_t j = 0; j < listed; j++) per_listed[j + 1] += per_listed[j];       // tuples of listed ID j: [per_listed[j], per_listed[j + 1]) once sorted
    {
        std::vector<Rec> sorted(recs.size());
        std::vector<uint32_t> at(per_listed.begin(), per_listed.end() - 1);
        for (const Rec &r : recs) sorted[at[r.listed]++] = r;
        recs.swap(sorted);
    }
    // path -> its listed IDs in canonical EC order (the CSR of the bootstrap, holding listed indices)
    std::vector<uint32_t> path_off((size_t)n_paths + 1, 0);
    for (uint32_t j = 0; j < listed; j++) path_off[ids[j] + 1]++;
    for (uint32_t p = 0; p < n_paths; p++) path_off[p + 1] += path_off[p];
    std::vector<uint32_t> path_listed(std::max<uint32_t>(listed, 1u));
    {
        std::vector<uint32_t> at(path_off.begin(), path_off.end() - 1);
        for (uint32_t j = 0; j < listed; j++) path_listed[at[ids[j]]++] = j;
    }
    // rows: per selected path, its (e, p) with tuples, in that order; the tuples laid out row by row
    std::vector<uint32_t> path_row((size_t)n_sel + 1, 0), sel_len(std::max<uint32_t>(n_sel, 1u), 0), row_listed, row_t{0}, t_row, t_pos, t_last;
    std::vector<uint64_t> row_base{0}, t_n;
    uint64_t max_sum = 0;
    for (uint32_t s = 0; s < n_sel; s++) {
        const uint32_t p = sel_paths[s];
        sel_len[s] = path_len[p];
        for (uint32_t k = path_off[p]; k < path_off[p + 1]; k++) {
            const uint32_t j = path_listed[k];
            if (per_listed[j] == per_listed[j + 1]) continue;
            if (row_listed.size() >= 0xFFFFFFFEull || t_row.size() + (per_listed[j + 1] - per_listed[j]) >= 0xFFFFFFFFull)
                return fail(nullptr, GROOT_E_UNSUPPORTED, "call support on the device: 2^32 - 1 rows or tuples and more");
            uint64_t sum = 0;
            for (uint32_t i = per_listed[j]; i < per_listed[j + 1]; i++) {
                t_row.push_back((uint32_t)row_listed.size()); t_pos.push_back(recs[i].pos); t_last.push_back(recs[i].last); t_n.push_back(recs[i].n);
                sum = sum + recs[i].n < sum ? ~0ull : sum + recs[i].n;
            }
            max_sum = std::max(max_sum, sum);
            row_listed.push_back(j);
            row_t.push_back((uint32_t)t_row.size());
            row_base.push_back(row_base.back() + (uint64_t)path_len[p] + 1);
        }
        path_row[s + 1] = (uint32_t)row_listed.size();
    }
    const uint32_t n_rows = (uint32_t)row_listed.size();
    const bool wide = max_sum >= (1ull << 32) || getenv("GROOT_TEST_CSUP_WIDE") != nullptr;
    const size_t width = wide ? 8 : 4;
    uint64_t budget = kCsupBytes;
    if (const char *e = getenv("GROOT_TEST_CSUP_BYTES")) budget = std::max<uint64_t>(strtoull(e, nullptr, 10), 1);
    // chunks of whole paths under the budget
    std::vector<uint32_t> chunk_s{0};
    uint64_t max_entries = 0;
    for (uint32_t s = 0, s0 = 0; s < n_sel; s++) {
        const uint64_t with = row_base[path_row[s + 1]] - row_base[path_row[s0]];
        if (s > s0 && with * width > budget) { chunk_s.push_back(s); s0 = s; }
        max_entries = std::max(max_entries, row_base[path_row[s + 1]] - row_base[path_row[s0]]);
        if (s + 1 == n_sel) chunk_s.push_back(n_sel);
    }
    tl_csup_info = CsupInfo{n_rows, (uint32_t)width, (uint32_t)chunk_s.size() - 1};
    if (n_sel == 0) return GROOT_OK;

    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(nullptr, GROOT_E_DEVICE, "no HIP device");
    if (device < 0 || device >= n_dev) return fail(nullptr, GROOT_E_DEVICE, "device %d of %d", device, n_dev);
    DeviceGuard dg;
    if (hipGetDevice(&dg.prev) != hipSuccess) dg.prev = -1;
    HIP_TRY(nullptr, hipSetDevice(device));
    StreamGuard sg;
    HIP_TRY(nullptr, hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    hipStream_t st = sg.s;

    DevBuf<uint32_t> d_ec_off, d_ec_ids, d_path_row, d_sel_len, d_row_listed, d_t_row, d_t_pos, d_t_last, d_cov;
    DevBuf<uint64_t> d_count, d_row_base, d_t_n;
    DevBuf<unsigned long long> d_bc;
    DevBuf<double> d_alpha, d_f;
    auto up = [&](auto &buf, const auto *src, size_t n) -> hipError_t {
        hipError_t e = buf.alloc(n);
        if (e == hipSuccess && n) e = hipMemcpyAsync(buf.p, src, n * sizeof(*src), hipMemcpyHostToDevice, st);
        return e;
    };
    HIP_TRY(nullptr, up(d_ec_off, ec_off.data(), ec_off.size()));
    HIP_TRY(nullptr, up(d_ec_ids, ids, listed));
    HIP_TRY(nullptr, up(d_count, count, ne));
    HIP_TRY(nullptr, up(d_path_row, path_row.data(), path_row.size()));
    HIP_TRY(nullptr, up(d_sel_len, sel_len.data(), n_sel));
    HIP_TRY(nullptr, up(d_row_listed, row_listed.data(), row_listed.size()));
    HIP_TRY(nullptr, up(d_row_base, row_base.data(), row_base.size()));
    HIP_TRY(nullptr, up(d_t_row, t_row.data(), t_row.size()));
    HIP_TRY(nullptr, up(d_t_pos, t_pos.data(), t_pos.size()));
    HIP_TRY(nullptr, up(d_t_last, t_last.data(), t_last.size()));
    HIP_TRY(nullptr, up(d_t_n, t_n.data(), t_n.size()));

    // replicates in chunks that bound the device memory of counts, alpha, f and covered (as the bootstrap's)
    const size_t per_rep = ((size_t)ne + n_paths + listed) * 8 + (size_t)n_sel * 4;
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>({(size_t)n_boot, (size_t)65535, kBootChunkBytes / std::max<size_t>(per_rep, 1)}));
    HIP_TRY(nullptr, d_bc.alloc((size_t)chunk * ne));
    HIP_TRY(nullptr, d_alpha.alloc((size_t)chunk * n_paths));
    HIP_TRY(nullptr, d_f.alloc((size_t)chunk * listed));
    HIP_TRY(nullptr, d_cov.alloc((size_t)chunk * n_sel));
    for (uint32_t b0 = 0; b0 < n_boot; b0 += chunk) {
        const uint32_t nb = std::min(chunk, n_boot - b0);
        if (ne) HIP_TRY(nullptr, hipMemcpyAsync(d_bc.p, boot_count + (size_t)b0 * ne, (size_t)nb * ne * 8, hipMemcpyHostToDevice, st));
        if (n_paths) HIP_TRY(nullptr, hipMemcpyAsync(d_alpha.p, alpha + (size_t)b0 * n_paths, (size_t)nb * n_paths * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(nullptr, hipMemsetAsync(d_cov.p, 0, (size_t)nb * n_sel * 4, st));
        if (ne) {
            CsupWeightArgs wa{d_ec_off.p, d_ec_ids.p, d_count.p, d_bc.p, d_alpha.p, d_f.p, ne, n_paths, nb};
            hipLaunchKernelGGL(csup_weight_kernel, dim3(grid_for((uint32_t)std::min<uint64_t>((uint64_t)nb * ne, 0xFFFFFFFFull))), dim3(kBlock), 0, st, wa);
            HIP_TRY(nullptr, hipGetLastError());
        }
        CsupFillArgs fa{d_t_row.p, d_t_pos.p, d_t_last.p, d_t_n.p, d_row_base.p, 0, 0, 0};
        CsupCoverArgs ca{d_path_row.p, d_sel_len.p, d_row_listed.p, d_row_base.p, d_f.p, d_cov.p, 0, listed, call_depth, 0, n_sel, nb, 0};
        if (int rc = wide ? csup_run<uint64_t>(st, chunk_s, path_row, row_base, row_t, fa, ca, nb, max_entries)
                          : csup_run<uint32_t>(st, chunk_s, path_row, row_base, row_t, fa, ca, nb, max_entries))
            return rc;
        HIP_TRY(nullptr, hipMemcpyAsync(covered_out + (size_t)b0 * n_sel, d_cov.p, (size_t)nb * n_sel * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(nullptr, hipStreamSynchronize(st));
    }
    return GROOT_OK;
}

} // extern "C"
