// rescue.hip -- the rescue family behind every batch's order stage, and its C ABI (include/groot_hip.h): mismatch rescue
// (kernels_rescue.hpp), gapped rescue (kernels_gap.hpp), rescued reads in the equivalence classes (kernels_rescue_ec.hpp) and in assigned
// coverage (kernels_rescue_acov.hpp), rescued mates in the fragments' units (kernels_rescue_pairs.hpp) and in assigned coverage over
// fragments (kernels_rescue_acov_pairs.hpp), gap-placed reads in the classes (kernels_gap_ec.hpp) and in assigned coverage (kernels_gap_acov.hpp),
// rescued records (kernels_rescue_rec.hpp) and gapped records (kernels_gap_rec.hpp).  One of the seven translation units of
// libgroot_hip.so (launch.hpp); counters.hip calls the hooks of rescue.hpp, everything else here is internal.
#include <cstring>   // before rocprim: its texture iterator calls host memset

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstddef>
#include <tuple>
#include <vector>

#include "ctx.hpp"
#include "index_tables.hpp"
#include "rescue.hpp"
#include "rescue_fold.hpp"
// The family's kernels build on the types and device functions of these four headers, whose own __global__ functions are counters.hip's
// (one unit per __global__ function, and a kernel is emitted wherever it is defined).  This unit launches none of them, so it reads them
// as plain device functions that nothing calls: none is emitted here, and no host stub collides with counters.hip's.
#pragma push_macro("__global__")
#pragma push_macro("__launch_bounds__")
#undef __global__
#undef __launch_bounds__
#define __global__ static __device__
#define __launch_bounds__(...)
#include "kernels_cov.hpp"
#include "kernels_shared.hpp"
#include "kernels_ec.hpp"
#include "kernels_acov.hpp"
#pragma pop_macro("__launch_bounds__")
#pragma pop_macro("__global__")
#include "kernels_gap.hpp"
#include "kernels_rescue.hpp"
#include "kernels_rescue_ec.hpp"
#include "kernels_rescue_pairs.hpp"
#include "kernels_rescue_acov.hpp"
#include "kernels_rescue_acov_pairs.hpp"
#include "kernels_rescue_rec.hpp"
#include "kernels_gap_rec.hpp"
#include "kernels_gap_ec.hpp"
#include "kernels_gap_acov.hpp"

using namespace groot;

// every switch of the family: a ctx, nothing in flight, the ctx's device current
static int switchable(groot_ctx *c, const char *what)
{
    if (!c) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "%s can only be switched while nothing is in flight", what);
    HIP_TRY(c, hipSetDevice(c->device));
    return GROOT_OK;
}

// a part's device counters behind a drain; all zero while the part is off
template <size_t N> static int part_stats(groot_ctx *c, bool on, const DevBuf<unsigned long long> &b, uint64_t (&st)[N])
{
    std::fill(st, st + N, 0);
    if (!on) return GROOT_OK;
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemcpy(st, b.p, sizeof(st), hipMemcpyDeviceToHost));
    return GROOT_OK;
}

// ---- what goes off with what ----
// gap-placed reads in the equivalence classes go off (with gapped rescue, or with the rescued reads in the classes)
static void gec_release(Counters &k)
{
    k.gec_e.release(); k.gec_stats.release();
    k.gec_on = false; k.gec_slow = 0;
    // (and with it the gap-placed reads in assigned coverage, which are keyed by these classes)
    k.gac_cand_ser.release(); k.gac_stats.release();
    k.gac_on = false; k.gac_host_records = k.gac_host_placements = 0;
}

namespace groot {
// rescued mates in assigned coverage over fragments go off (with the rescued mates' rule, or with assigned coverage)
void rescue_acov_pairs_release(Counters &k)
{
    k.rap_cand_ser.release(); k.rap_fclass.release(); k.rap_stats.release();
    k.rap_on = false; k.rap_log_cap = 0;
    std::fill(k.rap_host, k.rap_host + 4, 0);
}

// rescued reads in the equivalence classes go off (with mismatch rescue, or with the classes): nothing of it stays on the device
void rescue_ec_release(Counters &k)
{
    gec_release(k);                        // (the gap-placed reads' rows go through the rescued reads' table and merge)
    k.rec_path_bit.release(); k.rec_dstar.release(); k.rec_stats.release();
    k.rec_on = false; k.rec_rows = k.rec_bw = 0; k.rec_slow = 0;
    // (and with it the rule that lets them stand beside pairing; pairing itself stays)
    k.rp_state.release(); k.rp_stats.release();
    k.rp_on = false;
    rescue_acov_pairs_release(k);          // (and with the rule its part of assigned coverage over fragments; that table itself stays)
    // (and with it the rescued reads in assigned coverage, which are keyed by these classes)
    k.rac_cand_ser.release(); k.rac_stats.release();
    k.rac_on = false; k.rac_log_cap = 0; k.rac_host_records = 0;
}
} // namespace groot

static void gap_release(Counters &k)
{
    for (auto *b : {&k.gap_cand, &k.gap_ncand}) b->release();
    for (auto *b : {&k.gap_starts, &k.gap_ends, &k.gap_key, &k.gap_cnt, &k.gap_stats}) b->release();
    k.gap_on = false; k.gap_g = 0; k.gap_slots = 0;
}

static hipError_t gap_zero(Counters &k)
{
    if (!k.gap_on) return hipSuccess;
    const uint64_t slots = std::max<uint64_t>(k.h_cov_base.back(), 1);
    hipError_t e = hipMemset(k.gap_starts.p, 0, slots * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(k.gap_ends.p, 0, slots * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(k.gap_key.p, 0, k.gap_slots * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(k.gap_cnt.p, 0, k.gap_slots * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(k.gap_stats.p, 0, kGapStats * sizeof(unsigned long long));
    return e;
}

static void rescue_release(Counters &k)
{
    gap_release(k);                        // (gapped rescue looks at what rescue leaves: off with it)
    rescue_ec_release(k);                  // (and so do the rescued reads in the equivalence classes)
    for (auto *b : {&k.res_text, &k.res_tag, &k.res_cand, &k.res_ncand}) b->release();
    for (auto *b : {&k.res_rbuf, &k.res_starts, &k.res_ends, &k.res_alt, &k.res_stats}) b->release();
    k.res_path.release(); k.res_tab.release(); k.res_occ.release(); k.res_base.release();
    k.res_on = false; k.res_m = 0; k.res_rcap = 0;
}

static hipError_t rescue_zero(Counters &k)
{
    const uint64_t slots = std::max<uint64_t>(k.h_cov_base.back(), 1);
    hipError_t e = hipMemset(k.res_starts.p, 0, slots * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(k.res_ends.p, 0, slots * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(k.res_alt.p, 0, 4 * slots * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(k.res_stats.p, 0, kRescueStats * sizeof(unsigned long long));
    if (e == hipSuccess) e = gap_zero(k);  // (derived from the same reads)
    return e;
}

// ---- rescued records (kernels_rescue_rec.hpp) and gapped records (kernels_gap_rec.hpp): one implementation, told apart by these two ----
static_assert(sizeof(groot_rescue_record) == kRescueRecWords * sizeof(uint32_t) && offsetof(groot_rescue_record, mm) == 12 && offsetof(groot_rescue_record, strand) == 18 &&
              offsetof(groot_rescue_record, d) == 19, "rescue_rec_emit_kernel writes groot_rescue_record as five dwords");
static_assert(sizeof(groot_gap_record) == kGapRecWords * sizeof(uint32_t) && offsetof(groot_gap_record, k) == 12 && offsetof(groot_gap_record, mm) == 14 &&
              offsetof(groot_gap_record, strand) == 20 && offsetof(groot_gap_record, d) == 21 && offsetof(groot_gap_record, type) == 22 &&
              offsetof(groot_gap_record, g) == 23, "gap_rec_emit_kernel writes groot_gap_record as six dwords");

namespace {
struct Rescued {
    using Rec = groot_rescue_record;
    static constexpr uint32_t kWords = kRescueRecWords;
    static constexpr const char *kNoun = "rescued records", *kEnable = "groot_hip_rescue_rec_enable";
    static RecStream &of(Counters &k) { return k.rr; }
    static SlotRecStream<Rec> &of(SlotCounters &s) { return s.rr; }
    static uint64_t &total(CounterStatus &h) { return h.rr_total; }
};
struct Gapped {
    using Rec = groot_gap_record;
    static constexpr uint32_t kWords = kGapRecWords;
    static constexpr const char *kNoun = "gapped records", *kEnable = "groot_hip_gap_rec_enable";
    static RecStream &of(Counters &k) { return k.gr; }
    static SlotRecStream<Rec> &of(SlotCounters &s) { return s.gr; }
    static uint64_t &total(CounterStatus &h) { return h.gr_total; }
};
struct KeptToU64 {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};
} // namespace

// ahead of the kernel that leaves the kept placements: the slot's buffers (there since enable, but for a slot that is newer)
template <class K> static int recs_reserve(groot_ctx *c, Slot *s)
{
    HIP_TRY(c, K::of(s->ct).d_rec.reserve((size_t)K::of(c->ct).slots * K::kWords));
    HIP_TRY(c, K::of(s->ct).d_total.reserve(1));
    HIP_TRY(c, s->ct.h_status.reserve(1));
    return GROOT_OK;
}

// Behind that kernel on the tail stream: every read's segment by a scan over the reads' kept placements; its last output is the batch's
// total, which stays with the slot.  The emit kernel follows, and the two count as the stream's launches.
template <class K> static int recs_scan(groot_ctx *c, Slot *s)
{
    RecStream &r = K::of(c->ct);
    const size_t n = (size_t)s->n_reads + 1;
    auto in = rocprim::make_transform_iterator(r.kept.p, KeptToU64());
    size_t tmp_bytes = 0;
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, tmp_bytes, in, r.off.p, (uint64_t)0, n, rocprim::plus<uint64_t>(), c->tstream));
    if (tmp_bytes > c->scan_tmp.n) {
        HIP_TRY(c, hipStreamSynchronize(c->tstream));
        HIP_TRY(c, c->scan_tmp.alloc(tmp_bytes + tmp_bytes / 4));
    }
    HIP_TRY(c, rocprim::exclusive_scan(c->scan_tmp.p, tmp_bytes, in, r.off.p, (uint64_t)0, n, rocprim::plus<uint64_t>(), c->tstream));
    HIP_TRY(c, hipMemcpyAsync(K::of(s->ct).d_total.p, r.off.p + s->n_reads, sizeof(uint64_t), hipMemcpyDeviceToDevice, c->tstream));
    r.launches += 2;
    return GROOT_OK;
}

// the batch's total, on the copy-out stream
template <class K> static int recs_fetch(groot_ctx *c, Slot *s)
{
    SlotRecStream<typename K::Rec> &sr = K::of(s->ct);
    if (sr.on && s->n_reads && K::of(c->ct).on && sr.d_total.p)
        HIP_TRY(c, hipMemcpyAsync(&K::total(*s->ct.h_status.p), sr.d_total.p, sizeof(uint64_t), hipMemcpyDeviceToHost, c->d2h_stream));
    return GROOT_OK;
}

// At collect: as many records as the batch has, into the slot's pinned memory.  A batch with more than the slot has room for fails alone
// (its other results, the other kind's records among them, stay readable).  refetch: the total enqueue copied is that of the skipped pass.
template <class K> static int recs_collect(groot_ctx *c, Slot *s, bool refetch)
{
    RecStream &r = K::of(c->ct);
    SlotRecStream<typename K::Rec> &sr = K::of(s->ct);
    sr.n = 0;
    if (!sr.on || !s->n_reads || !sr.d_total.p || !r.on) return GROOT_OK;
    uint64_t &total = K::total(*s->ct.h_status.p);
    if (refetch) HIP_TRY(c, hipMemcpy(&total, sr.d_total.p, sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t n = total;
    if (!n) return GROOT_OK;
    if (n > r.slots) {
        r.failed++;
        if (s->status == GROOT_OK) {
            char buf[256];
            snprintf(buf, sizeof buf, "%s: a batch has %llu records, and a pipeline slot has room for %llu (slots_per_batch of %s)", K::kNoun, (unsigned long long)n,
                     (unsigned long long)r.slots, K::kEnable);
            s->status = GROOT_E_NOSPACE;
            s->status_msg = buf;
        }
        return GROOT_OK;
    }
    HIP_TRY(c, sr.h_rec.reserve(n + n / 4));
    HIP_TRY(c, hipMemcpy(sr.h_rec.p, sr.d_rec.p, n * sizeof(typename K::Rec), hipMemcpyDeviceToHost));
    sr.n = n;
    r.records += n;
    const typename K::Rec *h = sr.h_rec.p;
    for (uint64_t i = 0; i < n; i++) r.reads += i == 0 || h[i].read != h[i - 1].read;
    return GROOT_OK;
}

// off: the ctx's work space, every slot's records and the counts since enable (the launches stay)
template <class K> static void recs_release(groot_ctx *c)
{
    RecStream &r = K::of(c->ct);
    r.kept.release(); r.off.release(); r.aux.release();
    for (auto &s : c->slots) {
        SlotRecStream<typename K::Rec> &sr = K::of(s->ct);
        sr.d_rec.release(); sr.d_total.release(); sr.h_rec.release();
        sr.on = false; sr.n = 0;
    }
    r.on = false; r.slots = 0;
    r.records = r.reads = r.failed = 0;
}

// unsupported / state: why the stream cannot come on now (null: it can), looked at once it is known that it is to come on
template <class K> static int recs_enable(groot_ctx *c, uint64_t slots_per_batch, const char *unsupported, const char *state)
{
    if (int rc = switchable(c, K::kNoun)) return rc;
    RecStream &r = K::of(c->ct);
    if (!slots_per_batch) {
        recs_release<K>(c);
        return GROOT_OK;
    }
    if (unsupported) return fail(c, GROOT_E_UNSUPPORTED, "%s", unsupported);
    if (state) return fail(c, GROOT_E_STATE, "%s", state);
    if (slots_per_batch > (1ull << 40) / sizeof(typename K::Rec)) return fail(c, GROOT_E_INVALID, "%s: slots_per_batch %llu is beyond 2^40 bytes", K::kNoun, (unsigned long long)slots_per_batch);
    if (r.on && slots_per_batch == r.slots) return GROOT_OK;
    recs_release<K>(c);
    const size_t R = std::max<uint32_t>(c->prm.max_batch_reads, 1u);
    hipError_t e = r.kept.alloc(R + 1);
    if (e == hipSuccess) e = r.off.alloc(R + 1);
    if (e == hipSuccess) e = r.aux.alloc(R);
    for (auto &s : c->slots) {             // (now, and not at the first launch: no room is an error of this call)
        if (e == hipSuccess) e = K::of(s->ct).d_rec.alloc((size_t)slots_per_batch * K::kWords);
        if (e == hipSuccess) e = K::of(s->ct).d_total.alloc(1);
    }
    if (e != hipSuccess) {
        recs_release<K>(c);
        return fail(c, GROOT_E_DEVICE, "%s: %s", K::kNoun, hipGetErrorString(e));
    }
    r.slots = slots_per_batch;
    r.on = true;
    return GROOT_OK;
}

template <class K, class Stats> static int recs_stats(groot_ctx *c, Stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    const RecStream &r = K::of(c->ct);
    out->records = r.on ? r.records : 0; out->reads = r.on ? r.reads : 0; out->failed = r.on ? r.failed : 0;
    out->slots = r.on ? r.slots : 0;
    out->launches = r.launches;
    return GROOT_OK;
}

// ---- the family's slow reads in the classes and in assigned coverage, at collect (rescue_fold.hpp) ----
// Two kinds of entries share one buffer of the slot, the rescued reads' (h_r of them, counted at d_r) ahead of the gap-rescued reads' (h_g,
// d_g): a batch that needs more than cap fails before either kind is folded.  (More of the first kind alone than cap: rec_collect says so,
// in its own words.)  refetch: the copies enqueue made are stale (the batch was redone).
static int shared_room(groot_ctx *c, bool refetch, uint32_t &h_r, const uint32_t *d_r, uint32_t &h_g, const uint32_t *d_g, uint32_t cap, const char *msg)
{
    if (!d_g || !d_r) return GROOT_OK;     // (launched before the feature came on)
    if (refetch) {
        HIP_TRY(c, hipMemcpy(&h_r, d_r, sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(&h_g, d_g, sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (h_r <= cap && (uint64_t)h_r + h_g > cap) return fail(c, GROOT_E_NOSPACE, msg, h_r, h_g, cap);
    return GROOT_OK;
}

// n bitmaps from row r0 of the slot's pool, each as an ascending ID list into ec_host, the way ec_collect folds the exact slow reads, and
// n_log entries (bitmap row [| second], path, Pos, last) from entry l0 of its log into acov_host under the list of the entry's bitmap
static int fold_slow(groot_ctx *c, Slot *s, uint32_t r0, uint32_t n, uint32_t l0, uint32_t n_log, uint32_t second, uint64_t &slow, uint64_t &records, uint64_t &placements,
                     const char *bad_entry)
{
    Counters &k = c->ct;
    std::vector<uint64_t> bits((size_t)n * k.rec_bw);
    std::vector<uint4> log(n_log);
    HIP_TRY(c, hipMemcpy(bits.data(), s->ct.d_rec_bits.p + (size_t)r0 * k.rec_bw, bits.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (n_log) HIP_TRY(c, hipMemcpy(log.data(), s->ct.d_rac_log.p + l0, log.size() * sizeof(uint4), hipMemcpyDeviceToHost));
    const auto rows = unfold_rows(bits.data(), n, k.rec_bw, (uint32_t)k.h_len.size(), k.ec_host, slow);
    const int64_t bad = fold_log(log.data(), log.size(), rows, second, k.acov_host, records, placements);
    return bad < 0 ? GROOT_OK : fail(c, GROOT_E_DEVICE, bad_entry, (uint32_t)bad, n);
}

// The batch's slow rescued reads, and (rescued reads in assigned coverage) the log of their kept placements; both counts are checked
// before anything is folded.
static int rec_collect(groot_ctx *c, Slot *s, bool refetch)
{
    Counters &k = c->ct;
    if (!s->ct.d_rec_slow.p) return GROOT_OK;      // (launched before the feature came on)
    CounterStatus &h = *s->ct.h_status.p;
    if (refetch) HIP_TRY(c, hipMemcpy(&h.rec_slow, s->ct.d_rec_slow.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (!h.rec_slow) return GROOT_OK;
    if (h.rec_slow > k.rec_rows && k.rp_on) {      // the batch fails alone: the device counted nothing of it (rescue_pair_insert_kernel), and the ctx goes on
        if (s->status == GROOT_OK) {
            char buf[256];
            snprintf(buf, sizeof buf, "rescued mates in paired-end units: a batch's units that fit no row need %u bitmaps, and there is room for %u "
                     "(GROOT_TEST_RESCUE_EC_ROWS)", h.rec_slow, k.rec_rows);
            s->status = GROOT_E_NOSPACE;
            s->status_msg = buf;
        }
        return GROOT_OK;
    }
    if (k.rap_on && s->ct.d_rac_nlog.p) {  // rescued mates in assigned coverage over fragments: the fragments on bitmaps have their records in the log
        if (refetch) HIP_TRY(c, hipMemcpy(&h.rac_log, s->ct.d_rac_nlog.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (h.rac_log > k.rap_log_cap) {   // the batch fails alone, as above (rescue_acov_pair_insert_kernel)
            if (s->status == GROOT_OK) {
                char buf[256];
                snprintf(buf, sizeof buf, "rescued mates in assigned coverage over fragments: a batch's fragments that fit no row have %u records, and the log has "
                         "room for %u (GROOT_TEST_RESCUE_ACOV_LOG)", h.rac_log, k.rap_log_cap);
                s->status = GROOT_E_NOSPACE;
                s->status_msg = buf;
            }
            return GROOT_OK;
        }
        std::vector<uint64_t> bits((size_t)h.rec_slow * k.rec_bw);
        std::vector<uint4> log(h.rac_log);
        HIP_TRY(c, hipMemcpy(bits.data(), s->ct.d_rec_bits.p, bits.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (h.rac_log) HIP_TRY(c, hipMemcpy(log.data(), s->ct.d_rac_log.p, log.size() * sizeof(uint4), hipMemcpyDeviceToHost));
        const auto rows = unfold_rows(bits.data(), h.rec_slow, k.rec_bw, (uint32_t)k.h_len.size(), k.ec_host, k.rec_slow);
        const int64_t bad = fold_log_units(log.data(), log.size(), rows, kRapLogExact, k.acov_host, k.rap_host);
        return bad < 0 ? GROOT_OK : fail(c, GROOT_E_DEVICE, "rescued mates in assigned coverage over fragments: a logged record names bitmap %u of %u", (uint32_t)bad, h.rec_slow);
    }
    if (h.rec_slow > k.rec_rows)
        return fail(c, GROOT_E_NOSPACE, "rescued reads in the equivalence classes: a batch has %u rescued reads whose sets lie in more graphs than a row holds, and room for "
                    "the bitmaps of %u (GROOT_TEST_RESCUE_EC_ROWS)", h.rec_slow, k.rec_rows);
    const bool logged = k.rac_on && s->ct.d_rac_nlog.p;
    if (logged && refetch) HIP_TRY(c, hipMemcpy(&h.rac_log, s->ct.d_rac_nlog.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (logged && h.rac_log > k.rac_log_cap)
        return fail(c, GROOT_E_NOSPACE, "rescued reads in assigned coverage: a batch's rescued reads whose sets lie in more graphs than a row holds have %u kept "
                    "placements, and the log has room for %u (GROOT_TEST_RESCUE_ACOV_LOG)", h.rac_log, k.rac_log_cap);
    uint64_t placements = 0;               // (every entry of this log is one)
    return fold_slow(c, s, 0, h.rec_slow, 0, logged ? h.rac_log : 0, 0, k.rec_slow, k.rac_host_records, placements,
                     "rescued reads in assigned coverage: a logged placement names bitmap %u of %u");
}

// Behind rec_collect: the batch's slow gap-rescued reads, whose bitmaps and (gap-placed reads in assigned coverage) log entries lie behind
// the rescued reads'.  (shared_room has brought the counts up to date and found them to fit.)
static int gec_collect(groot_ctx *c, Slot *s)
{
    Counters &k = c->ct;
    if (!s->ct.d_gec_slow.p || !s->ct.d_rec_slow.p) return GROOT_OK;
    const CounterStatus &h = *s->ct.h_status.p;
    if (!h.gec_slow) return GROOT_OK;
    const bool logged = k.gac_on && s->ct.d_gac_nlog.p && s->ct.d_rac_nlog.p;
    return fold_slow(c, s, h.rec_slow, h.gec_slow, h.rac_log, logged ? h.gac_log : 0, kGapAcovSecond, k.gec_slow, k.gac_host_records, k.gac_host_placements,
                     "gap-placed reads in assigned coverage: a logged record names bitmap %u of %u");
}

// the count kernel of a batch: beside the pileup it hands the candidates it leaves unplaced on to gapped rescue (gap), leaves every read's
// kept placements for the rescued records (rr), writes every rescued read's path set as a row for the classes (rec)
static const void *count_kernel(bool gap, bool rr, bool rec)
{
    static const void *const of[8] = {
        (const void *)rescue_count_kernel<false>, (const void *)rescue_count_ec_kernel<false>, (const void *)rescue_count_rec_kernel<false, false>, (const void *)rescue_count_rec_kernel<false, true>,
        (const void *)rescue_count_kernel<true>, (const void *)rescue_count_ec_kernel<true>, (const void *)rescue_count_rec_kernel<true, false>, (const void *)rescue_count_rec_kernel<true, true>};
    return of[4 * gap + 2 * rr + rec];
}

// what every kernel of the family reads of slot s's batch and of the ctx's tables (the parts of rescued and gapped records and of gapped
// rescue are rescue_launch's to add)
static RescueArgs rescue_args(groot_ctx *c, Slot *s, const SharedArgs &sa)
{
    Counters &k = c->ct;
    RescueArgs ra{};
    ra.seq = s->seq(); ra.seq_off = s->off(); ra.ctr = s->d_ctr.p; ra.trav_off = c->trav_off.p;
    ra.rbuf = k.res_rbuf.p; ra.rcap = k.res_rcap; ra.cand = k.res_cand.p; ra.n_cand = k.res_ncand.p;
    ra.text = k.res_text.p; ra.tag = k.res_tag.p; ra.path = k.res_path.p; ra.tab = k.res_tab.p; ra.occ = k.res_occ.p; ra.slot_base = k.res_base.p;
    ra.starts = k.res_starts.p; ra.ends = k.res_ends.p; ra.alt = k.res_alt.p; ra.stats = k.res_stats.p;
    ra.tab_mask = (uint32_t)k.res_tab.n - 1u; ra.n_reads = s->n_reads; ra.max_mismatch = k.res_m;
    if (k.rec_on) {
        ra.path_bit = k.rec_path_bit.p; ra.set_graph = sa.set_graph; ra.set_mask = sa.set_mask; ra.dstar = k.rec_dstar.p;
        ra.pw = sa.pw; ra.max_segs = sa.max_segs;
    }
    return ra;
}

// the rows, the bitmaps and the counts of the rescued reads in the classes, as rescue_launch and rescue_acov_pairs_launch hand them to their kernels
static RescueEcArgs rescue_ec_args(groot_ctx *c, Slot *s, const RescueArgs &ra, const SharedArgs &sa)
{
    Counters &k = c->ct;
    RescueEcArgs ea{};
    ea.r = ra; ea.s = sa; ea.bits = s->ct.d_rec_bits.p; ea.n_slow = s->ct.d_rec_slow.p; ea.stats = k.rec_stats.p;
    ea.rows = k.rec_rows; ea.bw = k.rec_bw;
    return ea;
}

// rescued mates in assigned coverage over fragments: what its kernels on both sides of the merge share
static RescueAcovPairsArgs rescue_acov_pairs_args(groot_ctx *c, Slot *s, const RescueArgs &ra, const SharedArgs &sa)
{
    Counters &k = c->ct;
    RescueAcovPairsArgs p{};
    p.a.e = rescue_ec_args(c, s, ra, sa);
    static_assert(kRapDropped == kRapRescued + kRescueAcovDropped, "rescue_acov_body adds {added, dropped} at stats[0] and stats[kRescueAcovDropped]");
    p.a.tab_ser = k.acov_tab_ser.p; p.a.cand_ser = k.rap_cand_ser.p; p.a.fill = k.acov_fill.p; p.a.stats = k.rap_stats.p + kRapRescued;
    p.a.log = s->ct.d_rac_log.p; p.a.n_log = s->ct.d_rac_nlog.p; p.a.log_cap = k.rap_log_cap;
    p.ix = RapIndex{k.d_np_off.p, k.d_np.p, k.d_len.p};
    p.fclass = k.rap_fclass.p; p.read_ser = s->ct.d_acov_ser.p; p.stats = k.rap_stats.p;
    return p;
}

// ---- the hooks of rescue.hpp -------------------------------------------------------------------------------------------------
namespace groot {

// Everything reads the slot's reads, the order stage's scan -- both the tail stream's until the next batch's order stage -- and the ctx's
// own buffers.  What is on together (the enable and release functions below see to it):
//     gec_on implies gap_on && rec_on;   rac_on implies rec_on;   gac_on implies gec_on && rac_on;   gec_on && rac_on implies gac_on
// so the family's reads go into the classes and into assigned coverage in ONE sequence, each step in its plain or its acov form.
int rescue_launch(groot_ctx *c, Slot *s, const SharedArgs &sa, uint32_t tab)
{
    Counters &k = c->ct;
    if (!k.res_on) return GROOT_OK;
    const dim3 gr(grid_for(s->n_reads)), gt(grid_for(tab)), blk(kBlock);
    RescueArgs ra = rescue_args(c, s, sa);
    HIP_TRY(c, hipMemsetAsync(k.res_ncand.p, 0, sizeof(uint32_t), c->tstream));
    hipLaunchKernelGGL(rescue_pack_kernel, gr, blk, 0, c->tstream, ra);
    // (With the rescued classes on: the rows of the candidates are free, and with the rule of the rescued mates off so is the per-batch table: shared_expand_kernel,
    // launched by counters_launch ahead of this call on this stream, has cleared it.  With that rule on the table still holds the units of the fragments with
    // records on both mates -- the merge waits behind this call -- and their rows are rows of reads with records, which no candidate shares)
    if (k.rr.on) {           // rescued records: the count kernel also leaves every read's kept placements, zero for a read that is no candidate
        ra.n_kept = k.rr.kept.p; ra.rec_d = k.rr.aux.p;
        HIP_TRY(c, hipMemsetAsync(k.rr.kept.p, 0, ((size_t)s->n_reads + 1) * sizeof(uint32_t), c->tstream));
    }
    if (k.gap_on) {
        ra.gcand = k.gap_cand.p; ra.n_gcand = k.gap_ncand.p; ra.gstats = k.gap_stats.p;
        HIP_TRY(c, hipMemsetAsync(k.gap_ncand.p, 0, sizeof(uint32_t), c->tstream));
    }
    void *count_args[] = {&ra};
    HIP_TRY(c, hipLaunchKernel(count_kernel(k.gap_on, k.rr.on, k.rec_on), gr, blk, count_args, 0, c->tstream));
    GapRecArgs gra{};
    if (k.gap_on) {
        GapArgs &ga = gra.g;
        ga.r = ra; ga.gcand = k.gap_cand.p; ga.n_gcand = k.gap_ncand.p;
        ga.starts = k.gap_starts.p; ga.ends = k.gap_ends.p; ga.ev_key = k.gap_key.p; ga.ev_cnt = k.gap_cnt.p; ga.stats = k.gap_stats.p;
        ga.ev_mask = k.gap_slots - 1; ga.max_gap = k.gap_g;
        if (k.gr.on) {       // gapped records: the gap kernel also leaves every read's kept placements and every gap candidate's e*
            if (int rc = recs_reserve<Gapped>(c, s)) return rc;
            gra.n_gkept = k.gr.kept.p; gra.gap_e = k.gr.aux.p; gra.off = k.gr.off.p; gra.rec = s->ct.gr.d_rec.p; gra.cap = k.gr.slots;
            HIP_TRY(c, hipMemsetAsync(k.gr.kept.p, 0, ((size_t)s->n_reads + 1) * sizeof(uint32_t), c->tstream));
        }
        // the gap kernel, chosen here and nowhere else: with the classes on it also writes every gap-rescued read's set row
        if (k.gec_on && k.gr.on) hipLaunchKernelGGL(rescue_gap_ec_kernel<true>, gr, blk, 0, c->tstream, GapEcCountArgs{gra, k.gec_e.p});
        else if (k.gec_on) hipLaunchKernelGGL(rescue_gap_ec_kernel<false>, gr, blk, 0, c->tstream, GapEcCountArgs{gra, k.gec_e.p});
        else if (k.gr.on) hipLaunchKernelGGL(rescue_gap_rec_kernel, gr, blk, 0, c->tstream, gra);
        else hipLaunchKernelGGL(rescue_gap_kernel, gr, blk, 0, c->tstream, ga);
        k.gap_launches++;
    }
    HIP_TRY(c, hipGetLastError());
    k.res_launches += 2;
    if (k.rr.on) {
        if (int rc = recs_reserve<Rescued>(c, s)) return rc;
        if (int rc = recs_scan<Rescued>(c, s)) return rc;
        RescueRecArgs a{};
        a.r = ra; a.off = k.rr.off.p; a.rec = s->ct.rr.d_rec.p; a.cap = k.rr.slots;
        hipLaunchKernelGGL(rescue_rec_emit_kernel, gr, blk, 0, c->tstream, a);
        HIP_TRY(c, hipGetLastError());
    }
    if (k.gap_on && k.gr.on) {
        if (int rc = recs_scan<Gapped>(c, s)) return rc;
        hipLaunchKernelGGL(gap_rec_emit_kernel, gr, blk, 0, c->tstream, gra);
        HIP_TRY(c, hipGetLastError());
    }
    if (!k.rec_on) return GROOT_OK;

    // The family's reads in the classes (ec_reserve of counters_launch has made room for this merge too: its bound is over both), and with
    // rac_on in assigned coverage: claim and add in one pass, here and never at collect.
    const bool rac = k.rac_on, gec = k.gec_on, gac = k.gac_on;
    RescueAcovArgs aa{};
    RescueEcArgs &ea = aa.e;
    GapAcovArgs gaa{};
    HIP_TRY(c, s->ct.d_rec_bits.reserve((size_t)k.rec_rows * k.rec_bw));
    HIP_TRY(c, s->ct.d_rec_slow.reserve(1));
    HIP_TRY(c, hipMemsetAsync(s->ct.d_rec_slow.p, 0, sizeof(uint32_t), c->tstream));
    ea = rescue_ec_args(c, s, ra, sa);
    if (rac) {
        HIP_TRY(c, s->ct.d_rac_log.reserve(std::max<uint32_t>(k.rac_log_cap, 1u)));
        HIP_TRY(c, s->ct.d_rac_nlog.reserve(1));
        HIP_TRY(c, hipMemsetAsync(s->ct.d_rac_nlog.p, 0, sizeof(uint32_t), c->tstream));
        aa.tab_ser = k.acov_tab_ser.p; aa.cand_ser = k.rac_cand_ser.p; aa.fill = k.acov_fill.p; aa.stats = k.rac_stats.p;
        aa.log = s->ct.d_rac_log.p; aa.n_log = s->ct.d_rac_nlog.p; aa.log_cap = k.rac_log_cap;
    }
    if (gac) {               // (the gapped records share the rescued reads' log)
        HIP_TRY(c, s->ct.d_gac_nlog.reserve(1));
        HIP_TRY(c, hipMemsetAsync(s->ct.d_gac_nlog.p, 0, sizeof(uint32_t), c->tstream));
        gaa.tab_ser = k.acov_tab_ser.p; gaa.gcand_ser = k.gac_cand_ser.p; gaa.fill = k.acov_fill.p; gaa.stats = k.gac_stats.p;
        gaa.log = aa.log; gaa.n_rlog = aa.n_log; gaa.n_glog = s->ct.d_gac_nlog.p; gaa.log_cap = k.rac_log_cap;
    }
    if (gec) {               // (the gap-rescued reads' rows go behind the rescued reads', through the same table and merge)
        HIP_TRY(c, s->ct.d_gec_slow.reserve(1));
        HIP_TRY(c, hipMemsetAsync(s->ct.d_gec_slow.p, 0, sizeof(uint32_t), c->tstream));
        gaa.e.g = gra.g; gaa.e.s = sa; gaa.e.e = k.gec_e.p; gaa.e.bits = ea.bits; gaa.e.n_rslow = ea.n_slow; gaa.e.stats = k.gec_stats.p;
        gaa.e.rows = ea.rows; gaa.e.bw = ea.bw; gaa.e.n_gslow = s->ct.d_gec_slow.p;
    }
    if (k.rp_on) {           // rescued mates in paired-end units: every unit that is not exact + exact, a thread per fragment (rac, gec and gac are off beside it)
        RescuePairArgs pa{};
        // (counters_launch has held the merge and the expansion back: the table still holds the exact + exact fragments' units, whose rows no
        // candidate shares, and one merge behind this call folds every unit of the batch -- or none, when the bitmaps do not suffice)
        pa.e = ea; pa.state = k.rp_state.p; pa.total = k.rp_stats.p; pa.stats = k.rp_stats.p + kRescuePairStats; pa.tab_size = tab;
        HIP_TRY(c, hipMemsetAsync(k.rp_state.p, kRescueUnplaced, std::max<uint32_t>(s->n_reads, 1u), c->tstream));
        HIP_TRY(c, hipMemsetAsync(pa.stats, 0, kRescuePairStats * sizeof(unsigned long long), c->tstream));
        hipLaunchKernelGGL(rescue_pair_mark_kernel, gr, blk, 0, c->tstream, pa);
        if (k.rap_on) {      // ... and in assigned coverage over fragments: every fragment's class, and the records of the fragments on bitmaps into the slot's log
            HIP_TRY(c, s->ct.d_rac_log.reserve(std::max<uint32_t>(k.rap_log_cap, 1u)));
            HIP_TRY(c, s->ct.d_rac_nlog.reserve(1));
            HIP_TRY(c, hipMemsetAsync(s->ct.d_rac_nlog.p, 0, sizeof(uint32_t), c->tstream));
            HIP_TRY(c, hipMemsetAsync(k.rap_fclass.p, kRapNone, std::max<uint32_t>(s->n_reads / 2u, 1u), c->tstream));
            const RescueAcovPairSink sink{RapIndex{k.d_np_off.p, k.d_np.p, k.d_len.p}, k.rap_fclass.p, s->ct.d_rac_log.p, s->ct.d_rac_nlog.p, k.rap_log_cap};
            hipLaunchKernelGGL(rescue_acov_pair_kernel, dim3(grid_for(s->n_reads / 2u)), blk, 0, c->tstream, pa, sink);
            hipLaunchKernelGGL(rescue_acov_pair_insert_kernel, dim3(grid_for(std::max(s->n_reads, tab))), blk, 0, c->tstream, pa, s->ct.d_rac_nlog.p, k.rap_log_cap);
        } else {
            hipLaunchKernelGGL(rescue_pair_kernel, dim3(grid_for(s->n_reads / 2u)), blk, 0, c->tstream, pa);
            hipLaunchKernelGGL(rescue_pair_insert_kernel, dim3(grid_for(std::max(s->n_reads, tab))), blk, 0, c->tstream, pa);
        }
        HIP_TRY(c, hipGetLastError());
        k.rp_launches += 3;
        return GROOT_OK;
    }
    if (rac) hipLaunchKernelGGL(rescue_acov_slow_kernel, gr, blk, 0, c->tstream, aa);
    else hipLaunchKernelGGL(rescue_ec_slow_kernel, gr, blk, 0, c->tstream, ea);
    if (gac) hipLaunchKernelGGL(gap_acov_slow_kernel, gr, blk, 0, c->tstream, gaa);
    else if (gec) hipLaunchKernelGGL(gap_ec_slow_kernel, gr, blk, 0, c->tstream, gaa.e);
    hipLaunchKernelGGL(rescue_ec_insert_kernel, gr, blk, 0, c->tstream, ea);
    if (gec) hipLaunchKernelGGL(gap_ec_insert_kernel, gr, blk, 0, c->tstream, gaa.e);
    if (rac) hipLaunchKernelGGL(rescue_acov_merge_kernel, gt, blk, 0, c->tstream, sa, k.ec.table(), tab, ++k.ec_epoch, k.ec_fill.p, k.acov_tab_ser.p);
    else hipLaunchKernelGGL(rescue_ec_merge_kernel, gt, blk, 0, c->tstream, sa, k.ec.table(), tab, ++k.ec_epoch, k.ec_fill.p);
    if (rac) {
        hipLaunchKernelGGL(rescue_acov_serial_kernel, gr, blk, 0, c->tstream, aa);
        if (gac) hipLaunchKernelGGL(gap_acov_serial_kernel, gr, blk, 0, c->tstream, gaa);
        hipLaunchKernelGGL(rescue_acov_clear_kernel, gt, blk, 0, c->tstream, sa, tab);
        hipLaunchKernelGGL(rescue_acov_kernel, gr, blk, 0, c->tstream, aa, k.acov.table());
        if (gac) hipLaunchKernelGGL(gap_acov_kernel, gr, blk, 0, c->tstream, gaa, k.acov.table());
    }
    HIP_TRY(c, hipGetLastError());
    k.rec_launches += 3;
    if (rac) k.rac_launches += 3;
    if (gec) k.gec_launches += 2;
    if (gac) k.gac_launches += 4;
    return GROOT_OK;
}

// Behind ec_merge_kernel<true> and acov_serial_paired_kernel, ahead of the ordinary count and of shared_expand_kernel<true>: the unit rows and
// the per-batch table are live, tab_ser[] holds the units' serials.  One pass, here and never at collect.
int rescue_acov_pairs_launch(groot_ctx *c, Slot *s, const SharedArgs &sa)
{
    Counters &k = c->ct;
    if (!k.rap_on) return GROOT_OK;
    const RescueAcovPairsArgs p = rescue_acov_pairs_args(c, s, rescue_args(c, s, sa), sa);
    const dim3 gr(grid_for(s->n_reads)), blk(kBlock);
    hipLaunchKernelGGL(rescue_acov_pairs_serial_kernel, gr, blk, 0, c->tstream, p);
    hipLaunchKernelGGL(rescue_acov_pairs_exact_kernel, dim3(grid_for(s->n_reads / 2u)), blk, 0, c->tstream, p, k.acov.table());
    hipLaunchKernelGGL(rescue_acov_pairs_kernel, gr, blk, 0, c->tstream, p, k.acov.table());
    HIP_TRY(c, hipGetLastError());
    k.rap_launches += 3;
    return GROOT_OK;
}

int rescue_fetch(groot_ctx *c, Slot *s)
{
    const Counters &k = c->ct;
    if (int rc = recs_fetch<Rescued>(c, s)) return rc;
    if (int rc = recs_fetch<Gapped>(c, s)) return rc;
    CounterStatus *h = s->ct.h_status.p;    // (the classes' words: rec_on, and so the classes, are on with each of the four)
    if (k.rec_on) HIP_TRY(c, hipMemcpyAsync(&h->rec_slow, s->ct.d_rec_slow.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
    if (k.gec_on && s->ct.d_gec_slow.p) HIP_TRY(c, hipMemcpyAsync(&h->gec_slow, s->ct.d_gec_slow.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
    if (k.rac_on || k.rap_on) HIP_TRY(c, hipMemcpyAsync(&h->rac_log, s->ct.d_rac_nlog.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
    if (k.gac_on && s->ct.d_gac_nlog.p) HIP_TRY(c, hipMemcpyAsync(&h->gac_log, s->ct.d_gac_nlog.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
    return GROOT_OK;
}

int rescue_collect_records(groot_ctx *c, Slot *s, bool redone)
{
    if (int rc = recs_collect<Rescued>(c, s, redone)) return rc;
    return recs_collect<Gapped>(c, s, redone);
}

int rescue_collect_classes(groot_ctx *c, Slot *s, bool redone)
{
    Counters &k = c->ct;
    if (!k.rec_on) return GROOT_OK;
    CounterStatus &h = *s->ct.h_status.p;
    if (k.gec_on)            // the two kinds share the slot's bitmaps
        if (int rc = shared_room(c, redone, h.rec_slow, s->ct.d_rec_slow.p, h.gec_slow, s->ct.d_gec_slow.p, k.rec_rows,
                                 "gap-placed reads in the equivalence classes: a batch has %u rescued and %u gap-rescued reads whose sets lie in more graphs than a row "
                                 "holds, and room for the bitmaps of %u (GROOT_TEST_RESCUE_EC_ROWS)"))
            return rc;
    if (k.gac_on)            // ... and the slot's log
        if (int rc = shared_room(c, redone, h.rac_log, s->ct.d_rac_nlog.p, h.gac_log, s->ct.d_gac_nlog.p, k.rac_log_cap,
                                 "gap-placed reads in assigned coverage: a batch's rescued and gap-rescued reads whose sets lie in more graphs than a row holds have "
                                 "%u kept placements and %u gapped records, and the log has room for %u (GROOT_TEST_RESCUE_ACOV_LOG)"))
            return rc;
    if (int rc = rec_collect(c, s, redone)) return rc;
    return k.gec_on ? gec_collect(c, s) : GROOT_OK;
}

int rescue_ec_reset(groot_ctx *c)
{
    Counters &k = c->ct;                   // (the rescued and the gap-placed reads are counted with the classes they are in)
    if (k.rec_on) HIP_TRY(c, hipMemset(k.rec_stats.p, 0, kRescueEcStats * sizeof(unsigned long long)));
    if (k.gec_on) HIP_TRY(c, hipMemset(k.gec_stats.p, 0, kGapEcStats * sizeof(unsigned long long)));
    if (k.rp_on) HIP_TRY(c, hipMemset(k.rp_stats.p, 0, kRescuePairStats * sizeof(unsigned long long)));
    k.rec_slow = k.gec_slow = 0;           // (zero anyway while the part is off)
    return GROOT_OK;
}

int rescue_acov_reset(groot_ctx *c)
{
    Counters &k = c->ct;                   // (the rescued and the gapped records are counted with the table they are in)
    if (k.rac_on) HIP_TRY(c, hipMemset(k.rac_stats.p, 0, kRescueAcovStats * sizeof(unsigned long long)));
    if (k.gac_on) HIP_TRY(c, hipMemset(k.gac_stats.p, 0, kGapAcovStats * sizeof(unsigned long long)));
    k.rac_host_records = k.gac_host_records = k.gac_host_placements = 0;
    if (k.rap_on) HIP_TRY(c, hipMemset(k.rap_stats.p, 0, kRescueAcovPairStats * sizeof(unsigned long long)));
    std::fill(k.rap_host, k.rap_host + 4, 0);
    return GROOT_OK;
}

int rescue_acov_dropped(groot_ctx *c)
{
    const Counters &k = c->ct;
    uint64_t rst[kRescueAcovStats] = {}, gst[kGapAcovStats] = {};
    if (k.rac_on) HIP_TRY(c, hipMemcpy(rst, k.rac_stats.p, sizeof(rst), hipMemcpyDeviceToHost));
    if (k.gac_on) HIP_TRY(c, hipMemcpy(gst, k.gac_stats.p, sizeof(gst), hipMemcpyDeviceToHost));
    if (k.rap_on) {
        uint64_t pst[kRescueAcovPairStats];
        HIP_TRY(c, hipMemcpy(pst, k.rap_stats.p, sizeof(pst), hipMemcpyDeviceToHost));
        if (pst[kRapDropped])
            return fail(c, GROOT_E_NOSPACE, "assigned coverage: %llu records of fragments with a rescued mate found no room in a table of %u slots, which grows between "
                        "batches only: start it larger (min_slots of groot_hip_rescue_acov_pairs_enable, align --callSlots)", (unsigned long long)pst[kRapDropped], k.acov.cap);
    }
    const bool res = rst[kRescueAcovDropped] != 0;      // (the rescued records' count first, as ever)
    if (res || gst[kGapAcovDropped])
        return fail(c, GROOT_E_NOSPACE, "assigned coverage: %llu %s records found no room in a table of %u slots, which grows between batches only: start it "
                    "larger (min_slots of groot_hip_rescue_acov_enable, align --callSlots)", (unsigned long long)(res ? rst[kRescueAcovDropped] : gst[kGapAcovDropped]),
                    res ? "rescued" : "gapped", k.acov.cap);
    return GROOT_OK;
}

bool rescue_on(const groot_ctx *c) { return c->ct.res_on; }

} // namespace groot

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

// ---- mismatch rescue (kernels_rescue.hpp) --------------------------------------------------------------------------------
int groot_hip_rescue_enable(groot_ctx *c, const groot_index_view *idx, uint32_t max_mismatch)
{
    if (int rc = switchable(c, "mismatch rescue")) return rc;
    if (max_mismatch > kRescueMaxMismatch) return fail(c, GROOT_E_INVALID, "mismatch rescue: %u mismatches, at most %u are supported", max_mismatch, kRescueMaxMismatch);
    Counters &k = c->ct;
    if (!max_mismatch) {
        recs_release<Rescued>(c);                     // (the rescued records are rescue's placements: off with it)
        recs_release<Gapped>(c);                     // (and the gapped records gapped rescue's, which goes off below)
        rescue_release(k);
        return GROOT_OK;
    }
    if (k.asg_on) return fail(c, GROOT_E_UNSUPPORTED, "mismatch rescue tells the unaligned reads by their records, which assignment rewrites (groot_hip_assign_enable)");
    const bool same_index = idx && idx->n_paths == k.h_len.size() && (size_t)idx->n_nodes + 1 == k.h_np_off.size() && std::equal(k.h_len.begin(), k.h_len.end(), idx->path_len);
    if (idx && !same_index) return fail(c, GROOT_E_INVALID, "mismatch rescue: not the index the ctx was opened with");
    if (k.res_on) {                        // another M: the tables do not depend on it, the counts do
        if (max_mismatch != k.res_m) {
            hipError_t e = rescue_zero(k);
            if (e != hipSuccess) return fail(c, GROOT_E_DEVICE, "mismatch rescue: %s", hipGetErrorString(e));
            k.res_m = max_mismatch;
        }
        return GROOT_OK;
    }
    if (!idx) return fail(c, GROOT_E_INVALID, "mismatch rescue: the tables are built from the index the ctx was opened with, and none was given");
    RescueTables rt;
    if (!build_rescue_tables(idx, rt))
        return fail(c, GROOT_E_UNSUPPORTED, "mismatch rescue: path texts of %zu bases are beyond 32-bit bit offsets", rt.n_bases);
    const uint64_t slots = k.h_cov_base.back(), R = std::max<uint32_t>(c->prm.max_batch_reads, 1u);
    k.res_rcap = c->prm.max_batch_bases / 32 + R + 2;
    hipError_t e = upload(k.res_text, rt.text.data(), rt.text.size());
    if (e == hipSuccess) e = upload(k.res_tag, rt.tag.data(), rt.tag.size());
    if (e == hipSuccess) e = upload(k.res_path, rt.path.data(), rt.path.size());
    if (e == hipSuccess) e = upload(k.res_tab, rt.tab.data(), rt.tab.size());
    if (e == hipSuccess) e = upload(k.res_occ, rt.occ.data(), rt.occ.size());
    if (e == hipSuccess) e = upload(k.res_base, k.h_cov_base.data(), k.h_cov_base.size());
    if (e == hipSuccess) e = k.res_rbuf.alloc(2 * k.res_rcap);
    if (e == hipSuccess) e = k.res_cand.alloc(R);
    if (e == hipSuccess) e = k.res_ncand.alloc(1);
    if (e == hipSuccess) e = k.res_starts.alloc(slots);
    if (e == hipSuccess) e = k.res_ends.alloc(slots);
    if (e == hipSuccess) e = k.res_alt.alloc(4 * slots);
    if (e == hipSuccess) e = k.res_stats.alloc(kRescueStats);
    if (e == hipSuccess) e = rescue_zero(k);
    if (e != hipSuccess) {
        rescue_release(k);
        return fail(c, GROOT_E_DEVICE, "mismatch rescue: %s", hipGetErrorString(e));
    }
    k.res_text_paths = rt.n_text_paths;
    k.res_m = max_mismatch;
    k.res_on = true;
    return GROOT_OK;
}

// the run's stats; GROOT_E_DEVICE when a batch's candidates did not fit the 2-bit buffer (a device-resident batch above max_batch_bases)
static int rescue_fetch_stats(groot_ctx *c, uint64_t (&st)[kRescueStats])
{
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemcpy(st, c->ct.res_stats.p, sizeof(st), hipMemcpyDeviceToHost));
    if (st[6]) return fail(c, GROOT_E_DEVICE, "mismatch rescue: %llu reads of batches with more than max_batch_bases bases were left out", (unsigned long long)st[6]);
    return GROOT_OK;
}

int groot_hip_rescue_export(groot_ctx *c, uint64_t *depth, uint64_t *alt)
{
    // (h_cov_base.back() = sum of (path_len + 1): above the number of paths exactly when some path has a base, and then there is something to write)
    const bool any_base = c && c->ct.h_cov_base.back() > c->ct.h_len.size();
    if (!c || (any_base && (!depth || !alt))) return GROOT_E_INVALID;
    if (!c->ct.res_on) return fail(c, GROOT_E_STATE, "mismatch rescue is not enabled (groot_hip_rescue_enable)");
    uint64_t stats[kRescueStats];
    if (int rc = rescue_fetch_stats(c, stats)) return rc;
    const uint64_t slots = c->ct.h_cov_base.back();
    std::vector<uint64_t> st(slots), en(slots), al(4 * slots);
    if (slots) {
        HIP_TRY(c, hipMemcpy(st.data(), c->ct.res_starts.p, slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(en.data(), c->ct.res_ends.p, slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(al.data(), c->ct.res_alt.p, 4 * slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    uint64_t at = 0;
    for (size_t p = 0; p < c->ct.h_len.size(); p++) {
        const uint64_t b = c->ct.h_cov_base[p], len = c->ct.h_len[p];
        uint64_t d = 0;
        for (uint64_t i = 0; i < len; i++, at++) {
            d += st[b + i] - en[b + i];
            depth[at] = d;
            for (uint32_t x = 0; x < 4; x++) alt[4 * at + x] = al[4 * (b + i) + x];
        }
    }
    return GROOT_OK;
}

int groot_hip_rescue_stats(groot_ctx *c, groot_rescue_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    uint64_t st[kRescueStats] = {};
    if (c->ct.res_on)
        if (int rc = rescue_fetch_stats(c, st)) return rc;
    out->candidates = st[0]; out->rescued = st[1]; out->exact = st[2]; out->placements = st[3]; out->too_short = st[4]; out->non_acgt = st[5];
    out->text_paths = c->ct.res_on ? c->ct.res_text_paths : 0;
    out->launches = c->ct.res_launches;
    return GROOT_OK;
}

int groot_hip_rescue_reset(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.res_on) return GROOT_OK;
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, rescue_zero(c->ct));
    return GROOT_OK;
}

// ---- gapped rescue (kernels_gap.hpp) ---------------------------------------------------------------------------------------
int groot_hip_gap_enable(groot_ctx *c, uint32_t max_gap, uint64_t event_slots)
{
    if (int rc = switchable(c, "gapped rescue")) return rc;
    Counters &k = c->ct;
    if (!max_gap) {
        recs_release<Gapped>(c);                     // (the gapped records are gapped rescue's placements: off with it)
        gec_release(k);                    // (and so are the gap-placed reads in the classes)
        gap_release(k);
        return GROOT_OK;
    }
    if (!k.res_on) return fail(c, GROOT_E_STATE, "gapped rescue looks at the reads mismatch rescue leaves, and that is off (groot_hip_rescue_enable)");
    if (max_gap > kGapMax) return fail(c, GROOT_E_INVALID, "gapped rescue: a gap of %u bases, at most %u are supported", max_gap, kGapMax);
    if (event_slots & (event_slots - 1)) return fail(c, GROOT_E_INVALID, "gapped rescue: event_slots %llu is not a power of two", (unsigned long long)event_slots);
    if (!event_slots) event_slots = 1ull << 22;
    if (k.gap_on && event_slots == k.gap_slots) {      // another G: the buffers stay, the counts start over
        if (max_gap != k.gap_g) {
            hipError_t e = gap_zero(k);
            if (e != hipSuccess) return fail(c, GROOT_E_DEVICE, "gapped rescue: %s", hipGetErrorString(e));
            k.gap_g = max_gap;
        }
        return GROOT_OK;
    }
    gap_release(k);
    const uint64_t slots = k.h_cov_base.back();
    hipError_t e = k.gap_cand.alloc(std::max<uint32_t>(c->prm.max_batch_reads, 1u));
    if (e == hipSuccess) e = k.gap_ncand.alloc(1);
    if (e == hipSuccess) e = k.gap_starts.alloc(slots);
    if (e == hipSuccess) e = k.gap_ends.alloc(slots);
    if (e == hipSuccess) e = k.gap_key.alloc(event_slots);
    if (e == hipSuccess) e = k.gap_cnt.alloc(event_slots);
    if (e == hipSuccess) e = k.gap_stats.alloc(kGapStats);
    if (e == hipSuccess) {
        k.gap_on = true; k.gap_g = max_gap; k.gap_slots = event_slots;
        e = gap_zero(k);
    }
    if (e != hipSuccess) {
        recs_release<Gapped>(c);
        gec_release(k);
        gap_release(k);
        return fail(c, GROOT_E_DEVICE, "gapped rescue: %s", hipGetErrorString(e));
    }
    return GROOT_OK;
}

int groot_hip_gap_export(groot_ctx *c, uint64_t *gdepth, groot_gap_event *events, uint64_t cap, uint64_t *n_events)
{
    const bool any_base = c && c->ct.h_cov_base.back() > c->ct.h_len.size();
    if (!c || !n_events || (any_base && !gdepth) || (cap && !events)) return GROOT_E_INVALID;
    *n_events = 0;
    Counters &k = c->ct;
    if (!k.gap_on) return fail(c, GROOT_E_STATE, "gapped rescue is not enabled (groot_hip_gap_enable)");
    uint64_t rst[kRescueStats], st[kGapStats];
    if (int rc = rescue_fetch_stats(c, rst)) return rc;
    HIP_TRY(c, hipMemcpy(st, k.gap_stats.p, sizeof(st), hipMemcpyDeviceToHost));
    *n_events = st[6];
    if (st[7])
        return fail(c, GROOT_E_NOSPACE, "gapped rescue: %llu events found no room in a table of event_slots = %llu: give groot_hip_gap_enable a larger one",
                    (unsigned long long)st[7], (unsigned long long)k.gap_slots);
    if (cap < st[6]) return fail(c, GROOT_E_INVALID, "gapped rescue: %llu distinct events, room for %llu", (unsigned long long)st[6], (unsigned long long)cap);
    const uint64_t slots = k.h_cov_base.back();
    std::vector<uint64_t> s0(slots), s1(slots), key(k.gap_slots), cnt(k.gap_slots);
    if (slots) {
        HIP_TRY(c, hipMemcpy(s0.data(), k.gap_starts.p, slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(s1.data(), k.gap_ends.p, slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    HIP_TRY(c, hipMemcpy(key.data(), k.gap_key.p, k.gap_slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(cnt.data(), k.gap_cnt.p, k.gap_slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
    uint64_t at = 0;
    for (size_t p = 0; p < k.h_len.size(); p++) {
        const uint64_t b = k.h_cov_base[p], len = k.h_len[p];
        uint64_t d = 0;
        for (uint64_t i = 0; i < len; i++, at++) {
            d += s0[b + i] - s1[b + i];
            gdepth[at] = d;
        }
    }
    uint64_t n = 0;
    for (uint64_t i = 0; i < k.gap_slots; i++) {
        if (!key[i]) continue;
        if (n == st[6]) return fail(c, GROOT_E_DEVICE, "gapped rescue: more keys in the table than the %llu claimed", (unsigned long long)st[6]);
        const uint64_t slot = key[i] & ((1ull << 40) - 1);
        const size_t p = (size_t)(std::upper_bound(k.h_cov_base.begin(), k.h_cov_base.end(), slot) - k.h_cov_base.begin()) - 1;
        groot_gap_event &e = events[n++];
        e.path = (uint32_t)p; e.pos = (uint32_t)(slot - k.h_cov_base[p]);
        e.type = (uint8_t)((key[i] >> 40) & 1u); e.len = (uint8_t)(((key[i] >> 41) & 7u) + 1u); e.seq = (uint16_t)(key[i] >> 44);
        e.reserved = 0; e.reads = cnt[i];
    }
    if (n != st[6]) return fail(c, GROOT_E_DEVICE, "gapped rescue: %llu keys in the table, %llu claimed", (unsigned long long)n, (unsigned long long)st[6]);
    std::sort(events, events + n, [](const groot_gap_event &a, const groot_gap_event &b) {      // the table's order is not deterministic, this one is
        return std::make_tuple(a.path, a.pos, a.type, a.len, a.seq) < std::make_tuple(b.path, b.pos, b.type, b.len, b.seq);
    });
    return GROOT_OK;
}

int groot_hip_gap_stats(groot_ctx *c, groot_gap_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    uint64_t st[kGapStats] = {};
    if (c->ct.gap_on) {
        uint64_t rst[kRescueStats];
        if (int rc = rescue_fetch_stats(c, rst)) return rc;
        HIP_TRY(c, hipMemcpy(st, c->ct.gap_stats.p, sizeof(st), hipMemcpyDeviceToHost));
    }
    out->candidates = st[0]; out->rescued = st[1]; out->placements = st[2]; out->del_placements = st[3]; out->ins_placements = st[4];
    out->too_short = st[5]; out->events = st[6]; out->dropped = st[7];
    out->event_slots = c->ct.gap_on ? c->ct.gap_slots : 0;
    out->launches = c->ct.gap_launches;
    return GROOT_OK;
}

int groot_hip_gap_reset(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    if (!c->ct.gap_on) return GROOT_OK;
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, gap_zero(c->ct));
    return GROOT_OK;
}

// ---- rescued reads in the equivalence classes (kernels_rescue_ec.hpp; the definition is in groot_hip.h) ---------------------
// rescue, the classes, no pairing: checked by the caller
static int rec_alloc(groot_ctx *c)
{
    Counters &k = c->ct;
    if (k.rec_on) return GROOT_OK;
    const uint32_t n_paths = (uint32_t)k.h_len.size(), R = std::max<uint32_t>(c->prm.max_batch_reads, 1u);
    std::vector<uint2> pb(n_paths);
    for (uint32_t g = 0; g + 1 < k.h_gpo.size(); g++)
        for (uint32_t p = k.h_gpo[g]; p < std::min(k.h_gpo[g + 1], n_paths); p++) pb[p] = make_uint2(g, p - k.h_gpo[g]);
    k.rec_bw = std::max<uint32_t>((n_paths + 63u) / 64u, 1u);
    // a batch has at most max_batch_reads slow rescued reads; below that, what the byte budget holds (GROOT_RESCUE_EC_BYTES per slot)
    k.rec_rows = c->kn.rescue_ec_rows ? c->kn.rescue_ec_rows : (uint32_t)std::max<uint64_t>(GROOT_RESCUE_EC_BYTES / (8ull * k.rec_bw), 1);
    k.rec_rows = std::min(k.rec_rows, R);
    hipError_t e = upload(k.rec_path_bit, pb.data(), pb.size());
    if (e == hipSuccess) e = k.rec_dstar.alloc(R);
    if (e == hipSuccess) e = k.rec_stats.alloc(kRescueEcStats);
    if (e == hipSuccess) e = hipMemset(k.rec_stats.p, 0, kRescueEcStats * sizeof(unsigned long long));
    if (e != hipSuccess) {
        rescue_ec_release(k);
        return fail(c, GROOT_E_DEVICE, "rescued reads in the equivalence classes: %s", hipGetErrorString(e));
    }
    k.rec_slow = 0;
    k.rec_on = true;
    return GROOT_OK;
}

int groot_hip_rescue_ec_enable(groot_ctx *c, int on)
{
    if (int rc = switchable(c, "rescued reads in the equivalence classes")) return rc;
    Counters &k = c->ct;
    if (!on) {
        rescue_ec_release(k);
        return GROOT_OK;
    }
    if (!k.res_on) return fail(c, GROOT_E_STATE, "rescued reads in the equivalence classes: mismatch rescue is off (groot_hip_rescue_enable)");
    if (!k.ec_on) return fail(c, GROOT_E_STATE, "rescued reads in the equivalence classes: equivalence classes are off (groot_hip_ec_enable)");
    if (k.pairs_on && !k.rp_on) return fail(c, GROOT_E_UNSUPPORTED, "rescued reads in the equivalence classes with paired-end units are not supported: mates are rescued one by one");
    if (k.acov_on) return fail(c, GROOT_E_UNSUPPORTED, "rescued reads in the equivalence classes with assigned coverage are not supported: a rescued read has no record to weigh");
    return rec_alloc(c);
}

// ---- rescued reads in assigned coverage (kernels_rescue_acov.hpp; the definition is in groot_hip.h) --------------------------
int groot_hip_rescue_acov_enable(groot_ctx *c, int on, uint64_t min_slots)
{
    if (int rc = switchable(c, "rescued reads in assigned coverage")) return rc;
    Counters &k = c->ct;
    if (!on) {
        if (k.rac_on) rescue_ec_release(k);      // (the rescued classes came on with it and cannot stay beside assigned coverage without it)
        return GROOT_OK;
    }
    if (min_slots & (min_slots - 1)) return fail(c, GROOT_E_INVALID, "rescued reads in assigned coverage: min_slots = %llu is not a power of two", (unsigned long long)min_slots);
    if (min_slots > (1ull << 31)) return fail(c, GROOT_E_INVALID, "rescued reads in assigned coverage: min_slots = %llu, at most 2^31 are supported", (unsigned long long)min_slots);
    if (k.pairs_on) return fail(c, GROOT_E_UNSUPPORTED, "rescued reads in assigned coverage with paired-end units are not supported: mates are rescued one by one");
    if (k.gec_on && !k.gac_on)             // (beside each other only through groot_hip_gap_acov_enable, which gives the pileup its rule)
        return fail(c, GROOT_E_UNSUPPORTED, "rescued reads in assigned coverage with gap-placed reads in the equivalence classes are not supported: the pileup has no "
                              "rule for a gapped record (groot_hip_gap_ec_enable)");
    if (!k.res_on) return fail(c, GROOT_E_STATE, "rescued reads in assigned coverage: mismatch rescue is off (groot_hip_rescue_enable)");
    if (!k.ec_on) return fail(c, GROOT_E_STATE, "rescued reads in assigned coverage: equivalence classes are off (groot_hip_ec_enable)");
    if (!k.acov_on) return fail(c, GROOT_E_STATE, "rescued reads in assigned coverage: assigned coverage is off (groot_hip_acov_enable)");
    if (k.acov.cap < min_slots)
        if (int rc = acov_grow(c, (uint32_t)(min_slots / k.acov.cap))) return rc;
    if (k.rac_on) return GROOT_OK;
    if (int rc = rec_alloc(c)) return rc;
    k.rac_log_cap = c->kn.rescue_acov_log ? c->kn.rescue_acov_log : (uint32_t)(GROOT_RESCUE_ACOV_BYTES / sizeof(uint4));
    hipError_t e = k.rac_cand_ser.alloc(std::max<uint32_t>(c->prm.max_batch_reads, 1u));
    if (e == hipSuccess) e = k.rac_stats.alloc(kRescueAcovStats);
    if (e == hipSuccess) e = hipMemset(k.rac_stats.p, 0, kRescueAcovStats * sizeof(unsigned long long));
    if (e != hipSuccess) {
        rescue_ec_release(k);
        return fail(c, GROOT_E_DEVICE, "rescued reads in assigned coverage: %s", hipGetErrorString(e));
    }
    k.rac_host_records = 0;
    k.rac_on = true;
    return GROOT_OK;
}

int groot_hip_rescue_acov_stats(groot_ctx *c, groot_rescue_acov_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    uint64_t st[kRescueAcovStats];
    if (int rc = part_stats(c, c->ct.rac_on, c->ct.rac_stats, st)) return rc;
    out->host_records = c->ct.rac_on ? c->ct.rac_host_records : 0;
    out->records = st[0] + out->host_records;
    out->dropped = st[kRescueAcovDropped];
    out->log_rows = c->ct.rac_on ? c->ct.rac_log_cap : 0;
    out->launches = c->ct.rac_launches;
    return GROOT_OK;
}

int groot_hip_rescue_ec_stats(groot_ctx *c, groot_rescue_ec_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    uint64_t st[kRescueEcStats];
    if (int rc = part_stats(c, c->ct.rec_on, c->ct.rec_stats, st)) return rc;
    out->slow_reads = c->ct.rec_on ? c->ct.rec_slow : 0;
    out->reads = st[0] + out->slow_reads;
    out->rows = c->ct.rec_on ? c->ct.rec_rows : 0;
    out->launches = c->ct.rec_launches;
    if (c->ct.rp_on) {                     // the rescued mates that are in a unit, and those of them in a unit that took a bitmap
        uint64_t pt[kRescuePairStats];
        HIP_TRY(c, hipMemcpy(pt, c->ct.rp_stats.p, sizeof(pt), hipMemcpyDeviceToHost));
        out->reads = pt[6];
        out->slow_reads = pt[8];
    }
    return GROOT_OK;
}

// ---- rescued mates in paired-end units (kernels_rescue_pairs.hpp; the rule is in groot_hip.h) -----------------------------------
int groot_hip_rescue_pairs_enable(groot_ctx *c, int on)
{
    if (int rc = switchable(c, "rescued mates in paired-end units")) return rc;
    Counters &k = c->ct;
    if (!on) {
        if (k.rp_on) rescue_ec_release(k);       // (the rescued classes cannot stay beside pairing without the rule; the classes and pairing stay)
        return GROOT_OK;
    }
    if (k.rp_on) return GROOT_OK;
    if (k.asg_on) return fail(c, GROOT_E_UNSUPPORTED, "rescued mates in paired-end units count S(r), which assignment collapses (groot_hip_assign_enable)");
    if (!k.res_on) return fail(c, GROOT_E_STATE, "rescued mates in paired-end units: mismatch rescue is off (groot_hip_rescue_enable)");
    if (k.sh_on)
        return fail(c, GROOT_E_UNSUPPORTED, "rescued mates in paired-end units with shared reads are not supported: the triangle has no rescued reads, and the "
                    "fragments left to rescue would be missing from it (groot_hip_shared_enable)");
    if (k.acp_on)
        return fail(c, GROOT_E_UNSUPPORTED, "rescued mates in paired-end units with assigned coverage over fragments are not supported: a rescued mate has no "
                    "record to weigh (groot_hip_acov_pairs_enable)");
    if (k.acov_on)
        return fail(c, GROOT_E_UNSUPPORTED, "rescued mates in paired-end units with assigned coverage are not supported: a rescued mate has no record to weigh "
                    "(groot_hip_acov_enable)");
    if (k.gec_on)
        return fail(c, GROOT_E_UNSUPPORTED, "rescued mates in paired-end units with gap-placed reads in the equivalence classes are not supported: the fragment "
                    "rule knows records and mismatch rescue's sets only (groot_hip_gap_ec_enable)");
    // the enables of pairing and of the rescued classes refuse each other: each is made with the other one off
    const bool was_pairs = k.pairs_on, was_ec = k.ec_on, was_rec = k.rec_on;
    auto undo = [&](int rc) {
        if (!was_rec) rescue_ec_release(k);
        if (!was_ec) groot_hip_ec_enable(c, 0);
        return rc;
    };
    k.pairs_on = false;
    int rc = groot_hip_ec_enable(c, 1);
    if (!rc) rc = groot_hip_rescue_ec_enable(c, 1);
    k.pairs_on = was_pairs;
    if (rc) return undo(rc);
    hipError_t e = k.rp_state.alloc(std::max<uint32_t>(c->prm.max_batch_reads, 1u));
    if (e == hipSuccess) e = k.rp_stats.alloc(2 * kRescuePairStats);        // (the totals, and the words of the batch in hand)
    if (e == hipSuccess) e = hipMemset(k.rp_stats.p, 0, 2 * kRescuePairStats * sizeof(unsigned long long));
    if (e != hipSuccess) {
        k.rp_state.release(); k.rp_stats.release();
        return undo(fail(c, GROOT_E_DEVICE, "rescued mates in paired-end units: %s", hipGetErrorString(e)));
    }
    k.rp_on = true;
    if (!was_pairs)
        if (int rc2 = groot_hip_pairs_enable(c, 1)) {      // (no state with the rule and the rescued classes on and pairing off is left behind)
            if (was_rec) { k.rp_state.release(); k.rp_stats.release(); k.rp_on = false; }
            return undo(rc2);
        }
    return GROOT_OK;
}

int groot_hip_rescue_pairs_stats(groot_ctx *c, groot_rescue_pairs_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    uint64_t st[kRescuePairStats];
    if (int rc = part_stats(c, c->ct.rp_on, c->ct.rp_stats, st)) return rc;
    out->exact_rescued_joined = st[0]; out->exact_rescued_split = st[1];
    out->rescued_rescued_joined = st[2]; out->rescued_rescued_split = st[3];
    out->single_exact = st[4]; out->single_rescued = st[5];
    out->rescued_mates = st[6]; out->bitmap_units = st[7];
    out->launches = c->ct.rp_launches;
    return GROOT_OK;
}

// ---- rescued mates in assigned coverage over fragments (kernels_rescue_acov_pairs.hpp; the rule is in groot_hip.h) -------------------
int groot_hip_rescue_acov_pairs_enable(groot_ctx *c, int on, uint64_t min_slots)
{
    if (int rc = switchable(c, "rescued mates in assigned coverage over fragments")) return rc;
    Counters &k = c->ct;
    if (!on) return k.rap_on ? groot_hip_acov_enable(c, 0) : GROOT_OK;     // (the rule and its records go with the table; the classes, pairing and the rescued mates' rule stay)
    if (min_slots & (min_slots - 1)) return fail(c, GROOT_E_INVALID, "rescued mates in assigned coverage over fragments: min_slots = %llu is not a power of two", (unsigned long long)min_slots);
    if (min_slots > (1ull << 31)) return fail(c, GROOT_E_INVALID, "rescued mates in assigned coverage over fragments: min_slots = %llu, at most 2^31 are supported", (unsigned long long)min_slots);
    if (!k.res_on) return fail(c, GROOT_E_STATE, "rescued mates in assigned coverage over fragments: mismatch rescue is off (groot_hip_rescue_enable)");
    if (!k.rap_on) {
        if (k.asg_on) return fail(c, GROOT_E_UNSUPPORTED, "rescued mates in assigned coverage over fragments count S(r), which assignment collapses (groot_hip_assign_enable)");
        if (k.sh_on)
            return fail(c, GROOT_E_UNSUPPORTED, "rescued mates in assigned coverage over fragments with shared reads are not supported: the triangle has no rescued reads "
                        "(groot_hip_shared_enable)");
        if (k.gec_on)        // (and with it the gap-placed reads in the pileup, which need them)
            return fail(c, GROOT_E_UNSUPPORTED, "rescued mates in assigned coverage over fragments with gap-placed reads in the equivalence classes or the pileup are not "
                        "supported: the fragment rule knows records and mismatch rescue's sets only (groot_hip_gap_ec_enable, groot_hip_gap_acov_enable)");
        // The enables this one stands on refuse each other: each is made with the other side hidden.  First the rescued mates' rule (the
        // classes, the rescued classes, pairing), with assigned coverage out of sight; then assigned coverage over fragments, with the
        // rescued classes out of sight.  The unpaired rule of the rescued records has no meaning over fragments: it goes once both have come
        // on, the rescued classes stay.  A failure of the first leaves the ctx as it was; one behind it takes assigned coverage off, so that no
        // state with the rescued mates' rule and assigned coverage on and this rule off is left behind.
        const bool was_acov = k.acov_on, was_acp = k.acp_on;
        auto undo = [&](int rc) {
            const std::string why = c->err;
            groot_hip_acov_enable(c, 0);
            c->err = why;
            return rc;
        };
        k.acov_on = k.acp_on = false;
        int rc = groot_hip_rescue_pairs_enable(c, 1);
        k.acov_on = was_acov; k.acp_on = was_acp;
        if (rc) return rc;
        k.rec_on = false;
        rc = groot_hip_acov_pairs_enable(c, 1);
        k.rec_on = true;
        if (rc) return undo(rc);
        if (k.rac_on) {
            k.rac_cand_ser.release(); k.rac_stats.release();
            k.rac_on = false; k.rac_log_cap = 0; k.rac_host_records = 0;
        }
        k.rap_log_cap = c->kn.rescue_acov_log ? c->kn.rescue_acov_log : (uint32_t)(GROOT_RESCUE_ACOV_BYTES / sizeof(uint4));
        const uint32_t R = std::max<uint32_t>(c->prm.max_batch_reads, 1u);
        hipError_t e = k.rap_cand_ser.alloc(R);
        if (e == hipSuccess) e = k.rap_fclass.alloc(R);
        if (e == hipSuccess) e = k.rap_stats.alloc(kRescueAcovPairStats);
        if (e == hipSuccess) e = hipMemset(k.rap_stats.p, 0, kRescueAcovPairStats * sizeof(unsigned long long));
        if (e != hipSuccess) return undo(fail(c, GROOT_E_DEVICE, "rescued mates in assigned coverage over fragments: %s", hipGetErrorString(e)));
        std::fill(k.rap_host, k.rap_host + 4, 0);
        k.rap_on = true;
    }
    if (k.acov.cap < min_slots)
        if (int rc = acov_grow(c, (uint32_t)(min_slots / k.acov.cap))) return rc;
    return GROOT_OK;
}

int groot_hip_rescue_acov_pairs_stats(groot_ctx *c, groot_rescue_acov_pairs_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    uint64_t st[kRescueAcovPairStats];
    if (int rc = part_stats(c, c->ct.rap_on, c->ct.rap_stats, st)) return rc;
    const uint64_t *h = c->ct.rap_host;    // (zero while the rule is off)
    out->exact_records = st[kRapExact] + h[0]; out->exact_left_out = st[kRapExactLeft] + h[1];
    out->rescued_records = st[kRapRescued] + h[2]; out->rescued_left_out = st[kRapRescuedLeft] + h[3];
    out->host_records = h[0] + h[2];
    out->dropped = st[kRapDropped];
    out->log_rows = c->ct.rap_on ? c->ct.rap_log_cap : 0;
    out->launches = c->ct.rap_launches;
    return GROOT_OK;
}

// ---- rescued records (kernels_rescue_rec.hpp) and gapped records (kernels_gap_rec.hpp; the definitions are in groot_hip.h) ------
int groot_hip_rescue_rec_enable(groot_ctx *c, uint64_t slots_per_batch)
{
    return recs_enable<Rescued>(c, slots_per_batch,
                                c && c->ct.asg_on ? "rescued records come from mismatch rescue, which tells the unaligned reads by their records, and assignment rewrites those (groot_hip_assign_enable)" : nullptr,
                                c && !c->ct.res_on ? "rescued records are the placements of mismatch rescue, and that is off (groot_hip_rescue_enable)" : nullptr);
}

int groot_hip_rescue_rec_stats(groot_ctx *c, groot_rescue_rec_stats *out) { return recs_stats<Rescued>(c, out); }

int groot_hip_gap_rec_enable(groot_ctx *c, uint64_t slots_per_batch)
{
    return recs_enable<Gapped>(c, slots_per_batch, nullptr,
                               c && !c->ct.gap_on ? "gapped records are the placements of gapped rescue, and that is off (groot_hip_gap_enable)" : nullptr);
}

int groot_hip_gap_rec_stats(groot_ctx *c, groot_gap_rec_stats *out) { return recs_stats<Gapped>(c, out); }

// ---- gap-placed reads in the equivalence classes (kernels_gap_ec.hpp; the definition is in groot_hip.h) ----------------------
// gapped rescue and the rescued classes on: checked by the caller
static int gec_alloc(groot_ctx *c)
{
    Counters &k = c->ct;
    if (k.gec_on) return GROOT_OK;
    hipError_t e = k.gec_e.alloc(std::max<uint32_t>(c->prm.max_batch_reads, 1u));
    if (e == hipSuccess) e = k.gec_stats.alloc(kGapEcStats);
    if (e == hipSuccess) e = hipMemset(k.gec_stats.p, 0, kGapEcStats * sizeof(unsigned long long));
    if (e != hipSuccess) {
        gec_release(k);
        return fail(c, GROOT_E_DEVICE, "gap-placed reads in the equivalence classes: %s", hipGetErrorString(e));
    }
    k.gec_slow = 0;
    k.gec_on = true;
    return GROOT_OK;
}

int groot_hip_gap_ec_enable(groot_ctx *c, int on)
{
    if (int rc = switchable(c, "gap-placed reads in the equivalence classes")) return rc;
    Counters &k = c->ct;
    if (!on) {
        gec_release(k);
        return GROOT_OK;
    }
    if (!k.gap_on) return fail(c, GROOT_E_STATE, "gap-placed reads in the equivalence classes: gapped rescue is off (groot_hip_gap_enable)");
    if (!k.rec_on) return fail(c, GROOT_E_STATE, "gap-placed reads in the equivalence classes: the rescued reads in the equivalence classes are off (groot_hip_rescue_ec_enable)");
    if (k.rp_on) return fail(c, GROOT_E_UNSUPPORTED, "gap-placed reads in the equivalence classes with rescued mates in paired-end units are not supported: the fragment rule "
                             "knows records and mismatch rescue's sets only (groot_hip_rescue_pairs_enable)");
    if (k.rac_on && !k.gac_on)             // (beside each other only through groot_hip_gap_acov_enable, which gives the pileup its rule)
        return fail(c, GROOT_E_UNSUPPORTED, "gap-placed reads in the equivalence classes with rescued reads in assigned coverage are not supported: the pileup has no "
                              "rule for a gapped record, and a DEL covers two intervals (groot_hip_rescue_acov_enable)");
    return gec_alloc(c);
}

int groot_hip_gap_ec_stats(groot_ctx *c, groot_gap_ec_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    uint64_t st[kGapEcStats];
    if (int rc = part_stats(c, c->ct.gec_on, c->ct.gec_stats, st)) return rc;
    out->slow_reads = c->ct.gec_on ? c->ct.gec_slow : 0;
    out->reads = st[0] + out->slow_reads;
    out->launches = c->ct.gec_launches;
    return GROOT_OK;
}

// ---- gap-placed reads in assigned coverage (kernels_gap_acov.hpp; the definition is in groot_hip.h) --------------------------
int groot_hip_gap_acov_enable(groot_ctx *c, int on)
{
    if (int rc = switchable(c, "gap-placed reads in assigned coverage")) return rc;
    Counters &k = c->ct;
    if (!on) {
        if (k.gac_on) gec_release(k);      // (the gap-placed classes came on with it and cannot stay beside the rescued records without it)
        return GROOT_OK;
    }
    if (!k.gap_on) return fail(c, GROOT_E_STATE, "gap-placed reads in assigned coverage: gapped rescue is off (groot_hip_gap_enable)");
    if (!k.rac_on) return fail(c, GROOT_E_STATE, "gap-placed reads in assigned coverage: the rescued reads in assigned coverage are off (groot_hip_rescue_acov_enable)");
    if (k.gac_on) return GROOT_OK;
    if (int rc = gec_alloc(c)) return rc;  // (rac_on: mismatch rescue, the classes, the rescued classes and assigned coverage are on, pairing is off)
    hipError_t e = k.gac_cand_ser.alloc(std::max<uint32_t>(c->prm.max_batch_reads, 1u));
    if (e == hipSuccess) e = k.gac_stats.alloc(kGapAcovStats);
    if (e == hipSuccess) e = hipMemset(k.gac_stats.p, 0, kGapAcovStats * sizeof(unsigned long long));
    if (e != hipSuccess) {
        gec_release(k);
        return fail(c, GROOT_E_DEVICE, "gap-placed reads in assigned coverage: %s", hipGetErrorString(e));
    }
    k.gac_host_records = k.gac_host_placements = 0;
    k.gac_on = true;
    return GROOT_OK;
}

int groot_hip_gap_acov_stats(groot_ctx *c, groot_gap_acov_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    uint64_t st[kGapAcovStats];
    if (int rc = part_stats(c, c->ct.gac_on, c->ct.gac_stats, st)) return rc;
    out->host_records = c->ct.gac_on ? c->ct.gac_host_records : 0;
    out->placements = st[0] + (c->ct.gac_on ? c->ct.gac_host_placements : 0);
    out->records = st[kGapAcovRecords] + out->host_records;
    out->dropped = st[kGapAcovDropped];
    out->launches = c->ct.gac_launches;
    return GROOT_OK;
}
} // extern "C"
