// align: what the contexts count on the device beside the records (--report, --sharedReads, --abundance, --calls, --paired, --assignFrom, --variants, --indels),
// added up on the host.  A ctx is harvested before it closes (a reopen in the middle of the stream) and once at the end of the stream.
#pragma once
#include "align_plan.hpp"

namespace {

struct AcovExport {                          // --calls: a ctx's ECs and assigned-coverage table, as exported (groot_host_acov_merge)
    std::vector<uint64_t> off, cnt, tn;
    std::vector<uint32_t> ids, tuples;
};

struct Harvested {                           // the sums over every harvest so far
    std::vector<uint64_t> cov_records, cov_depth;            // --report: records per path, depth per base (groot_hip_coverage_*)
    std::vector<uint32_t> sh_a, sh_b;                        // --sharedReads: every ctx's nonzero pairs, appended
    std::vector<uint64_t> sh_n;
    std::vector<uint64_t> ec_off{0}, ec_cnt;                 // --abundance: the equivalence classes of every ctx, appended (CSR)
    std::vector<uint32_t> ec_ids;
    uint64_t fr_joined = 0, fr_split = 0, fr_single = 0;     // --paired / --interleaved: fragments per class
    std::vector<std::unique_ptr<AcovExport>> acov;           // --calls: one export per harvest
    groot_assign_stats assign{};                             // --assignFrom
    std::vector<uint64_t> res_depth, res_alt;                // --variants: rescued depth per base, A / C / G / T counts per base (groot_hip_rescue_*)
    groot_rescue_stats rescue{};
    std::vector<uint64_t> gap_depth;                         // --indels: gap depth per base, the events of every ctx merged by key (groot_hip_gap_*)
    std::map<std::array<uint32_t, 5>, uint64_t> gap_events;  // (path, pos, type, len, seq) -> reads: ascending as the export is
    groot_gap_stats gap{};
    groot_rescue_ec_stats rescue_ec{};                       // --abundanceRescued: the rescued reads in the classes (groot_hip_rescue_ec_*)
    groot_gap_ec_stats gap_ec{};                             // --abundanceGapped: the gap-placed reads in the classes (groot_hip_gap_ec_*)
    groot_rescue_acov_stats rescue_acov{};                   // --callsRescued: their records in the pileup (groot_hip_rescue_acov_*)
    groot_gap_acov_stats gap_acov{};                         // --callsGapped: the gap-placed reads' records in the pileup (groot_hip_gap_acov_*)
    groot_rescue_pairs_stats rescue_pairs{};                 // --rescuedPaired: the fragments with a rescued or a lone mate, by kind (groot_hip_rescue_pairs_*)
    groot_rescue_acov_pairs_stats rescue_acov_pairs{};       // --callsRescuedPaired: the one-pass records of the fragments with a rescued mate (groot_hip_rescue_acov_pairs_*)
    groot_acov_pairs_stats acov_pairs{};                     // --callsPaired: the records piled up and left out under the rule for fragments (groot_hip_acov_pairs_*)
};

class RunCounters {
public:
    // (--assignFrom: alpha of the first pass is read here, and handed to every ctx with the other switches)
    RunCounters(const Args &a, const AlignPlan &plan, const groot_index_view &v) : a_(a), plan_(plan), v_(v)
    {
        for (uint32_t p = 0; p < v.n_paths; p++) cov_slots_ += v.path_len[p];
        h_.cov_records.resize(plan.coverage ? v.n_paths : 0);
        h_.cov_depth.resize(plan.coverage ? cov_slots_ : 0);
        h_.res_depth.resize(plan.variants || plan.indels ? cov_slots_ : 0);
        h_.res_alt.resize(plan.variants || plan.indels ? 4 * cov_slots_ : 0);
        h_.gap_depth.resize(plan.indels ? cov_slots_ : 0);
        if (!plan.assign) return;
        uint64_t named = 0;
        assign_alpha_.resize(v.n_paths);
        if (groot_host_abundance_read(&v, a.assign_from.c_str(), assign_alpha_.data(), &named)) die("%s", groot_host_last_error());
        logf("\tassignment: em_reads of %llu ARG(s) read from %s, minimum posterior %g", (unsigned long long)named, a.assign_from.c_str(), a.min_posterior);
    }

    // both: 0, or the status of the library call that failed (groot_hip_last_error(ctx) has the text)
    int enable(groot_ctx *ctx, int on) const
    {
        if (plan_.assign)
            if (int rc = groot_hip_assign_enable(ctx, on ? assign_alpha_.data() : nullptr, v_.n_paths, a_.min_posterior)) return rc;
        if (plan_.frags && !((plan_.calls_paired || plan_.rescued_paired) && on))      // (--callsPaired: pairing comes on with assigned coverage, below; --rescuedPaired: with the rescued classes)
            if (int rc = groot_hip_pairs_enable(ctx, on)) return rc;
        if (plan_.coverage)
            if (int rc = groot_hip_coverage_enable(ctx, on)) return rc;
        if (plan_.rescue)
            if (int rc = groot_hip_rescue_enable(ctx, &v_, on ? (uint32_t)a_.rescue : 0u)) return rc;
        if (plan_.rescued_bam && on)    // (off: the rescued records go with rescue)
            if (int rc = groot_hip_rescue_rec_enable(ctx, a_.rescued_bam_slots_given ? (uint64_t)a_.rescued_bam_slots : 16ull * std::max<uint32_t>(a_.batch, 1u))) return rc;
        if (plan_.indels && on)     // (off: gapped rescue goes with rescue)
            if (int rc = groot_hip_gap_enable(ctx, (uint32_t)a_.rescue_gap, (uint64_t)a_.gap_event_slots)) return rc;
        if (plan_.rescued_bam_gaps && on)   // behind gapped rescue (off: the gapped records go with it)
            if (int rc = groot_hip_gap_rec_enable(ctx, a_.gap_record_slots_given ? (uint64_t)a_.gap_record_slots : 4ull * std::max<uint32_t>(a_.batch, 1u))) return rc;
        if (plan_.shared)
            if (int rc = groot_hip_shared_enable(ctx, on)) return rc;
        if (plan_.calls_rescued_paired && on)      // (the rule brings the classes, pairing, the rescued mates' rule and assigned coverage over fragments with it)
            return groot_hip_rescue_acov_pairs_enable(ctx, 1, (uint64_t)a_.call_slots);
        if (plan_.calls && on)
            if (int rc = plan_.calls_paired ? groot_hip_acov_pairs_enable(ctx, 1) : groot_hip_acov_enable(ctx, 1)) return rc;
        if (plan_.abundance)
            if (int rc = groot_hip_ec_enable(ctx, on)) return rc;        // (off: assigned coverage goes with it, and so do the rescued reads in the classes)
        if (plan_.calls_rescued && on) {     // (it switches the rescued reads in the classes on itself)
            if (int rc = groot_hip_rescue_acov_enable(ctx, 1, (uint64_t)a_.call_slots)) return rc;
            return plan_.calls_gapped ? groot_hip_gap_acov_enable(ctx, 1) : 0;      // (and this one the gap-placed reads in the classes: --abundanceGapped beside --calls)
        }
        if (plan_.ab_rescued && on)         // (--rescuedPaired: the rule brings the rescued reads in the classes and pairing with it)
            if (int rc = plan_.rescued_paired ? groot_hip_rescue_pairs_enable(ctx, 1) : groot_hip_rescue_ec_enable(ctx, 1)) return rc;
        return plan_.ab_gapped && on ? groot_hip_gap_ec_enable(ctx, 1) : 0;   // behind gapped rescue and the rescued reads in the classes (off: it goes with either)
    }

    // assign stats, pair stats, acov-or-EC export, rescued reads in the ECs, gapped rescue, rescue, coverage, shared pairs: each added under the lock (the mappers harvest side by side)
    int harvest(groot_ctx *ctx)
    {
        if (plan_.assign) {
            groot_assign_stats st{};
            if (int rc = groot_hip_assign_stats(ctx, &st)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            groot_assign_stats &t = h_.assign;
            t.reads += st.reads; t.assigned += st.assigned; t.unassigned += st.unassigned; t.below += st.below;
            t.ties += st.ties; t.records_in += st.records_in; t.records_kept += st.records_kept;
            t.travs_emptied += st.travs_emptied;
        }
        if (plan_.frags) {
            uint64_t j = 0, sp = 0, si = 0;
            if (int rc = groot_hip_pairs_stats(ctx, &j, &sp, &si)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            h_.fr_joined += j; h_.fr_split += sp; h_.fr_single += si;
        }
        if (plan_.calls_paired) {
            groot_acov_pairs_stats st{};
            if (int rc = groot_hip_acov_pairs_stats(ctx, &st)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            groot_acov_pairs_stats &t = h_.acov_pairs;
            t.records += st.records; t.left_out += st.left_out; t.joined_reads += st.joined_reads; t.slow_fragments += st.slow_fragments;
        }
        if (plan_.calls) {
            uint64_t ne = 0, ni = 0, nt = 0;
            if (int rc = groot_hip_acov_export(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, &ne, &ni, &nt)) return rc;
            std::unique_ptr<AcovExport> x(new AcovExport());
            x->off.resize(ne + 1); x->cnt.resize(ne + 1); x->ids.resize(ni + 1); x->tuples.resize(4 * nt + 4); x->tn.resize(nt + 1);
            if (ne || nt)
                if (int rc = groot_hip_acov_export(ctx, x->off.data(), x->ids.data(), x->cnt.data(), x->tuples.data(), x->tn.data(), ne, ni, nt, &ne, &ni, &nt)) return rc;
            x->cnt.resize(ne); x->ids.resize(ni); x->tuples.resize(4 * nt); x->tn.resize(nt);
            std::lock_guard<std::mutex> lk(mu_);
            append_ecs(x->off.data(), x->ids.data(), x->cnt.data(), ne, ni);
            h_.acov.push_back(std::move(x));
        } else if (plan_.abundance) {
            uint64_t ne = 0, ni = 0, me = 0, mi = 0;
            if (int rc = groot_hip_ec_export(ctx, nullptr, nullptr, nullptr, 0, 0, &ne, &ni)) return rc;
            std::vector<uint64_t> off(ne + 1), cnt(ne);
            std::vector<uint32_t> ids(ni);
            if (ne)
                if (int rc = groot_hip_ec_export(ctx, off.data(), ids.data(), cnt.data(), ne, ni, &me, &mi)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            append_ecs(off.data(), ids.data(), cnt.data(), ne, ni);
        }
        if (plan_.ab_rescued) {
            groot_rescue_ec_stats st{};
            if (int rc = groot_hip_rescue_ec_stats(ctx, &st)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            h_.rescue_ec.reads += st.reads; h_.rescue_ec.slow_reads += st.slow_reads; h_.rescue_ec.launches += st.launches; h_.rescue_ec.rows = st.rows;
        }
        if (plan_.rescued_paired) {
            groot_rescue_pairs_stats st{};
            if (int rc = groot_hip_rescue_pairs_stats(ctx, &st)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            groot_rescue_pairs_stats &t = h_.rescue_pairs;
            t.exact_rescued_joined += st.exact_rescued_joined; t.exact_rescued_split += st.exact_rescued_split;
            t.rescued_rescued_joined += st.rescued_rescued_joined; t.rescued_rescued_split += st.rescued_rescued_split;
            t.single_exact += st.single_exact; t.single_rescued += st.single_rescued;
            t.rescued_mates += st.rescued_mates; t.bitmap_units += st.bitmap_units; t.launches += st.launches;
        }
        if (plan_.ab_gapped) {
            groot_gap_ec_stats st{};
            if (int rc = groot_hip_gap_ec_stats(ctx, &st)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            h_.gap_ec.reads += st.reads; h_.gap_ec.slow_reads += st.slow_reads; h_.gap_ec.launches += st.launches;
        }
        if (plan_.calls_rescued) {  // (a table that dropped rescued records has failed above, at the export, with the reason: no calls file is written)
            groot_rescue_acov_stats st{};
            if (int rc = groot_hip_rescue_acov_stats(ctx, &st)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            groot_rescue_acov_stats &t = h_.rescue_acov;
            t.records += st.records; t.host_records += st.host_records; t.dropped += st.dropped; t.launches += st.launches; t.log_rows = st.log_rows;
        }
        if (plan_.calls_rescued_paired) {      // (one-pass records without room have failed the export above too)
            groot_rescue_acov_pairs_stats st{};
            if (int rc = groot_hip_rescue_acov_pairs_stats(ctx, &st)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            groot_rescue_acov_pairs_stats &t = h_.rescue_acov_pairs;
            t.exact_records += st.exact_records; t.exact_left_out += st.exact_left_out; t.rescued_records += st.rescued_records; t.rescued_left_out += st.rescued_left_out;
            t.host_records += st.host_records; t.dropped += st.dropped; t.launches += st.launches; t.log_rows = st.log_rows;
        }
        if (plan_.calls_gapped) {   // (gapped records without room have failed the export above as well)
            groot_gap_acov_stats st{};
            if (int rc = groot_hip_gap_acov_stats(ctx, &st)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            groot_gap_acov_stats &t = h_.gap_acov;
            t.placements += st.placements; t.records += st.records; t.host_records += st.host_records; t.dropped += st.dropped; t.launches += st.launches;
        }
        if (plan_.indels) {         // (a table that dropped events fails here, with the reason: no indels file is written)
            groot_gap_stats st{};
            uint64_t n = 0;
            if (int rc = groot_hip_gap_stats(ctx, &st)) return rc;
            std::vector<uint64_t> d(cov_slots_);
            std::vector<groot_gap_event> ev(st.events);
            if (int rc = groot_hip_gap_export(ctx, d.data(), ev.data(), ev.size(), &n)) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            groot_gap_stats &t = h_.gap;
            t.candidates += st.candidates; t.rescued += st.rescued; t.placements += st.placements; t.del_placements += st.del_placements;
            t.ins_placements += st.ins_placements; t.too_short += st.too_short; t.launches += st.launches; t.event_slots = st.event_slots;
            for (size_t i = 0; i < d.size(); i++) h_.gap_depth[i] += d[i];
            for (uint64_t i = 0; i < n; i++) h_.gap_events[{ev[i].path, ev[i].pos, ev[i].type, ev[i].len, ev[i].seq}] += ev[i].reads;
        }
        if (plan_.variants || plan_.indels) {
            groot_rescue_stats st{};
            std::vector<uint64_t> d(cov_slots_), al(4 * cov_slots_);
            if (int rc = groot_hip_rescue_stats(ctx, &st)) return rc;
            if (int rc = groot_hip_rescue_export(ctx, d.data(), al.data())) return rc;
            std::lock_guard<std::mutex> lk(mu_);
            groot_rescue_stats &t = h_.rescue;
            t.candidates += st.candidates; t.rescued += st.rescued; t.exact += st.exact; t.placements += st.placements;
            t.too_short += st.too_short; t.non_acgt += st.non_acgt; t.launches += st.launches; t.text_paths = st.text_paths;
            for (size_t i = 0; i < d.size(); i++) h_.res_depth[i] += d[i];
            for (size_t i = 0; i < al.size(); i++) h_.res_alt[i] += al[i];
        }
        if (!plan_.coverage) return 0;
        std::vector<uint64_t> r(v_.n_paths), d(cov_slots_);
        if (int rc = groot_hip_coverage_export(ctx, r.data(), d.data())) return rc;
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t i = 0; i < r.size(); i++) h_.cov_records[i] += r[i];
        for (size_t i = 0; i < d.size(); i++) h_.cov_depth[i] += d[i];
        if (!plan_.shared) return 0;
        // --sharedReads: the ctx's nonzero pairs, appended (a read goes to one ctx only: the sums are exact, groot_host_shared_from_counts
        // adds up repeated pairs)
        uint64_t n = 0, m = 0;
        if (int rc = groot_hip_shared_export(ctx, nullptr, nullptr, nullptr, 0, &n)) return rc;
        std::vector<uint32_t> pa(n), pb(n);
        std::vector<uint64_t> cnt(n);
        if (n)
            if (int rc = groot_hip_shared_export(ctx, pa.data(), pb.data(), cnt.data(), n, &m)) return rc;
        h_.sh_a.insert(h_.sh_a.end(), pa.begin(), pa.end());
        h_.sh_b.insert(h_.sh_b.end(), pb.begin(), pb.end());
        h_.sh_n.insert(h_.sh_n.end(), cnt.begin(), cnt.end());
        return 0;
    }

    const Harvested &totals() const { return h_; }   // for the writers, once the mappers are joined

private:
    // a ctx's n_ec classes over n_ids path ids behind the merged CSR (mu_ held)
    void append_ecs(const uint64_t *off, const uint32_t *ids, const uint64_t *cnt, uint64_t n_ec, uint64_t n_ids)
    {
        const uint64_t base = h_.ec_ids.size();
        for (uint64_t e = 0; e < n_ec; e++) h_.ec_off.push_back(base + off[e + 1]);
        h_.ec_ids.insert(h_.ec_ids.end(), ids, ids + n_ids);
        h_.ec_cnt.insert(h_.ec_cnt.end(), cnt, cnt + n_ec);
    }

    const Args &a_;
    const AlignPlan &plan_;
    const groot_index_view &v_;
    uint64_t cov_slots_ = 0;
    std::vector<double> assign_alpha_;
    std::mutex mu_;
    Harvested h_;
};

} // namespace
