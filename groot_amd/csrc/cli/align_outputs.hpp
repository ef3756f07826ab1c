// align, stages 8 to 10: the files written from what the contexts counted (--abundance, --calls, --rarefy, --report, --sharedReads), the
// weighted and pruned graphs, the stats file.  Everything here runs on the main thread after the stream; an error ends the run (die).
#pragma once
#include "align_stream.hpp"

namespace {

struct Ecs {                                 // equivalence classes as CSR: n classes, off[n + 1], ids[off[n]], cnt[n] (the vectors may be longer)
    std::vector<uint64_t> off, cnt;
    std::vector<uint32_t> ids;
    uint64_t n = 0;
};

// the merged ECs of every ctx in canonical order: what the bootstrap and the curve of the abundance file alone are drawn from
Ecs canonical_ecs(const groot_index_view &v, const Harvested &h)
{
    Ecs c;
    c.off.resize(h.ec_cnt.size() + 1); c.cnt.resize(h.ec_cnt.size() + 1); c.ids.resize(h.ec_ids.size() + 1);
    if (groot_host_ecs_canonical(v.n_paths, h.ec_cnt.size(), h.ec_off.data(), h.ec_ids.data(), h.ec_cnt.data(), c.off.data(), c.ids.data(), c.cnt.data(), &c.n))
        die("%s", groot_host_last_error());
    return c;
}

// --rarefy of `align`: the drawn depths fitted (and with --calls piled up) on the run's first GPU, over canonical ECs; the file through the host writer
void rarefy_on_gpu(const Args &a, const groot_index_view &v, int device, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *cnt, bool calls,
                   uint64_t n_tp, const uint32_t *tup, const uint64_t *tn)
{
    auto t0 = std::chrono::steady_clock::now();
    const uint32_t R = a.rarefy_reps, D = a.rarefy_steps;
    uint64_t units = 0;
    for (uint64_t e = 0; e < n_ec; e++) units += cnt[e];
    std::vector<uint64_t> m(D), drawn;
    if (groot_host_rarefy_depths(units, D, m.data())) die("%s", groot_host_last_error());
    for (uint32_t s = 0; s + 1 < D; s++)
        if (m[s]) drawn.push_back(m[s]);
    const uint32_t K = (uint32_t)drawn.size();
    std::vector<uint64_t> rc(calls ? (size_t)R * K * n_ec + 1 : 1);
    std::vector<double> ra((size_t)R * K * v.n_paths + 1);
    std::vector<uint32_t> its(std::max<size_t>((size_t)R * K, 1), 0), sel, covered;
    if (K && groot_hip_em_rarefy(device, v.n_paths, n_ec, off, ids, cnt, R, K, drawn.data(), a.rarefy_seed, GROOT_EM_MIN_ITER, GROOT_EM_MAX_ITER,
                                 calls ? rc.data() : nullptr, ra.data(), its.data()))
        die("%s", groot_hip_last_error(nullptr));
    if (K && calls) {
        // every path detected at some depth of some replicate, ascending: the writer selects the same
        std::vector<uint8_t> seen(v.n_paths, 0);
        for (size_t x = 0; x < (size_t)R * K; x++)
            for (uint32_t p = 0; p < v.n_paths; p++)
                if (ra[x * v.n_paths + p] >= a.abundance_min) seen[p] = 1;
        for (uint32_t p = 0; p < v.n_paths; p++)
            if (seen[p]) sel.push_back(p);
        covered.resize((size_t)R * K * sel.size() + 1);
        if (!sel.empty() && groot_hip_call_support(device, v.n_paths, v.path_len, n_ec, off, ids, cnt, n_tp, tup, tn, R * K, rc.data(), ra.data(), a.call_depth,
                                                   (uint32_t)sel.size(), sel.data(), covered.data()))
            die("%s", groot_hip_last_error(nullptr));
    }
    uint64_t n_lines = 0;
    if (groot_host_rarefy_from_ecs(&v, n_ec, off, ids, cnt, a.abundance_min, R, D, a.rarefy_seed, 1, calls && K ? rc.data() : nullptr, K ? ra.data() : nullptr,
                                   calls ? 1 : 0, n_tp, tup, tn, a.call_depth, a.cov_cutoff, (uint32_t)sel.size(), sel.empty() ? nullptr : covered.data(),
                                   a.rarefy_out.c_str(), &n_lines))
        die("%s", groot_host_last_error());
    logf("\trarefaction: %u step(s), %u replicate(s) of %llu unit(s) in %llu equivalence class(es) on GPU %d (seed %llu), EM of %u to %u iteration(s), %llu line(s)%s in %.3f s, written to %s",
         D, R, (unsigned long long)units, (unsigned long long)n_ec, device, (unsigned long long)a.rarefy_seed, *std::min_element(its.begin(), its.end()),
         *std::max_element(its.begin(), its.end()), (unsigned long long)n_lines, calls ? " with the called columns" : "", seconds_since(t0), a.rarefy_out.c_str());
}

struct Bootstrap {                           // the bootstrap's canonical ECs, draw counts and estimates: --callSupport piles up the same replicates
    Ecs ecs;
    std::vector<uint64_t> count;
    std::vector<double> alpha;
};

// --abundance [--bootstraps] [--rarefy without --calls]; the replicates are drawn and fitted on `device`, the run's first GPU
Bootstrap write_abundance(const Args &a, const AlignPlan &plan, const groot_index_view &v, const Harvested &h, int device)
{
    Bootstrap b;
    uint64_t n_lines = 0;
    uint32_t iters = 0;
    auto t_em = std::chrono::steady_clock::now();
    if (a.bootstraps) {
        // the replicates: over the merged ECs in canonical order
        auto t_boot = std::chrono::steady_clock::now();
        Ecs c = canonical_ecs(v, h);
        std::vector<uint32_t> its(a.bootstraps);
        b.alpha.resize((size_t)a.bootstraps * v.n_paths);
        if (a.call_support) b.count.resize((size_t)a.bootstraps * c.n);
        if (groot_hip_em_bootstrap(device, v.n_paths, c.n, c.off.data(), c.ids.data(), c.cnt.data(), a.bootstraps, a.boot_seed, 0, GROOT_EM_MIN_ITER,
                                   GROOT_EM_MAX_ITER, a.call_support ? b.count.data() : nullptr, b.alpha.data(), its.data()))
            die("%s", groot_hip_last_error(nullptr));
        logf("\tbootstrap: %u replicate(s) of %llu equivalence class(es) on GPU %d (seed %llu), EM of %u to %u iteration(s), %.3f s", a.bootstraps,
             (unsigned long long)c.n, device, (unsigned long long)a.boot_seed, *std::min_element(its.begin(), its.end()),
             *std::max_element(its.begin(), its.end()), seconds_since(t_boot));
        if (a.call_support) b.ecs = std::move(c);
    }
    if (a.bootstraps ? groot_host_abundance_boot_from_ecs(&v, h.ec_cnt.size(), h.ec_off.data(), h.ec_ids.data(), h.ec_cnt.data(), a.abundance_min, a.bootstraps,
                                                          a.boot_seed, b.alpha.data(), 1, a.abundance_out.c_str(), &n_lines, &iters)
                     : groot_host_abundance_from_ecs(&v, h.ec_cnt.size(), h.ec_off.data(), h.ec_ids.data(), h.ec_cnt.data(), a.abundance_min, a.abundance_out.c_str(),
                                                     &n_lines, &iters))
        die("%s", groot_host_last_error());
    logf("\tabundance: %llu equivalence class(es), EM of %u iteration(s) in %.3f s, %llu ARG(s) with at least %g reads written to %s",
         (unsigned long long)h.ec_cnt.size(), iters, seconds_since(t_em), (unsigned long long)n_lines, a.abundance_min, a.abundance_out.c_str());
    if (plan.rescued_paired) {
        const groot_rescue_pairs_stats &r = h.rescue_pairs;
        logf("\tabundance: %llu rescued mate(s) counted in their fragments, placed with up to %ld substitution(s): exact + rescued %llu joined, %llu split; "
             "rescued + rescued %llu joined, %llu split; one mate alone %llu exact, %llu rescued; %llu unit(s) on ARGs of more than 4 graphs",
             (unsigned long long)r.rescued_mates, a.rescue, (unsigned long long)r.exact_rescued_joined, (unsigned long long)r.exact_rescued_split,
             (unsigned long long)r.rescued_rescued_joined, (unsigned long long)r.rescued_rescued_split, (unsigned long long)r.single_exact,
             (unsigned long long)r.single_rescued, (unsigned long long)r.bitmap_units);
    } else if (plan.ab_rescued) {
        uint64_t units = 0;
        for (uint64_t c : h.ec_cnt) units += c;
        logf("\tabundance: %llu rescued read(s) counted in the equivalence classes beside %llu read(s) with an exact alignment, placed with up to %ld substitution(s); "
             "%llu of them on ARGs of more than 4 graphs",
             (unsigned long long)h.rescue_ec.reads, (unsigned long long)(units - h.rescue_ec.reads - h.gap_ec.reads), a.rescue, (unsigned long long)h.rescue_ec.slow_reads);
    }
    if (plan.ab_gapped)
        logf("\tabundance: %llu gap-placed read(s) counted in the equivalence classes with them, placed with one deletion or insertion of up to %ld base(s); "
             "%llu of them on ARGs of more than 4 graphs",
             (unsigned long long)h.gap_ec.reads, a.rescue_gap, (unsigned long long)h.gap_ec.slow_reads);
    if (plan.rarefy && !plan.calls) {
        // the curve of the abundance file alone: over the merged ECs in canonical order, as the bootstrap takes them
        const Ecs c = canonical_ecs(v, h);
        rarefy_on_gpu(a, v, device, c.n, c.off.data(), c.ids.data(), c.cnt.data(), false, 0, nullptr, nullptr);
    }
    return b;
}

// --calls [--callSupport] [--rarefy]: the assigned-coverage tables of every harvest merged, then one line per line of the abundance file
void write_calls(const Args &a, const AlignPlan &plan, const groot_index_view &v, const Harvested &h, int device, const Bootstrap &boot)
{
    auto t_calls = std::chrono::steady_clock::now();
    const size_t k = h.acov.size();
    std::vector<const uint64_t *> p_off(k), p_cnt(k), p_tn(k);
    std::vector<const uint32_t *> p_ids(k), p_tup(k);
    std::vector<uint64_t> n_ec(k), n_tp(k);
    uint64_t s_ec = 0, s_ids = 0, s_tp = 0;
    for (size_t i = 0; i < k; i++) {
        const AcovExport &x = *h.acov[i];
        p_off[i] = x.off.data(); p_cnt[i] = x.cnt.data(); p_tn[i] = x.tn.data(); p_ids[i] = x.ids.data(); p_tup[i] = x.tuples.data();
        n_ec[i] = x.cnt.size(); n_tp[i] = x.tn.size();
        s_ec += x.cnt.size(); s_ids += x.ids.size(); s_tp += x.tn.size();
    }
    std::vector<uint64_t> m_off(s_ec + 1), m_cnt(s_ec + 1), m_tn(s_tp + 1);
    std::vector<uint32_t> m_ids(s_ids + 1), m_tup(4 * s_tp + 4);
    uint64_t m_ec = 0, m_tp = 0, n_lines = 0, n_called = 0;
    if (groot_host_acov_merge(v.n_paths, (uint32_t)k, p_off.data(), p_ids.data(), p_cnt.data(), n_ec.data(), p_tup.data(), p_tn.data(), n_tp.data(), m_off.data(),
                              m_ids.data(), m_cnt.data(), m_tup.data(), m_tn.data(), &m_ec, &m_tp))
        die("%s", groot_host_last_error());
    if (a.call_support && m_ec) {
        // the replicates of --bootstraps, piled up on the run's first GPU; the merged table's ECs are the bootstrap's canonical ECs
        auto t_sup = std::chrono::steady_clock::now();
        const Ecs &c = boot.ecs;
        if (m_ec != c.n || !std::equal(c.off.begin(), c.off.begin() + c.n + 1, m_off.begin()) || !std::equal(c.ids.begin(), c.ids.begin() + c.off[c.n], m_ids.begin()) ||
            !std::equal(c.cnt.begin(), c.cnt.begin() + c.n, m_cnt.begin()))
            die("--callSupport: the equivalence classes of the calls table are not those of the bootstrap");
        std::vector<double> alpha(v.n_paths);
        if (groot_host_em(v.n_paths, m_ec, m_off.data(), m_ids.data(), m_cnt.data(), GROOT_EM_MIN_ITER, GROOT_EM_MAX_ITER, alpha.data(), nullptr))
            die("%s", groot_host_last_error());
        std::vector<uint32_t> sel;
        for (uint32_t p = 0; p < v.n_paths; p++)
            if (alpha[p] >= a.abundance_min) sel.push_back(p);
        std::vector<uint32_t> covered((size_t)a.bootstraps * sel.size() + 1);
        if (groot_hip_call_support(device, v.n_paths, v.path_len, m_ec, m_off.data(), m_ids.data(), m_cnt.data(), m_tp, m_tup.data(), m_tn.data(), a.bootstraps,
                                   boot.count.data(), boot.alpha.data(), a.call_depth, (uint32_t)sel.size(), sel.data(), covered.data()))
            die("%s", groot_hip_last_error(nullptr));
        uint64_t rows = 0;
        uint32_t width = 0;
        groot_hip_call_support_info(&rows, &width, nullptr);
        logf("\tcall support: %u replicate(s), %zu path(s), %llu row(s) of u%u on GPU %d in %.3f s", a.bootstraps, sel.size(), (unsigned long long)rows, 8 * width,
             device, seconds_since(t_sup));
        if (groot_host_calls_support_from_table(&v, m_ec, m_off.data(), m_ids.data(), m_cnt.data(), alpha.data(), m_tp, m_tup.data(), m_tn.data(), a.abundance_min,
                                                a.call_depth, a.cov_cutoff, a.bootstraps, a.boot_seed, 1, boot.count.data(), boot.alpha.data(), covered.data(),
                                                a.calls_out.c_str(), &n_lines, &n_called))
            die("%s", groot_host_last_error());
    } else if (groot_host_calls_from_table(&v, m_ec, m_off.data(), m_ids.data(), m_cnt.data(), nullptr, m_tp, m_tup.data(), m_tn.data(), a.abundance_min, a.call_depth,
                                           a.cov_cutoff, a.calls_out.c_str(), &n_lines, &n_called))
        die("%s", groot_host_last_error());
    logf("\tcalls: %llu tuple(s) of (class, ARG, interval) from %zu context(s), %llu line(s), %llu called at depth >= %g over >= %.2f of the length, in %.3f s, written to %s",
         (unsigned long long)m_tp, k, (unsigned long long)n_lines, (unsigned long long)n_called, a.call_depth, a.cov_cutoff, seconds_since(t_calls), a.calls_out.c_str());
    if (plan.calls_rescued_paired)
        logf("\tcalls: fragments with a rescued mate: %llu exact record(s) beside a rescued partner piled up and %llu left out, %llu placement(s) of rescued mates piled up "
             "and %llu left out on ARGs outside their unit; %llu of them on ARGs of more than 4 graphs; the table started with %lld slot(s)",
             (unsigned long long)h.rescue_acov_pairs.exact_records, (unsigned long long)h.rescue_acov_pairs.exact_left_out, (unsigned long long)h.rescue_acov_pairs.rescued_records,
             (unsigned long long)h.rescue_acov_pairs.rescued_left_out, (unsigned long long)h.rescue_acov_pairs.host_records, a.call_slots);
    else if (plan.calls_rescued)
        logf("\tcalls: %llu rescued record(s) counted in the pileup, one per placement of a rescued read, %llu of them on ARGs of more than 4 graphs; the table started with %lld slot(s)",
             (unsigned long long)h.rescue_acov.records, (unsigned long long)h.rescue_acov.host_records, a.call_slots);
    if (plan.calls_gapped)
        logf("\tcalls: %llu gapped placement(s) of gap-placed reads piled up as %llu record(s), a deletion as two and an insertion as one, %llu of them on ARGs of more than 4 graphs",
             (unsigned long long)h.gap_acov.placements, (unsigned long long)h.gap_acov.records, (unsigned long long)h.gap_acov.host_records);
    if (plan.calls_paired)
        logf("\tcalls: %llu record(s) of fragments piled up, %llu left out on ARGs outside their fragment's set; %llu read(s) in joined fragments, %llu fragment(s) on ARGs of more than 4 graphs",
             (unsigned long long)h.acov_pairs.records, (unsigned long long)h.acov_pairs.left_out, (unsigned long long)h.acov_pairs.joined_reads,
             (unsigned long long)h.acov_pairs.slow_fragments);
    if (plan.rarefy) rarefy_on_gpu(a, v, device, m_ec, m_off.data(), m_ids.data(), m_cnt.data(), true, m_tp, m_tup.data(), m_tn.data());
}

// --report [--sharedReads]
void write_report(const Args &a, const AlignPlan &plan, const groot_index_view &v, const Harvested &h)
{
    uint64_t n_rep = 0;
    if (groot_host_report_coverage(&v, h.cov_records.data(), h.cov_depth.data(), a.cov_cutoff, a.low_cov ? 1 : 0, a.report_out.c_str(), &n_rep))
        die("%s", groot_host_last_error());
    logf("\treport: %llu ARG(s) written to %s (coverage cutoff %.2f%s)", (unsigned long long)n_rep, a.report_out.c_str(), a.low_cov ? 0.97 : a.cov_cutoff,
         a.low_cov ? ", --lowCov" : "");
    if (!plan.shared) return;
    uint64_t n_lines = 0;
    if (groot_host_shared_from_counts(&v, h.cov_records.data(), h.cov_depth.data(), a.cov_cutoff, a.low_cov ? 1 : 0, h.sh_a.size(), h.sh_a.data(), h.sh_b.data(),
                                      h.sh_n.data(), a.shared_out.c_str(), &n_lines))
        die("%s", groot_host_last_error());
    logf("\tshared reads: %llu pair(s) of reported ARGs written to %s", (unsigned long long)n_lines, a.shared_out.c_str());
}

// cmd/align.go:153-161: one file per kept graph, independent of each other: written side by side
void save_gfas(const Args &a, const groot_index_view &v, const std::string &graph_dir, const std::vector<double> &kf, const std::vector<uint8_t> &gk,
               const std::vector<uint8_t> &pk, const std::vector<uint8_t> &nr, uint64_t total_kmers)
{
    std::atomic<uint32_t> next_g{0};
    std::atomic<bool> gfa_failed{false};
    std::mutex gfa_mu;
    std::string gfa_err;
    auto save = [&]() {
        for (uint32_t g = next_g.fetch_add(1); g < v.n_graphs; g = next_g.fetch_add(1)) {
            if (!gk[g]) continue;
            const std::string fn = graph_dir + "/groot-graph-" + std::to_string(g) + ".gfa";
            int written = 0;
            if (groot_host_save_gfa(&v, g, kf.data(), pk.data(), nr.data(), total_kmers, nullptr, fn.c_str(), &written)) {
                std::lock_guard<std::mutex> lk(gfa_mu);
                if (!gfa_failed.exchange(true)) gfa_err = groot_host_last_error();
            }
        }
    };
    std::vector<std::thread> savers;
    for (int t = 1; t < std::max(1, std::min(a.proc, 16)); t++) savers.emplace_back(save);
    save();
    for (auto &t : savers) t.join();
    if (gfa_failed) die("%s", gfa_err.c_str());
}

// graph weights: exact call counts from the devices (summed over the GPUs: one RCCL all-reduce of a table with one row per kmerCount
// that occurred), one replay of IncrementSubPath on the host; then Prune and the GFAs of what remains (sketch.go:335-427)
void weigh_prune_save(Stream &s, const std::string &graph_dir)
{
    const groot_index_view &v = s.v;
    logf("\ttotal number of unmapped reads: %llu", (unsigned long long)(s.received - s.mapped_reads)); // sketch.go:335-339
    logf("\ttotal number of mapped reads: %llu", (unsigned long long)s.mapped_reads);
    logf("\t\tmapped to one graph: %llu", (unsigned long long)(s.mapped_reads - s.multimapped));
    logf("\t\tmapped to multiple graphs: %llu", (unsigned long long)s.multimapped);
    logf("\ttotal number of exact alignments: %llu", (unsigned long long)s.alignments);
    // (a context that met a longer read was reopened with a larger limit, the others were not: the tables can only be summed
    // over contexts with the same kmerCount range, so the shorter ones follow now)
    uint32_t longest = 0;
    for (auto &g : s.gpus) longest = std::max(longest, g->max_read_len);
    for (auto &g : s.gpus) {
        if (g->max_read_len == longest) continue;
        char why[200];
        snprintf(why, sizeof why, "\tGPU %d: reopening its context for reads up to %u bases (another context met one) before the call counts are summed", g->device, longest);
        if (const char *err = s.reopen(*g, longest, false, why)) die("%s", err);
    }
    std::vector<groot_ctx *> ctxs;
    for (auto &g : s.gpus) ctxs.push_back(g->ctx);
    if (groot_hip_attempts_allreduce(ctxs.data(), (int)ctxs.size())) die("%s", groot_hip_last_error(ctxs[0]));
    uint32_t n_rows = 0, nw = 0;
    std::vector<uint32_t> qv, counts;
    if (export_attempts(ctxs[0], qv, counts, &n_rows, &nw)) die("%s", groot_hip_last_error(ctxs[0]));
    std::vector<double> kf(v.n_nodes);
    std::vector<uint64_t> kt(v.n_graphs);
    if (groot_host_weights_rows(&v, qv.data(), n_rows, counts.data(), kf.data(), kt.data())) die("%s", groot_host_last_error());
    uint64_t total_kmers = 0;
    for (auto t : kt) total_kmers += t;
    logf("processing graphs...");
    logf("\ttotal number of k-mers projected onto graphs: %llu", (unsigned long long)total_kmers);   // sketch.go:346-347
    std::vector<uint8_t> gk(v.n_graphs), pk(v.n_paths), nr(v.n_nodes);
    if (groot_host_prune(&v, kf.data(), s.a.min_kmer_cov, gk.data(), pk.data(), nr.data())) die("%s", groot_host_last_error());
    uint32_t kept_graphs = 0, kept_paths = 0;
    for (uint32_t g = 0; g < v.n_graphs; g++) {
        if (!gk[g]) continue;
        kept_graphs++;
        // sketch.go:409: len(g.Paths) is never shrunk by Prune, so the reference logs the full path count
        logf("\tgraph %u has %u remaining paths after weighting and pruning", g, v.graph_path_off[g + 1] - v.graph_path_off[g]);
        for (uint32_t p = v.graph_path_off[g]; p < v.graph_path_off[g + 1]; p++)
            logf("\t- [%.*s]", (int)(v.path_name_off[p + 1] - v.path_name_off[p]), v.path_names + v.path_name_off[p]);
        kept_paths += v.graph_path_off[g + 1] - v.graph_path_off[g];
    }
    logf("\ttotal number of graphs pruned: %u", v.n_graphs);                                 // sketch.go:421-427
    if (!kept_graphs) { logf("\tno graphs remaining after pruning"); return; }
    logf("\ttotal number of graphs remaining: %u", kept_graphs);
    logf("\ttotal number of possible haplotypes found: %u", kept_paths);
    logf("saving graphs...");
    save_gfas(s.a, v, graph_dir, kf, gk, pk, nr, total_kmers);
}

struct RunTimes { double load_s, stream_s, post_s, total_s; };

// --stats: bench.py reads the keys
void write_stats(const Stream &s, const RunTimes &t, uint64_t bam_bytes)
{
    FILE *sf = fopen(s.a.stats_file.c_str(), "w");
    if (!sf) return;
    fprintf(sf, "{\"reads\": %llu, \"mapped\": %llu, \"alignments\": %llu, \"gpu_contexts\": %zu, \"load_s\": %.6f, \"stream_s\": %.6f, "
                "\"post_s\": %.6f, \"total_s\": %.6f, \"bam_bytes\": %llu, \"bam_level\": %d, \"threads\": %u, \"batches\": %llu, "
                "\"parse_busy_s\": %.6f, \"bam_busy_s\": %.6f, \"collect_wait_s\": %.6f, \"full_sketch_reads\": %llu}\n",
            (unsigned long long)s.received, (unsigned long long)s.mapped_reads, (unsigned long long)s.alignments, s.gpus.size(), t.load_s, t.stream_s,
            t.post_s, t.total_s, (unsigned long long)bam_bytes, s.a.bam_level, s.cores ? s.cores : groot_host_usable_cpus(),
            (unsigned long long)s.n_batches.load(), s.parse_s, s.bam_s, (double)s.collect_wait_us.load() / 1e6, (unsigned long long)s.full_sketch);
    fclose(sf);
}

// --variants: the summed rescue tables beside the exact depth of report coverage, and the run's stats in the log
void write_variants(const Args &a, const groot_index_view &v, const Harvested &h)
{
    uint64_t n = 0;
    if (groot_host_variants_write(&v, h.res_depth.data(), h.res_alt.data(), h.cov_depth.data(), (uint64_t)a.variant_min_reads, a.variant_min_share,
                                  a.variants_out.c_str(), &n))
        die("%s", groot_host_last_error());
    const groot_rescue_stats &r = h.rescue;
    logf("\tvariants: %llu unaligned read(s) tried with up to %ld substitution(s): %llu rescued (%llu without one) in %llu placement(s); left out: %llu too short, %llu not "
         "A/C/G/T; %llu line(s) written to %s (at least %lld read(s), share %g)",
         (unsigned long long)r.candidates, a.rescue, (unsigned long long)r.rescued, (unsigned long long)r.exact, (unsigned long long)r.placements,
         (unsigned long long)r.too_short, (unsigned long long)r.non_acgt, (unsigned long long)n, a.variants_out.c_str(), a.variant_min_reads, a.variant_min_share);
}

// --indels: the merged events beside the three depths, and the run's stats in the log
void write_indels(const Args &a, const groot_index_view &v, const Harvested &h)
{
    std::vector<groot_gap_event> ev;
    ev.reserve(h.gap_events.size());
    for (const auto &kv : h.gap_events) {
        groot_gap_event e{};
        e.path = kv.first[0]; e.pos = kv.first[1]; e.type = (uint8_t)kv.first[2]; e.len = (uint8_t)kv.first[3]; e.seq = (uint16_t)kv.first[4]; e.reads = kv.second;
        ev.push_back(e);
    }
    uint64_t n = 0;
    if (groot_host_indels_write(&v, ev.data(), ev.size(), h.gap_depth.data(), h.res_depth.data(), h.cov_depth.data(), (uint64_t)a.variant_min_reads, a.variant_min_share,
                                a.indels_out.c_str(), &n))
        die("%s", groot_host_last_error());
    const groot_gap_stats &g = h.gap;
    logf("\tindels: %llu read(s) left by up to %ld substitution(s) tried with one gap of up to %ld base(s): %llu rescued in %llu placement(s) (%llu DEL, %llu INS), %zu distinct "
         "event(s); left out: %llu too short; %llu line(s) written to %s (at least %lld read(s), share %g)",
         (unsigned long long)g.candidates, a.rescue, a.rescue_gap, (unsigned long long)g.rescued, (unsigned long long)g.placements, (unsigned long long)g.del_placements,
         (unsigned long long)g.ins_placements, ev.size(), (unsigned long long)g.too_short, (unsigned long long)n, a.indels_out.c_str(), a.variant_min_reads, a.variant_min_share);
}

} // namespace
