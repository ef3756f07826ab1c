// align, stages 1 and 2: what the flags ask for (or why they are refused), and the input files and directories.
#pragma once
#include "cli_common.hpp"

namespace {

struct AlignPlan {
    bool report = false, shared = false, abundance = false, calls = false, assign = false, rarefy = false, variants = false, indels = false;
    bool rescue = false;     // mismatch rescue runs: --variants, --indels or --abundanceRescued
    bool ab_rescued = false; // --abundanceRescued: the rescued reads join the equivalence classes
    bool ab_gapped = false;  // --abundanceGapped: and so do the gap-placed reads
    bool calls_rescued = false; // --callsRescued: and their kept placements the pileup of --calls
    bool calls_gapped = false;  // --callsGapped: and so do the gap-placed reads' (a DEL as two intervals, an INS as one)
    bool rescued_paired = false; // --rescuedPaired: --abundanceRescued over fragments (a rescued mate joins its fragment's unit with its rescued set)
    bool calls_rescued_paired = false; // --callsRescuedPaired: --calls over fragments with rescued mates (a record or placement counts on the paths of its mate's unit)
    bool calls_paired = false;  // --callsPaired: --calls over fragments (a joined fragment's records count on the paths of its set only)
    bool rescued_bam = false;   // --rescuedBam: the kept placements of the rescued reads as BAM records in a file of their own
    bool rescued_bam_gaps = false; // --rescuedBamGaps: and the kept placements of the gap-rescued reads with them
    bool coverage = false;   // report coverage is counted: --report, or --variants / --indels for its exact depth
    bool frags = false;      // --paired / --interleaved
    bool counters = false;   // a ctx carries switches: set at open and reopen, harvested before it closes
};

__attribute__((format(printf, 1, 2))) int refuse(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return 1;
}

// Every refusal of the flags, the first failing check first; 1 = refused (message written, nothing else touched: the log is not open yet)
int plan_align(const Args &a, AlignPlan *p)
{
    if (a.index_dir.empty()) { puts("please specify a directory with the index files (--indexDir)"); return 1; }
    if (a.fasta) return refuse("--fasta is an experimental reference feature that is not supported");
    p->report = !a.report_out.empty();
    if (p->report && a.no_align) return refuse("--report needs the exact alignments: it cannot be combined with --noAlign");
    if (p->report && a.cov_cutoff > 1.0) return refuse("supplied coverage cutoff exceeds 1.0 (100%%): %g", a.cov_cutoff);   // cmd/report.go:95-97
    p->shared = !a.shared_out.empty();
    if (p->shared && !p->report) return refuse("--sharedReads lists pairs of reported ARGs: it needs --report");
    p->abundance = !a.abundance_out.empty();
    if (p->abundance && a.no_align) return refuse("--abundance needs the exact alignments: it cannot be combined with --noAlign");
    if (a.bootstraps && !p->abundance) return refuse("--bootstraps adds columns to the abundance file: it needs --abundance");
    p->calls = !a.calls_out.empty();
    p->assign = !a.assign_from.empty();
    p->rarefy = !a.rarefy_out.empty();
    if (p->assign) {
        // the counters of S(r) see what assignment leaves of it -- one path per read
        const struct { bool on; const char *flag, *why; } refused[] = {
            {p->rarefy, "--rarefy", "it redoes the estimate of --abundance on subsamples, and an assigned read lies on one ARG: run it with the first pass"},
            {p->shared, "--sharedReads", "it counts the reads two ARGs share, and an assigned read lies on one ARG"},
            {p->abundance, "--abundance", "it estimates from every ARG a read lies on, and an assigned read lies on one: run it as the first pass"},
            {p->calls, "--calls", "it weighs every record of a read, and an assigned read keeps the records on one ARG"},
            {a.paired, "--paired", "fragments are not assigned yet: the mates would be assigned one by one"},
            {a.interleaved, "--interleaved", "fragments are not assigned yet: the mates would be assigned one by one"},
            {a.no_align, "--noAlign", "assignment filters the exact alignments, which it leaves out"},
        };
        for (const auto &r : refused)
            if (r.on) return refuse("--assignFrom cannot be combined with %s: %s", r.flag, r.why);
        if (!(a.min_posterior >= 0.0 && a.min_posterior <= 1.0)) return refuse("--minPosterior is a share: %g is not in [0, 1]", a.min_posterior);
        if (!is_file(a.assign_from)) return refuse("--assignFrom: no file found at %s", a.assign_from.c_str());
    } else if (a.min_posterior != 0.0) return refuse("--minPosterior is the threshold of --assignFrom: it needs it");
    if (p->rarefy && !p->abundance) return refuse("--rarefy redoes the estimate of --abundance at every depth: it needs --abundance");
    if (p->rarefy && (!a.rarefy_steps || !a.rarefy_reps)) return refuse("--rarefySteps and --rarefyReps must be at least 1");
    if (p->calls && !p->abundance) return refuse("--calls has a line per line of the abundance file: it needs --abundance");
    if (p->calls && a.no_align) return refuse("--calls needs the exact alignments: it cannot be combined with --noAlign");
    if (p->calls && (a.paired || a.interleaved) && !a.calls_paired)
        return refuse("--calls cannot be combined with --paired / --interleaved yet: a fragment's set is the intersection of its mates' sets, and the records "
                      "outside the intersection have no weight rule");
    if (a.call_support && !p->calls) return refuse("--callSupport adds columns to the calls file: it needs --calls");
    if (a.call_support && !a.bootstraps) return refuse("--callSupport is computed from the bootstrap replicates: it needs --bootstraps");
    if (p->calls && a.cov_cutoff > 1.0) return refuse("supplied coverage cutoff exceeds 1.0 (100%%): %g", a.cov_cutoff);
    if (a.no_bam && !p->report && !p->abundance) return refuse("--noBam without --report would leave no output of the alignments");
    if (a.no_bam && !a.bam_out.empty()) return refuse("--noBam and --bam contradict each other");
    if (a.paired && a.interleaved) return refuse("--paired and --interleaved contradict each other: the mates come in two files or in one");
    p->frags = a.paired || a.interleaved;
    if (p->frags && !p->shared && !p->abundance)
        return refuse("%s changes what --sharedReads and --abundance count, and nothing else: it needs one of them", a.paired ? "--paired" : "--interleaved");
    if (a.paired && (a.fastq.empty() || a.fastq.size() % 2))
        return refuse("--paired takes the -f files two at a time (R1,R2[,R1b,R2b...]): %zu file(s) given", a.fastq.size());
    // --variants: checked behind everything above
    p->variants = !a.variants_out.empty();
    if (p->variants && a.no_align) return refuse("--variants rescues the reads the exact alignments leave out: it cannot be combined with --noAlign");
    if (p->variants && p->assign) return refuse("--variants cannot be combined with --assignFrom: assignment rewrites the records that tell which reads are unaligned");
    p->indels = !a.indels_out.empty();
    p->ab_rescued = a.abundance_rescued;
    p->rescued_bam = !a.rescued_bam_out.empty();
    p->rescue = p->variants || p->indels || p->ab_rescued || p->rescued_bam;
    if (a.rescue_given && !p->rescue) return refuse("--rescue is the number of substitutions --variants allows: it needs it");
    if (a.variant_min_given && !p->variants && !p->indels) return refuse("--variantMinReads and --variantMinShare are the thresholds of --variants: they need it");
    if (p->rescue && (a.rescue < 1 || a.rescue > 3)) return refuse("--rescue allows 1, 2 or 3 substitutions: %ld", a.rescue);
    if (p->rescue && a.variant_min_reads < 0) return refuse("--variantMinReads is a number of reads: %lld", a.variant_min_reads);
    if (p->rescue && !(a.variant_min_share >= 0.0 && a.variant_min_share <= 1.0)) return refuse("--variantMinShare is a share: %g is not in [0, 1]", a.variant_min_share);
    // --indels: checked behind everything above
    if (p->indels && a.no_align) return refuse("--indels rescues the reads the exact alignments leave out: it cannot be combined with --noAlign");
    if (p->indels && p->assign) return refuse("--indels cannot be combined with --assignFrom: assignment rewrites the records that tell which reads are unaligned");
    if ((a.rescue_gap_given || a.gap_slots_given) && !p->indels) return refuse("--rescueGap and --gapEventSlots are the gap length and the table size of --indels: they need it");
    if (p->indels && (a.rescue_gap < 1 || a.rescue_gap > 8)) return refuse("--rescueGap allows a gap of 1 to 8 bases: %ld", a.rescue_gap);
    if (p->indels && a.gap_slots_given && (a.gap_event_slots < 1 || (a.gap_event_slots & (a.gap_event_slots - 1))))
        return refuse("--gapEventSlots is a number of table slots, a power of two: %lld", a.gap_event_slots);
    // --abundanceRescued: checked behind everything above
    if (p->ab_rescued && !p->abundance) return refuse("--abundanceRescued adds the rescued reads to the classes --abundance estimates from: it needs --abundance");
    if (p->ab_rescued && p->calls && !a.calls_rescued) return refuse("--abundanceRescued cannot be combined with --calls: its pileup weighs records, and a rescued read has none");
    if (p->ab_rescued && p->frags && !a.rescued_paired && a.calls_rescued_paired)      // (the one place a missing --rescuedPaired can be told: behind this check it would never be reached)
        return refuse("--callsRescuedPaired piles up under the units of --rescuedPaired: it needs --rescuedPaired");
    if (p->ab_rescued && p->frags && !a.rescued_paired)
        return refuse("--abundanceRescued cannot be combined with %s yet: mates are rescued one by one, and a fragment's set has no rule for them",
                      a.paired ? "--paired" : "--interleaved");
    // --callsRescued: checked behind everything above
    if (a.calls_rescued && !(p->calls && p->ab_rescued))
        return refuse("--callsRescued puts the reads --abundanceRescued adds to the classes into the pileup of --calls: it needs both --calls and --abundanceRescued");
    if (a.call_slots_given && !a.calls_rescued) return refuse("--callSlots is the size the table of --callsRescued starts with: it needs it");
    if (a.call_slots_given && (a.call_slots < 1 || a.call_slots > (1ll << 31) || (a.call_slots & (a.call_slots - 1))))
        return refuse("--callSlots is a number of table slots, a power of two up to 2^31: %lld", a.call_slots);
    p->calls_rescued = a.calls_rescued;
    // --rescuedBam: checked behind everything above
    if (p->rescued_bam && a.no_align) return refuse("--rescuedBam holds the reads the exact alignments leave out: it cannot be combined with --noAlign");
    if (p->rescued_bam && p->assign) return refuse("--rescuedBam cannot be combined with --assignFrom: assignment rewrites the records that tell which reads are unaligned");
    if (a.rescued_bam_slots_given && !p->rescued_bam) return refuse("--rescuedBamSlots is the room for the records of --rescuedBam: it needs it");
    if (a.rescued_bam_slots_given && a.rescued_bam_slots < 1) return refuse("--rescuedBamSlots is a number of records per batch, at least 1: %lld", a.rescued_bam_slots);
    if (p->rescued_bam && a.rescued_bam_out == a.bam_out) return refuse("--rescuedBam and --bam name the same file: %s", a.bam_out.c_str());
    // --rescuedBamGaps: checked behind everything above
    p->rescued_bam_gaps = a.rescued_bam_gaps;
    if (p->rescued_bam_gaps && !p->rescued_bam) return refuse("--rescuedBamGaps adds the gap-placed reads to the file of --rescuedBam: it needs it");
    if (p->rescued_bam_gaps && !p->indels) return refuse("--rescuedBamGaps writes the placements of gapped rescue, which --indels switches on: it needs it");
    if (a.gap_record_slots_given && !p->rescued_bam_gaps) return refuse("--gapRecordSlots is the room for the records of --rescuedBamGaps: it needs it");
    if (a.gap_record_slots_given && a.gap_record_slots < 1) return refuse("--gapRecordSlots is a number of records per batch, at least 1: %lld", a.gap_record_slots);
    // --abundanceGapped: checked behind everything above
    p->ab_gapped = a.abundance_gapped;
    if (p->ab_gapped && !p->ab_rescued) return refuse("--abundanceGapped adds the gap-placed reads to the classes beside the reads --abundanceRescued adds: it needs it");
    if (p->ab_gapped && !p->indels) return refuse("--abundanceGapped counts the reads gapped rescue places, which --indels switches on: it needs it");
    if (p->ab_gapped && p->calls && !(a.calls_gapped && p->calls_rescued))     // (--callsGapped is the rule)
        return refuse("--abundanceGapped cannot be combined with --calls%s: its pileup has no rule for a gapped record, and a deletion covers two intervals",
                      p->calls_rescued ? " --callsRescued" : "");
    // --callsGapped: checked behind everything above
    if (a.calls_gapped && !p->calls) return refuse("--callsGapped puts the reads --abundanceGapped adds to the classes into the pileup of --calls: it needs --calls");
    if (a.calls_gapped && !p->calls_rescued) return refuse("--callsGapped piles the gap-placed reads up beside the rescued reads' records: it needs --callsRescued");
    if (a.calls_gapped && !p->ab_gapped) return refuse("--callsGapped piles up the reads --abundanceGapped adds to the classes: it needs it");
    p->calls_gapped = a.calls_gapped;
    // --callsPaired: checked behind everything above (--assignFrom has refused --calls and --paired, --abundanceRescued and with it --callsRescued have refused --paired)
    if (a.calls_paired && !p->calls) return refuse("--callsPaired piles up the records of fragments in the file of --calls: it needs --calls");
    if (a.calls_paired && !p->frags) return refuse("--callsPaired is the rule for the records of fragments: it needs --paired or --interleaved");
    p->calls_paired = a.calls_paired;
    // --rescuedPaired: checked behind everything above (--assignFrom has refused --abundance and --paired)
    if (a.rescued_paired && !p->ab_rescued) return refuse("--rescuedPaired is the rule for the rescued mates of fragments: it needs --abundanceRescued");
    if (a.rescued_paired && !p->frags) return refuse("--rescuedPaired is the rule for the rescued mates of fragments: it needs --paired or --interleaved");
    if (a.rescued_paired && p->shared)
        return refuse("--rescuedPaired cannot be combined with --sharedReads: its pairs hold no rescued reads, and the fragments with a rescued mate would be missing from them");
    if (a.rescued_paired && p->calls && !a.calls_rescued_paired) return refuse("--rescuedPaired cannot be combined with --calls: its pileup has no rule for a fragment with a rescued mate");
    if (a.rescued_paired && p->ab_gapped) return refuse("--rescuedPaired cannot be combined with --abundanceGapped: the rule for fragments knows exact and mismatch-rescued mates only");
    p->rescued_paired = a.rescued_paired;
    // --callsRescuedPaired: checked behind everything above (it is the rule --rescuedPaired lacked beside --calls, and passes over that refusal alone)
    if (a.calls_rescued_paired && !p->calls) return refuse("--callsRescuedPaired piles up the fragments with rescued mates in the file of --calls: it needs --calls");
    if (a.calls_rescued_paired && !p->calls_paired) return refuse("--callsRescuedPaired extends the rule of --callsPaired to rescued mates: it needs --callsPaired");
    if (a.calls_rescued_paired && !p->calls_rescued) return refuse("--callsRescuedPaired piles up the placements --callsRescued counts, over fragments: it needs --callsRescued");
    // (--callsPaired has asked for fragments and --callsRescued for --abundanceRescued: a missing --rescuedPaired was refused where those two meet, above)
    p->calls_rescued_paired = a.calls_rescued_paired;
    p->coverage = p->report || p->variants || p->indels;
    p->counters = p->report || p->abundance || p->assign || p->rescue;
    return 0;
}

struct AlignInputs {
    std::string gidx, gg, lshe, graph_dir;   // <indexDir>/groot.gidx, or the reference's own groot.gg + groot.lshe; where the GFAs go
};

// The FASTQ files, the index directory and the graph directory (created here), with the log lines of cmd/align.go:165-197
AlignInputs check_inputs(const Args &a)
{
    logf("checking parameters...");
    for (auto &f : a.fastq) {
        if (!is_file(f)) die("no file found at %s", f.c_str());
        static const char *exts[] = {"fastq", "fq", "fasta", "fna", "fa"};   // misc.CheckExt (cmd/align.go:175)
        std::string base = f;
        if (base.size() > 3 && base.compare(base.size() - 3, 3, ".gz") == 0) base.resize(base.size() - 3);
        size_t dot = base.rfind('.');
        bool ok = false;
        for (auto e : exts) ok |= dot != std::string::npos && base.substr(dot + 1) == e;
        if (!ok) die("file does not have recognised extension: %s", f.c_str());
    }
    if (a.fastq.empty()) logf("\tinput file: using STDIN");
    if (!is_dir(a.index_dir)) die("no directory found at %s", a.index_dir.c_str());
    AlignInputs in;
    in.gidx = a.index_dir + "/groot.gidx";
    // an index directory of the reference itself (cmd/align.go:181-182: groot.gg + groot.lshe) is read through the gob reader
    in.gg = a.index_dir + "/groot.gg";
    in.lshe = a.index_dir + "/groot.lshe";
    if (!is_file(in.gidx) && !(is_file(in.gg) && is_file(in.lshe))) die("no file found at %s (nor groot.gg + groot.lshe)", in.gidx.c_str());
    in.graph_dir = a.graph_dir;
    if (in.graph_dir.empty()) {   // cmd/align.go:24: ./groot-graphs-<timestamp>
        char ts[32];
        time_t now = time(nullptr);
        struct tm tmv;
        localtime_r(&now, &tmv);
        strftime(ts, sizeof ts, "%Y%m%d%H%M%S", &tmv);
        in.graph_dir = std::string("./groot-graphs-") + ts;
    }
    make_dir(in.graph_dir);
    logf("\tminimum k-mer coverage: %.0f", a.min_kmer_cov);
    logf("\tprocessors: %d", a.proc);
    for (auto &f : a.fastq) logf("\tinput file: %s", f.c_str());
    return in;
}

} // namespace
