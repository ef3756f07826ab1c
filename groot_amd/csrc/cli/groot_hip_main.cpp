// groot-hip -- flag-compatible `index` and `align` subcommands on top of libgroot_host.so / libgroot_hip.so.
//
//   groot-hip index -m <msaDir> -i <indexDir> [-k 31 -s 21 -w 100 -x 8 -y 4 --maxSketchSpan 30 -p N --log F]
//        cmd/index.go:44-133: writes <indexDir>/groot.gidx (flat index) and the reference's groot.gg + groot.lshe
//   groot-hip align -i <indexDir> -f a.fq[,b.fq.gz] [-t 0.99 -c 1.0 -g <graphDir> --noAlign -p N --log F] > out.bam
//        cmd/align.go:30-197 + src/pipeline/sketch.go (DataStreamer..GraphPruner): BAM on stdout, weighted GFAs in
//        graphDir, the reference's log lines in --log (default groot.log)
//
// Extra flags: --gpu <id> (device) or --gpus <N> (reads shard over N GPUs), --batch <reads> (reads per device batch),
// --maxReadLen, --bam <file> (Info.Sketch.BAMout), --bamLevel, --stats <json>, --report <file> [--covCutoff --lowCov --noBam]
// (the `report` of the run from coverage counted on the GPU, with or without a BAM) [--sharedReads <file>] (for every pair of
// reported ARGs, the reads with records on both, counted on the GPU; needs --report); index: --writeGob.
// report: --sharedReads <file> writes the same pairs from the BAM, a read being one QNAME (the device counts input reads: the two
// agree whenever read names are unique).
// align / report: --abundance <file> [--abundanceMin 1.0]: per ARG the reads an EM over equivalence classes (distinct read sets,
// counted on the GPU under align, from the BAM by QNAME under report) assigns to it.
// The align hot path runs only on the GPU: no device -> error, never a CPU fallback.
//
// One translation unit.  This file: flags, usage, `index`, `report`, main, and run_align as the list of its stages; the stages are in
// the headers beside it, each including the one before: cli_common.hpp (log, die, Args) <- align_plan.hpp (refusals, input checks) <-
// align_counters.hpp (what the contexts count) <- align_stream.hpp (producer, mappers, writer, reopen) <- align_outputs.hpp (writers).
#include "align_outputs.hpp"

namespace {

void usage()
{
    fprintf(stderr,
            "groot-hip %s (MI355X-native groot align hot path)\n\n"
            "  groot-hip index -m <msaDir> -i <indexDir> [-k 31] [-s 21] [-w 100] [-x 8] [-y 4] [--maxSketchSpan 30] [-p N] [--log F]\n"
            "                  [--gpu 0]      (sketch the graph windows on that GPU instead of the host)\n"
            "                  [--writeGob]   (also write the reference's groot.gg + groot.lshe: experimental, unpinned against a Go-written file)\n"
            "  groot-hip align -i <indexDir> -f <fastq>[,<fastq>...] [-t 0.99] [-c 1.0] [-g <graphDir>] [--noAlign] [-p N] [--log F]\n"
            "                  [--gpu 0 | --gpus N] [--batch 1048576] [--maxReadLen 512] [--bam out.bam] [--bamLevel -2..9] [--stats f.json]\n"
            "                  [--memo auto|on|off|<MiB>]   (the device's memo of indexed strings; auto: on for inputs of 20 GB and more)\n"
            "                  [--report r.tsv [--covCutoff 0.97] [--lowCov] [--sharedReads s.tsv]] [--abundance a.tsv [--abundanceMin 1.0] [--abundanceRescued [--rescue 2]]]\n"
            "                  [--noBam] [--bootstraps B [--bootSeed 1]] [--paired | --interleaved] [--calls c.tsv [--callDepth 1.0] [--callSupport]]\n"
            "                  [--abundanceRescued --calls c.tsv --callsRescued [--callSlots 16777216]]\n"
            "                  [--abundance a.tsv --abundanceRescued --indels i.tsv --abundanceGapped [--rescueGap 3]]\n"
            "                  [--abundance a.tsv --abundanceRescued --indels i.tsv --abundanceGapped --calls c.tsv --callsRescued --callsGapped]\n"
            "                  [(--paired | --interleaved) --abundance a.tsv --calls c.tsv --callsPaired]\n"
            "                  [(--paired | --interleaved) --abundance a.tsv --abundanceRescued --rescuedPaired]\n"
            "                  [(--paired | --interleaved) --abundance a.tsv --abundanceRescued --rescuedPaired --calls c.tsv --callsPaired --callsRescued\n"
            "                   --callsRescuedPaired [--callSlots 16777216]]\n"
            "                  [--rarefy r.tsv [--rarefySteps 10] [--rarefyReps 20] [--rarefySeed 1]]\n"
            "                  [--assignFrom a.tsv [--minPosterior 0.0]]\n"
            "                  [--variants v.tsv [--rescue 2] [--variantMinReads 2] [--variantMinShare 0.1]]\n"
            "                  [--indels i.tsv [--rescueGap 3] [--gapEventSlots 4194304] [--rescue 2] [--variantMinReads 2] [--variantMinShare 0.1]]\n"
            "                  [--rescuedBam r.bam [--rescue 2] [--rescuedBamSlots N] [--rescuedBamGaps [--gapRecordSlots N]]]\n"
            "                  (BAM goes to stdout unless --bam; --gpus N shards the reads over N GPUs, index replicated;\n"
            "                   --report: the lines of `report` for this run, counted on the GPU; --noBam: no BAM at all (with --report or --abundance);\n"
            "                   --sharedReads: `nameA nameB reads` for every pair of reported ARGs with reads in common;\n"
            "                   --abundance: `name reads em_reads fraction` per ARG with em_reads >= --abundanceMin, by EM over the reads' path sets;\n"
            "                   --abundanceRescued: with --abundance, a read WITHOUT an exact alignment that mismatch rescue places with up to --rescue (1..3)\n"
            "                   substitutions counts too, with the set of ARGs it was placed on: `reads` then counts the reads that lie on the ARG exactly or\n"
            "                   rescued, and the EM, --bootstraps and --rarefy see them all.  Not with --paired or --interleaved, and with --calls only beside\n"
            "                   --callsRescued: then every placement of a rescued read is a record of the pileup too, over the bases it covers; --callSlots: the\n"
            "                   slots the pileup's table on the GPU starts with, a power of two (a run whose rescued records find no room fails and says so);\n"
            "                   --abundanceGapped: with --abundanceRescued and --indels, a read that gapped rescue places with one deletion or insertion of up\n"
            "                   to --rescueGap bases counts too, with the set of ARGs it was gap-placed on: `reads`, the EM, --bootstraps and --rarefy see it\n"
            "                   as they see the others.  With --calls only beside --callsRescued --callsGapped: then every gapped placement is piled up on\n"
            "                   the text bases it covers, a deletion as two records around the hole it leaves, an insertion as one;\n"
            "                   --bootstraps: with --abundance, four more columns `boot_mean boot_sd boot_lo boot_hi` from B replicates of the reads\n"
            "                   resampled with replacement (--bootSeed), each with its own EM, drawn and fitted on the GPU;\n"
            "                   --calls: with --abundance, per line of the abundance file `name em_reads length depth breadth cigar called`: the pileup of\n"
            "                   the reads the EM assigns to the ARG (a record weighs its read's posterior on that ARG); a base is covered at depth >=\n"
            "                   --callDepth, called = 1 at breadth >= --covCutoff;\n"
            "                   --callSupport: with --calls and --bootstraps, three more columns `support breadth_lo breadth_hi`: the pileup redone with\n"
            "                   every replicate's estimate and draw counts, on the GPU; support = the share of replicates in which the ARG is called;\n"
            "                   --rarefy: with --abundance, the rarefaction curve `fraction units args_mean args_lo args_hi` (with --calls also\n"
            "                   `called_mean called_lo called_hi`): the run's reads subsampled without replacement to s/--rarefySteps of its depth,\n"
            "                   nested, --rarefyReps times (--rarefySeed), the estimate redone at every depth, drawn and fitted on the GPU: a curve\n"
            "                   that has flattened says the sample was sequenced deeply enough;\n"
            "                   --assignFrom: a second pass over the same reads with the abundance file of a first (`--abundance a.tsv --noBam`): per read only\n"
            "                   the records on the ARG with the largest em_reads among those the read lies on are kept (ties: the first in BAM header order),\n"
            "                   and only when its share of their sum is >= --minPosterior; MAPQ = 3 per halving of the share of the others, 0..60.  The filter\n"
            "                   runs on the GPU ahead of the BAM writer and of --report, which then covers what was assigned.  Not with --sharedReads,\n"
            "                   --abundance, --calls, --paired, --interleaved or --noAlign;\n"
            "                   --variants: the reads WITHOUT an exact alignment are laid ungapped on the ARGs with up to --rescue (1..3) substitutions, on the\n"
            "                   GPU; `name pos ref alt alt_reads rescued_depth exact_depth share` for every base where at least --variantMinReads rescued reads\n"
            "                   show another base and they are at least --variantMinShare of the depth there.  The BAM and every other file stay as they are.\n"
            "                   Not with --assignFrom or --noAlign;\n"
            "                   --indels: the reads that stay unplaced even so are laid on the ARGs with ONE gap of up to --rescueGap (1..8) bases and up to --rescue\n"
            "                   substitutions, on the GPU; `name pos type len seq reads gap_depth rescued_depth exact_depth share` for every deletion or insertion\n"
            "                   that at least --variantMinReads of them show and that is at least --variantMinShare of the depth at pos, the base before the gap.\n"
            "                   With or without --variants; --gapEventSlots: the slots of the event table on the GPU, a power of two (a run that fills it fails);\n"
            "                   --rescuedBam: a BAM of its own with one record per placement of every read WITHOUT an exact alignment that mismatch rescue\n"
            "                   places with up to --rescue (1..3) substitutions: FLAG 0x10 for the reverse strand, 0x100 on a read's further placements, CIGAR\n"
            "                   <len>M, NM and MD tags; the main BAM and every other file stay as they are.  --rescuedBamSlots: room for that many records per\n"
            "                   batch on the GPU, 16 per read of --batch unless given (a batch with more fails the run and says so).  Not with --assignFrom or\n"
            "                   --noAlign;  --rescuedBamGaps (with --indels): the file also holds the reads gapped rescue places with one deletion or\n"
            "                   insertion of up to --rescueGap bases, one record per placement, merged with the others in read order: CIGAR <k>M<g>D<n>M or\n"
            "                   <k>M<g>I<n>M, NM = substitutions + gap bases, MD with ^ and the deleted bases.  --gapRecordSlots: room for that many of\n"
            "                   those records per batch on the GPU, 4 per read of --batch unless given (a batch with more fails the run and names the flag);\n"
            "                   --paired: the -f files are R1,R2[,R1b,R2b...], first with second, third with fourth; --interleaved: the mates alternate in\n"
            "                   one stream.  --sharedReads, --abundance and --bootstraps then count fragments, not mates: the mates' path sets intersected,\n"
            "                   or both sets when they do not intersect; the BAM holds the mates as ordinary records in interleaved order.  --calls only\n"
            "                   beside --callsPaired: both mates' records are piled up under the fragment's class, and a record of a fragment whose mates' sets\n"
            "                   intersect counts on the ARGs of the intersection only -- elsewhere the fragment has no posterior.  Not with --callsRescued.\n"
            "                   --abundanceRescued only beside --rescuedPaired: a mate without an exact alignment that mismatch rescue places counts in its\n"
            "                   fragment with the ARGs it was placed on, so an exact mate narrows a rescued one and two rescued mates still make a fragment.\n"
            "                   Not with --sharedReads, --calls, --abundanceGapped or --assignFrom.\n"
            "                   --callsRescuedPaired, beside --calls --callsPaired --callsRescued --rescuedPaired: the calls file over fragments with rescued\n"
            "                   mates -- a record or a placement of a mate counts on the ARGs of the mate's unit, the fragment's when its mates' sets\n"
            "                   intersect, and is left out elsewhere.  --callSlots is the room for the records piled up in one pass: the rescued mates'\n"
            "                   placements and the exact records of a mate joined with a rescued one (a run that drops one fails and names the flag))\n"
            "  groot-hip report [--bamFile x.bam] [-c 0.97] [--lowCov] [--sharedReads s.tsv] [--abundance a.tsv [--abundanceMin 1.0]] [--log F]\n"
            "                  [--bootstraps B [--bootSeed 1]] [-p N] [--calls c.tsv [--callDepth 1.0] [--callSupport]]\n"
            "                  [--rarefy r.tsv [--rarefySteps 10] [--rarefyReps 20] [--rarefySeed 1]]\n"
            "                  (BAM from stdin unless --bamFile; --bootstraps, --callSupport, --rarefy: the same columns as align writes, computed on -p\n"
            "                  host threads)\n",
            groot_host_version());
}

Args parse(int argc, char **argv)
{
    Args a;
    if (argc < 2) { usage(); exit(1); }
    a.cmd = argv[1];
    const bool ar = a.cmd == "align" || a.cmd == "report";
    auto need = [&](int &i) -> const char * {
        if (i + 1 >= argc) { fprintf(stderr, "flag needs an argument: %s\n", argv[i]); exit(1); }
        return argv[++i];
    };
    for (int i = 2; i < argc; i++) {
        std::string f = argv[i];
        std::string val;
        size_t eq = f.find('=');
        bool has_val = false;
        if (f.rfind("--", 0) == 0 && eq != std::string::npos) { val = f.substr(eq + 1); f = f.substr(0, eq); has_val = true; }
        auto v = [&]() -> std::string { return has_val ? val : std::string(need(i)); };
        if (f == "-i" || f == "--indexDir") a.index_dir = v();
        else if (f == "-m" || f == "--msaDir") a.msa_dir = v();
        else if (f == "--log") a.log_file = v();
        else if (f == "-p" || f == "--processors") a.proc = atoi(v().c_str());
        else if (f == "-k" || f == "--kmerSize") a.k = (uint32_t)atoi(v().c_str());
        else if (f == "-s" || f == "--sketchSize") a.s = (uint32_t)atoi(v().c_str());
        else if (f == "-w" || f == "--windowSize") a.w = (uint32_t)atoi(v().c_str());
        else if (f == "-x" || f == "--numPart") a.x = (uint32_t)atoi(v().c_str());
        else if (f == "-y" || f == "--maxK") a.y = (uint32_t)atoi(v().c_str());
        else if (f == "--maxSketchSpan") a.max_span = (uint32_t)atoi(v().c_str());
        else if (f == "-f" || f == "--fastq") { for (auto &x : split(v(), ',')) a.fastq.push_back(x); }
        else if (f == "-t" || f == "--contThresh") a.threshold = atof(v().c_str());
        else if ((a.cmd == "report" && (f == "-c" || f == "--covCutoff")) || (a.cmd == "align" && f == "--covCutoff")) a.cov_cutoff = atof(v().c_str());
        else if (a.cmd == "align" && f == "--report") a.report_out = v();
        else if (ar && f == "--sharedReads") a.shared_out = v();
        else if (ar && f == "--abundance") a.abundance_out = v();
        else if (ar && f == "--calls") a.calls_out = v();
        else if (ar && f == "--callDepth") a.call_depth = atof(v().c_str());
        else if (a.cmd == "align" && f == "--abundanceRescued") a.abundance_rescued = true;
        else if (a.cmd == "align" && f == "--abundanceGapped") a.abundance_gapped = true;
        else if (ar && f == "--abundanceMin") a.abundance_min = atof(v().c_str());
        else if (ar && f == "--bootstraps") a.bootstraps = (uint32_t)std::max(0l, atol(v().c_str()));
        else if (ar && f == "--bootSeed") a.boot_seed = strtoull(v().c_str(), nullptr, 10);
        else if (ar && f == "--callSupport") a.call_support = true;
        else if (ar && f == "--rarefy") a.rarefy_out = v();
        else if (ar && f == "--rarefySteps") a.rarefy_steps = (uint32_t)std::max(0l, atol(v().c_str()));
        else if (ar && f == "--rarefyReps") a.rarefy_reps = (uint32_t)std::max(0l, atol(v().c_str()));
        else if (ar && f == "--rarefySeed") a.rarefy_seed = strtoull(v().c_str(), nullptr, 10);
        else if (a.cmd == "align" && f == "--assignFrom") a.assign_from = v();
        else if (a.cmd == "align" && f == "--minPosterior") {   // (it decides which reads are kept: a value that is no number is refused, not read as 0)
            const std::string t = v();
            char *end = nullptr;
            a.min_posterior = strtod(t.c_str(), &end);
            if (t.empty() || end != t.c_str() + t.size()) { fprintf(stderr, "--minPosterior is a number in [0, 1]: %s\n", t.c_str()); exit(1); }
        }
        else if (a.cmd == "align" && f == "--variants") a.variants_out = v();
        else if (a.cmd == "align" && (f == "--rescue" || f == "--variantMinReads" || f == "--variantMinShare")) {   // (numbers that decide what is reported: refused when they are none)
            const std::string t = v();
            char *end = nullptr;
            if (f == "--rescue") { a.rescue = strtol(t.c_str(), &end, 10); a.rescue_given = true; }
            else if (f == "--variantMinReads") { a.variant_min_reads = strtoll(t.c_str(), &end, 10); a.variant_min_given = true; }
            else { a.variant_min_share = strtod(t.c_str(), &end); a.variant_min_given = true; }
            if (t.empty() || end != t.c_str() + t.size()) { fprintf(stderr, "%s takes a number: %s\n", f.c_str(), t.c_str()); exit(1); }
        }
        else if (a.cmd == "align" && f == "--indels") a.indels_out = v();
        else if (a.cmd == "align" && (f == "--rescueGap" || f == "--gapEventSlots")) {
            const std::string t = v();
            char *end = nullptr;
            if (f == "--rescueGap") { a.rescue_gap = strtol(t.c_str(), &end, 10); a.rescue_gap_given = true; }
            else { a.gap_event_slots = strtoll(t.c_str(), &end, 10); a.gap_slots_given = true; }
            if (t.empty() || end != t.c_str() + t.size()) { fprintf(stderr, "%s takes a number: %s\n", f.c_str(), t.c_str()); exit(1); }
        }
        else if (a.cmd == "align" && f == "--callsRescued") a.calls_rescued = true;
        else if (a.cmd == "align" && f == "--callsGapped") a.calls_gapped = true;
        else if (a.cmd == "align" && f == "--callsPaired") a.calls_paired = true;
        else if (a.cmd == "align" && f == "--rescuedPaired") a.rescued_paired = true;
        else if (a.cmd == "align" && f == "--callsRescuedPaired") a.calls_rescued_paired = true;
        else if (a.cmd == "align" && f == "--callSlots") {
            const std::string t = v();
            char *end = nullptr;
            a.call_slots = strtoll(t.c_str(), &end, 10); a.call_slots_given = true;
            if (t.empty() || end != t.c_str() + t.size()) { fprintf(stderr, "%s takes a number: %s\n", f.c_str(), t.c_str()); exit(1); }
        }
        else if (a.cmd == "align" && f == "--rescuedBam") a.rescued_bam_out = v();
        else if (a.cmd == "align" && f == "--rescuedBamSlots") {
            const std::string t = v();
            char *end = nullptr;
            a.rescued_bam_slots = strtoll(t.c_str(), &end, 10); a.rescued_bam_slots_given = true;
            if (t.empty() || end != t.c_str() + t.size()) { fprintf(stderr, "%s takes a number: %s\n", f.c_str(), t.c_str()); exit(1); }
        }
        else if (a.cmd == "align" && f == "--rescuedBamGaps") a.rescued_bam_gaps = true;
        else if (a.cmd == "align" && f == "--gapRecordSlots") {
            const std::string t = v();
            char *end = nullptr;
            a.gap_record_slots = strtoll(t.c_str(), &end, 10); a.gap_record_slots_given = true;
            if (t.empty() || end != t.c_str() + t.size()) { fprintf(stderr, "%s takes a number: %s\n", f.c_str(), t.c_str()); exit(1); }
        }
        else if (a.cmd == "align" && f == "--noBam") a.no_bam = true;
        else if (ar && f == "--paired") a.paired = true;
        else if (ar && f == "--interleaved") a.interleaved = true;
        else if (f == "--bamFile") a.bam_file = v();
        else if (f == "--lowCov") a.low_cov = true;
        else if (f == "-c" || f == "--minKmerCov") a.min_kmer_cov = atof(v().c_str());
        else if (f == "-g" || f == "--graphDir") a.graph_dir = v();
        else if (f == "--noAlign") a.no_align = true;
        else if (f == "--fasta") a.fasta = true;
        else if (f == "--profiling") {}
        else if (f == "--gpu") { a.gpu = atoi(v().c_str()); a.gpu_given = true; }
        else if (f == "--batch") a.batch = (uint32_t)atol(v().c_str());
        else if (f == "--gpus") a.gpus = atoi(v().c_str());
        else if (f == "--ctxPerGpu") a.ctx_per_gpu = std::max(1, atoi(v().c_str()));
        else if (f == "--maxReadLen") a.max_read_len = (uint32_t)atol(v().c_str());
        else if (f == "--depth") a.depth = (uint32_t)atol(v().c_str());
        else if (f == "--bamLevel") a.bam_level = atoi(v().c_str());
        else if (f == "--blockBytes") a.block_bytes = (uint64_t)atoll(v().c_str());
        else if (f == "--stats") a.stats_file = v();
        else if (f == "--writeGob") a.write_gob = true;
        else if (f == "--bam") a.bam_out = v();
        else if (f == "--memo") a.memo = v();
        else if (f == "-h" || f == "--help") { usage(); exit(0); }
        else { fprintf(stderr, "unknown flag: %s\n", f.c_str()); usage(); exit(1); }
    }
    return a;
}

// ---------------------------------------------------------------------------------------------
int run_index(const Args &a)   // cmd/index.go:57-133
{
    if (a.index_dir.empty()) { puts("please specify a directory for the index files (--indexDir)"); return 1; }
    if (a.msa_dir.empty()) { fprintf(stderr, "required flag(s) \"msaDir\" not set\n"); return 1; }
    start_logging(a);
    auto t0 = std::chrono::steady_clock::now();
    logf("i am groot (version %s)", groot_host_version());
    logf("starting the index subcommand");
    logf("checking parameters...");
    logf("\tdirectory containing MSA files: %s", a.msa_dir.c_str());
    if (!is_dir(a.msa_dir)) die("no directory found at %s", a.msa_dir.c_str());
    if (a.k > a.w) die("supplied k-mer size greater than read length");
    make_dir(a.index_dir);
    logf("\tprocessors: %d", a.proc);
    logf("\tk-mer size: %u", a.k);
    logf("\tsketch size: %u", a.s);
    logf("\tgraph window size: %u", a.w);
    logf("\tnum. partitions: %u", a.x);
    logf("\tmax. K: %u", a.y);
    logf("\tmax. sketch span: %u", a.max_span);
    logf("creating graphs, sketching traversals and indexing...");
    groot_index_params p;
    groot_index_params_default(&p);
    p.kmer_size = a.k; p.sketch_size = a.s; p.window_size = a.w; p.num_part = a.x; p.max_k = a.y; p.max_sketch_span = a.max_span;
    p.n_threads = a.proc > 0 ? (uint32_t)a.proc : 0;
    groot_index *idx = nullptr;
    if (a.gpu_given) {
        // window sketches on the GPU: a ctx opened on an index view without graphs is a pure RunMinHash engine
        logf("\tsketching graph windows on GPU %d", a.gpu);
        groot_index_view empty;
        memset(&empty, 0, sizeof empty);
        empty.kmer_size = a.k; empty.sketch_size = a.s; empty.window_size = a.w; empty.num_part = a.x; empty.max_k = a.y;
        empty.num_window_kmers = a.w - a.k + 1; empty.path_words = 1;
        groot_params prm;
        groot_params_default(&prm);
        prm.max_read_len = std::max<uint32_t>(a.w, 64);
        prm.max_batch_reads = 1u << 16;
        groot_ctx *ctx = nullptr;
        if (groot_hip_open(&ctx, a.gpu, &empty, &prm)) die("%s", groot_hip_last_error(nullptr));
        struct Sk { groot_ctx *ctx; uint32_t s, max_n; } sk{ctx, a.s, prm.max_batch_reads};
        auto fn = [](void *user, const uint8_t *seq, const uint64_t *off, uint32_t n, uint64_t *out) -> int {
            Sk *k = (Sk *)user;
            std::vector<uint64_t> rel;
            for (uint32_t i = 0; i < n; i += k->max_n) {
                const uint32_t m = std::min(k->max_n, n - i);
                rel.resize(m + 1);
                for (uint32_t j = 0; j <= m; j++) rel[j] = off[i + j] - off[i];
                if (groot_hip_sketch(k->ctx, seq + off[i], rel.data(), m, out + (size_t)i * k->s)) return -1;
            }
            return 0;
        };
        const int rc = groot_index_build_msa_dir_with(a.msa_dir.c_str(), &p, fn, &sk, &idx);
        if (rc) die("%s (%s)", groot_host_last_error(), groot_hip_last_error(ctx));
        groot_hip_close(ctx);
    } else if (groot_index_build_msa_dir(a.msa_dir.c_str(), &p, &idx)) die("%s", groot_host_last_error());
    groot_index_view v;
    groot_index_get_view(idx, &v);
    uint32_t masked = 0;
    for (uint32_t g = 0; g < v.n_graphs; g++) masked += v.graph_masked[g];
    logf("\tnumber of groot graphs built: %u", v.n_graphs);
    logf("\t\tgraphs sketched: %u", v.n_graphs - masked);
    logf("\tnumber of sketches added to the LSH Ensemble index: %u", v.n_windows);
    const std::string out = a.index_dir + "/groot.gidx";
    logf("writing index files in \"%s\"...", a.index_dir.c_str());
    if (groot_index_save(idx, out.c_str())) die("%s", groot_host_last_error());
    // the reference's own files (cmd/index.go:130-131) only on request: no Go-written groot.gg / groot.lshe has been
    // round-tripped yet, so a layout or hash-constant slip would make the reference mis-seed silently
    if (a.write_gob) {
        logf("\twriting groot.gg + groot.lshe (experimental: not yet checked against files written by the reference)");
        if (groot_index_save_gob(idx, a.index_dir.c_str(), a.max_span)) die("%s", groot_host_last_error());
    }
    groot_index_free(idx);
    logf("finished in %.3fs", seconds_since(t0));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// align (cmd/align.go:54-163), stage by stage; the stages themselves are in align_plan.hpp .. align_outputs.hpp
int run_align(const Args &a)
{
    AlignPlan plan;
    if (plan_align(a, &plan)) return 1;                                                          // 1. plan
    start_logging(a);
    auto t0 = std::chrono::steady_clock::now();
    logf("i am groot (version %s)", groot_host_version());
    logf("starting the sketch subcommand");
    const AlignInputs in = check_inputs(a);                                                      // 2. check inputs
    Stream s(a, plan);
    s.open_reads();                                                                              // 3. start the parser
    std::thread producer(&Stream::producer, &s);
    logf("loading the index information...");                                                    // 4. load the index while HIP starts
    // (the HIP runtime starts up on a thread of its own while the index is read: a few tenths of a second each)
    int n_dev = 0, dev_rc = 0;
    std::thread hip_init([&]() { dev_rc = groot_hip_device_count(&n_dev); });
    groot_index *idx = nullptr;
    const int load_rc = is_file(in.gidx) ? groot_index_load(in.gidx.c_str(), &idx) : groot_index_load_gob(in.gg.c_str(), in.lshe.c_str(), &idx);
    hip_init.join();
    if (load_rc) die("%s", groot_host_last_error());
    const groot_index_view &v = s.v;
    groot_index_get_view(idx, &s.v);
    logf("\tk-mer size: %u", v.kmer_size);
    logf("\tsketch size: %u", v.sketch_size);
    logf("\twindow size used in indexing: %u", v.window_size);
    logf("loading the graphs...");
    logf("\tnumber of variation graphs: %u", v.n_graphs);
    logf("rebuilding the LSH Ensemble...");
    if (dev_rc || n_dev == 0) die("no HIP device available (groot-hip align has no CPU fallback): %s", groot_hip_last_error(nullptr));
    s.open_contexts(n_dev);                                                                      // 5. open contexts
    logf("\tcontainment threshold: %.2f", a.threshold);
    if (a.no_align) logf("\tprevent exact alignments and using approximated mapping only");
    logf("initialising alignment pipeline...");
    logf("\tinitialising the processes");
    logf("\tconnecting data streams");
    logf("\tnumber of processes added to the alignment pipeline: 5");
    if (s.gpus.size() > 1) logf("\treads shard over %zu GPU contexts (index replicated)", s.gpus.size());
    RunTimes t{};
    t.load_s = seconds_since(t0);
    if (!a.no_align && !a.no_bam && groot_bam_open(a.bam_out.empty() ? nullptr : a.bam_out.c_str(), &v, nullptr, &s.bam)) die("%s", groot_host_last_error());
    if (s.bam) { groot_bam_set_threads(s.bam, s.cores); if (groot_bam_set_level(s.bam, a.bam_level)) die("%s", groot_host_last_error()); }
    if (plan.rescued_bam && groot_bam_open(a.rescued_bam_out.c_str(), &v, nullptr, &s.rescued_bam)) die("%s", groot_host_last_error());

    logf("now streaming reads...");                                                              // 6. stream
    auto t_stream = std::chrono::steady_clock::now();
    s.mapped.cap = s.gpus.size() * s.depth + 2;
    s.mappers_left = (int)s.gpus.size();
    s.gpus_ready = true;
    std::vector<std::thread> mappers;
    for (auto &g : s.gpus) mappers.emplace_back(&Stream::mapper, &s, std::ref(*g));
    s.writer();
    for (auto &m : mappers) m.join();
    producer.join();
    for (auto &g : s.gpus) if (g->ctx) groot_hip_open_abandon(g->ctx);   // (a short input can end before the background part of the open has)
    if (s.failed) die("%s", s.fatal.c_str());
    groot_reads_close(s.reads);
    if (s.received == 0) die("no fastq reads received");                                         // sketch.go:275-277
    logf("\tnumber of reads received from input: %llu", (unsigned long long)s.received);         // sketch.go:278-280
    logf("\tmean read length: %.0f", (double)s.length_total.load() / (double)s.received);
    logf("\tnumber of reads sketched: %llu", (unsigned long long)s.received);                    // sketch.go:321
    const uint64_t bam_bytes = s.bam ? groot_bam_bytes_written(s.bam) : 0;
    if (s.bam && groot_bam_close(s.bam)) die("%s", groot_host_last_error());
    if (s.rescued_bam) {
        if (groot_bam_close(s.rescued_bam)) die("%s", groot_host_last_error());
        logf("\trescued reads: %llu record(s) of %llu read(s) written to %s (up to %ld substitution(s))", (unsigned long long)s.rescued_records,
             (unsigned long long)s.rescued_reads, a.rescued_bam_out.c_str(), a.rescue);
        if (plan.rescued_bam_gaps)
            logf("\tgap-placed reads: %llu record(s) of %llu read(s) among them (one gap of up to %ld base(s))", (unsigned long long)s.gapped_records,
                 (unsigned long long)s.gapped_reads, a.rescue_gap);
    }
    if (plan.counters)                                                                           // 7. harvest
        // every batch has been collected: what each ctx counted is final (it is switched off, so a ctx reopened below starts without it)
        for (auto &g : s.gpus)
            if (s.counters->harvest(g->ctx) || s.counters->enable(g->ctx, 0)) die("%s", groot_hip_last_error(g->ctx));
    const Harvested &h = s.counters->totals();
    if (plan.assign)
        logf("\tassignment: %llu read(s) with records: %llu assigned (%llu on a tie), %llu unassigned, %llu below the minimum posterior; %llu record(s) in, %llu kept, %llu traversal(s) emptied",
             (unsigned long long)h.assign.reads, (unsigned long long)h.assign.assigned, (unsigned long long)h.assign.ties, (unsigned long long)h.assign.unassigned,
             (unsigned long long)h.assign.below, (unsigned long long)h.assign.records_in, (unsigned long long)h.assign.records_kept,
             (unsigned long long)h.assign.travs_emptied);
    if (plan.frags)
        logf("\tpaired-end input: %llu fragment(s), %llu joined, %llu split, %llu single", (unsigned long long)(s.received / 2), (unsigned long long)h.fr_joined,
             (unsigned long long)h.fr_split, (unsigned long long)h.fr_single);
    const int first_device = s.gpus[0]->device;                                                  // 8. write outputs
    Bootstrap boot;
    if (plan.abundance) boot = write_abundance(a, plan, v, h, first_device);
    if (plan.calls) write_calls(a, plan, v, h, first_device, boot);
    if (plan.report) write_report(a, plan, v, h);
    if (plan.variants) write_variants(a, v, h);
    if (plan.indels) write_indels(a, v, h);
    t.stream_s = seconds_since(t_stream);
    auto t_post = std::chrono::steady_clock::now();
    if (s.mapped_reads == 0) logf("no reads could be mapped to the reference graphs");           // sketch.go:328-334
    else weigh_prune_save(s, in.graph_dir);                                                      // 9. weigh, prune and save
    // (the contexts and the index are NOT torn down: the process ends here -- log and stats written, BAM and GFAs closed -- and handing a few
    // GB of HBM and host memory back buffer by buffer, then unloading the HIP runtime, costs a tenth of a second that no output needs:
    // main() leaves through _exit once everything is flushed)
    for (auto &g : s.gpus) if (g->ctx) groot_hip_open_abandon(g->ctx);
    (void)idx;
    t.post_s = seconds_since(t_post);
    t.total_s = seconds_since(t0);
    if (!a.stats_file.empty()) write_stats(s, t, bam_bytes);                                     // 10. stats
    logf("finished in %.3fs", t.total_s);
    return 0;
}

// cmd/report.go:104-129
int run_report(const Args &a)
{
    if (a.paired || a.interleaved) {
        fprintf(stderr, "report cannot pair the records of a BAM: it carries no mate flags, and mates with equal QNAMEs cannot be told apart -- use "
                        "`align --paired` (or --interleaved) with --sharedReads / --abundance\n");
        return 1;
    }
    start_logging(a);
    logf("i am groot (version %s)", groot_host_version());
    logf("starting the report subcommand");
    logf("checking parameters...");
    if (a.call_support && a.calls_out.empty()) die("--callSupport adds columns to the calls file: it needs --calls");
    if (a.call_support && !a.bootstraps) die("--callSupport is computed from the bootstrap replicates: it needs --bootstraps");
    if (!a.rarefy_out.empty() && a.abundance_out.empty()) die("--rarefy redoes the estimate of --abundance at every depth: it needs --abundance");
    if (!a.rarefy_out.empty() && (!a.rarefy_steps || !a.rarefy_reps)) die("--rarefySteps and --rarefyReps must be at least 1");
    if (a.bam_file.empty()) logf("\tBAM file: using STDIN");
    else {
        if (!is_file(a.bam_file)) die("BAM file does not exist: %s", a.bam_file.c_str());
        const size_t dot = a.bam_file.rfind('.');
        if (dot == std::string::npos || a.bam_file.substr(dot + 1) != "bam") die("the BAM file does not have a `.bam` extension: %s", a.bam_file.c_str());
        logf("\tBAM file: %s", a.bam_file.c_str());
    }
    if (a.cov_cutoff > 1.0) die("supplied coverage cutoff exceeds 1.0 (100%%): %g", a.cov_cutoff);
    if (a.bootstraps && a.abundance_out.empty()) die("--bootstraps adds columns to the abundance file: it needs --abundance");
    if (!a.calls_out.empty() && a.abundance_out.empty()) die("--calls has a line per line of the abundance file: it needs --abundance");
    logf("\tcoverage cutoff: %.2f", a.cov_cutoff);
    logf("\tprocessors: %d", a.proc);
    uint64_t n = 0, n_lines = 0;
    const char *bam = a.bam_file.empty() ? nullptr : a.bam_file.c_str();
    // --abundance reads the BAM a second time: a BAM on stdin is spooled to a temporary file first
    std::string spool;
    if (!bam && !a.abundance_out.empty()) {
        const char *td = getenv("TMPDIR");
        spool = std::string(td && *td ? td : "/tmp") + "/groot-report-XXXXXX";
        const int fd = mkstemp(&spool[0]);
        FILE *f = fd < 0 ? nullptr : fdopen(fd, "wb");
        if (!f) die("cannot create a temporary file for the BAM on stdin");
        std::vector<char> buf(1 << 20);
        for (size_t k; (k = fread(buf.data(), 1, buf.size(), stdin)) > 0;)
            if (fwrite(buf.data(), 1, k, f) != k) { fclose(f); unlink(spool.c_str()); die("cannot write %s", spool.c_str()); }
        fclose(f);
        bam = spool.c_str();
    }
    if (a.shared_out.empty() ? groot_host_report(bam, a.cov_cutoff, a.low_cov ? 1 : 0, nullptr, &n)
                             : groot_host_report_shared(bam, a.cov_cutoff, a.low_cov ? 1 : 0, nullptr, a.shared_out.c_str(), &n, &n_lines))
        die("%s", groot_host_last_error());
    if (!a.shared_out.empty()) logf("\tshared reads: %llu pair(s) of reported ARGs written to %s", (unsigned long long)n_lines, a.shared_out.c_str());
    if (!a.abundance_out.empty()) {
        if (a.bootstraps ? groot_host_report_abundance_boot(bam, a.abundance_min, a.bootstraps, a.boot_seed, (uint32_t)std::max(1, a.proc),
                                                            a.abundance_out.c_str(), &n_lines)
                         : groot_host_report_abundance(bam, a.abundance_min, a.abundance_out.c_str(), &n_lines))
            die("%s", groot_host_last_error());
        if (a.bootstraps) logf("\tbootstrap: %u replicate(s) on %d host thread(s) (seed %llu)", a.bootstraps, std::max(1, a.proc), (unsigned long long)a.boot_seed);
        logf("\tabundance: %llu ARG(s) with at least %g reads written to %s", (unsigned long long)n_lines, a.abundance_min, a.abundance_out.c_str());
    }
    if (!a.calls_out.empty()) {
        uint64_t n_called = 0, n_tuples = 0;
        auto t_calls = std::chrono::steady_clock::now();
        if (a.call_support ? groot_host_report_calls_support(bam, a.abundance_min, a.call_depth, a.cov_cutoff, a.bootstraps, a.boot_seed, (uint32_t)std::max(1, a.proc),
                                                             a.calls_out.c_str(), &n_lines, &n_called, &n_tuples)
                           : groot_host_report_calls(bam, a.abundance_min, a.call_depth, a.cov_cutoff, a.calls_out.c_str(), &n_lines, &n_called, &n_tuples))
            die("%s", groot_host_last_error());
        if (a.call_support) logf("\tcall support: %u replicate(s) on %d host thread(s) (seed %llu)", a.bootstraps, std::max(1, a.proc), (unsigned long long)a.boot_seed);
        logf("\tcalls: %llu tuple(s) of (class, ARG, interval), %llu line(s), %llu called at depth >= %g over >= %.2f of the length, in %.3f s, written to %s",
             (unsigned long long)n_tuples, (unsigned long long)n_lines, (unsigned long long)n_called, a.call_depth, a.cov_cutoff, seconds_since(t_calls), a.calls_out.c_str());
    }
    if (!a.rarefy_out.empty()) {
        auto t_rare = std::chrono::steady_clock::now();
        uint32_t its[2] = {0, 0};
        if (groot_host_report_rarefy(bam, a.abundance_min, a.rarefy_reps, a.rarefy_steps, a.rarefy_seed, (uint32_t)std::max(1, a.proc), a.calls_out.empty() ? 0 : 1,
                                     a.call_depth, a.cov_cutoff, a.rarefy_out.c_str(), &n_lines, its))
            die("%s", groot_host_last_error());
        logf("\trarefaction: %u step(s), %u replicate(s) on %d host thread(s) (seed %llu), EM of %u to %u iteration(s), %llu line(s)%s in %.3f s, written to %s",
             a.rarefy_steps, a.rarefy_reps, std::max(1, a.proc), (unsigned long long)a.rarefy_seed, its[0], its[1], (unsigned long long)n_lines,
             a.calls_out.empty() ? "" : " with the called columns", seconds_since(t_rare), a.rarefy_out.c_str());
    }
    if (!spool.empty()) unlink(spool.c_str());
    logf("finished");
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    Args a = parse(argc, argv);
    if (a.cmd == "index") return run_index(a);
    if (a.cmd == "align") {
        const int rc = run_align(a);
        fflush(nullptr);
        _exit(rc);                                      // (see the end of run_align)
    }
    if (a.cmd == "report") return run_report(a);
    if (a.cmd == "version") { printf("%s\n", groot_host_version()); return 0; }
    usage();
    return 1;
}
