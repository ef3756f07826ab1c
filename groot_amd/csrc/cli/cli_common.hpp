// groot-hip is ONE translation unit: groot_hip_main.cpp includes this and the align_*.hpp beside it once each, as the .hip units do with
// their kernels_*.hpp.  Here: what every subcommand shares -- the log (Go's log.LstdFlags), die, the parsed flags, small file helpers.
#pragma once
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <ctime>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "groot_hip.h"

namespace {

FILE *g_log = nullptr;

void logf(const char *fmt, ...)
{
    char ts[32];
    time_t now = time(nullptr);
    struct tm tmv;
    localtime_r(&now, &tmv);
    strftime(ts, sizeof ts, "%Y/%m/%d %H:%M:%S", &tmv);   // Go's log.LstdFlags
    fprintf(g_log ? g_log : stderr, "%s ", ts);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(g_log ? g_log : stderr, fmt, ap);
    va_end(ap);
    fputc('\n', g_log ? g_log : stderr);
    fflush(g_log ? g_log : stderr);
}

[[noreturn]] void die(const char *fmt, ...)   // misc.ErrorCheck -> log.Fatalf
{
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    logf("%s", buf);
    if (g_log) fprintf(stderr, "%s\n", buf);
    fflush(nullptr);
    _exit(1);                                           // (parser / mapper / HIP threads may be running: no static destructors under their feet)
}

struct Args {
    std::string cmd, index_dir, msa_dir, log_file = "groot.log", graph_dir, bam_out, bam_file, report_out, shared_out, abundance_out, calls_out, assign_from;
    double cov_cutoff = 0.97, abundance_min = 1.0, call_depth = 1.0, min_posterior = 0.0;   // --assignFrom <abundance file> [--minPosterior P]
    bool low_cov = false, no_bam = false;
    bool paired = false, interleaved = false;   // --paired / --interleaved: the FASTQ input is fragments (groot_reads_open_paired, groot_hip_pairs_enable)
    uint32_t bootstraps = 0;               // --bootstraps: replicates behind the four bootstrap columns of --abundance (0 = none)
    uint64_t boot_seed = 1;
    bool call_support = false;             // --callSupport: three more columns of the calls file from the bootstrap replicates
    std::string rarefy_out;                // --rarefy: the rarefaction curve of --abundance (and --calls): nested subsamples without replacement
    uint32_t rarefy_steps = GROOT_RAREFY_STEPS, rarefy_reps = GROOT_RAREFY_REPS;
    uint64_t rarefy_seed = 1;
    std::string variants_out;              // --variants: what the reads without an exact alignment, rescued with up to --rescue substitutions, say differs
    long rescue = 2;                       // --rescue M (1..3)
    long long variant_min_reads = 2;       // --variantMinReads N
    double variant_min_share = 0.1;        // --variantMinShare S
    bool rescue_given = false, variant_min_given = false;
    bool abundance_rescued = false;          // --abundanceRescued: the reads mismatch rescue places join the equivalence classes of --abundance
    bool abundance_gapped = false;           // --abundanceGapped: and so do the reads gapped rescue (--indels) places
    bool rescued_paired = false;             // --rescuedPaired: with --abundanceRescued and --paired / --interleaved, a rescued mate joins its fragment's unit with its rescued set
    bool calls_paired = false;               // --callsPaired: with --calls and --paired / --interleaved, the pileup counts a joined fragment's records on the paths of its set only
    bool calls_rescued_paired = false;       // --callsRescuedPaired: with --calls, --callsPaired, --callsRescued and --rescuedPaired, the pileup over fragments with rescued mates
    bool calls_gapped = false;               // --callsGapped: with --calls, --callsRescued and --abundanceGapped, the gap-placed reads' placements join the pileup too
    bool calls_rescued = false;              // --callsRescued: with --calls and --abundanceRescued, the rescued reads' placements join the pileup
    long long call_slots = 1ll << 24;        // --callSlots N (a power of two): the slots the assigned-coverage table starts with under --callsRescued
    bool call_slots_given = false;
    std::string indels_out;                // --indels: the gaps that the reads neither aligned nor rescued show, placed with one gap of up to --rescueGap bases
    long rescue_gap = 3;                   // --rescueGap G (1..8)
    long long gap_event_slots = 0;         // --gapEventSlots N (a power of two; 0: the library's default)
    bool rescue_gap_given = false, gap_slots_given = false;
    std::string rescued_bam_out;           // --rescuedBam: a BAM of its own with one record per kept placement of every read mismatch rescue places
    long long rescued_bam_slots = 0;       // --rescuedBamSlots N: room for that many of them per batch and pipeline slot (0: 16 per read of --batch)
    bool rescued_bam_slots_given = false;
    bool rescued_bam_gaps = false;         // --rescuedBamGaps: the file of --rescuedBam also holds the reads gapped rescue (--indels) places, with I / D CIGARs
    long long gap_record_slots = 0;        // --gapRecordSlots N: room for that many of their records per batch and pipeline slot (0: 4 per read of --batch)
    bool gap_record_slots_given = false;
    std::vector<std::string> fastq;
    int proc = 1, gpu = 0, gpus = 0, ctx_per_gpu = 1, bam_level = -1;
    bool gpu_given = false, write_gob = false;
    uint32_t k = 31, s = 21, w = 100, x = 8, y = 4, max_span = 30, batch = 1u << 20, max_read_len = 512, depth = 3;
    uint64_t block_bytes = 0;
    std::string stats_file;
    double threshold = 0.99, min_kmer_cov = 1.0;
    bool no_align = false, fasta = false;
    std::string memo = "auto";             // auto | on | off | <MiB>
};

std::vector<std::string> split(const std::string &s, char d)
{
    std::vector<std::string> out;
    size_t a = 0;
    for (;;) {
        size_t b = s.find(d, a);
        if (b == std::string::npos) { if (a < s.size()) out.push_back(s.substr(a)); break; }
        if (b > a) out.push_back(s.substr(a, b - a));
        a = b + 1;
    }
    return out;
}

bool is_dir(const std::string &p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
bool is_file(const std::string &p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}
void make_dir(const std::string &p)
{
    if (!is_dir(p) && mkdir(p.c_str(), 0700) != 0) die("can't create specified output directory");
}

void start_logging(const Args &a)
{
    if (!a.log_file.empty()) {
        g_log = fopen(a.log_file.c_str(), "w");
        if (!g_log) { fprintf(stderr, "can't open log file %s\n", a.log_file.c_str()); exit(1); }
    }
}

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

} // namespace
