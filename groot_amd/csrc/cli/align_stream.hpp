// align, stages 3 to 6: parse | map | write as three overlapping stages.
//   producer thread   groot_reads_next: FASTQ text -> parsed + packed batches (reader thread per file, parse over -p cores)
//   mapper threads    one per GPU: groot_hip_submit_packed16 / groot_hip_collect, several batches in flight per ctx
//   writer thread     batches back in input order: traversal records -> sam.Records -> BGZF over -p cores
// The reference's pipeline has the same shape with goroutines and channels (DataStreamer -> FastqHandler -> ReadMapper with
// its bamwriter goroutine, sketch.go:41-350, boss.go:86-104); reads shard over the GPUs batch by batch, the index is
// replicated, and the only exchange is the sum of the IncrementSubPath call counts at the end (RCCL).
#pragma once
#include "align_counters.hpp"

namespace {

struct WorkItem {
    uint64_t seq = 0;                 // position of the batch in the input
    groot_reads_batch *batch = nullptr;
    groot_reads_view view{};
    // filled by the mapper
    int gpu = -1;
    groot_batch_result res{};
    const groot_rescue_record *rr = nullptr;   // --rescuedBam: the batch's rescued records, in the ctx's pinned memory until the ticket is released
    uint64_t n_rr = 0;
    const groot_gap_record *gr = nullptr;      // --rescuedBamGaps: and its gapped records, likewise
    uint64_t n_gr = 0;
};

template <class T> struct BoundedQueue {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<T> q;
    size_t cap;
    bool closed = false;
    explicit BoundedQueue(size_t c) : cap(c) {}
    void push(T v)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return q.size() < cap; });
        q.push_back(std::move(v));
        cv.notify_all();
    }
    // 1 = got one, 0 = none right now (only when !block), -1 = closed and empty
    int pop(T &out, bool block)
    {
        std::unique_lock<std::mutex> lk(mu);
        if (block) cv.wait(lk, [&] { return !q.empty() || closed; });
        if (q.empty()) return closed ? -1 : 0;
        out = std::move(q.front());
        q.pop_front();
        cv.notify_all();
        return 1;
    }
    void close()
    {
        std::lock_guard<std::mutex> lk(mu);
        closed = true;
        cv.notify_all();
    }
};

struct Gpu {
    int index = 0, device = 0;        // position in Stream::gpus; HIP device
    groot_ctx *ctx = nullptr;
    uint32_t max_read_len = 0;
    std::mutex mu;                    // tickets the writer is done with (the ctx itself belongs to the mapper thread)
    std::condition_variable cv;
    std::vector<uint64_t> done_tickets;
    uint32_t held = 0, inflight = 0;
    std::deque<WorkItem> pending;     // submitted, in order
};

// Ask for the sizes, then fill: the call counts of a ctx as rows of nw words (groot_hip_attempts_export); the status of the call that failed
int export_attempts(groot_ctx *ctx, std::vector<uint32_t> &qv, std::vector<uint32_t> &cnt, uint32_t *n_rows, uint32_t *nw)
{
    if (int rc = groot_hip_attempts_export(ctx, nullptr, nullptr, 0, n_rows, nw)) return rc;
    qv.resize(*n_rows);
    cnt.resize((size_t)*n_rows * *nw);
    return *n_rows ? groot_hip_attempts_export(ctx, qv.data(), cnt.data(), *n_rows, n_rows, nw) : 0;
}

constexpr size_t kParsedAhead = 8;    // batches the parser may be ahead of the mappers

struct Stream {
    const Args &a;
    const AlignPlan &plan;
    const uint32_t cores, depth;
    groot_reads *reads = nullptr;
    // known once the index is loaded and the contexts are open: set before the mappers and the writer start
    groot_index_view v{};
    uint32_t memo_budget = GROOT_MEMO_OFF;
    std::unique_ptr<RunCounters> counters;
    groot_bam *bam = nullptr;
    groot_bam *rescued_bam = nullptr;                 // --rescuedBam
    uint64_t rescued_records = 0, rescued_reads = 0;  // ... what went into it
    uint64_t gapped_records = 0, gapped_reads = 0;    // --rescuedBamGaps: the gapped records among them, and their reads
    std::vector<std::unique_ptr<Gpu>> gpus;
    std::atomic<bool> gpus_ready{false};
    BoundedQueue<WorkItem> parsed{kParsedAhead};
    BoundedQueue<WorkItem> mapped{4};                 // (its real capacity is set once the contexts are known, before anyone uses it)
    std::atomic<int> mappers_left{0};
    // the failure latch: the first message stays, every queue and every waiting mapper is woken
    std::mutex fatal_mu;
    std::string fatal;
    std::atomic<bool> failed{false};
    // what the run adds up
    std::atomic<uint64_t> length_total{0}, collect_wait_us{0}, n_batches{0};
    double parse_s = 0, bam_s = 0;                    // busy time of the producer / the writer
    uint64_t received = 0, mapped_reads = 0, multimapped = 0, alignments = 0, full_sketch = 0;

    Stream(const Args &args, const AlignPlan &p) : a(args), plan(p), cores(args.proc > 0 ? (uint32_t)args.proc : 0), depth(std::max(2u, args.depth)) {}

    void fail_with(const std::string &msg)
    {
        std::lock_guard<std::mutex> lk(fatal_mu);
        if (fatal.empty()) fatal = msg;
        failed = true;
        parsed.close(); mapped.close();
        if (gpus_ready)
            for (auto &g : gpus) { std::lock_guard<std::mutex> l2(g->mu); g->cv.notify_all(); }
    }

    groot_params params_for(uint32_t max_read_len) const
    {
        groot_params prm;
        groot_params_default(&prm);
        prm.containment_threshold = a.threshold;
        prm.no_exact_align = a.no_align ? 1 : 0;
        prm.max_batch_reads = a.batch;
        prm.max_read_len = max_read_len;
        prm.max_batch_bases = (uint64_t)a.batch * std::min<uint32_t>(max_read_len, 512);
        prm.pipeline_depth = depth;
        prm.memo_budget_mb = memo_budget;
        prm.results_on_device = a.no_bam ? 1 : 0;   // (no BAM: the records stay in HBM, nothing crosses PCIe but the counters)
        return prm;
    }

    void open_reads();
    void open_contexts(int n_dev);
    const char *reopen(Gpu &g, uint32_t new_max_len, bool carry_counters, const char *why);
    void producer();
    void mapper(Gpu &g);
    void writer();

private:
    void drain_released(Gpu &g, bool wait);
    bool collect_one(Gpu &g);
    bool grow_ctx(Gpu &g, uint32_t need);
    void hand_back(WorkItem &w);
};

// ---- the FASTQ parser starts before the index is read and the GPU context opened: inflating and packing the first batches takes as long
// as those do (a gzip FASTQ inflates on one thread, as bufio over gzip.Reader does in the reference), and neither needs the other; up to
// kParsedAhead batches wait for the mappers ----
void Stream::open_reads()
{
    const uint64_t max_batch_bases = (uint64_t)a.batch * std::min<uint32_t>(a.max_read_len, 512);
    std::vector<const char *> files;
    for (auto &f : a.fastq) files.push_back(f.c_str());
    if (plan.frags) {
        std::vector<const char *> f1, f2;       // --paired: first with second, third with fourth; --interleaved: one stream, no second list
        for (size_t i = 0; i < files.size(); i++) (a.paired && (i & 1) ? f2 : f1).push_back(files[i]);
        if (groot_reads_open_paired(f1.empty() ? nullptr : f1.data(), (uint32_t)f1.size(), f2.empty() ? nullptr : f2.data(), (uint32_t)f2.size(), cores, a.block_bytes,
                                    a.batch, max_batch_bases, &reads))
            die("%s", groot_host_last_error());
    } else if (groot_reads_open(files.empty() ? nullptr : files.data(), (uint32_t)files.size(), cores, a.block_bytes, a.batch, max_batch_bases, &reads))
        die("%s", groot_host_last_error());
}

void Stream::producer()
{
    uint64_t seq = 0;
    for (;;) {
        if (failed) break;
        WorkItem w;
        auto tp = std::chrono::steady_clock::now();
        const int prc = groot_reads_next(reads, &w.batch);
        parse_s += seconds_since(tp);
        if (prc) { fail_with(groot_host_last_error()); break; }
        if (!w.batch) break;
        groot_reads_batch_view(w.batch, &w.view);
        length_total += w.view.n_bases;
        w.seq = seq++;
        parsed.push(std::move(w));
    }
    parsed.close();
}

// ---- one ctx per GPU (index replicated), opened concurrently; the counters the plan asks for are switched on ----
void Stream::open_contexts(int n_dev)
{
    std::vector<int> devices;
    if (a.gpus > 0) {
        if (a.gpus > n_dev) die("--gpus %d but only %d device(s) visible", a.gpus, n_dev);
        for (int i = 0; i < a.gpus; i++) devices.push_back(i);
    } else devices.push_back(a.gpu);
    for (int extra = 1; extra < a.ctx_per_gpu; extra++)          // test hook: several ctxs on one device (exercises the N>1 path on a one-GPU box)
        for (size_t i = 0, n = devices.size() / (size_t)extra; i < n; i++) devices.push_back(devices[i]);
    // The memo of groot_hip_open answers reads that equal an indexed string without hashing or graph walk: it costs a third
    // of a second per GB of path bases at open and saves ~0.4 ms of GPU time per million such reads -- in this process the GPU waits for
    // the FASTQ parser and the BAM writer, so it only pays on inputs that keep it busy for minutes.  auto: on from 20 GB of
    // input (gzip counted four-fold; stdin: off).
    if (a.memo == "on") memo_budget = 0;
    else if (a.memo == "auto") {
        uint64_t bytes = 0;
        for (auto &f : a.fastq) {
            struct stat st;
            if (stat(f.c_str(), &st) == 0) bytes += (uint64_t)st.st_size * (f.size() > 3 && f.compare(f.size() - 3, 3, ".gz") == 0 ? 4 : 1);
        }
        if (bytes >= (20ull << 30)) memo_budget = 0;
    } else if (a.memo != "off") {
        char *end = nullptr;
        const long mb = strtol(a.memo.c_str(), &end, 10);
        if (a.memo.empty() || *end || mb < 1 || mb > (1L << 30)) die("--memo: '%s' is neither auto, on, off nor a number of MiB", a.memo.c_str());
        memo_budget = (uint32_t)mb;
    }
    // --report and its kin: every ctx counts on the device; what a ctx has counted is added up before it closes (reopen) and at the end of the stream
    counters.reset(new RunCounters(a, plan, v));
    for (int d : devices) {
        std::unique_ptr<Gpu> g(new Gpu());
        g->index = (int)gpus.size(); g->device = d; g->max_read_len = a.max_read_len;
        gpus.push_back(std::move(g));
    }
    std::vector<std::thread> th;
    std::vector<std::string> errs(gpus.size());
    for (size_t i = 0; i < gpus.size(); i++)
        th.emplace_back([this, &errs, i]() {
            groot_params prm = params_for(gpus[i]->max_read_len);
            if (groot_hip_open_flags(&gpus[i]->ctx, gpus[i]->device, &v, &prm, GROOT_OPEN_BACKGROUND)) errs[i] = groot_hip_last_error(nullptr);
        });
    for (auto &t : th) t.join();
    for (auto &e : errs) if (!e.empty()) die("%s", e.c_str());
    if (plan.counters)
        for (auto &g : gpus) if (counters->enable(g->ctx, 1)) die("%s", groot_hip_last_error(g->ctx));
}

// Export the call counts, close, open for reads up to new_max_len, import: a ctx that has no room for a read (grow_ctx, in the middle of
// the stream: carry_counters, the ctx's counters are harvested before the close and switched on again after the open) or that has to reach
// the kmerCount range of the others before the call counts are summed (at the end: the counters are off by then).  `why` is the caller's
// log line.  nullptr, or the message of the call that failed: the mapper latches it, the main thread dies with it.
const char *Stream::reopen(Gpu &g, uint32_t new_max_len, bool carry_counters, const char *why)
{
    uint32_t n_rows = 0, nw = 0;
    std::vector<uint32_t> qv, cnt;
    if (export_attempts(g.ctx, qv, cnt, &n_rows, &nw)) return groot_hip_last_error(g.ctx);
    if (carry_counters && counters->harvest(g.ctx)) return groot_hip_last_error(g.ctx);
    groot_hip_close(g.ctx);
    g.ctx = nullptr;
    g.max_read_len = new_max_len;
    groot_params prm = params_for(new_max_len);
    logf("%s", why);
    if (groot_hip_open_flags(&g.ctx, g.device, &v, &prm, GROOT_OPEN_BACKGROUND)) return groot_hip_last_error(nullptr);
    if (n_rows && groot_hip_attempts_import(g.ctx, qv.data(), cnt.data(), n_rows)) return groot_hip_last_error(g.ctx);
    if (carry_counters && counters->enable(g.ctx, 1)) return groot_hip_last_error(g.ctx);
    return nullptr;
}

void Stream::drain_released(Gpu &g, bool wait)
{
    std::unique_lock<std::mutex> lk(g.mu);
    if (wait) g.cv.wait(lk, [&] { return !g.done_tickets.empty() || failed; });
    for (uint64_t t : g.done_tickets) { groot_hip_release(g.ctx, t); g.held--; }
    g.done_tickets.clear();
}

bool Stream::collect_one(Gpu &g)
{
    WorkItem w = std::move(g.pending.front());
    g.pending.pop_front();
    auto tc = std::chrono::steady_clock::now();
    const int rc = groot_hip_collect(g.ctx, &w.res);
    collect_wait_us += (uint64_t)(seconds_since(tc) * 1e6);
    n_batches++;
    // the reference's panics (short read, RevComplement on a byte > 'T') and over-long reads end the run
    if (rc == GROOT_E_NOSPACE && plan.rescued_bam_gaps && strstr(groot_hip_last_error(g.ctx), "groot_hip_gap_rec_enable")) {
        fail_with(std::string(groot_hip_last_error(g.ctx)) + ": give --gapRecordSlots a larger value");
        return false;
    }
    if (rc) { fail_with(groot_hip_last_error(g.ctx)); return false; }
    // (asked for here: the ctx is the mapper's, the writer only reads the pinned memory the pointer names)
    if (plan.rescued_bam && groot_hip_rescue_rec_batch(g.ctx, w.res.ticket, &w.rr, &w.n_rr)) { fail_with(groot_hip_last_error(g.ctx)); return false; }
    if (plan.rescued_bam_gaps && groot_hip_gap_rec_batch(g.ctx, w.res.ticket, &w.gr, &w.n_gr)) { fail_with(groot_hip_last_error(g.ctx)); return false; }
    g.inflight--; g.held++;
    w.gpu = g.index;
    mapped.push(std::move(w));
    return true;
}

// a batch with a read longer than the ctx was opened for: finish what is in flight, carry the call counts over
// into a ctx with room for it (the reference has no read-length limit)
bool Stream::grow_ctx(Gpu &g, uint32_t need)
{
    while (g.inflight) if (!collect_one(g)) return false;
    while (g.held && !failed) drain_released(g, true);
    if (failed) return false;
    const uint32_t room = std::min<uint32_t>(65535, need + need / 2);
    char why[160];
    snprintf(why, sizeof why, "\tread of %u bases: reopening the GPU context for reads up to %u bases", need, room);
    if (const char *err = reopen(g, room, plan.counters, why)) { fail_with(err); return false; }
    return true;
}

// One mapper per ctx.  A batch is taken when a slot is free -- depth >= 2 slots, each either in flight or held by the writer -- and waited
// for only when the ctx is idle; otherwise the oldest batch in flight is collected, or a slot is waited for.
void Stream::mapper(Gpu &g)
{
    bool input_done = false;
    while (!failed) {
        drain_released(g, false);
        const uint32_t free_slots = depth - g.held - g.inflight;
        if (!input_done && free_slots > 0) {
            WorkItem w;
            const int got = parsed.pop(w, g.inflight == 0 && g.held == 0);   // (idle: nothing to do but wait for input)
            if (got < 0) input_done = true;
            else if (got > 0) {
                if (w.view.max_len > g.max_read_len && !grow_ctx(g, w.view.max_len)) break;
                if (groot_hip_submit_packed16(g.ctx, w.view.packed, w.view.seq_len, w.view.n_reads, 0, w.view.exc_pos, w.view.exc_byte, w.view.n_exc)) {
                    fail_with(groot_hip_last_error(g.ctx));
                    break;
                }
                g.inflight++;
                g.pending.push_back(std::move(w));
                continue;
            }
        }
        if (g.inflight) { if (!collect_one(g)) break; continue; }
        if (input_done && g.held == 0) break;
        if (g.held) drain_released(g, true);                // everything is with the writer: wait for a slot
    }
    if (--mappers_left == 0) mapped.close();
}

void Stream::hand_back(WorkItem &w)
{
    groot_reads_batch_free(w.batch);
    Gpu &g = *gpus[(size_t)w.gpu];
    { std::lock_guard<std::mutex> lk(g.mu); g.done_tickets.push_back(w.res.ticket); }
    g.cv.notify_all();
}

// ---- writer: batches in input order (on the main thread) ----
void Stream::writer()
{
    std::map<uint64_t, WorkItem> waiting;
    uint64_t next_seq = 0;
    for (;;) {
        WorkItem w;
        const int got = mapped.pop(w, true);
        if (got < 0) break;
        waiting.emplace(w.seq, std::move(w));
        while (!waiting.empty() && waiting.begin()->first == next_seq) {
            WorkItem it = std::move(waiting.begin()->second);
            waiting.erase(waiting.begin());
            next_seq++;
            const groot_counts &c = it.res.counts;
            received += c.received; mapped_reads += c.mapped; multimapped += c.multimapped; alignments += c.alignments;
            full_sketch += c.full_sketch_reads;
            if (bam && it.res.n_travs && !failed) {
                uint64_t nrec = 0;
                auto tw = std::chrono::steady_clock::now();
                const int wrc = groot_bam_write_batch(bam, &v, &it.view, 0, it.res.travs, it.res.masks, it.res.mask_ckpt, it.res.n_travs, &nrec);
                bam_s += seconds_since(tw);
                if (wrc) fail_with(groot_host_last_error());
                else if (nrec != c.alignments && !plan.assign)   // (assignment: the counts are the unfiltered run's, the records what it kept)
                    fail_with("internal error: " + std::to_string(nrec) + " records written, " + std::to_string(c.alignments) + " alignments counted");
            }
            if (rescued_bam && (it.n_rr || it.n_gr) && !failed) {   // right behind the main BAM's batch, in input order
                uint64_t nrec = 0;
                auto tw = std::chrono::steady_clock::now();
                // (--rescuedBamGaps: the batch's gapped records merged in by read; without it the call and the bytes it always made)
                const int wrc = plan.rescued_bam_gaps ? groot_bam_write_rescued_gapped(rescued_bam, &v, &it.view, it.rr, it.n_rr, it.gr, it.n_gr, &nrec)
                                                      : groot_bam_write_rescued(rescued_bam, &v, &it.view, it.rr, it.n_rr, &nrec);
                bam_s += seconds_since(tw);
                if (wrc) fail_with(groot_host_last_error());
                else {
                    rescued_records += nrec;
                    for (uint64_t i = 0; i < it.n_rr; i++) rescued_reads += i == 0 || it.rr[i].read != it.rr[i - 1].read;
                    uint64_t gr_reads = 0;
                    for (uint64_t i = 0; i < it.n_gr; i++) gr_reads += i == 0 || it.gr[i].read != it.gr[i - 1].read;
                    gapped_records += it.n_gr; gapped_reads += gr_reads; rescued_reads += gr_reads;
                }
            }
            hand_back(it);
        }
    }
    // after a failure: hand back whatever is still queued so that the mappers can finish
    for (auto &kv : waiting) hand_back(kv.second);
}

} // namespace
