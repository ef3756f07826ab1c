// ctx.hpp -- the ctx of libgroot_hip.so as its translation units see it: the buffer types, one batch in flight (Slot), the work sets and
// groot_ctx itself, with the state of the counters behind the order stage (counters.hip, rescue.hip) as ONE member each of the ctx and of a slot.
// Internal to groot_hip.hip (pipeline + C ABI), open.hip (groot_hip_open*), counters.hip and rescue.hip; the calls between them are at the end, in open.hpp, in counters.hpp and in rescue.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdlib>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "device_types.hpp"

using namespace groot;


// ---------------------------------------------------------------------------------------------
// ctx
// ---------------------------------------------------------------------------------------------
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count)
    {
        release();
        n = count;
        return hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
    }
    hipError_t reserve(size_t count) { return count <= n && p ? hipSuccess : alloc(count); }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

// page-locked host memory: the only kind hipMemcpyAsync really overlaps with kernels
template <class T> struct PinBuf {
    T *p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count)
    {
        release();
        n = count;
        return hipHostMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault);
    }
    hipError_t reserve(size_t count) { return count <= n && p ? hipSuccess : alloc(count); }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    ~PinBuf() { release(); }
};

// The environment switches of the shipped library, read when a ctx is opened (everything else that used to be tunable from the
// environment was an experiment and went in round 4: DESIGN.md "Removed").  The three NO_* switch a tier of the seed stage off (tests
// compare the tiers with each other and with the CPU checker); TEST_SMALL_BUFFERS starts every growable buffer and list too small, so that
// a test batch walks the grow-and-redo and the fall-back paths; OPEN_STATS prints where groot_hip_open spent its time.
struct Knobs {
    bool no_outcome_table = false, no_text_table = false, no_sig = false, force_rccl = false, small_buffers = false, open_stats = false, poison = false, lean = false, no_path = false,
         shared_slow = false, serial_tail = false, assign_global = false, library_sort = false;
    uint32_t ec_slots = 0;                 // GROOT_TEST_EC_SLOTS: initial slots of the equivalence-class table (0 = the default)
    uint32_t acov_slots = 0;               // GROOT_TEST_ACOV_SLOTS: initial slots of the assigned-coverage table (0 = the default)
    uint32_t rescue_ec_rows = 0;           // GROOT_TEST_RESCUE_EC_ROWS: bitmaps of slow rescued reads per batch (0 = from the byte budget)
    uint32_t rescue_acov_log = 0;          // GROOT_TEST_RESCUE_ACOV_LOG: logged placements of slow rescued reads per batch (0 = from the byte budget)
    static Knobs read()
    {
        Knobs k;
        k.no_outcome_table = getenv("GROOT_NO_OUTCOME_TABLE") != nullptr; k.no_text_table = getenv("GROOT_NO_TEXT_TABLE") != nullptr;
        k.no_sig = getenv("GROOT_NO_SIG") != nullptr;                     k.force_rccl = getenv("GROOT_FORCE_RCCL") != nullptr;
        k.small_buffers = getenv("GROOT_TEST_SMALL_BUFFERS") != nullptr;  k.open_stats = getenv("GROOT_OPEN_STATS") != nullptr;
        k.poison = getenv("GROOT_TEST_POISON") != nullptr;
        k.lean = getenv("GROOT_LEAN") != nullptr;                         // the node-by-node first pass (kernels_lean.hpp) instead of the path-text one
        k.no_path = getenv("GROOT_NO_PATH_PASS") != nullptr;              // no first pass: align_kernel alone
        k.shared_slow = getenv("GROOT_TEST_SHARED_SLOW") != nullptr;      // shared reads: every read in more than one graph takes the slow path
        k.serial_tail = getenv("GROOT_SERIAL_TAIL") != nullptr;           // the tail of the align stage stays on the walk stream (no tail stream: the A/B baseline)
        k.assign_global = getenv("GROOT_TEST_ASSIGN_GLOBAL") != nullptr;  // assignment: alpha is read from global memory even when it fits in LDS
        k.library_sort = getenv("GROOT_LIBRARY_SORT") != nullptr;         // the processing-order sort of every batch through rocprim::radix_sort_pairs (order_sort.hpp: the A/B baseline)
        if (const char *e = getenv("GROOT_TEST_EC_SLOTS")) k.ec_slots = (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), 1ul << 30);
        if (const char *e = getenv("GROOT_TEST_ACOV_SLOTS")) k.acov_slots = (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), 1ul << 30);
        if (const char *e = getenv("GROOT_TEST_RESCUE_EC_ROWS")) k.rescue_ec_rows = (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), 1ul << 30);
        if (const char *e = getenv("GROOT_TEST_RESCUE_ACOV_LOG")) k.rescue_acov_log = (uint32_t)std::min<unsigned long>(strtoul(e, nullptr, 10), 1ul << 28);
        return k;
    }
};

// ---- the counters behind the order stage (counters.hip, and rescue.hip for the rescue family) ----
namespace groot {
struct EcTable;
struct AcovTable;
} // namespace groot

// The run-wide table of equivalence classes (kernels_ec.hpp): its buffers for cap slots (a power of two).  Growth allocates a second
// one, rehashes into it and swaps.
struct EcBufs {
    uint32_t cap = 0;
    DevBuf<uint32_t> claim, graph;
    DevBuf<uint64_t> mask;
    DevBuf<unsigned long long> cnt;
    DevBuf<uint32_t> serial;               // [cap] the serial of every claimed slot (EcTable::serial)
    hipError_t alloc(uint32_t slots, uint32_t pw, hipStream_t st);   // free (no slot claimed; the memset is enqueued on st); pw words per path set
    EcTable table() const;
    void swap(EcBufs &o);
    void release();
};

// The run-wide table of assigned coverage (kernels_acov.hpp), likewise
struct AcovBufs {
    uint32_t cap = 0;
    DevBuf<unsigned long long> k0, k1, cnt;
    hipError_t alloc(uint32_t slots, hipStream_t st);                // free (k0 = 0, k1 = all ones, no counts; the memsets are enqueued on st)
    AcovTable table() const;
    void swap(AcovBufs &o);
    void release();
};

// what the host reads back of a batch's counting kernels (copied behind them, ahead of the DeviceCounters)
struct CounterStatus {
    uint32_t ec_slow;                      // equivalence classes: the batch's slow-path reads
    uint32_t ec_fill;                      // ... and the table's fill behind this batch's merge
    uint32_t acov_state;                   // assigned coverage: SlotCounters::d_acov_state[0]
    uint32_t acov_fill;                    // ... and its table's fill
    uint32_t rec_slow;                     // rescued reads in the ECs: the batch's slow rescued reads (SlotCounters::d_rec_slow[0])
    uint32_t rac_log;                      // rescued reads in assigned coverage: the kept placements of those reads (SlotCounters::d_rac_nlog[0])
    uint64_t rr_total;                     // rescued records: the batch's records (SlotCounters::rr.d_total[0])
    uint64_t gr_total;                     // gapped records: the batch's records (SlotCounters::gr.d_total[0])
    uint32_t gec_slow;                     // gap-placed reads in the ECs: the batch's slow gap-rescued reads (SlotCounters::d_gec_slow[0])
    uint32_t gac_log;                      // gap-placed reads in assigned coverage: the log entries of those reads (SlotCounters::d_gac_nlog[0])
};

// One kind of record a batch hands out beside its traversals -- rescued records, gapped records (rescue.hip) -- as the ctx keeps it ...
struct RecStream {
    bool on = false;
    uint64_t slots = 0;                    // records per batch (fixed at enable)
    DevBuf<uint32_t> kept;                 // [max_batch_reads + 1] every read's kept placements (tail stream: one batch at a time, as the candidates are)
    DevBuf<uint64_t> off;                  // [max_batch_reads + 1] their exclusive scan: every read's first record, and the batch's total
    DevBuf<uint8_t> aux;                   // [max_batch_reads] what the count kernel leaves the emit kernel per candidate (d* / e*)
    uint64_t records = 0, reads = 0, failed = 0;   // handed out / distinct reads among them / batches failed for room, since enable
    uint64_t launches = 0;                 // the scan and the emit kernel since open (stays put while it is off)
};
// ... and as a slot does
template <class Rec> struct SlotRecStream {
    DevBuf<uint32_t> d_rec;                // [slots][sizeof(Rec) / 4 dwords] the batch's records (the emit kernel), copied out at collect
    DevBuf<uint64_t> d_total;              // [0] their number, whether they found room or not (the scan's last output)
    PinBuf<Rec> h_rec;                     // what the *_rec_batch call hands out: as many as the batch has
    uint64_t n = 0;                        // the batch's records in h_rec
    bool on = false;                       // the feature was on when the batch was submitted
};

struct SlotCounters {
    DevBuf<uint32_t> d_ec_slow;            // equivalence classes: the batch's slow-path reads (ec_merge_kernel), read at collect
    PinBuf<CounterStatus> h_status;
    DevBuf<uint32_t> d_acov_ser;           // assigned coverage: the EC serial of every read of the batch (acov_serial_kernel); the counting kernels read it, also when collect repeats them
    DevBuf<uint32_t> d_acov_state;         // [0] 1 = the batch's claim phase ran out of room (its add phase then did nothing), 2 = a key went missing
    DevBuf<uint2> d_acov_mate;             // assigned coverage over fragments: per read of a joined fragment the span of its mate's records (acov_serial_paired_kernel);
                                           // with d_acov_ser all the rule needs when collect repeats the count (the unit rows are the ctx's, and gone by then)
    DevBuf<uint32_t> d_best;              // assignment: best path / MAPQ of every read of the batch (assign_kernel), copied out with the batch
    DevBuf<uint8_t> d_mapq;
    PinBuf<uint32_t> h_best;
    PinBuf<uint8_t> h_mapq;
    bool assigned = false;                 // the batch went through assign_kernel: h_best / h_mapq are its
    DevBuf<unsigned long long> d_rec_bits; // rescued reads in the ECs: [rec_rows][rec_bw] the path bitmaps of the batch's slow rescued reads, read at collect
    DevBuf<uint32_t> d_rec_slow;           // [0] their number, with or without a bitmap (rescue_ec_slow_kernel)
    DevBuf<uint4> d_rac_log;               // rescued reads in assigned coverage: [rac_log_cap] (bitmap row, path, X, last) of those reads' kept placements, read at collect
    DevBuf<uint32_t> d_rac_nlog;           // [0] their number, logged or not (rescue_acov_slow_kernel)
    SlotRecStream<groot_rescue_record> rr; // rescued records: five dwords each (rescue_rec_emit_kernel), handed out by groot_hip_rescue_rec_batch
    SlotRecStream<groot_gap_record> gr;    // gapped records: six dwords each (gap_rec_emit_kernel), handed out by groot_hip_gap_rec_batch
    DevBuf<uint32_t> d_gec_slow;           // gap-placed reads in the ECs: [0] the batch's slow gap-rescued reads, with or without a bitmap (gap_ec_slow_kernel);
                                           // their bitmaps are the rows of d_rec_bits behind the rescued reads'
    DevBuf<uint32_t> d_gac_nlog;           // gap-placed reads in assigned coverage: [0] the log entries of the batch's slow gap-rescued reads, logged or not
                                           // (gap_acov_slow_kernel); the entries are those of d_rac_log behind the rescued reads'
};

struct Counters {
    // The per-node path-position tables, kept on the host from open (a few MB).  ONE device copy serves report coverage, shared reads,
    // equivalence classes and assigned coverage: uploaded when the first of them comes on, released when the last goes off.
    std::vector<uint32_t> h_np_off, h_gpo, h_len;        // node_np_off, graph_path_off, path_len
    std::vector<uint2> h_np;                             // (path, position) of every entry
    DevBuf<uint32_t> d_np_off, d_gpo, d_len;
    DevBuf<uint2> d_np;
    // report coverage (groot_hip_coverage_*, kernels_cov.hpp): off until enabled, then cov_count_kernel runs behind every batch's
    // order stage.  The device holds the counters only while on.
    bool cov_on = false;
    std::vector<uint64_t> h_cov_base;      // first slot of every path, + the total
    DevBuf<uint64_t> cov_base;
    DevBuf<unsigned long long> cov_starts, cov_ends;
    // shared reads (groot_hip_shared_*, kernels_shared.hpp): off until enabled, then four kernels behind every batch's order stage count,
    // for every pair of paths a <= b, the reads with records on both.  Nothing on the device while off.
    bool sh_on = false;
    uint32_t sh_tab_cap = 0;               // slots of the set table: a power of two >= 2 max_batch_reads
    DevBuf<uint32_t> sh_set_graph, sh_tab_rep, sh_tab_cnt, sh_slow, sh_batch;
    DevBuf<uint64_t> sh_set_mask;
    DevBuf<unsigned long long> sh_tri, sh_stats;
    // equivalence classes (groot_hip_ec_*, kernels_ec.hpp): the gather and insert kernels of shared reads run while either is on, and
    // ec_merge_kernel folds each batch's distinct sets into a run-wide table; slow-path reads are folded on the host at collect
    bool ec_on = false;
    bool pairs_on = false;                 // groot_hip_pairs_enable: reads 2i, 2i+1 of a batch are one fragment (the kPaired kernels of kernels_shared.hpp)
    EcBufs ec;
    uint32_t ec_epoch = 0;                 // epoch of the newest launch on the table
    DevBuf<uint32_t> ec_fill;
    uint64_t ec_fill_known = 0;            // the fill read back at the newest collect
    uint64_t ec_grows = 0, ec_slow_reads = 0;
    std::map<std::vector<uint32_t>, uint64_t> ec_host;   // the exact S(r) of slow-path reads -> reads
    // assigned coverage (groot_hip_acov_*, kernels_acov.hpp): the run's records grouped by (EC serial, path, Pos, last) in a run-wide
    // open-addressing table; needs equivalence classes on.  Slow-path reads are grouped on the host at collect (ec_collect).
    bool acov_on = false;
    AcovBufs acov;
    DevBuf<uint32_t> acov_fill, acov_err, acov_tab_ser;
    uint64_t acov_grows = 0, acov_slow_records = 0, acov_redone = 0;
    uint64_t acov_launches = 0;            // kernels launched for it since open (stays put while it is off)
    std::map<std::vector<uint32_t>, std::map<std::array<uint32_t, 3>, uint64_t>> acov_host;   // S(r) -> (path, Pos, last) -> records, of slow-path reads
    // assigned coverage over fragments (groot_hip_acov_pairs_*; the kPaired kernels of kernels_acov.hpp): the one state in which assigned
    // coverage and pairing are on together.  A record of a joined fragment counts on the paths of the fragment's set only.
    bool acp_on = false;
    DevBuf<unsigned long long> acp_stats;  // [kAcovPairStats] records left out on the device, reads of joined fragments
    uint64_t acp_host_left = 0, acp_slow_frags = 0;   // records left out on the host / joined fragments folded there, since enable / groot_hip_acov_reset
    // assignment (groot_hip_assign_*, kernels_assign.hpp): assign_kernel rewrites every batch's records inside the order stage, ahead
    // of everything that reads them.  Nothing on the device while off.
    bool asg_on = false;
    double asg_min_post = 0.0;
    DevBuf<double> asg_alpha;              // [n_paths]
    DevBuf<uint32_t> asg_gpo;              // graph_path_off (a copy of its own: the position tables above are not needed)
    DevBuf<unsigned long long> asg_stats;  // [kAssignStats]
    uint64_t asg_launches = 0;             // kernels launched for it since open (stays put while it is off)
    // mismatch rescue (groot_hip_rescue_*, kernels_rescue.hpp): rescue_pack_kernel and rescue_count_kernel behind every batch's order
    // stage place the reads without a record on the path texts with up to res_m substitutions.  Nothing on the device while off.
    bool res_on = false;
    uint32_t res_m = 0, res_text_paths = 0;
    DevBuf<uint32_t> res_text, res_tag, res_cand, res_ncand;
    DevBuf<uint4> res_path, res_tab;       // RescueTables (index_tables.hpp)
    DevBuf<uint2> res_occ;
    DevBuf<uint64_t> res_base;             // h_cov_base
    DevBuf<unsigned long long> res_rbuf;   // [2][res_rcap] the batch's candidates at 2 bits per base (tail stream: one batch at a time)
    uint64_t res_rcap = 0;
    DevBuf<unsigned long long> res_starts, res_ends, res_alt, res_stats;   // report coverage's layout; alt: four per slot
    uint64_t res_launches = 0;             // kernels launched for it since open (stays put while it is off)
    // gapped rescue (groot_hip_gap_*, kernels_gap.hpp): needs mismatch rescue on.  rescue_count_kernel<true> hands on the candidates it left
    // unplaced, rescue_gap_kernel behind it places them with one gap of up to gap_g bases.  Nothing on the device while off.
    bool gap_on = false;
    uint32_t gap_g = 0;
    uint64_t gap_slots = 0;                // slots of the event table: a power of two, fixed at enable
    DevBuf<uint32_t> gap_cand, gap_ncand;
    DevBuf<unsigned long long> gap_starts, gap_ends, gap_key, gap_cnt, gap_stats;   // report coverage's layout; the event table
    uint64_t gap_launches = 0;             // rescue_gap_kernel launches since open (stays put while it is off)
    // rescued reads in the equivalence classes (groot_hip_rescue_ec_*, kernels_rescue_ec.hpp): needs mismatch rescue and equivalence classes
    // on.  rescue_count_ec_kernel also writes every rescued read's path set as a row, three kernels behind it fold the rows into the
    // table of ECs; the sets in too many graphs come back as bitmaps and are folded on the host at collect.  Nothing on the device while off.
    bool rec_on = false;
    uint32_t rec_rows = 0, rec_bw = 0;     // bitmaps per batch (fixed at enable), words per bitmap
    DevBuf<uint2> rec_path_bit;            // RescueArgs::path_bit
    DevBuf<uint8_t> rec_dstar;             // RescueArgs::dstar
    DevBuf<unsigned long long> rec_stats;  // [kRescueEcStats]
    uint64_t rec_slow = 0;                 // slow rescued reads folded at collect since enable / groot_hip_ec_reset
    uint64_t rec_launches = 0;             // kernels launched for it since open, rescue_count_ec_kernel not among them (it counts as rescue's)
    // rescued mates in paired-end units (groot_hip_rescue_pairs_*, kernels_rescue_pairs.hpp): the one state in which pairing and the rescued
    // reads in the ECs are on together (rp_on implies both, and both imply rp_on).  The gather defers the fragments with records on one mate
    // only, and three kernels behind rescue_count_ec_kernel make every unit that is not exact + exact.
    bool rp_on = false;
    DevBuf<uint8_t> rp_state;              // RescuePairArgs::state (tail stream: one batch at a time, as the candidates are)
    DevBuf<unsigned long long> rp_stats;   // [2][kRescuePairStats] the totals, and the words of the batch in hand (added to the totals when its bitmaps found room)
    uint64_t rp_launches = 0;              // the three kernels of kernels_rescue_pairs.hpp since open (stays put while it is off)
    // rescued reads in assigned coverage (groot_hip_rescue_acov_*, kernels_rescue_acov.hpp): needs mismatch rescue, equivalence classes and
    // assigned coverage on, and switches the rescued reads in the ECs on itself.  Every kept placement of a rescued read is a record of the
    // assigned-coverage table; those of the reads with a bitmap come back in a log and are folded on the host at collect.
    bool rac_on = false;
    uint32_t rac_log_cap = 0;              // log entries per batch (fixed at enable)
    DevBuf<uint32_t> rac_cand_ser;         // RescueAcovArgs::cand_ser (tail stream: one batch at a time, as the candidates are)
    DevBuf<unsigned long long> rac_stats;  // [kRescueAcovStats]
    uint64_t rac_host_records = 0;         // rescued records folded on the host since enable / groot_hip_acov_reset
    uint64_t rac_launches = 0;             // kernels launched for it since open; the two that take the place of rec's count there
    // rescued mates in assigned coverage over fragments (groot_hip_rescue_acov_pairs_*, kernels_rescue_acov_pairs.hpp): the one state in which
    // the rescued mates' rule and assigned coverage are on together (rap_on implies rp_on and acp_on, and both imply rap_on; rac_on is off
    // beside it).  The kept placements, and the exact records of a mate joined with a rescued partner, are claimed and added in one pass
    // behind the batch's merge; those of the fragments on bitmaps come back in the slot's log and are folded on the host at collect.
    bool rap_on = false;
    uint32_t rap_log_cap = 0;              // log entries per batch (fixed at enable)
    DevBuf<uint32_t> rap_cand_ser;         // RescueAcovArgs::cand_ser (tail stream: one batch at a time, as the candidates are)
    DevBuf<uint8_t> rap_fclass;            // RescueAcovPairSink::fclass (the same)
    DevBuf<unsigned long long> rap_stats;  // [kRescueAcovPairStats]
    uint64_t rap_host[4] = {0, 0, 0, 0};   // exact records counted / left out, rescued records counted / left out on the host since enable / groot_hip_acov_reset
    uint64_t rap_launches = 0;             // the kernels of kernels_rescue_acov_pairs.hpp since open (stays put while it is off)
    // rescued records (groot_hip_rescue_rec_*, kernels_rescue_rec.hpp; needs mismatch rescue on) and gapped records (groot_hip_gap_rec_*,
    // kernels_gap_rec.hpp; needs gapped rescue on).  The count kernel / the gap kernel also leaves every read's number of kept placements, a
    // scan and the emit kernel behind it write the batch's records into a buffer of the slot, and collect copies as many as there are into
    // pinned memory.  Nothing on the device while off.  (rescue_count_rec_kernel / rescue_gap_rec_kernel count as rescue's / gapped rescue's launches.)
    RecStream rr, gr;
    // gap-placed reads in the equivalence classes (groot_hip_gap_ec_*, kernels_gap_ec.hpp): needs gapped rescue and the rescued reads in the
    // ECs on.  rescue_gap_ec_kernel takes the gap kernel's place and also writes every gap-rescued read's path set as a row; two kernels
    // among those of the rescued reads fold the rows into the table of ECs, the sets in too many graphs come back as bitmaps of the
    // rescued reads' pool and are folded on the host at collect.  Nothing on the device while off.
    bool gec_on = false;
    DevBuf<uint8_t> gec_e;                 // GapEcCountArgs::e (tail stream: one batch at a time, as the gap candidates are)
    DevBuf<unsigned long long> gec_stats;  // [kGapEcStats]
    uint64_t gec_slow = 0;                 // slow gap-rescued reads folded at collect since enable / groot_hip_ec_reset
    uint64_t gec_launches = 0;             // gap_ec_slow_kernel and gap_ec_insert_kernel since open (rescue_gap_ec_kernel counts as gapped rescue's)
    // gap-placed reads in assigned coverage (groot_hip_gap_acov_*, kernels_gap_acov.hpp): needs gapped rescue and the rescued reads in
    // assigned coverage on, and switches the gap-placed reads in the ECs on itself.  Every kept gapped placement is two records (DEL) or
    // one (INS) of the assigned-coverage table; those of the reads with a bitmap come back in the rescued reads' log and are folded on
    // the host at collect.  gac_on implies gec_on and rac_on; it goes off with either (gec_release).
    bool gac_on = false;
    DevBuf<uint32_t> gac_cand_ser;         // GapAcovArgs::gcand_ser (tail stream: one batch at a time, as the gap candidates are)
    DevBuf<unsigned long long> gac_stats;  // [kGapAcovStats]
    uint64_t gac_host_records = 0, gac_host_placements = 0;   // folded on the host since enable / groot_hip_acov_reset
    uint64_t gac_launches = 0;             // the four kernels of kernels_gap_acov.hpp since open
};

// One batch in flight.  Inputs and outputs are per slot (copy-in of batch b+1 and copy-out of batch b-1 overlap the
// kernels of batch b); everything the kernels only use between themselves is shared by all slots (one compute stream).
struct Slot {
    enum State { FREE, ACQUIRED, IN_FLIGHT, D2H_ISSUED, COLLECTED };
    State state = FREE;
    uint64_t ticket = 0;
    uint32_t n_reads = 0, first_read_id = 0, max_len = 0;
    uint32_t set = 0;                      // groot_ctx::ws the batch runs through
    uint32_t uniform_len = 0;              // IN_PACKED16: every read has this length (0 = lengths differ): no length array on the wire
    bool mixed_len = false;                // the reads are known to differ in length (the align stage then refills its wavefronts earlier)
    bool text_used = false;                // text_lookup_kernel ran first (the list behind it goes through the full-width kernel)
    bool sig_used = false;                 // the signature kernel ran in front of the full-width kernel for this batch
    uint32_t packed_q = 0;                 // SeedArgs::packed_q of the batch's signature kernel (0: it left no codes)
    bool lean_used = false;                // align_lean_kernel ran in front of align_kernel for this batch
    bool path_used = false;                // align_path_kernel ran in front of align_kernel for this batch
    uint32_t path_reads = 0;               // ... and finished this many reads
    float path_ms = 0;                     // ... in this time (profiling on: the pass, which also appends the list of the reads it leaves)
    bool one_len = false;                  // the reads are known to have max_len bases each, or the caller said so (submit_device with max_len)
    uint64_t n_bases = 0, n_exc = 0;
    enum Input { IN_ASCII, IN_PACKED, IN_PACKED16, IN_DEVICE } input = IN_ASCII;
    const uint8_t *ext_seq = nullptr;      // IN_DEVICE
    const uint64_t *ext_off = nullptr;
    // pinned staging (inputs)
    PinBuf<uint8_t> h_bases;               // ASCII or packed bases
    PinBuf<uint16_t> h_len;
    PinBuf<uint64_t> h_off, h_exc_pos;
    PinBuf<uint8_t> h_exc_byte;
    // HBM inputs
    DevBuf<uint16_t> d_len;
    DevBuf<uint32_t> d_packed;
    bool exc_at_home = false;                      // the batch's exception list is read from the pinned staging by the kernel that applies it
    DevBuf<uint8_t> d_seq, d_exc_byte;
    DevBuf<uint64_t> d_off, d_exc_pos;
    // outputs
    uint32_t trav_cap = 0;
    DevBuf<groot_trav> d_trav;
    DevBuf<uint64_t> d_mask;
    DevBuf<DeviceCounters> d_ctr;
    PinBuf<DeviceCounters> h_ctr;
    PinBuf<groot_trav> h_trav;                     // what collect hands out (expanded on the host from h_ctrav when the records travel packed)
    DevBuf<groot_ctrav> d_ctrav;                   // 12-byte records for the copy-out
    PinBuf<groot_ctrav> h_ctrav;
    PinBuf<uint8_t> h_mask;                        // COMPACT path sets: ceil(paths(graph) / 8) bytes per traversal
    PinBuf<uint32_t> h_ckpt;                       // offset into h_mask of every 256th traversal
    DevBuf<uint8_t> d_cmask;                       // the compact copy the copy-out takes (host-result mode)
    DevBuf<uint32_t> d_mwords, d_moff, d_ckpt;
    uint32_t n_trav = 0, copied = 0;               // records of the batch / records the copy-out enqueued at submit covers
    uint64_t n_mask_bytes = 0, copied_bytes = 0;
    bool host_results = false;             // the traversal records of this batch are in h_trav / h_mask
    hipEvent_t ev_seed = nullptr;          // behind the batch's seed stage on the compute stream: its align stage waits for it
    hipEvent_t ev_walk = nullptr;          // behind the batch's first pass (which appends the list of the reads it leaves) on the walk stream: its tail waits for it
    hipEvent_t ev_h2d0 = nullptr, ev_h2d = nullptr, ev_compute = nullptr, ev_ctr = nullptr, ev_d2h0 = nullptr, ev_d2h = nullptr;
    hipEvent_t ev[14]{};                   // [7..8] around the first seed kernel, [9..10] around order_first_kernel, [11] start of the align stage (align stream), [12] behind the list pass
                                           // [0..6] stage boundaries on the compute stream (profiling)
    groot_counts counts{};
    int status = GROOT_OK;
    std::string status_msg;
    groot_stage_ms ms{};
    SlotCounters ct;                       // what the counters behind the order stage keep per batch (counters.hip, rescue.hip)
    const uint8_t *seq() const { return input == IN_DEVICE ? ext_seq : d_seq.p; }
    const uint64_t *off() const { return input == IN_DEVICE ? ext_off : d_off.p; }
};

// One of the two sets of buffers a batch's seed stage fills for its align and order stages (groot_ctx::ws)
struct WorkSet {
    DevBuf<uint32_t> seed_count, seed_win, perm, perm_count, trav_cnt, tab_idx;
    DevBuf<uint32_t> perm2;                              // the reads the first pass left (LeanArgs::left); their number is ovf_cnt[kOvfShards + 2]
    DevBuf<uint4> packed;                                // SeedArgs::packed
    DevBuf<ReadRec> read_rec;
    DevBuf<uint4> vitem, split_list;                     // AlignArgs::vitem, sort_seed_lists_kernel
    DevBuf<uint32_t> vcount;                             // [0] items, [1] split reads of the batch
    DevBuf<groot_trav> trav_first;
    DevBuf<uint64_t> mask_first, sketches;
    // records beyond a read's first (both passes of the align stage append, order_ovf_kernel reads): per set, since the first pass of batch b+1
    // (walk stream) runs beside align_kernel and the order stage of batch b (tail stream); groot_ctx::ovf_cap slots per shard
    DevBuf<groot_trav> ovf_trav;
    DevBuf<uint64_t> ovf_mask;
    DevBuf<uint32_t> ovf_cnt;
    hipEvent_t ev_free = nullptr;          // on the tail stream behind the order stage of the batch that used the set last
    bool used = false;
    Slot *owner = nullptr;                 // whose seeds / sketches the set holds
    uint64_t ticket = 0;
};

struct groot_ctx {
    int device = 0;
    std::string err;
    groot_params prm{};
    Knobs kn;
    uint32_t s = 0, k = 0, max_k = 0, l_max = 0, pw_view = 0, pw = 0, n_windows = 0, max_q = 0, band_hash_bits = 0;
    hipEvent_t h2d_last = nullptr;         // the copy-in of the newest host-fed batch (its slot's event)
    Slot *newest = nullptr;                // the newest submitted batch (groot_hip_redo_status)
    hipEvent_t last_compute = nullptr;     // behind the order stage of the newest batch, on the tail stream (groot_hip_stream_join)
    // stream: seed stage (the caller's, if given); astream: the walk stream (first pass of the align stage, which appends the list of what it leaves);
    // tstream: the tail stream (align_kernel, order stage, host-copy and counting kernels) -- astream itself under GROOT_SERIAL_TAIL=1
    hipStream_t own_stream = nullptr, stream = nullptr, astream = nullptr, tstream = nullptr, own_tstream = nullptr, h2d_stream = nullptr, d2h_stream = nullptr;
    bool profiling = false;

    // index in HBM
    DevBuf<uint32_t> graph_win_end;
    DevBuf<uint4> cn_pre;                  // DeviceIndex::cn_pre
    DevBuf<uint64_t> node_l2b;             // DeviceIndex::node_l2b
    DevBuf<uint32_t> win_prefix, edges, win_graph, cn_node,
        band_keys, band_ids;
    DevBuf<ExactEntry> band_hash;
    DevBuf<uint8_t> band_sig;
    DevBuf<uint32_t> band_run;
    DevBuf<uint8_t> bases, q_k, q_l;
    DevBuf<uint16_t> q_min_eq;
    DevBuf<uint64_t> win_sketch;
    DevBuf<unsigned char> node_rec;
    DevBuf<LeanExt> lean_ext;
    DevBuf<LeanNode> lean_nodes;           // first pass of the align stage (kernels_lean.hpp): nodes, graph bases and ContainedNodes prefixes at 2 bits per base
    DevBuf<uint32_t> bases2;
    DevBuf<uint4> cn_pre2;
    DevBuf<uint8_t> win_ok;
    DevBuf<uint4> lean_stk;                // LeanArgs::stk (align stream)
    bool lean = false;                     // the first pass is align_lean_kernel (GROOT_LEAN=1)
    bool path = false;                     // the first pass is align_path_kernel (the default; pw == 3)
    DevBuf<uint4> path_node, path_hold;    // LeanArgs::path_* (kernels_path.hpp)
    DevBuf<uint32_t> path_text, path_tag, path_nodes;
    DevBuf<uint64_t> path_tab;
    DevBuf<WinRec> win_rec;
    DevBuf<ExactEntry> exact;
    DevBuf<SigEntry> sig;                  // sketch_sig_kernel: signature index + window texts (absent: that kernel is not used)
    DevBuf<uint4> sig_dir;
    DevBuf<uint8_t> win_text, win_nodes;
    DevBuf<uint32_t> sig_info;             // per window-text string: verdict byte, or where its tabulated outcome is (DeviceIndex::sig_info)
    DevBuf<uint4> out_tab;                 // AlignRead outcomes of the window-text strings (DeviceIndex::out_tab)
    std::vector<uint32_t> h_out_tab;       // the host's copy (groot_hip_read_seeds: seed windows of reads the text lookup answered)
    uint64_t out_strings = 0, out_tabulated = 0, out_entries = 0;   // strings that confirm reads / of them tabulated / table entries
    double out_build_ms = 0, open_ms = 0;
    uint32_t incr_cap = kIncrCap;
    bool tab_capture = false;              // the capture pass of groot_hip_open is running (align stage records the IncrementSubPath windows)
    DevBuf<uint32_t> tab_idx, tab_hist, incr_cnt, incr_win;
    DevBuf<uint4> text_tab;                // text_lookup_kernel: strings with a tabulated outcome, keyed by their bases
    uint64_t text_entries = 0;
    uint32_t batches_without_text = 0, text_retry_gap = 8;   // the lookup is tried again after this many batches without it; the gap doubles (up to 256) while it keeps missing
    double text_hit_frac = 1.0;            // share of the latest batch's reads the outcome table answered: picks the first kernel of the seed stage
    std::vector<uint16_t> h_q_min_eq;      // host copy of DeviceIndex::q_min_eq: which seed kernel a batch of one read length gets
    uint32_t sig_disabled = 0;             // windows whose text did not reproduce Key.Sketch (they cannot confirm reads)
    DeviceIndex dix{};

    // groot_hip_open_flags(GROOT_OPEN_BACKGROUND): the prefix tables and the signature index are built on a thread of its own while the
    // first batches already run (through the full-width kernel, without the seed stage's verdicts: same results, a little slower);
    // what it builds is described in bg_dix and moves into dix between two batches (install_background)
    std::thread bg;
    std::atomic<int> bg_state{0};          // 0 nothing pending, 1 running, 2 finished, 3 failed, 4 abandoned
    std::atomic<bool> bg_cancel{false};    // groot_hip_open_abandon / groot_hip_close: the builder stops at its next checkpoint
    int bg_rc = 0;
    std::string bg_err;
    DeviceIndex bg_dix{};
    uint32_t bg_seed_slots = 0, bg_max_read_len = 0;   // what the builder thread may know of the ctx's mutable state: copies taken before it starts
    hipStream_t bg_stream = nullptr;
    DevBuf<unsigned long long> bg_shards;
    // where the table builders of groot_hip_open work: the ctx's own index description / compute stream / shard counters, or the
    // background thread's
    DeviceIndex *build_dix = nullptr;
    hipStream_t build_stream = nullptr;
    unsigned long long *build_shards = nullptr;

    // pipeline
    std::vector<std::unique_ptr<Slot>> slots;
    std::deque<Slot *> inflight;           // submission order: IN_FLIGHT / D2H_ISSUED
    uint64_t next_ticket = 1;
    Slot *waited = nullptr;                // the batch groot_hip_wait collected (released by the next submit / wait)
    double todo_frac = 1.0;                // share of the latest finished batch's reads that the first seed kernel left to the list pass
    double lsh_frac = -1.0, long_frac = -1.0;   // shares of the latest finished batch's reads on lsh_heavy_kernel's and sort_seed_lists_kernel's lists (negative: no batch yet): their grids
    double lean_left_frac = 1.0;           // share of the latest finished batch's reads that the first pass of the align stage left to the second
    uint32_t n_cu = 256;
    double dfs_frac = 1.0;                 // share of the latest finished batch's reads that needed the align stage's graph walk (the rest: no seeds / tabulated outcomes)
    double trav_per_read = 1.25;           // traversal records per read of the latest finished batch: sizes the next copy-out
    double bytes_per_trav = 0;             // compact path-set bytes per traversal, likewise (0 = not seen yet: 8 * path_words)
    bool packed_travs = false;             // the copy-out sends 12-byte records (batches of at most 2^24 reads), collect expands them
    std::vector<uint32_t> h_node_graph;    // graph of every node (the expansion)
    DevBuf<uint8_t> graph_words;           // ceil(paths / 8) per graph: BYTES of a traversal's compact path set
    std::vector<uint8_t> h_graph_words;
    // What the seed stage of a batch leaves for its align and order stages lives in one of TWO work sets, taken in turn: the seed
    // stage of batch b+1 (compute stream) runs beside the align + order stages of batch b (align stream) -- the reference's sketching
    // minions and graph minions run side by side too (boss.go:134-203, graphminion.go:46-102).  Hashing is VALU-issue bound, the
    // graph walk waits on dependent loads: they want different resources.
    WorkSet ws[2];
    uint32_t next_set = 0;

    // shared work buffers: used on ONE of the three streams only, inside one stage
    uint32_t seed_slots = 0;
    DevBuf<uint32_t> sort_key, sort_key_out, perm_in, todo_list, todo_count;   // seed stage
    DevBuf<uint32_t> long_list, long_count;              // SeedArgs::long_list (seed stage)
    uint32_t vcap = 0;
    uint32_t lsh_defer_rows = 0, lsh_cap = 0;   // SeedArgs::lsh_defer_rows
    DevBuf<unsigned long long> seed_shards;
    DevBuf<uint32_t> lsh_list, lsh_count;  // reads on the LSH-Forest branch with many candidate rows + their sketches, for lsh_heavy_kernel (seed stage)
    DevBuf<uint64_t> lsh_sketch;
    DevBuf<char> sort_tmp, in_tmp;         // rocprim scratch of the seed stage / of the input decoding (compute stream)
    // The processing-order sort under the project's own launcher (order_sort.hpp; compute stream): its one scratch block for batches of up to
    // order_cap reads.  The block's state is all zero between two sorts; order_dirty_* is the sort whose clear is still to be issued (n = 0: none).
    DevBuf<uint32_t> order_buf;
    size_t order_cap = 0;
    uint32_t order_dirty_n = 0, order_dirty_begin = 0, order_dirty_end = 0;
    uint32_t ovf_cap = 0;
    DevBuf<uint32_t> trav_off;             // order stage (tail stream)
    DevBuf<char> scan_tmp;                 // rocprim scratch of the order stage (tail stream)
    // DFS stacks
    uint32_t align_threads = 0, stk_depth = 0;
    DevBuf<uint64_t> stk_hdr, stk_mask;
    // IncrementSubPath call counts: [rows][n_windows], one row per kmerCount that occurred
    DevBuf<uint32_t> attempts, q_row, q_seen, q_of_row, q_nrows;
    uint32_t *attempts_ptr = nullptr;      // own buffer or the caller's (groot_hip_attempts_layout)
    uint32_t att_cap = 0;                  // rows the table can hold
    bool att_external = false;
    Counters ct;                           // report coverage, shared reads, equivalence classes, assigned coverage, pairing (counters.hip); the rescue family (rescue.hip)
};

#define HIP_TRY(ctx, expr)                                                                             \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) return fail(ctx, GROOT_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

template <class T> static hipError_t upload(DevBuf<T> &d, const T *src, size_t n, size_t pad = 0)
{
    hipError_t e = d.alloc(n + pad);
    if (e != hipSuccess) return e;
    if (pad) {
        e = hipMemset(d.p, 0, (n + pad) * sizeof(T));
        if (e != hipSuccess) return e;
    }
    if (n) e = hipMemcpy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

// what counters.hip, rescue.hip and open.hip need of the pipeline (groot_hip.hip); open.hip's further calls: open.hpp
namespace groot {
int fail(groot_ctx *ctx, int code, const char *fmt, ...);   // sets the ctx's (no ctx: the thread's) error text, returns code
int drain(groot_ctx *c);                                    // everything submitted has finished on the device (results stay collectable)
bool idle(const groot_ctx *c);                              // nothing is in flight
} // namespace groot
