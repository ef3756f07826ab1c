// groot_hip.hip -- libgroot_hip.so: the batch pipeline of a ctx (ctx.hpp) and the C ABI of include/groot_hip.h.  groot_hip_open* -- the device tables,
// the work buffers, the memo -- are open.hip (open.hpp); the counters behind the order stage and their part of the ABI are counters.hip (the rescue family among them: rescue.hip), reached
// through the hooks of counters.hpp.
// gfx950 only; no CPU fallback anywhere in this library.
#include <cstring>   // before rocprim: its texture iterator calls host memset

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <atomic>
#include <chrono>
#include <deque>
#include <iterator>
#include <array>
#include <map>
#include <tuple>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../common/cpus.hpp"
#include "counters.hpp"
#include "ctx.hpp"
#include "kernels_misc.hpp"
#include "kernels_path.hpp"
#include "launch.hpp"
#include "open.hpp"
#include "order_sort.hpp"

using namespace groot;

// A ctx drives five HIP streams at once -- seed stage, walk (first pass of the align stage), tail (align_kernel + order stage), copy-in,
// copy-out -- beside whatever the host process uses itself.  The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and streams that share one
// run one after the other: with a fifth stream in the process the copy-in and the copy-out of neighbouring batches took turns
// (host-fed rate 1 355 -> 717 Mreads/s).  Ask for eight before the runtime reads the setting (first HIP call of the process); a
// value the user has set stands.
__attribute__((constructor)) static void groot_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

static thread_local std::string g_open_err;

static thread_local bool tl_background = false;       // this thread is a ctx's background builder

namespace groot {

int fail(groot_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) (tl_background ? ctx->bg_err : ctx->err) = buf;
    else g_open_err = buf;
    return code;
}

void enter_background_thread() { tl_background = true; }
bool on_background_thread() { return tl_background; }

} // namespace groot

// ---------------------------------------------------------------------------------------------
// batch execution
// ---------------------------------------------------------------------------------------------
int groot::alloc_seed_slots(groot_ctx *c, uint32_t slots)
{
    c->seed_slots = slots;
    // (both work sets get new buffers with a new stride: whatever seeds they held are gone -- groot_hip_read_seeds must not find an owner)
    for (WorkSet &w : c->ws) { HIP_TRY(c, w.seed_win.alloc((size_t)slots * c->prm.max_batch_reads)); w.owner = nullptr; w.ticket = 0; }
    return GROOT_OK;
}

static int alloc_trav(groot_ctx *c, Slot *s, uint32_t cap)
{
    s->trav_cap = cap;
    HIP_TRY(c, s->d_trav.alloc((size_t)cap + 2));
    HIP_TRY(c, s->d_mask.alloc((size_t)cap * c->pw_view + 2));
    if (!c->prm.results_on_device) {
        HIP_TRY(c, s->h_trav.alloc((size_t)cap + 2));
        HIP_TRY(c, s->h_mask.alloc((size_t)cap * c->pw_view * 8 + 16));
        HIP_TRY(c, s->h_ckpt.alloc((size_t)cap / 256 + 2));
        HIP_TRY(c, s->d_cmask.alloc((size_t)cap * c->pw_view * 8 + 16));
        HIP_TRY(c, s->d_mwords.alloc(cap));
        HIP_TRY(c, s->d_moff.alloc(cap));
        HIP_TRY(c, s->d_ckpt.alloc((size_t)cap / 256 + 2));
        if (c->packed_travs) {
            HIP_TRY(c, s->d_ctrav.alloc((size_t)cap + 2));
            HIP_TRY(c, s->h_ctrav.alloc((size_t)cap + 2));
        }
    }
    return GROOT_OK;
}

int groot::alloc_ovf(groot_ctx *c, uint32_t cap_per_shard)
{
    c->ovf_cap = cap_per_shard;
    for (WorkSet &w : c->ws) {
        HIP_TRY(c, w.ovf_trav.alloc((size_t)kOvfShards * cap_per_shard));
        HIP_TRY(c, w.ovf_mask.alloc((size_t)kOvfShards * cap_per_shard * c->pw));
    }
    return GROOT_OK;
}

// call-count table with room for `rows` kmerCounts; existing rows are kept (device-to-device copy)
int groot::grow_attempts(groot_ctx *c, uint32_t rows)
{
    if (c->att_external) return fail(c, GROOT_E_NOSPACE, "a kmerCount outside the fixed layout of groot_hip_attempts_layout occurred");
    DevBuf<uint32_t> bigger;
    HIP_TRY(c, bigger.alloc((size_t)rows * c->n_windows));
    HIP_TRY(c, hipMemset(bigger.p, 0, (size_t)rows * c->n_windows * sizeof(uint32_t)));
    if (c->attempts.p && c->att_cap)
        HIP_TRY(c, hipMemcpy(bigger.p, c->attempts.p, (size_t)std::min(rows, c->att_cap) * c->n_windows * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    std::swap(c->attempts.p, bigger.p);
    std::swap(c->attempts.n, bigger.n);
    c->attempts_ptr = c->attempts.p;
    c->att_cap = rows;
    return GROOT_OK;
}

constexpr double kSparseBelow = 0.05;   // share of a batch left for the graph walk below which the processing order is a stream compaction and half the persistent grid runs
struct HasKey {     // reads the seed stage left for the align stage's graph walk carry a scheduling key
    const uint32_t *key;
    __host__ __device__ bool operator()(uint32_t r) const { return key[r] != kEmpty; }
};
#ifndef GROOT_SPAN_BITS
#define GROOT_SPAN_BITS 6
#endif
// The list pass copies each read into its lane's LDS slice while five workgroups per CU still fit (reads up to ~104 bases: 1.77 vs 1.57
// Greads/s on 100-base reads with errors); for longer reads it reads the bases from HBM -- the copy would cost the fifth wavefront
// per SIMD and a dependent trip (seed stage of 8 M reads of 75..150 bases: 7.0 ms with the copy, 5.9 ms without).
static uint32_t list_lds_stride(uint32_t stride_dw)
{
    return kLdsReads + (uint64_t)kBlock * stride_dw * 4 <= 32 * 1024 ? stride_dw : 0;
}
// workgroups of the two wavefront-per-read kernels of the seed stage's tail (grid-stride over their lists): many small shares level out reads that
// cost between a few and a few thousand rows (round 5, 8 M reads of 75..150 bases, t = 0.99 / 0.90: heavy reads 512 / 2 048 / 8 192 / 32 768 workgroups
// -> 1 306 / 1 330 / 1 347 / 1 356 and 667 / 728 / 750 / 748 Mreads/s; seed-list sort 512 / 2 048 / 8 192 -> 1 283 / 1 330 / 1 360 and 680 / 728 / 748)
#ifndef GROOT_HEAVY_BLOCKS
#define GROOT_HEAVY_BLOCKS 16384u
#endif
#ifndef GROOT_SORTLIST_BLOCKS
#define GROOT_SORTLIST_BLOCKS 16384
#endif
// The processing-order sort runs beside the previous batch's first pass, whose 256-thread workgroups hold the whole register file of every CU.
// rocprim's default onesweep for gfx950 (1 024 threads, 16 items) needs four free wavefront places on every SIMD of a CU at once, which happens
// only when the first pass runs dry: the sort waited for it.  256-thread workgroups (one wavefront per SIMD) fit the hole one retiring first-pass
// workgroup leaves.  Same digits (8 bits), same stable ranking: perm is bit-identical.  
// Which rocprim algorithm a batch of n reads takes under this configuration: n <= 1 024 the single-block sort (256 x 4, rocprim's default), n <= GROOT_SORT_MERGE_LIMIT
// rocprim's merge sort (default configuration), above it the onesweep configured here.  rocprim's own limit is 2^20; 2 048 = two blocks of the single sort,
// so that every batch that needs more than a handful of workgroups gets the kernels that fit beside the first pass, and so that the suite reaches them
// with small batches (tests/test_order_handoff.py).  All three are stable sorts of the same bits.  List-mode batches (few reads walked) are not sorted at all.
#ifndef GROOT_SORT_ITEMS
#define GROOT_SORT_ITEMS 16
#endif
#ifndef GROOT_SORT_MERGE_LIMIT
#define GROOT_SORT_MERGE_LIMIT 2048
#endif
using OrderSortConfig = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, GROOT_SORT_ITEMS>, rocprim::kernel_config<256, GROOT_SORT_ITEMS>, 8,
                                        rocprim::block_radix_rank_algorithm::match>,
    GROOT_SORT_MERGE_LIMIT>;

// Round 28: the grid of a wavefront-per-read kernel over a list whose length the latest finished batch predicts (frac: its share of that batch's reads,
// negative = no batch has finished yet).  A wavefront per expected read and a quarter more, at least a workgroup per CU, at most `most` -- round 5's grid,
// which every list of 4 x most / 1.25 reads or more keeps, as does a ctx that has seen no batch: on configs[2] the lists are empty or nearly so and
// 16 384 workgroups that find nothing cost 0.06 ms of grid dispatch each.  Grid-stride loops: a list longer than predicted is slower, never wrong.
static uint32_t wave_list_blocks(const groot_ctx *c, const Slot *s, double frac, uint32_t most)
{
    if (frac < 0.0) return most;
    const double want = frac * 1.25 * (double)s->n_reads / (kBlock / 64) + 1.0;
    return want >= (double)most ? most : std::min(most, std::max<uint32_t>((uint32_t)want, c->n_cu));
}

// a batch of one read length of which fewer than six reads in ten (but not next to none) are walked, by the latest finished batch: reads with errors --
// the exact ones seed, the others do not.  The hashing kernels of the next batch are the longer stage there.
static bool error_batch(const groot_ctx *c, const Slot *s) { return c->dfs_frac >= kSparseBelow && c->dfs_frac < 0.6 && !s->mixed_len; }

// the one fill of the order sort's scratch (order_sort.hpp): zeroes what the latest sort through it dirtied.  On the compute stream, behind that sort.
static int clear_order_sort(groot_ctx *c)
{
    if (!c->order_dirty_n) return GROOT_OK;
    const order_sort::Scratch sc{c->order_buf.p, c->order_cap};
    const uint32_t n = c->order_dirty_n;
    c->order_dirty_n = 0;
    HIP_TRY(c, order_sort::clear(sc, n, c->order_dirty_begin, c->order_dirty_end, c->stream));
    return GROOT_OK;
}

static int launch_seed_stage(groot_ctx *c, Slot *s, bool update_weights)
{
    WorkSet *w = &c->ws[s->set];
    SeedArgs a{};
    s->packed_q = 0;
    a.ix = c->dix;
    a.seq = s->seq();
    a.seq_off = s->off();
    a.n_reads = s->n_reads;
    a.max_read_len = c->prm.max_read_len;
    const uint64_t want = (uint64_t)kBlock * s->max_len + 32;
    a.lds_read_bytes = (uint32_t)std::min<uint64_t>(want, kMaxLdsReadBytes);
    a.seed_slots = c->seed_slots;
    a.seed_count = w->seed_count.p;
    a.seed_win = w->seed_win.p;
    a.sketch_out = c->prm.keep_sketches ? w->sketches.p : nullptr;
    a.sort_key = c->sort_key.p;
    a.read_rec = w->read_rec.p;
    a.q_seen = c->q_seen.p;
    a.trav_cnt = w->trav_cnt.p;
    a.shards = c->seed_shards.p;
    a.ctr = s->d_ctr.p;
    a.long_list = c->long_list.p; a.long_count = c->long_count.p;
    if (c->dix.out_tab) {                                   // reads the signature kernel finds in the outcome table say so here
        a.tab_idx = w->tab_idx.p;
        a.tab_hist = c->tab_hist.p;
    }
    // processing order of the align stage: reads sorted by (node span of the first seed window, that window, likely
    // orientation).  key = span << (32-span_bits) | window << 2 | class; reads without seeds carry 0xFFFFFFFF and sort last
    unsigned win_bits = 2;                                  // 2 class bits + the bits of the largest window id
    for (uint32_t v = c->n_windows ? c->n_windows - 1 : 0; v; v >>= 1) win_bits++;
    win_bits = std::min(32u, std::max(3u, win_bits));
    // (round 5: the span class sits right above the window bits, five bits when that makes the sorted range 24 bits -- three passes of the radix sort
    // instead of four; the two class bits below the window are not sorted on: reads of one window are neighbours either way)
    a.sort_span_bits = std::min((unsigned)GROOT_SPAN_BITS, 32u - win_bits);
    if (win_bits - 2u + a.sort_span_bits > 24u && win_bits - 2u + 4u <= 24u) a.sort_span_bits = 24u - (win_bits - 2u);
    // (reads without seeds carry 0xFFFFFFFF: all ones in the span field, which no window has -- every window contains a node -- so they sort last)
    a.sort_span_shift = win_bits;
    // (the low window bits matter: sorted without the lowest 4 / 8 of them -- two radix passes instead of three -- configs[2] through the kernels ran at
    // 1 832 / 1 406 instead of 2 035 Mreads/s, the align kernel 3.6 / 5.4 ms instead of 3.1: neighbouring windows walk the same nodes)
    const unsigned begin_bit = 2u, end_bit = win_bits + a.sort_span_bits;
    const dim3 grid((s->n_reads + kBlock - 1) / kBlock);
    // workgroups of the list pass (grid-stride over the list).  Round 5: as many as the list is expected to need at a read per thread -- the latest
    // finished batch says how long it was --, not the 1 280 (five per CU) that are resident at once: reads of the LSH-Forest branch cost between a
    // few and a few hundred row visits, a workgroup that walks eight or nine sets of 256 of them in a fixed order ends when its slowest sets add up,
    // and workgroups dealt out as CUs become free level that (8 M reads of 75..150 bases, 2.84 M on the list, t = 0.99 / 0.90: 1 024 -> 1 229 / 665,
    // 1 280 -> 1 255 / 699, 2 560 -> 1 294 / 710, 5 120 -> 1 340 / 726, 20 480 -> 1 346 / 730 Mreads/s).  At least 1 280, so that a batch that
    // differs from the one before is not left with a handful.
#ifndef GROOT_LIST_BLOCKS_MIN
#define GROOT_LIST_BLOCKS_MIN 1280
#endif
    const uint32_t list_blocks = std::max<uint32_t>(GROOT_LIST_BLOCKS_MIN, (uint32_t)std::min<double>(4.0e6, c->todo_frac * 1.25 * (double)s->n_reads / kBlock + 1.0));
    // a batch of one read length that is not on the exact-table branch (lower thresholds, reads shorter than the windows) would
    // send every read through the list: the full-width kernel alone is 25-30 % faster then (tools/threshold_probe.py)
    bool sig_useful = true;
    if (s->one_len && s->max_len >= c->k) {
        const uint32_t q = s->max_len - c->k + 1;
        sig_useful = q < c->h_q_min_eq.size() && c->h_q_min_eq[q] == c->s;
    }
    s->sig_used = c->dix.sig && !c->prm.keep_sketches && sig_useful;
    // Which kernel sees the batch first?  When the outcome table answered most of the latest batch, the text lookup (no hashing at
    // all; what it does not find goes through the full-width kernel, read by read); else the signature kernel as before.
    // (the share is only known exactly while the lookup runs: it is tried again after 8, 16, ... 256 batches)
    const double list_below = kSparseBelow;
    const bool list_mode = c->dfs_frac < list_below;       // few reads need the graph walk (the latest batch says so)
    const bool text_try = c->text_hit_frac >= 0.7 || ++c->batches_without_text >= c->text_retry_gap;
    s->text_used = !c->prm.keep_sketches && c->dix.text_tab && c->dix.out_tab && text_try && s->max_len >= c->dix.w && !c->tab_capture;
    if (s->text_used) c->batches_without_text = 0;
    if (c->lsh_list.p && !c->prm.keep_sketches) {
        a.lsh_list = c->lsh_list.p; a.lsh_count = c->lsh_count.p; a.lsh_sketch = c->lsh_sketch.p;
        a.lsh_defer_rows = c->lsh_defer_rows; a.lsh_cap = c->lsh_cap;
    }
    // (lsh_count, todo_count, long_count: zero -- assign_q_rows_kernel at the end of the seed stage before left them so; w->vcount: order_ovf_kernel
    // of the batch that used the work set before did; both were cleared when they were allocated)
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[7], c->stream));
    if (s->text_used) {
        a.todo_list = c->todo_list.p;
        a.todo_count = c->todo_count.p;
        const uint32_t stride_dw = ((s->max_len + 3) / 4 + 1) | 1u;
        a.list_stride_dw = list_lds_stride(stride_dw);
        const size_t lds = kTextBad + (size_t)((a.lds_read_bytes + 15) / 16) * 4 + 96;
        if (list_mode) {       // the reads left for the graph walk are a subset of the lookup's misses: the list pass appends them itself
            a.dfs_list = w->perm.p; a.dfs_count = w->perm_count.p;
            HIP_TRY(c, hipMemsetAsync(w->perm_count.p, 0, sizeof(uint32_t), c->stream));
        }
        launch_text_lookup(text_key_dwords((c->dix.w + 15) / 16), a, grid, lds, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[8], c->stream));
        launch_list(c->s, a, dim3(std::min<uint32_t>(grid.x, list_blocks)), c->stream);
    } else if (s->sig_used) {
        // signature kernel first; what it cannot decide goes through the full-width kernel, read by read
        a.todo_list = c->todo_list.p;
        a.todo_count = c->todo_count.p;
        const uint32_t stride_dw = ((s->max_len + 3) / 4 + 1) | 1u;     // the LIST pass copies each read into its lane's LDS slice
        a.list_stride_dw = list_lds_stride(stride_dw);
        // (the reads it decides it also leaves as 2-bit codes for the first pass of the align stage)
        if ((c->lean || c->path) && !c->tab_capture && w->packed.p) { a.packed = w->packed.p; a.packed_q = s->max_len <= 128 ? 2u : 4u; }
        s->packed_q = a.packed ? a.packed_q : 0;
        launch_sig(c->s, a, s->max_len, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[8], c->stream));
        launch_list(c->s, a, dim3(std::min<uint32_t>(grid.x, list_blocks)), c->stream);
    } else {
        const size_t lds = kLdsReads + ((a.lds_read_bytes + 15) & ~15u);
        launch_seed(c->s, c->max_k, a, c->prm.keep_sketches != 0, grid, lds, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[8], c->stream));
    }
    // the reads of the LSH-Forest branch with many candidate rows: a wavefront each
    if (a.lsh_list) hipLaunchKernelGGL(lsh_heavy_kernel, dim3(std::min<uint32_t>(grid.x, wave_list_blocks(c, s, c->lsh_frac, GROOT_HEAVY_BLOCKS))), dim3(kBlock), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[12], c->stream));   // (the list pass behind the first kernel + the heavy LSH-Forest reads)
    // seed lists of more than four windows that are not ascending (LSH-Forest hits come in band order): sorted, a wavefront per read
    // ... and the longest ones cut into items that different lanes of the align stage take
    {
        SplitArgs sa{};
        sa.list = c->long_list.p; sa.count = c->long_count.p; sa.seed_count = w->seed_count.p; sa.seed_win = w->seed_win.p;
        sa.n_reads = s->n_reads; sa.seed_slots = c->seed_slots; sa.read_rec = w->read_rec.p; sa.win_rec = c->dix.win_rec;
        sa.split = c->vcap && !c->tab_capture && !c->prm.no_exact_align;
        sa.vitem = w->vitem.p; sa.vcount = w->vcount.p; sa.vcap = c->vcap; sa.split_list = w->split_list.p;
        sa.ctr = s->d_ctr.p; sa.update_weights = update_weights ? 1 : 0;
        hipLaunchKernelGGL(sort_seed_lists_kernel, dim3(wave_list_blocks(c, s, c->long_frac, GROOT_SORTLIST_BLOCKS)), dim3(kBlock), 0, c->stream, sa);
    }
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[2], c->stream));
    hipLaunchKernelGGL(assign_q_rows_kernel, dim3(1), dim3(64), 0, c->stream, c->q_seen.p, c->q_row.p, c->q_of_row.p, c->q_nrows.p, c->att_cap,
                       c->max_q, s->d_ctr.p, c->seed_shards.p, c->long_count.p, c->todo_count.p, c->lsh_count.p, w->ovf_cnt.p);
    if (a.tab_hist) {
        hipLaunchKernelGGL(fold_tab_hist_kernel, dim3(std::min<uint32_t>((c->n_windows + kBlock - 1) / kBlock, 1024u)), dim3(kBlock), 0, c->stream, c->tab_hist.p,
                           c->attempts_ptr, c->q_row.p, c->dix.w - c->k + 1, c->n_windows, s->d_ctr.p, update_weights ? 1u : 0u);
        HIP_TRY(c, hipGetLastError());
    }
    if (list_mode && a.dfs_list) return GROOT_OK;           // (the processing order was written by the seed stage)
    if (list_mode) {
        // Few reads need the graph walk (the latest batch says so; most are answered from the outcome table or have no seeds): sorting
        // ten million keys to order a few of them costs more than their order saves.  The processing order is then simply the reads
        // with a key, ascending -- one stream compaction (0.05 instead of 0.45 ms per 10 M reads).  Processing order only.
        size_t tb = 0;
        HasKey pred{c->sort_key.p};
        rocprim::counting_iterator<uint32_t> ids(0u);
        HIP_TRY(c, rocprim::select(nullptr, tb, ids, w->perm.p, w->perm_count.p, (size_t)s->n_reads, pred, c->stream));
        if (tb > c->sort_tmp.n) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, c->sort_tmp.alloc(tb + tb / 4));
        }
        HIP_TRY(c, rocprim::select(c->sort_tmp.p, tb, ids, w->perm.p, w->perm_count.p, (size_t)s->n_reads, pred, c->stream));
        return GROOT_OK;
    }
    size_t tmp_bytes = 0;
    // keys are (window << 2 | class) below 2^end_bit, or 0xFFFFFFFF for reads without seeds: sorting the low
    // end_bit bits keeps those last as long as bit end_bit-1.. are all ones for them, which they are
    // (batches of one read length of which fewer than six reads in ten are walked -- reads with errors: the previous batch's first pass is the shorter
    // stage there and the sort does not wait for it; the small blocks cost 0.1 ms alone and 3 % of that workload's rate, so it keeps rocprim's default)
    const bool small_blocks = !error_batch(c, s);
    // Round 28: the batches that take the onesweep configured above go through the project's own launcher (order_sort.hpp): rocprim's device code, but no
    // fill between two of its kernels -- the one clear of its scratch is issued by run_batch_async behind ev_seed, beside the first pass.  Batches at or
    // below GROOT_SORT_MERGE_LIMIT and batches that keep rocprim's default call the library as before; GROOT_LIBRARY_SORT: every batch does.
    if (small_blocks && !c->kn.library_sort && s->n_reads > GROOT_SORT_MERGE_LIMIT && s->n_reads <= order_sort::kMaxItems) {
        if (s->n_reads > c->order_cap) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            const size_t cap = (size_t)s->n_reads + s->n_reads / 4;
            c->order_cap = 0;
            HIP_TRY(c, c->order_buf.alloc(order_sort::Scratch::bytes(cap) / sizeof(uint32_t)));
            c->order_cap = cap;
            c->order_dirty_n = 0;
            HIP_TRY(c, hipMemsetAsync(c->order_buf.p, 0, order_sort::state_words(cap, order_sort::kMaxPlaces) * sizeof(uint32_t), c->stream));
        }
        const order_sort::Scratch sc{c->order_buf.p, c->order_cap};
        if (int rc = clear_order_sort(c)) return rc;         // (a sort whose clear an error return skipped)
        c->order_dirty_n = s->n_reads; c->order_dirty_begin = begin_bit; c->order_dirty_end = end_bit;
        HIP_TRY(c, order_sort::sort_pairs(sc, c->sort_key.p, c->sort_key_out.p, c->perm_in.p, w->perm.p, s->n_reads, begin_bit, end_bit, c->stream));
        return GROOT_OK;
    }
    auto sort = [&](void *tmp) {
        return small_blocks ? rocprim::radix_sort_pairs<OrderSortConfig>(tmp, tmp_bytes, c->sort_key.p, c->sort_key_out.p, c->perm_in.p, w->perm.p, s->n_reads,
                                                                         begin_bit, end_bit, c->stream)
                            : rocprim::radix_sort_pairs(tmp, tmp_bytes, c->sort_key.p, c->sort_key_out.p, c->perm_in.p, w->perm.p, s->n_reads, begin_bit, end_bit,
                                                        c->stream);
    };
    HIP_TRY(c, sort(nullptr));
    if (tmp_bytes > c->sort_tmp.n) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, c->sort_tmp.alloc(tmp_bytes + tmp_bytes / 4));
    }
    HIP_TRY(c, sort(c->sort_tmp.p));
    return GROOT_OK;
}

static int launch_align_stage(groot_ctx *c, Slot *s, bool update_weights)
{
    WorkSet *w = &c->ws[s->set];
    AlignArgs a{};
    a.ix = c->dix;
    a.seq = s->seq();
    a.seq_off = s->off();
    a.n_reads = s->n_reads;
    a.first_read_id = s->first_read_id;
    a.seed_slots = c->seed_slots;
    a.seed_count = w->seed_count.p;
    a.seed_win = w->seed_win.p;
    a.perm = w->perm.p;
    a.read_rec = w->read_rec.p;
    a.no_align = c->prm.no_exact_align;
    a.update_weights = update_weights ? 1 : 0;
    a.attempts = c->attempts_ptr;
    a.node_rec = c->node_rec.p;
    a.trav_first = w->trav_first.p;
    a.mask_first = w->mask_first.p;
    a.trav_cnt = w->trav_cnt.p;
    a.ovf_trav = w->ovf_trav.p;
    a.ovf_mask = w->ovf_mask.p;
    a.ovf_cnt = w->ovf_cnt.p;
    a.ovf_cap = c->ovf_cap;
    if (c->vcap) { a.vitem = w->vitem.p; a.vcount = w->vcount.p; a.vcap = c->vcap; }
    a.stk_hdr = c->stk_hdr.p;
    a.stk_mask = c->stk_mask.p;
    uint32_t blocks = std::min<uint32_t>((s->n_reads + kBlock - 1) / kBlock, c->align_threads / kBlock);
    // (few reads left for the walk -- the latest batch says so: half the persistent grid starts and drains 0.05 ms sooner and the
    // slowest read, not the number of wavefronts, sets the duration anyway)
    // (... unless there are reads enough to give every wavefront of the whole grid a round of 16: reads that fail -- reads with an error that
    // kept their minimisers -- do not march in step, and more wavefronts with fewer of them each end sooner)
    if (c->dfs_frac < kSparseBelow && c->dfs_frac * (double)s->n_reads < 16.0 * (double)(blocks * (kBlock / 64))) blocks = std::max(1u, blocks / 2);
    // (round 5: when fewer than six reads in ten need the walk -- reads with errors: the exact ones seed, the others do not -- the hashing kernels of the
    // next batch are the longer stage, and a persistent grid of two workgroups per CU leaves them half the registers: configs[2] with 1 % substitutions
    // 2 345 -> 2 680 Mreads/s; no difference on mixed-length batches; on error-free reads, where every read is walked, the full grid is 4 % faster)
    else if (error_batch(c, s) && blocks >= 4) blocks /= 2;
    // (the first pass takes most reads: what it left in the latest batch sizes the persistent grid of the second -- a wavefront per 64 reads left,
    // at least one workgroup per CU; the registers it does not hold go to the next batch's hashing kernels)
    // (only when a first pass runs for THIS batch: long-read and sparse batches keep the whole grid)
    // (s->lean_used / s->path_used: run_batch_async decided them, and with them the stream the stage starts on)
    if ((s->lean_used || s->path_used) && c->lean_left_frac < 0.25) {
        uint32_t want = (uint32_t)(c->lean_left_frac * 1.25 * (double)s->n_reads / 64.0 / (kBlock / 64)) + 1u;
        blocks = std::max(1u, std::min(blocks, std::max(want, c->n_cu)));
    }
    a.n_threads = blocks * kBlock;
    a.stk_depth = c->stk_depth;
    // stage reads in LDS when 256 lanes x (longest read + slack) stays within 64 KB
    {
        // 8 zero bytes, then the read in whole 16-byte pieces up to 12 bytes past its end; odd dword stride = no bank conflicts
        const uint32_t stride = (2 + 4 * ((s->max_len + 27) / 16)) | 1u;
        a.lds_stride_dw = (size_t)kBlock * stride * 4 <= 64 * 1024 ? stride : 0;
    }
    if (c->tab_capture) {
        a.incr_cnt = c->incr_cnt.p; a.incr_win = c->incr_win.p; a.incr_cap = c->incr_cap;
        HIP_TRY(c, hipMemsetAsync(c->incr_cnt.p, 0, (size_t)s->n_reads * sizeof(uint32_t), c->tstream));   // (no first pass while capturing: the whole stage is on the tail stream)
    }
    a.head_lanes = s->mixed_len ? 16u : 0u;              // (8: best at 2 M reads before the items of split reads took the head; 16: 2.9 / 5.2 ms at 2 M / 8 M reads, 8 gave 3.05 / 5.6)
    // (round 5: 48 when fewer than six reads in ten are walked -- reads with errors: some align at once, some fail through the hierarchy, and lanes that
    // have finished take new reads before the whole round has: configs[2] with 1 % substitutions, memo off, 2 625 -> 2 740 Mreads/s; on error-free reads,
    // which march in step, 64 stays: 1 966 against 1 892 / 1 895 / 1 908 at 32 / 48 / 56)
#ifndef GROOT_REFILL_ERR
#define GROOT_REFILL_ERR 48       // (2 / 16 / 32 / 48: 2 674 / 2 712 / 2 736 / 2 755 Mreads/s on configs[2] with 1 % substitutions, memo off)
#endif
#ifndef GROOT_REFILL_MIXED
#define GROOT_REFILL_MIXED 2      // mixed read lengths: a lane that has finished takes its next read at once -- no rounds (2 / 8 / 16 / 32 / 48: 1 258 / 1 253 / 1 249 / 1 208 /
                                  // 1 172 Mreads/s at t = 0.99 on 8 M reads of 75..150 bases, 694 / 678 / 680 / 676 / 653 at t = 0.90; batches of 2 M: 850-890 -> 912)
#endif
    a.refill = s->mixed_len ? (uint32_t)GROOT_REFILL_MIXED : (error_batch(c, s) ? (uint32_t)GROOT_REFILL_ERR : 64u);                   // reads of many lengths finish their walks far apart (tools/mixed_probe.py)
#ifdef GROOT_WORK_COUNTERS
    if (const char *e = getenv("GROOT_DEV_ROUND")) a.round_lanes = (uint32_t)atoi(e);   // instrumented builds only (tools/slow_reads_probe.py: one read per round)
#endif
    a.ctr = s->d_ctr.p;
    // Walk stream: the first pass, which appends the list of what it leaves.  Tail stream: align_kernel and everything behind it -- the tail of batch b runs
    // beside the first pass of batch b+1.  A batch without a first pass has no walk part: its whole stage goes on the tail stream, so that the
    // persistent align_kernel launches (they share the DFS stacks) stay in order with one another.
    const bool first_pass = s->lean_used || s->path_used;
    // (w->ovf_cnt -- the shard counts, the two chunk cursors and the length of the first pass's list -- is zero: assign_q_rows_kernel of this batch's seed
    // stage cleared it, so nothing stands on the walk stream between the wait for ev_seed and the first pass)
    // First pass (kernels_lean.hpp): a thread per read in processing order finishes the reads of one seed window whose walks never branch;
    // the reads it leaves it appends to a list (a wavefront at a time, in the order the wavefronts finish), and align_kernel takes that list.
    const uint32_t lean_stride = lean_stride_dw(s->max_len);
    // (GROOT_LEAN=1: every batch that has reads to walk.  Measured, DESIGN.md section 3: alone on the chip the two passes take 2.2 + 0.7 ms where align_kernel
    // takes 3.0 on configs[2]; beside the next batch's hashing kernels the step is between 1.5 % shorter and 8 % longer from box to box, and batches of
    // mixed lengths or of reads with errors are slower -- hence off by default.)
    if (first_pass) {
        LeanArgs l{};
        l.nodes = c->lean_nodes.p; l.ext = c->lean_ext.p; l.bases2 = c->bases2.p; l.cn_pre2 = c->cn_pre2.p; l.win_ok = c->win_ok.p;
        l.win_rec = c->dix.win_rec; l.node_l2b = c->dix.node_l2b; l.q_row = c->q_row.p;
        l.seq = s->seq(); l.packed = s->packed_q ? w->packed.p : nullptr; l.packed_q = s->packed_q; l.perm = w->perm.p; l.read_rec = w->read_rec.p;
        l.n_reads = s->n_reads; l.first_read_id = s->first_read_id; l.n_windows = c->n_windows; l.k = c->k;
        l.update_weights = update_weights ? 1 : 0;
        l.lds_stride_dw = lean_stride; l.max_len = s->max_len;
        l.attempts = c->attempts_ptr;
        l.trav_first = w->trav_first.p; l.mask_first = w->mask_first.p; l.trav_cnt = w->trav_cnt.p;
        l.left = w->perm2.p; l.left_cnt = w->ovf_cnt.p + kOvfShards + 2; l.ctr = s->d_ctr.p;
        l.stk = c->lean_stk.p; l.ovf_trav = w->ovf_trav.p; l.ovf_mask = w->ovf_mask.p; l.ovf_cnt = w->ovf_cnt.p; l.ovf_cap = c->ovf_cap;
        // workgroups for the reads expected to have seeds (the latest batch says how many: they come first in the processing order); the slots
        // beyond them, if the batch has more, go to align_kernel behind the list (AlignArgs::rest: addressed in place, not copied)
        const uint32_t lean_blocks = std::min<uint32_t>((s->n_reads + kBlock - 1) / kBlock, (uint32_t)(c->dfs_frac * 1.05 * (double)s->n_reads / kBlock) + 64u);
        if (s->path_used) {
            l.path_node = c->path_node.p; l.path_text = c->path_text.p; l.path_tag = c->path_tag.p; l.path_nodes = c->path_nodes.p; l.path_tab = c->path_tab.p;
            l.hold = c->path_hold.p;
            launch_align_path(c->pw, l, dim3(lean_blocks), c->astream);
        } else launch_align_lean(c->pw, l, dim3(lean_blocks), c->astream);
        HIP_TRY(c, hipGetLastError());
        a.perm = w->perm2.p;
        a.n_perm = l.left_cnt;
        a.rest = w->perm.p;
        a.rest_lo = lean_blocks * (uint32_t)kBlock;
        if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[13], c->astream));
        if (c->tstream != c->astream) {
            HIP_TRY(c, hipEventRecord(s->ev_walk, c->astream));
            HIP_TRY(c, hipStreamWaitEvent(c->tstream, s->ev_walk, 0));
        }
    }
    launch_align(c->pw, a, dim3(blocks), c->tstream);
    HIP_TRY(c, hipGetLastError());
    return GROOT_OK;
}

// traversal records -> (read, ord) order: exclusive scan of the per-read counts, then two scatters into the slot's output
static int launch_order_stage(groot_ctx *c, Slot *s, bool update_weights)
{
    WorkSet *w = &c->ws[s->set];
    const uint32_t n = s->n_reads;
    size_t tmp_bytes = 0;
    // split reads: their items' counts become the read's count, every item learns where its records go in the read's run
    if (c->vcap) hipLaunchKernelGGL(split_fix_kernel, dim3(256), dim3(kBlock), 0, c->tstream, w->split_list.p, w->vcount.p, w->vitem.p, w->trav_cnt.p, n, s->d_ctr.p,
                                    w->trav_first.p, w->mask_first.p, c->pw, s->first_read_id);
    HIP_TRY(c, rocprim::exclusive_scan(nullptr, tmp_bytes, w->trav_cnt.p, c->trav_off.p, 0u, n, rocprim::plus<uint32_t>(), c->tstream));
    if (tmp_bytes > c->scan_tmp.n) {
        HIP_TRY(c, hipStreamSynchronize(c->tstream));
        HIP_TRY(c, c->scan_tmp.alloc(tmp_bytes + tmp_bytes / 4));
    }
    HIP_TRY(c, rocprim::exclusive_scan(c->scan_tmp.p, tmp_bytes, w->trav_cnt.p, c->trav_off.p, 0u, n, rocprim::plus<uint32_t>(), c->tstream));
    // (the batch's record count, n_trav: one thread of order_first_kernel writes it)
    OrderTabArgs ot{};
    if (c->dix.out_tab) {
        ot.tab_idx = w->tab_idx.p; ot.out_tab = c->dix.out_tab; ot.stride_q = c->dix.out_stride_q; ot.first_read_id = s->first_read_id;
        ot.update_weights = update_weights ? 1 : 0;
        ot.attempts = c->attempts_ptr; ot.q_row = c->q_row.p;
        ot.q_tab = c->dix.w - c->k + 1; ot.n_windows = c->n_windows;
    }
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[9], c->tstream));
    hipLaunchKernelGGL(order_first_kernel, dim3(std::min<uint32_t>((n + kBlock - 1) / kBlock, 2048u)), dim3(kBlock), 0, c->tstream, w->trav_first.p,
                       w->mask_first.p, c->trav_off.p, w->trav_cnt.p, n, s->d_trav.p, s->d_mask.p, s->trav_cap, c->pw,
                       c->pw_view, s->d_ctr.p, ot);
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[10], c->tstream));
    if (c->vcap) hipLaunchKernelGGL(order_split_kernel, dim3(std::min<uint32_t>((c->vcap + kBlock - 1) / kBlock, 256u)), dim3(kBlock), 0, c->tstream, w->vitem.p, w->vcount.p, c->vcap, w->trav_cnt.p,
                                    c->trav_off.p, w->trav_first.p, w->mask_first.p, n, s->first_read_id, s->d_trav.p, s->d_mask.p, s->trav_cap, c->pw, c->pw_view, s->d_ctr.p);
    hipLaunchKernelGGL(order_ovf_kernel, dim3((c->ovf_cap + kBlock - 1) / kBlock, kOvfShards), dim3(kBlock), 0, c->tstream,
                       w->ovf_trav.p, w->ovf_mask.p, w->ovf_cnt.p, c->ovf_cap, c->trav_off.p, s->first_read_id, s->d_trav.p,
                       s->d_mask.p, s->trav_cap, c->pw, c->pw_view, s->d_ctr.p, w->vitem.p, n, w->vcount.p);
    HIP_TRY(c, hipGetLastError());
    // assignment (groot_hip_assign_enable): the records are complete and nothing has read them yet -- the compact copy-out below, the packed
    // records, the counters and groot_hip_read_travs all see what it leaves.  It runs once per pass on freshly written records, never twice
    // on the same ones: the filter is not idempotent.
    if (int rc = counters_assign(c, s)) return rc;
    if (!c->prm.results_on_device) {
        // compact path sets for the copy-out (kernels.hpp): words per traversal, their exclusive scan, the copy
        const dim3 g((s->trav_cap + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(mask_words_kernel, g, dim3(kBlock), 0, c->tstream, s->d_trav.p, s->d_ctr.p, s->trav_cap, c->graph_words.p, (uint32_t)c->h_graph_words.size(),
                           s->d_mwords.p);
        size_t tb = 0;
        HIP_TRY(c, rocprim::exclusive_scan(nullptr, tb, s->d_mwords.p, s->d_moff.p, 0u, s->trav_cap, rocprim::plus<uint32_t>(), c->tstream));
        if (tb > c->scan_tmp.n) {
            HIP_TRY(c, hipStreamSynchronize(c->tstream));
            HIP_TRY(c, c->scan_tmp.alloc(tb + tb / 4));
        }
        HIP_TRY(c, rocprim::exclusive_scan(c->scan_tmp.p, tb, s->d_mwords.p, s->d_moff.p, 0u, s->trav_cap, rocprim::plus<uint32_t>(), c->tstream));
        hipLaunchKernelGGL(mask_compact_kernel, g, dim3(kBlock), 0, c->tstream, s->d_trav.p, s->d_mask.p, c->pw_view, s->d_ctr.p, s->trav_cap,
                           c->graph_words.p, (uint32_t)c->h_graph_words.size(), s->d_moff.p, s->d_cmask.p, s->d_ckpt.p);
        if (c->packed_travs) hipLaunchKernelGGL(trav_pack_kernel, g, dim3(kBlock), 0, c->tstream, s->d_trav.p, s->d_ctr.p, s->trav_cap, s->first_read_id, s->d_ctrav.p);
        HIP_TRY(c, hipGetLastError());
    }
    return GROOT_OK;
}


// sketch+seed -> schedule (compute stream) | align -> order (align stream) for the batch of slot s
static int run_batch_async(groot_ctx *c, Slot *s, bool update_weights)
{
    WorkSet *w = &c->ws[s->set];
    // compute stream: the seed stage, once the batch that used this work set last is through its order stage
    if (w->used) HIP_TRY(c, hipStreamWaitEvent(c->stream, w->ev_free, 0));
    HIP_TRY(c, hipMemsetAsync(s->d_ctr.p, 0, sizeof(DeviceCounters), c->stream));
    if (c->kn.poison) {
        // GROOT_TEST_POISON: what the seed stage writes per read is wiped first.  A work set keeps the values of the batch that used it last, and a
        // stream of equal batches hides a read that no kernel of the seed stage handled -- round 4's one-in-a-million signature kernel dropped a
        // dozen reads per 10 M from the list of the full-width pass, visible only in the first batch through each work set (tools/first_use_check.py)
        const size_t n = s->n_reads;
        HIP_TRY(c, hipMemsetAsync(w->seed_count.p, 0, n * sizeof(uint32_t), c->stream));
        HIP_TRY(c, hipMemsetAsync(w->read_rec.p, 0, n * sizeof(ReadRec), c->stream));
        HIP_TRY(c, hipMemsetAsync(w->trav_cnt.p, 0, n * sizeof(uint32_t), c->stream));
        HIP_TRY(c, hipMemsetAsync(c->sort_key.p, 0xFF, n * sizeof(uint32_t), c->stream));
        if (w->tab_idx.p) HIP_TRY(c, hipMemsetAsync(w->tab_idx.p, 0xFF, n * sizeof(uint32_t), c->stream));
        HIP_TRY(c, hipMemsetAsync(c->todo_list.p, 0, n * sizeof(uint32_t), c->stream));
    }
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[1], c->stream));
    if (int rc = launch_seed_stage(c, s, update_weights)) return rc;
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[3], c->stream));
    HIP_TRY(c, hipEventRecord(s->ev_seed, c->stream));
    // (the order sort's scratch is cleared for the next batch here: behind the last iteration and behind the event the walk stream waits for, so the
    // fill runs beside the first pass and not between two kernels of the chain)
    if (int rc = clear_order_sort(c)) return rc;
    // walk + tail streams: graph walk and ordering, beside the seed stage of the next batch.  The stage starts on the walk stream when a first
    // pass runs for this batch (launch_align_stage moves to the tail stream behind it), on the tail stream otherwise.
    s->lean_used = c->lean && !c->tab_capture && s->n_reads && s->max_len <= kLeanMaxLen && c->dfs_frac >= 0.02;
    s->path_used = c->path && !c->tab_capture && s->n_reads && s->max_len <= kLeanMaxLen && c->dfs_frac >= 0.02;
    hipStream_t start = s->lean_used || s->path_used ? c->astream : c->tstream;
    HIP_TRY(c, hipStreamWaitEvent(start, s->ev_seed, 0));
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[11], start));
    if (int rc = launch_align_stage(c, s, update_weights)) return rc;
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[4], c->tstream));
    if (int rc = launch_order_stage(c, s, update_weights)) return rc;
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[5], c->tstream));
    HIP_TRY(c, hipEventRecord(w->ev_free, c->tstream));
    if (int rc = counters_launch(c, s)) return rc;   // (reads the slot's records and read offsets and the ctx's own buffers only: the next batch's seed stage need not wait for it)
    w->used = true;
    w->owner = s;
    w->ticket = s->ticket;
    return GROOT_OK;
}

// lengths on the wire -> u64 offsets in HBM
struct LenToU64 {
    __host__ __device__ uint64_t operator()(uint16_t v) const { return (uint64_t)v; }
};

constexpr uint64_t kExcAtHomeBytes = 2u << 20;

static void par_copy(void *dst, const void *src, size_t bytes)
{
    const size_t kMin = 8u << 20;
    unsigned nt = (unsigned)std::min<size_t>(8, bytes / kMin);
    if (nt <= 1) { memcpy(dst, src, bytes); return; }
    std::vector<std::thread> th;
    const size_t per = ((bytes + nt - 1) / nt + 63) & ~(size_t)63;
    for (unsigned t = 0; t < nt; t++) {
        const size_t lo = std::min(bytes, t * per), hi = std::min(bytes, lo + per);
        if (lo < hi) th.emplace_back([=]() { memcpy((char *)dst + lo, (const char *)src + lo, hi - lo); });
    }
    for (auto &x : th) x.join();
}

// input staging + output buffers of a slot, sized once for the ctx's batch capacity
int groot::ensure_slot(groot_ctx *c, Slot *s, Slot::Input in, uint64_t n_exc)
{
    const uint32_t R = c->prm.max_batch_reads;
    const uint64_t B = c->prm.max_batch_bases;
    if (!s->d_ctr.p) {
        HIP_TRY(c, s->d_ctr.alloc(1));
        HIP_TRY(c, s->h_ctr.alloc(1));
        // (GROOT_TEST_SMALL_BUFFERS: start with buffers that every batch outgrows, so that the tests walk the grow-and-redo paths)
        const bool tiny = c->kn.small_buffers;
        if (int rc = alloc_trav(c, s, tiny ? 64u : std::max<uint32_t>(1024, R + R / 4))) return rc;
    }
    if (in == Slot::IN_DEVICE) return GROOT_OK;
    HIP_TRY(c, s->d_seq.reserve(B + 64));
    HIP_TRY(c, s->d_off.reserve((size_t)R + 1));
    if (in == Slot::IN_ASCII) {
        HIP_TRY(c, s->h_bases.reserve(B + 64));
        HIP_TRY(c, s->h_off.reserve((size_t)R + 1));
        return GROOT_OK;
    }
    HIP_TRY(c, s->h_bases.reserve((B + 3) / 4 + 64));
    HIP_TRY(c, s->d_packed.reserve((B + 15) / 16 + 1));
    if (in == Slot::IN_PACKED) HIP_TRY(c, s->h_off.reserve((size_t)R + 1));
    else {
        HIP_TRY(c, s->h_len.reserve(R));
        HIP_TRY(c, s->d_len.reserve(R));
    }
    const uint64_t exc_cap = std::max<uint64_t>(n_exc + n_exc / 4, std::max<uint64_t>(4096, B / 256));
    if (s->h_exc_pos.n < std::max<uint64_t>(n_exc, 1)) {
        HIP_TRY(c, s->h_exc_pos.alloc(exc_cap)); HIP_TRY(c, s->h_exc_byte.alloc(exc_cap));
        HIP_TRY(c, s->d_exc_pos.alloc(exc_cap)); HIP_TRY(c, s->d_exc_byte.alloc(exc_cap));
    }
    return GROOT_OK;
}

void groot::release_slot(groot_ctx *c, Slot *s)
{
    s->state = Slot::FREE;
    s->host_results = false;
    if (c->waited == s) c->waited = nullptr;
}

static Slot *free_slot(groot_ctx *c)
{
    if (c->waited) release_slot(c, c->waited);      // one-batch-at-a-time callers never release explicitly
    for (auto &s : c->slots)
        if (s->state == Slot::FREE) return s.get();
    return nullptr;
}


// copy-in, decode, kernels, counter copy-out of slot s: everything asynchronous
int groot::enqueue(groot_ctx *c, Slot *s)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = install_background(c, false)) return rc;
    s->status = GROOT_OK; s->status_msg.clear();
    s->n_trav = 0; s->host_results = false;
    memset(&s->counts, 0, sizeof s->counts);
    memset(&s->ms, 0, sizeof s->ms);
    s->ticket = c->next_ticket++;
    s->lean_used = s->path_used = false; s->path_reads = 0;   // (an empty batch runs no stage: not what the slot's last batch left)
    s->ct.assigned = c->ct.asg_on;                            // (likewise, and for a batch that fails ahead of the order stage)
    s->ct.rr.on = c->ct.rr.on; s->ct.rr.n = 0;                 // (rescued records: an empty batch has none)
    s->ct.gr.on = c->ct.gr.on; s->ct.gr.n = 0;                 // (gapped records likewise)
    if (s->n_reads == 0) {      // nothing to run: completes at once
        memset(s->h_ctr.p, 0, sizeof(DeviceCounters));
        HIP_TRY(c, hipEventRecord(s->ev_ctr, c->d2h_stream));
        s->state = Slot::IN_FLIGHT;
        c->inflight.push_back(s);
        return GROOT_OK;
    }
    if (s->input != Slot::IN_DEVICE) {
        hipStream_t h = c->h2d_stream;
        // One copy-in at a time: the caller waits here for the copy-in of the batch before.  (Every copy queued on a stream is given an SDMA
        // engine when it is submitted and waits THERE for the copy before it; the copy-out of a finished batch then lands behind such a
        // waiting copy-in and takes 11-15 ms instead of 3.5.  A host-fed stream ran at 1 950 Mreads/s with three batches in flight, 1 600
        // with four, 1 250 with five; with this wait it runs at 1 900-1 950 whatever the depth.  Reading the staging from a kernel instead
        // of the copy engine was tried as well: its 64-byte read requests crowd the link's upstream direction and the copy-out halves.)
        if (c->h2d_last) HIP_TRY(c, hipEventSynchronize(c->h2d_last));
        c->h2d_last = s->ev_h2d;
        if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev_h2d0, h));
        if (s->input == Slot::IN_ASCII) {
            HIP_TRY(c, hipMemcpyAsync(s->d_seq.p, s->h_bases.p, s->n_bases, hipMemcpyHostToDevice, h));
            HIP_TRY(c, hipMemcpyAsync(s->d_off.p, s->h_off.p, ((size_t)s->n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h));
        } else {
            HIP_TRY(c, hipMemcpyAsync(s->d_packed.p, s->h_bases.p, (size_t)((s->n_bases + 3) / 4), hipMemcpyHostToDevice, h));
            if (s->input == Slot::IN_PACKED)
                HIP_TRY(c, hipMemcpyAsync(s->d_off.p, s->h_off.p, ((size_t)s->n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h));
            else if (!s->uniform_len)
                HIP_TRY(c, hipMemcpyAsync(s->d_len.p, s->h_len.p, (size_t)s->n_reads * sizeof(uint16_t), hipMemcpyHostToDevice, h));
            // A short exception list stays at home: patch_reads_kernel reads it through the pinned mapping.  (Copies of that size are done by
            // blit kernels, and the two of them kept the copy-in stream busy for 0.5 ms between one batch's bases and the next batch's: a
            // tenth of the batch period of a host-fed stream.)
            s->exc_at_home = s->n_exc * 9 <= kExcAtHomeBytes;
            if (s->n_exc && !s->exc_at_home) {
                HIP_TRY(c, hipMemcpyAsync(s->d_exc_pos.p, s->h_exc_pos.p, s->n_exc * sizeof(uint64_t), hipMemcpyHostToDevice, h));
                HIP_TRY(c, hipMemcpyAsync(s->d_exc_byte.p, s->h_exc_byte.p, s->n_exc, hipMemcpyHostToDevice, h));
            }
        }
        HIP_TRY(c, hipEventRecord(s->ev_h2d, h));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, s->ev_h2d, 0));
    }
    if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev[0], c->stream));
    if (s->input == Slot::IN_PACKED || s->input == Slot::IN_PACKED16) {
        const uint64_t n_words = (s->n_bases + 15) / 16;                  // 16 bases per packed word
        if (n_words)
            hipLaunchKernelGGL(unpack_reads_kernel, dim3((unsigned)((n_words + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, s->d_packed.p,
                               n_words, reinterpret_cast<uint4 *>(s->d_seq.p));
        if (s->n_exc)
            hipLaunchKernelGGL(patch_reads_kernel, dim3((unsigned)((s->n_exc + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                               s->exc_at_home ? s->h_exc_pos.p : s->d_exc_pos.p, s->exc_at_home ? s->h_exc_byte.p : s->d_exc_byte.p, s->n_exc, s->d_seq.p);
        HIP_TRY(c, hipGetLastError());
        if (s->input == Slot::IN_PACKED16 && s->uniform_len) {
            hipLaunchKernelGGL(uniform_offsets_kernel, dim3((s->n_reads + kBlock) / kBlock), dim3(kBlock), 0, c->stream, s->d_off.p, s->n_reads,
                               s->uniform_len);
            HIP_TRY(c, hipGetLastError());
        } else if (s->input == Slot::IN_PACKED16) {
            HIP_TRY(c, hipMemsetAsync(s->d_off.p, 0, sizeof(uint64_t), c->stream));
            auto in = rocprim::make_transform_iterator(s->d_len.p, LenToU64());
            size_t tmp_bytes = 0;
            HIP_TRY(c, rocprim::inclusive_scan(nullptr, tmp_bytes, in, s->d_off.p + 1, s->n_reads, rocprim::plus<uint64_t>(), c->stream));
            if (tmp_bytes > c->in_tmp.n) {
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                HIP_TRY(c, c->in_tmp.alloc(tmp_bytes + tmp_bytes / 4));
            }
            HIP_TRY(c, rocprim::inclusive_scan(c->in_tmp.p, tmp_bytes, in, s->d_off.p + 1, s->n_reads, rocprim::plus<uint64_t>(), c->stream));
        }
    }
    s->set = c->next_set;
    c->next_set ^= 1u;
    if (int rc = run_batch_async(c, s, true)) return rc;
    HIP_TRY(c, hipEventRecord(s->ev_compute, c->tstream));
    c->last_compute = s->ev_compute;
    c->newest = s;
    // Copy-out on its own stream with no host in between.  The record count is only known on the device, and asking for it
    // would put a host round trip between the last kernel and the copy; so the copy engine is given a PREDICTED count now
    // -- records per read of the latest finished batch, plus a margin -- and collect fetches the rest in the rare batch
    // that has more.  (A device-driven copy kernel writing straight into pinned host memory gets the exact size too, but
    // its posted PCIe writes back up into the write path the other kernels share: the next batch's first memory-bound
    // kernel stalled until the copy was through.  Measured, dropped.)
    HIP_TRY(c, hipStreamWaitEvent(c->d2h_stream, s->ev_compute, 0));
    if (!c->prm.results_on_device) {
        if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev_d2h0, c->d2h_stream));
        // margin: a few standard deviations of a per-read count over n reads, at least 1 %
        const double margin = 1.0 + std::max(0.01, 4.0 / std::sqrt((double)s->n_reads + 1.0));
        const uint64_t predicted = (uint64_t)((double)s->n_reads * c->trav_per_read * margin) + 1024;
        s->copied = (uint32_t)std::min<uint64_t>(predicted, s->trav_cap);
        const double bpt = c->bytes_per_trav > 0 ? c->bytes_per_trav : 8.0 * (double)c->pw_view;
        s->copied_bytes = std::min<uint64_t>((uint64_t)((double)s->copied * bpt * margin) + 4096, (uint64_t)s->trav_cap * c->pw_view * 8);
        if (c->packed_travs) HIP_TRY(c, hipMemcpyAsync(s->h_ctrav.p, s->d_ctrav.p, (size_t)s->copied * sizeof(groot_ctrav), hipMemcpyDeviceToHost, c->d2h_stream));
        else HIP_TRY(c, hipMemcpyAsync(s->h_trav.p, s->d_trav.p, (size_t)s->copied * sizeof(groot_trav), hipMemcpyDeviceToHost, c->d2h_stream));
        HIP_TRY(c, hipMemcpyAsync(s->h_mask.p, s->d_cmask.p, (size_t)s->copied_bytes, hipMemcpyDeviceToHost, c->d2h_stream));
        HIP_TRY(c, hipMemcpyAsync(s->h_ckpt.p, s->d_ckpt.p, ((size_t)s->copied / 256 + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->d2h_stream));
        if (c->profiling) HIP_TRY(c, hipEventRecord(s->ev_d2h, c->d2h_stream));
    }
    if (int rc = counters_fetch(c, s)) return rc;   // (ahead of the counters: there when they are)
    HIP_TRY(c, hipMemcpyAsync(s->h_ctr.p, s->d_ctr.p, sizeof(DeviceCounters), hipMemcpyDeviceToHost, c->d2h_stream));
    HIP_TRY(c, hipEventRecord(s->ev_ctr, c->d2h_stream));
    s->state = Slot::IN_FLIGHT;
    c->inflight.push_back(s);
    return GROOT_OK;
}

// 12-byte records (read position | flags, node, offset) -> groot_trav: the graph is the node's, ord counts the records of a read
static void expand_travs(const groot_ctx *c, Slot *s)
{
    const size_t n = s->n_trav;
    const groot_ctrav *in = s->h_ctrav.p;
    groot_trav *out = s->h_trav.p;
    const uint32_t first = s->first_read_id;
    const uint32_t *node_graph = c->h_node_graph.data();
    const uint8_t *mapq = s->ct.assigned ? s->ct.h_mapq.p : nullptr;
    auto span = [=](size_t lo, size_t hi) {
        if (lo >= hi) return;
        uint32_t ord = 0, prev = ~0u;
        if (lo) {                                          // records of the same read before this span
            prev = in[lo - 1].read_flags & 0x00FFFFFFu;
            if ((in[lo].read_flags & 0x00FFFFFFu) == prev) {
                size_t j = lo;
                while (j > 0 && (in[j - 1].read_flags & 0x00FFFFFFu) == prev) j--;
                ord = (uint32_t)(lo - j) - 1;              // ord of the record at lo - 1
            }
        }
        for (size_t i = lo; i < hi; i++) {
            const uint32_t pos = in[i].read_flags & 0x00FFFFFFu;
            ord = pos == prev ? ord + 1 : 0;
            prev = pos;
            groot_trav t;
            t.read_id = first + pos; t.graph_id = node_graph[in[i].node]; t.node = in[i].node; t.offset = in[i].offset;
            t.ord = (uint16_t)ord; t.flags = (uint8_t)(in[i].read_flags >> 24);
            t.reserved = mapq && (t.flags & GROOT_TRAV_MAPQ) ? mapq[pos] : (uint8_t)0;   // (the 12-byte record carries the flag, the read's MAPQ travels beside it)
            out[i] = t;
        }
    };
    const unsigned nt = (unsigned)std::min<size_t>(std::min(16u, granted_cpus()), n / (1u << 18));   // (memory bound: 2-3 ms per 10 M records)
    if (nt <= 1) { span(0, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) th.emplace_back(span, std::min(n, t * per), std::min(n, (t + 1) * per));
    for (auto &x : th) x.join();
}

// The counters of slot s have arrived: grow-and-redo on overflow, then start the copy-out of its traversal records.
static int finish_counters(groot_ctx *c, Slot *s)
{
    DeviceCounters &h = *s->h_ctr.p;
    auto refetch = [&](DeviceCounters &dst) -> int {
        HIP_TRY(c, hipMemcpyAsync(s->h_ctr.p, s->d_ctr.p, sizeof(DeviceCounters), hipMemcpyDeviceToHost, c->tstream));
        HIP_TRY(c, hipStreamSynchronize(c->tstream));
        dst = *s->h_ctr.p;
        return GROOT_OK;
    };
    DeviceCounters first = h;
    bool have_first = false;              // weights + read counters already taken from an earlier pass
    bool redone = false;
    for (int attempt = 0; s->n_reads; attempt++) {
        const uint32_t fl = h.flags;
        if (!(fl & (kFlagSeedOverflow | kFlagQOverflow | kFlagOvfOverflow | kFlagTravOverflow))) break;
        if (attempt > 8) return fail(c, GROOT_E_NOSPACE, "output buffers keep overflowing (flags=0x%x)", fl);
        // Later batches may already have run through the shared work buffers: let them finish, grow, and redo this
        // batch as a whole.  A pass whose align stage did nothing (seed slots / table rows ran out) is simply repeated;
        // after any other overflow the weights and read counters of the first pass stand and only records are re-made.
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->astream));
        HIP_TRY(c, hipStreamSynchronize(c->tstream));
        bool redo_weights = !have_first;
        if (fl & (kFlagSeedOverflow | kFlagQOverflow)) {
            if (fl & kFlagSeedOverflow) { if (int rc = alloc_seed_slots(c, h.max_seeds + 4)) return rc; }
            if (fl & kFlagQOverflow) {
                if (c->att_external) {
                    s->status = GROOT_E_NOSPACE;
                    s->status_msg = "a kmerCount outside the fixed layout of groot_hip_attempts_layout occurred";
                    h.n_trav = 0;
                    break;
                }
                if (int rc = grow_attempts(c, std::max(h.q_rows, c->att_cap * 2))) return rc;
            }
        } else {
            if (!have_first) { first = h; have_first = true; }
            redo_weights = false;
            if (fl & kFlagOvfOverflow) { if (int rc = alloc_ovf(c, c->ovf_cap * 4)) return rc; }
            if (fl & kFlagTravOverflow) { if (int rc = alloc_trav(c, s, h.n_trav + h.n_trav / 8 + 1024)) return rc; }
        }
        if (int rc = run_batch_async(c, s, redo_weights)) return rc;
        redone = true;
        DeviceCounters again{};
        if (int rc = refetch(again)) return rc;
        if (have_first) {
            const uint32_t keep = first.flags & ~(kFlagOvfOverflow | kFlagTravOverflow | kFlagSeedOverflow | kFlagQOverflow);
            DeviceCounters merged = first;
            merged.n_trav = again.n_trav; merged.alignments = again.alignments; merged.seeds = again.seeds; merged.max_seeds = again.max_seeds;
            merged.flags = keep | again.flags;
            merged.q_rows = again.q_rows;
            merged.mask_words = again.mask_words;
            merged.todo_reads = again.todo_reads; merged.tab_reads = again.tab_reads; merged.lean_reads = again.lean_reads; merged.path_reads = again.path_reads;
            h = merged;
        } else h = again;
    }
    s->n_trav = s->n_reads ? h.n_trav : 0;
    if (int rc = counters_collect(c, s, redone)) return rc;
    groot_counts &o = s->counts;
    o.received = s->n_reads;              // boss.go:194 receivedReads++ for every read
    o.mapped = h.mapped; o.multimapped = h.multimapped; o.alignments = h.alignments; o.seeds = h.seeds;
    o.travs = s->n_trav; o.revcomp_panics = h.revcomp_panics; o.short_reads = h.short_reads;
    o.full_sketch_reads = (s->sig_used || s->text_used) ? h.todo_reads : s->n_reads;
    o.walked_reads = h.seeded_reads;
    o.lean_reads = h.lean_reads;
    s->path_reads = s->path_used ? h.path_reads : 0;
    if (s->status == GROOT_OK) {
        char buf[256];
        if (h.flags & kFlagLongRead) { s->status = GROOT_E_NOSPACE; snprintf(buf, sizeof buf, "a read is longer than max_read_len=%u", c->prm.max_read_len); s->status_msg = buf; }
        else if (h.flags & kFlagOrdOverflow) { s->status = GROOT_E_NOSPACE; s->status_msg = "a read produced more than 65535 traversals"; }
        else if (h.flags & kFlagShortRead) {
            s->status = GROOT_E_SHORT_READ;
            snprintf(buf, sizeof buf, "k size is greater than sequence length for %llu read(s) (the reference panics: boss.go:164-166)", h.short_reads);
            s->status_msg = buf;
        } else if (h.revcomp_panics) {
            s->status = GROOT_E_REVCOMP;
            snprintf(buf, sizeof buf, "%llu read(s) hold a byte > 'T' and reached RevComplement (the reference panics: seqio.go:126)", h.revcomp_panics);
            s->status_msg = buf;
        }
    }
#if defined(GROOT_WORK_COUNTERS) && GROOT_WORK_COUNTERS == 3
    if (h.dbg[4]) {
        fprintf(stderr, "[groot timeline] wavefronts with work %llu, rounds %llu, iterations: mean %.0f max %llu; wave duration: mean %.3f ms max %.3f ms\n", h.dbg[4], h.dbg[5],
                (double)h.dbg[0] / (double)h.dbg[4], h.dbg[1], (double)h.dbg[2] / (double)h.dbg[4] / 1e5, (double)h.dbg[3] / 1e5);
        for (unsigned long long i = 0; i < 14 && i < h.dbg[17]; i++)
            fprintf(stderr, "[groot timeline] late read %llu%s: %llu windows, %llu graphs, %llu traversals, from %llu to %llu us, %llu wave iterations, %llu steps of its own\n", h.dbg[18 + 3 * i] & 0xFFFFFFFFull,
                    (h.dbg[18 + 3 * i] >> 63) ? " (item)" : "", (h.dbg[18 + 3 * i] >> 32) & 0x7FFFFFFFull, h.dbg[20 + 3 * i] >> 56, (h.dbg[20 + 3 * i] >> 48) & 0xFFull, h.dbg[19 + 3 * i] & 0xFFFFFFFFull, h.dbg[19 + 3 * i] >> 32,
                    h.dbg[20 + 3 * i] & 0xFFFFFFFFull, (h.dbg[20 + 3 * i] >> 32) & 0xFFFFull);
        fprintf(stderr, "[groot timeline] late reads in all: %llu\n", h.dbg[17]);
        fprintf(stderr, "[groot timeline] ms summed over wavefronts: all %.1f = cooperative scans %.1f (%llu services) + fork/join %.1f + FETCH %.1f (%llu steps) + SCAN %.1f (%llu) + DFS %.1f (%llu) + rest\n",
                (double)h.dbg[2] / 1e5, (double)h.dbg[8] / 1e5, h.dbg[16], (double)h.dbg[9] / 1e5, (double)h.dbg[10] / 1e5, h.dbg[13], (double)h.dbg[11] / 1e5, h.dbg[14], (double)h.dbg[12] / 1e5, h.dbg[15]);
        for (int hh = 0; hh < 2; hh++) {
            fprintf(stderr, "[groot timeline] %s (buckets of 50 us):", hh ? "length of a wavefront's last round" : "wavefront ends after");
            for (int b = 0; b < 64; b++) fprintf(stderr, " %llu", h.dbg[64 + 64 * hh + b]);
            fprintf(stderr, "\n");
        }
    }
#elif defined(GROOT_WORK_COUNTERS) && GROOT_WORK_COUNTERS == 4
    if (h.dbg[151]) {
        const double nw = (double)h.dbg[151];
        fprintf(stderr, "[groot lean] wavefronts %llu; per wavefront: %.1f iterations (with a level-1 / level-2 / level-3-4 / walk lane: %.1f / %.1f / %.1f / %.1f); lane-steps per wavefront: %.0f / %.0f / %.0f / %.0f; staging %.2f us, loop %.2f us\n",
                h.dbg[151], (double)h.dbg[148] / nw, (double)h.dbg[140] / nw, (double)h.dbg[141] / nw, (double)h.dbg[142] / nw, (double)h.dbg[143] / nw,
                (double)h.dbg[144] / nw, (double)h.dbg[145] / nw, (double)h.dbg[146] / nw, (double)h.dbg[147] / nw, (double)h.dbg[149] / nw / 100.0, (double)h.dbg[150] / nw / 100.0);
        fprintf(stderr, "[groot lean] finished without an alignment %llu; left to align_kernel: seeds > 4: %llu, byte > T / length: %llu, byte other than ACGT: %llu, window with an N: %llu, node with an N: %llu, N ahead: %llu, three neighbours: %llu, third pending: %llu, too many steps: %llu\n",
                h.dbg[160], h.dbg[161], h.dbg[163], h.dbg[164], h.dbg[165], h.dbg[166], h.dbg[167], h.dbg[168], h.dbg[169], h.dbg[170]);
        if (s->path_used)
            fprintf(stderr, "[groot path] left to align_kernel: node on no path with a text %llu, event on the start base %llu, more than %u records %llu; segments ended: empty path set %llu, read's end %llu, end of the path's text %llu, flagged boundary %llu, jump %llu\n",
                    h.dbg[171], h.dbg[172], kPathHold + 1, h.dbg[173], h.dbg[176], h.dbg[177], h.dbg[178], h.dbg[179], h.dbg[180]);
    }
#elif defined(GROOT_WORK_COUNTERS)
    for (int e = 0; e < 32; e++)
        if (h.dbg[e]) fprintf(stderr, "[groot work] event %2d: wave iterations %llu lanes %llu\n", e, h.dbg[e], h.dbg[32 + e]);
    fprintf(stderr, "[groot work] longest round: %llu wave iterations\n", h.dbg[63]);
#if GROOT_WORK_COUNTERS == 2
    fprintf(stderr, "[groot work] slow reads (%llu):", h.dbg[128]);
    for (int i = 0; i < 30 && (unsigned long long)i < h.dbg[128]; i++)
        fprintf(stderr, " %llu:%llu:%llu/%llu/%llu", h.dbg[129 + 2 * i] & 0xFFFFFFFFull, h.dbg[129 + 2 * i] >> 32, h.dbg[130 + 2 * i] & 0xFFFFFull,
                (h.dbg[130 + 2 * i] >> 20) & 0xFFFFFull, h.dbg[130 + 2 * i] >> 40);
    fprintf(stderr, "\n");
#endif
    for (int i = 0; i < 5; i++) fprintf(stderr, "[groot work] FETCH part %d: %.1f ms summed over wavefronts\n", i, (double)h.dbg[40 + i] / 1e5);
    for (int ph = 0; ph < 3; ph++)
        fprintf(stderr, "[groot work] phase %d: %llu steps, %.2f us per step (wall clock, per wave)\n", ph, h.dbg[27 + ph],
                h.dbg[27 + ph] ? (double)h.dbg[24 + ph] / 100.0 / (double)h.dbg[27 + ph] : 0.0);
    for (int hh = 0; hh < 2; hh++) {
        fprintf(stderr, "[groot work] %s (buckets of 2 iterations):", hh ? "round length" : "lane finish");
        for (int b = 0; b < 64; b++) fprintf(stderr, " %llu", h.dbg[64 + 64 * hh + b]);
        fprintf(stderr, "\n");
    }
#endif
    // the records were copied out by copy_out_kernel right behind the kernels; after a redo they are fetched again here
    if (s->n_reads) c->trav_per_read = (double)s->n_trav / (double)s->n_reads;
    if (s->n_reads && !c->tab_capture) c->dfs_frac = (double)h.seeded_reads / (double)s->n_reads;
    if (s->n_reads && !c->tab_capture && (s->lean_used || s->path_used)) {
        const uint32_t first = s->path_used ? h.path_reads : h.lean_reads;
        c->lean_left_frac = (double)(h.seeded_reads - std::min(h.seeded_reads, first)) / (double)s->n_reads;
    }
    if (s->n_reads && (s->sig_used || s->text_used)) c->todo_frac = (double)h.todo_reads / (double)s->n_reads;
    if (s->n_reads) { c->lsh_frac = (double)h.lsh_reads / (double)s->n_reads; c->long_frac = (double)h.long_reads / (double)s->n_reads; }
    if (s->n_reads && !c->tab_capture && c->dix.text_tab) {
        c->text_hit_frac = s->text_used ? 1.0 - (double)h.todo_reads / (double)s->n_reads : (double)h.tab_reads / (double)s->n_reads;
        // (a batch that tried the lookup in vain sent all its reads through the list pass: on a stream the memo cannot answer --
        // mixed read lengths, another organism -- the next try comes later and later)
        if (s->text_used) c->text_retry_gap = c->text_hit_frac >= 0.7 ? 8u : std::min(256u, c->text_retry_gap * 2u);
    }
    s->n_mask_bytes = s->n_trav ? h.mask_words : 0;
    if (!c->prm.results_on_device && s->n_trav) {
        c->bytes_per_trav = (double)s->n_mask_bytes / (double)s->n_trav;
        const uint32_t have = redone ? 0 : std::min(s->copied, s->n_trav);      // a redo re-made the records: fetch them all
        if (have < s->n_trav) {
            if (c->packed_travs) HIP_TRY(c, hipMemcpy(s->h_ctrav.p + have, s->d_ctrav.p + have, (size_t)(s->n_trav - have) * sizeof(groot_ctrav), hipMemcpyDeviceToHost));
            else HIP_TRY(c, hipMemcpy(s->h_trav.p + have, s->d_trav.p + have, (size_t)(s->n_trav - have) * sizeof(groot_trav), hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(s->h_ckpt.p, s->d_ckpt.p, ((size_t)s->n_trav / 256 + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        const uint64_t have_w = redone ? 0 : std::min<uint64_t>(s->copied_bytes, s->n_mask_bytes);
        if (have_w < s->n_mask_bytes)
            HIP_TRY(c, hipMemcpy(s->h_mask.p + have_w, s->d_cmask.p + have_w, (size_t)(s->n_mask_bytes - have_w), hipMemcpyDeviceToHost));
        if (c->packed_travs) expand_travs(c, s);
        s->host_results = true;
    }
    s->state = Slot::D2H_ISSUED;
    return GROOT_OK;
}

// Move batches whose counters have arrived on to their copy-out, in submission order: blocking up to and including
// `must`, opportunistically (event query) beyond it or when must is null.
static int progress(groot_ctx *c, Slot *must = nullptr)
{
    bool blocking = must != nullptr;
    for (Slot *s : c->inflight) {
        if (s->state == Slot::IN_FLIGHT) {
            if (blocking) HIP_TRY(c, hipEventSynchronize(s->ev_ctr));
            else {
                const hipError_t q = hipEventQuery(s->ev_ctr);
                if (q == hipErrorNotReady) break;
                if (q != hipSuccess) return fail(c, GROOT_E_DEVICE, "hipEventQuery: %s", hipGetErrorString(q));
            }
            if (int rc = finish_counters(c, s)) return rc;
        }
        if (s == must) blocking = false;
    }
    return GROOT_OK;
}

int groot::collect_impl(groot_ctx *c, Slot **out)
{
    if (c->inflight.empty()) return fail(c, GROOT_E_STATE, "no batch submitted");
    HIP_TRY(c, hipSetDevice(c->device));
    Slot *s = c->inflight.front();
    if (s->state == Slot::IN_FLIGHT) {       // waits for the batch's counters, which travel behind its records
        if (int rc = progress(c, s)) return rc;
    }
    if (c->profiling && s->n_reads) {
        if (s->input != Slot::IN_DEVICE) (void)hipEventElapsedTime(&s->ms.h2d, s->ev_h2d0, s->ev_h2d);
        (void)hipEventElapsedTime(&s->ms.unpack, s->ev[0], s->ev[1]);
        (void)hipEventElapsedTime(&s->ms.sketch_seed, s->ev[1], s->ev[2]);
        (void)hipEventElapsedTime(&s->ms.schedule, s->ev[2], s->ev[3]);
        (void)hipEventElapsedTime(&s->ms.align, s->ev[11], s->ev[4]);
        (void)hipEventElapsedTime(&s->ms.sort, s->ev[4], s->ev[5]);
        (void)hipEventElapsedTime(&s->ms.total, s->ev[0], s->ev[5]);
        (void)hipEventElapsedTime(&s->ms.first_seed_kernel, s->ev[7], s->ev[8]);
        (void)hipEventElapsedTime(&s->ms.order_kernel, s->ev[9], s->ev[10]);
        (void)hipEventElapsedTime(&s->ms.list_pass, s->ev[8], s->ev[12]);
        s->ms.lean_pass = 0; s->path_ms = 0;
        if (s->lean_used) (void)hipEventElapsedTime(&s->ms.lean_pass, s->ev[11], s->ev[13]);
        if (s->path_used) (void)hipEventElapsedTime(&s->path_ms, s->ev[11], s->ev[13]);
        (void)hipEventElapsedTime(&s->ms.wall, s->ev[1], s->ev[5]);
        if (!c->prm.results_on_device) (void)hipEventElapsedTime(&s->ms.d2h, s->ev_d2h0, s->ev_d2h);
    }
    c->inflight.pop_front();
    s->state = Slot::COLLECTED;
    *out = s;
    (void)progress(c);       // keep the copy-outs of the batches behind it going
    return GROOT_OK;
}

// a free slot for a batch of n_reads (the submit calls; the capture batches of open.hip)
int groot::take_slot(groot_ctx *c, uint32_t n_reads, Slot **out)
{
    if (n_reads > c->prm.max_batch_reads) return fail(c, GROOT_E_NOSPACE, "batch of %u reads exceeds max_batch_reads=%u", n_reads, c->prm.max_batch_reads);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = progress(c)) return rc;
    Slot *s = free_slot(c);
    if (!s) return fail(c, GROOT_E_STATE, "pipeline full: %u batches submitted and not released (groot_hip_collect + groot_hip_release first)", c->prm.pipeline_depth);
    *out = s;
    return GROOT_OK;
}

namespace groot {

int drain(groot_ctx *c)     // everything submitted has finished on the device (results stay collectable)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->inflight.empty()) { if (int rc = progress(c, c->inflight.back())) return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->astream));
    HIP_TRY(c, hipStreamSynchronize(c->tstream));
    HIP_TRY(c, hipStreamSynchronize(c->d2h_stream));
    return GROOT_OK;
}

bool idle(const groot_ctx *c)
{
    return c->inflight.empty();
}

void launch_uniform_offsets(uint64_t *off, uint32_t n, uint32_t len, hipStream_t st)
{
    hipLaunchKernelGGL(uniform_offsets_kernel, dim3(n / kBlock + 1), dim3(kBlock), 0, st, off, n, len);
}

} // namespace groot

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

void groot_params_default(groot_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->containment_threshold = 0.99;   // cmd/align.go:47
    p->max_read_len = 256;
    p->max_batch_reads = 1u << 20;
    p->max_seeds_per_read = 8;
    p->pipeline_depth = 3;
}

int groot_hip_device_count(int *n)
{
    if (!n) return GROOT_E_INVALID;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        return fail(nullptr, GROOT_E_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *n = c;
    return GROOT_OK;
}

const char *groot_hip_last_error(const groot_ctx *ctx) { return ctx ? ctx->err.c_str() : g_open_err.c_str(); }

void groot_hip_close(groot_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    ctx->bg_cancel = true;
    if (ctx->bg.joinable()) ctx->bg.join();
    if (ctx->bg_stream) { (void)hipStreamSynchronize(ctx->bg_stream); (void)hipStreamDestroy(ctx->bg_stream); }
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->astream) (void)hipStreamSynchronize(ctx->astream);
    if (ctx->tstream) (void)hipStreamSynchronize(ctx->tstream);
    if (ctx->h2d_stream) (void)hipStreamSynchronize(ctx->h2d_stream);
    if (ctx->d2h_stream) (void)hipStreamSynchronize(ctx->d2h_stream);
    for (auto &s : ctx->slots) {
        for (hipEvent_t e : {s->ev_seed, s->ev_walk, s->ev_h2d0, s->ev_h2d, s->ev_compute, s->ev_ctr, s->ev_d2h0, s->ev_d2h})
            if (e) (void)hipEventDestroy(e);
        for (auto &e : s->ev)
            if (e) (void)hipEventDestroy(e);
    }
    ctx->slots.clear();
    for (WorkSet &w : ctx->ws)
        if (w.ev_free) (void)hipEventDestroy(w.ev_free);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->astream) (void)hipStreamDestroy(ctx->astream);
    if (ctx->own_tstream) (void)hipStreamDestroy(ctx->own_tstream);
    if (ctx->h2d_stream) (void)hipStreamDestroy(ctx->h2d_stream);
    if (ctx->d2h_stream) (void)hipStreamDestroy(ctx->d2h_stream);
    delete ctx;
}

int groot_hip_set_stream(groot_ctx *c, void *hip_stream)
{
    if (!c) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "cannot change stream while a batch is in flight");
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return GROOT_OK;
}

int groot_hip_stream_join(groot_ctx *c, void *hip_stream)
{
    if (!c) return GROOT_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // batches run in submission order on the align stream: the newest batch's event covers the ones before it
    // (the newest batch's event: a slot's event is recorded anew only by a newer batch still, and a finished one makes the wait a no-op)
    if (c->last_compute) HIP_TRY(c, hipStreamWaitEvent(st, c->last_compute, 0));
    return GROOT_OK;
}

int groot_hip_redo_status(groot_ctx *c, const uint32_t **d_status, uint32_t *redo_mask)
{
    if (!c || !d_status || !redo_mask) return GROOT_E_INVALID;
    if (!c->newest) return fail(c, GROOT_E_STATE, "no batch submitted");
    *d_status = &c->newest->d_ctr.p->flags;
    *redo_mask = kFlagSeedOverflow | kFlagTravOverflow | kFlagOvfOverflow | kFlagQOverflow;    // what finish_counters grows and redoes
    return GROOT_OK;
}

int groot_hip_set_profiling(groot_ctx *c, int enable)
{
    if (!c) return GROOT_E_INVALID;
    c->profiling = enable != 0;
    return GROOT_OK;
}

// ---- submit ---------------------------------------------------------------------------------------------------------
// offsets must start at 0 and not decrease; *max_len = the longest read (branch-free pass so that it vectorises: 10 M reads per batch)
static int check_offsets(groot_ctx *c, const uint64_t *seq_off, uint32_t n_reads, uint32_t *max_len, uint32_t *min_len = nullptr)
{
    if (seq_off[0] != 0) return fail(c, GROOT_E_INVALID, "seq_off[0] must be 0");
    uint64_t longest = 0, shortest = ~0ULL, bad = 0;
    for (uint32_t i = 0; i < n_reads; i++) {
        bad |= (uint64_t)(seq_off[i + 1] < seq_off[i]);
        longest = std::max(longest, seq_off[i + 1] - seq_off[i]);
        shortest = std::min(shortest, seq_off[i + 1] - seq_off[i]);
    }
    if (bad) {
        uint32_t i = 0;
        while (seq_off[i + 1] >= seq_off[i]) i++;
        return fail(c, GROOT_E_INVALID, "seq_off not monotone at read %u", i);
    }
    if (seq_off[n_reads] > c->prm.max_batch_bases)
        return fail(c, GROOT_E_NOSPACE, "batch of %llu bases exceeds max_batch_bases=%llu", (unsigned long long)seq_off[n_reads], (unsigned long long)c->prm.max_batch_bases);
    *max_len = (uint32_t)std::min<uint64_t>(longest, 0xFFFFFFFFu);
    if (min_len) *min_len = (uint32_t)std::min<uint64_t>(shortest, 0xFFFFFFFFu);
    return GROOT_OK;
}

// (ten million lengths are 4.6 ms of one core: the batch period of a host-fed stream is 4.9 ms -- the scan is dealt over the granted cores)
static int check_lengths(groot_ctx *c, const uint16_t *len, uint32_t n_reads, uint64_t *total, uint32_t *max_len, uint32_t *min_len)
{
    struct Part { uint64_t sum = 0; uint32_t longest = 0, shortest = 0xFFFFu; char pad[48]; };
    auto scan = [len](uint32_t lo, uint32_t hi, Part *p) {
        uint64_t sum = 0;
        uint32_t longest = 0, shortest = 0xFFFFu;
        for (uint32_t i0 = lo; i0 < hi; i0 += 4096) {            // (32-bit partial sums: the inner loop vectorises)
            const uint32_t i1 = std::min(hi, i0 + 4096);
            uint32_t part = 0;
            for (uint32_t i = i0; i < i1; i++) { const uint32_t v = len[i]; part += v; longest = v > longest ? v : longest; shortest = v < shortest ? v : shortest; }
            sum += part;
        }
        p->sum = sum; p->longest = longest; p->shortest = shortest;
    };
    const unsigned nt = std::max(1u, (unsigned)std::min<size_t>(std::min(16u, granted_cpus()), n_reads >> 19));
    std::vector<Part> parts(nt);
    if (nt == 1) scan(0, n_reads, &parts[0]);
    else {
        std::vector<std::thread> th;
        const uint32_t per = (n_reads + nt - 1) / nt;
        for (unsigned t = 0; t < nt; t++) th.emplace_back(scan, std::min(n_reads, t * per), std::min(n_reads, (t + 1) * per), &parts[t]);
        for (auto &x : th) x.join();
    }
    uint64_t sum = 0;
    uint32_t longest = 0, shortest = 0xFFFFFFFFu;
    for (const Part &p : parts) { sum += p.sum; longest = std::max(longest, p.longest); shortest = std::min(shortest, p.shortest); }
    if (!n_reads) shortest = 0xFFFFFFFFu;
    *min_len = shortest;
    if (sum > c->prm.max_batch_bases)
        return fail(c, GROOT_E_NOSPACE, "batch of %llu bases exceeds max_batch_bases=%llu", (unsigned long long)sum, (unsigned long long)c->prm.max_batch_bases);
    *total = sum; *max_len = longest;
    return GROOT_OK;
}

static int check_exceptions(groot_ctx *c, const uint64_t *exc_pos, uint64_t n_exc, uint64_t total)
{
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n_exc; i++) bad |= (uint64_t)(exc_pos[i] >= total);
    if (bad) return fail(c, GROOT_E_INVALID, "an exception position lies outside the batch");
    return GROOT_OK;
}

// paired mode: a batch is whole fragments (checked by every submit before anything else is touched)
static int pairs_check(groot_ctx *c, uint32_t n_reads)
{
    if (c->ct.pairs_on && (n_reads & 1)) return fail(c, GROOT_E_INVALID, "pairing is on: a batch of %u reads is not whole fragments", n_reads);
    return GROOT_OK;
}

int groot_hip_submit(groot_ctx *c, const uint8_t *seq_concat, const uint64_t *seq_off, uint32_t n_reads, uint32_t first_read_id)
{
    if (!c) return GROOT_E_INVALID;
    if (int rc = pairs_check(c, n_reads)) return rc;
    if (n_reads && (!seq_concat || !seq_off)) return fail(c, GROOT_E_INVALID, "null read buffers");
    uint32_t max_len = 0, min_len = 0;
    if (n_reads) { if (int rc = check_offsets(c, seq_off, n_reads, &max_len, &min_len)) return rc; }
    Slot *s = nullptr;
    if (int rc = take_slot(c, n_reads, &s)) return rc;
    if (int rc = ensure_slot(c, s, Slot::IN_ASCII, 0)) return rc;
    s->input = Slot::IN_ASCII; s->n_reads = n_reads; s->first_read_id = first_read_id;
    s->mixed_len = min_len != max_len; s->one_len = n_reads && min_len == max_len;
    s->n_bases = n_reads ? seq_off[n_reads] : 0; s->n_exc = 0;
    s->max_len = std::min(max_len, c->prm.max_read_len);
    if (n_reads) {   // the caller's memory is not referenced after this call returns
        par_copy(s->h_bases.p, seq_concat, s->n_bases);
        par_copy(s->h_off.p, seq_off, ((size_t)n_reads + 1) * sizeof(uint64_t));
    }
    return enqueue(c, s);
}

int groot_hip_submit_packed(groot_ctx *c, const uint8_t *packed, const uint64_t *seq_off, uint32_t n_reads, uint32_t first_read_id,
                            const uint64_t *exc_pos, const uint8_t *exc_byte, uint64_t n_exc)
{
    if (!c) return GROOT_E_INVALID;
    if (int rc = pairs_check(c, n_reads)) return rc;
    if (n_reads && (!packed || !seq_off)) return fail(c, GROOT_E_INVALID, "null read buffers");
    if (n_exc && (!exc_pos || !exc_byte)) return fail(c, GROOT_E_INVALID, "null exception list");
    uint32_t max_len = 0, min_len = 0;
    if (n_reads) {
        if (int rc = check_offsets(c, seq_off, n_reads, &max_len, &min_len)) return rc;
        if (int rc = check_exceptions(c, exc_pos, n_exc, seq_off[n_reads])) return rc;
    }
    Slot *s = nullptr;
    if (int rc = take_slot(c, n_reads, &s)) return rc;
    if (int rc = ensure_slot(c, s, Slot::IN_PACKED, n_exc)) return rc;
    s->input = Slot::IN_PACKED; s->n_reads = n_reads; s->first_read_id = first_read_id;
    s->mixed_len = min_len != max_len; s->one_len = n_reads && min_len == max_len;
    s->n_bases = n_reads ? seq_off[n_reads] : 0; s->n_exc = n_reads ? n_exc : 0;
    s->max_len = std::min(max_len, c->prm.max_read_len);
    if (n_reads) {
        par_copy(s->h_bases.p, packed, (size_t)((s->n_bases + 3) / 4));
        par_copy(s->h_off.p, seq_off, ((size_t)n_reads + 1) * sizeof(uint64_t));
        if (n_exc) { memcpy(s->h_exc_pos.p, exc_pos, n_exc * sizeof(uint64_t)); memcpy(s->h_exc_byte.p, exc_byte, n_exc); }
    }
    return enqueue(c, s);
}

int groot_hip_submit_packed16(groot_ctx *c, const uint8_t *packed, const uint16_t *seq_len, uint32_t n_reads, uint32_t first_read_id,
                              const uint64_t *exc_pos, const uint8_t *exc_byte, uint64_t n_exc)
{
    if (!c) return GROOT_E_INVALID;
    if (int rc = pairs_check(c, n_reads)) return rc;
    if (n_reads && (!packed || !seq_len)) return fail(c, GROOT_E_INVALID, "null read buffers");
    if (n_exc && (!exc_pos || !exc_byte)) return fail(c, GROOT_E_INVALID, "null exception list");
    uint64_t total = 0;
    uint32_t max_len = 0, min_len = 0;
    if (n_reads) {
        if (int rc = check_lengths(c, seq_len, n_reads, &total, &max_len, &min_len)) return rc;
        if (int rc = check_exceptions(c, exc_pos, n_exc, total)) return rc;
    }
    Slot *s = nullptr;
    if (int rc = take_slot(c, n_reads, &s)) return rc;
    if (int rc = ensure_slot(c, s, Slot::IN_PACKED16, n_exc)) return rc;
    s->input = Slot::IN_PACKED16; s->n_reads = n_reads; s->first_read_id = first_read_id;
    s->n_bases = total; s->n_exc = n_reads ? n_exc : 0;
    s->max_len = std::min(max_len, c->prm.max_read_len);
    s->uniform_len = n_reads && min_len == max_len ? max_len : 0;
    s->mixed_len = n_reads && min_len != max_len; s->one_len = n_reads && min_len == max_len;
    if (n_reads) {
        par_copy(s->h_bases.p, packed, (size_t)((total + 3) / 4));
        if (!s->uniform_len) par_copy(s->h_len.p, seq_len, (size_t)n_reads * sizeof(uint16_t));
        if (n_exc) { memcpy(s->h_exc_pos.p, exc_pos, n_exc * sizeof(uint64_t)); memcpy(s->h_exc_byte.p, exc_byte, n_exc); }
    }
    return enqueue(c, s);
}

int groot_hip_acquire(groot_ctx *c, groot_batch_buffers *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    Slot *s = nullptr;
    if (int rc = take_slot(c, 0, &s)) return rc;
    if (int rc = ensure_slot(c, s, Slot::IN_PACKED16, 0)) return rc;
    s->state = Slot::ACQUIRED;
    s->ticket = c->next_ticket++;
    memset(out, 0, sizeof *out);
    out->ticket = s->ticket;
    out->packed = s->h_bases.p; out->seq_len = s->h_len.p; out->exc_pos = s->h_exc_pos.p; out->exc_byte = s->h_exc_byte.p;
    out->packed_cap = (c->prm.max_batch_bases + 3) / 4; out->exc_cap = s->h_exc_pos.n; out->reads_cap = c->prm.max_batch_reads;
    return GROOT_OK;
}

static Slot *slot_by_ticket(groot_ctx *c, uint64_t ticket, Slot::State st)
{
    for (auto &s : c->slots)
        if (s->ticket == ticket && s->state == st) return s.get();
    return nullptr;
}

int groot_hip_submit_acquired(groot_ctx *c, uint64_t ticket, uint32_t n_reads, uint64_t n_exc, uint32_t first_read_id)
{
    if (!c) return GROOT_E_INVALID;
    Slot *s = slot_by_ticket(c, ticket, Slot::ACQUIRED);
    if (!s) return fail(c, GROOT_E_STATE, "ticket %llu is not an acquired batch", (unsigned long long)ticket);
    if (int rc = pairs_check(c, n_reads)) return rc;     // (the batch stays acquired)
    if (n_reads > c->prm.max_batch_reads) return fail(c, GROOT_E_NOSPACE, "batch of %u reads exceeds max_batch_reads=%u", n_reads, c->prm.max_batch_reads);
    if (n_exc > s->h_exc_pos.n) return fail(c, GROOT_E_NOSPACE, "more exceptions than the acquired buffers hold");
    uint64_t total = 0;
    uint32_t max_len = 0, min_len = 0;
    if (n_reads) {
        if (int rc = check_lengths(c, s->h_len.p, n_reads, &total, &max_len, &min_len)) return rc;
        if (int rc = check_exceptions(c, s->h_exc_pos.p, n_exc, total)) return rc;
    }
    s->input = Slot::IN_PACKED16; s->n_reads = n_reads; s->first_read_id = first_read_id;
    s->n_bases = total; s->n_exc = n_reads ? n_exc : 0;
    s->max_len = std::min(max_len, c->prm.max_read_len);
    s->uniform_len = n_reads && min_len == max_len ? max_len : 0;
    s->mixed_len = n_reads && min_len != max_len; s->one_len = n_reads && min_len == max_len;
    s->state = Slot::FREE;           // enqueue re-labels it
    return enqueue(c, s);
}

int groot_hip_submit_device(groot_ctx *c, const void *d_seq, const void *d_seq_off, uint32_t n_reads, uint32_t first_read_id,
                            uint32_t max_len)
{
    if (!c) return GROOT_E_INVALID;
    if (int rc = pairs_check(c, n_reads)) return rc;
    if (n_reads && (!d_seq || !d_seq_off)) return fail(c, GROOT_E_INVALID, "null device buffers");
    if (((uintptr_t)d_seq & 15) != 0) return fail(c, GROOT_E_INVALID, "d_seq must be 16-byte aligned");
    Slot *s = nullptr;
    if (int rc = take_slot(c, n_reads, &s)) return rc;
    if (int rc = ensure_slot(c, s, Slot::IN_DEVICE, 0)) return rc;
    s->input = Slot::IN_DEVICE; s->n_reads = n_reads; s->first_read_id = first_read_id; s->n_bases = 0; s->n_exc = 0;
    s->ext_seq = (const uint8_t *)d_seq; s->ext_off = (const uint64_t *)d_seq_off;
    const bool mixed = (max_len & GROOT_MAXLEN_MIXED) != 0;     // the caller's word: the reads differ in length
    max_len &= ~GROOT_MAXLEN_MIXED;
    s->max_len = max_len ? std::min(max_len, c->prm.max_read_len) : c->prm.max_read_len;
    s->mixed_len = mixed;                  // (else unknown: the offsets are on the device)
    s->one_len = max_len != 0 && !mixed;   // (the caller's word: the longest read, taken as THE read length when choosing kernels)
    return enqueue(c, s);
}

// ---- collect --------------------------------------------------------------------------------------------------------
int groot_hip_collect(groot_ctx *c, groot_batch_result *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    Slot *s = nullptr;
    if (int rc = collect_impl(c, &s)) return rc;
    memset(out, 0, sizeof *out);
    out->ticket = s->ticket; out->first_read_id = s->first_read_id; out->n_reads = s->n_reads;
    out->counts = s->counts;
    out->n_travs = s->n_trav;
    out->travs = s->host_results ? s->h_trav.p : nullptr;
    out->masks = s->host_results ? s->h_mask.p : nullptr;
    out->mask_ckpt = s->host_results ? s->h_ckpt.p : nullptr;
    out->n_mask_bytes = s->host_results ? s->n_mask_bytes : 0;
    out->d_travs = s->d_trav.p; out->d_masks = s->d_mask.p;
    out->path_words = c->pw_view;
    out->status = s->status;
    out->ms = s->ms;
    if (s->status) return fail(c, s->status, "%s", s->status_msg.c_str());
    return GROOT_OK;
}

int groot_hip_release(groot_ctx *c, uint64_t ticket)
{
    if (!c) return GROOT_E_INVALID;
    Slot *s = slot_by_ticket(c, ticket, Slot::COLLECTED);
    if (!s) s = slot_by_ticket(c, ticket, Slot::ACQUIRED);     // an acquired batch may be abandoned
    if (!s) return fail(c, GROOT_E_STATE, "ticket %llu is not a collected batch", (unsigned long long)ticket);
    release_slot(c, s);
    return GROOT_OK;
}

int groot_hip_assign_batch(groot_ctx *c, uint64_t ticket, const uint32_t **best, const uint8_t **mapq)
{
    if (!c) return GROOT_E_INVALID;
    Slot *s = ticket ? slot_by_ticket(c, ticket, Slot::COLLECTED) : c->waited;
    if (!s) return fail(c, GROOT_E_STATE, "ticket %llu is not a collected batch", (unsigned long long)ticket);
    if (!s->ct.assigned) return fail(c, GROOT_E_STATE, "assignment was off when the batch was submitted (groot_hip_assign_enable)");
    if (best) *best = s->ct.h_best.p;
    if (mapq) *mapq = s->ct.h_mapq.p;
    return GROOT_OK;
}

int groot_hip_rescue_rec_batch(groot_ctx *c, uint64_t ticket, const groot_rescue_record **recs, uint64_t *n)
{
    if (!c || !recs || !n) return GROOT_E_INVALID;
    Slot *s = ticket ? slot_by_ticket(c, ticket, Slot::COLLECTED) : c->waited;
    if (!s) return fail(c, GROOT_E_STATE, "ticket %llu is not a collected batch", (unsigned long long)ticket);
    if (!s->ct.rr.on) return fail(c, GROOT_E_STATE, "rescued records were off when the batch was submitted (groot_hip_rescue_rec_enable)");
    *recs = s->ct.rr.n ? s->ct.rr.h_rec.p : nullptr;
    *n = s->ct.rr.n;
    return GROOT_OK;
}

int groot_hip_gap_rec_batch(groot_ctx *c, uint64_t ticket, const groot_gap_record **recs, uint64_t *n)
{
    if (!c || !recs || !n) return GROOT_E_INVALID;
    Slot *s = ticket ? slot_by_ticket(c, ticket, Slot::COLLECTED) : c->waited;
    if (!s) return fail(c, GROOT_E_STATE, "ticket %llu is not a collected batch", (unsigned long long)ticket);
    if (!s->ct.gr.on) return fail(c, GROOT_E_STATE, "gapped records were off when the batch was submitted (groot_hip_gap_rec_enable)");
    *recs = s->ct.gr.n ? s->ct.gr.h_rec.p : nullptr;
    *n = s->ct.gr.n;
    return GROOT_OK;
}

int groot_hip_in_flight(groot_ctx *c, uint32_t *submitted_not_collected, uint32_t *free_slots)
{
    if (!c) return GROOT_E_INVALID;
    if (submitted_not_collected) *submitted_not_collected = (uint32_t)c->inflight.size();
    if (free_slots) {
        uint32_t n = 0;
        for (auto &s : c->slots) n += s->state == Slot::FREE || s.get() == c->waited;
        *free_slots = n;
    }
    return GROOT_OK;
}

int groot_hip_wait(groot_ctx *c, groot_counts *counts)
{
    if (!c) return GROOT_E_INVALID;
    if (c->inflight.empty()) {
        if (!c->waited) return fail(c, GROOT_E_STATE, "no batch submitted");
    } else {
        if (c->waited) release_slot(c, c->waited);
        Slot *s = nullptr;
        if (int rc = collect_impl(c, &s)) return rc;
        c->waited = s;
    }
    if (counts) *counts = c->waited->counts;
    if (c->waited->status) return fail(c, c->waited->status, "%s", c->waited->status_msg.c_str());
    return GROOT_OK;
}

int groot_hip_read_travs(groot_ctx *c, groot_trav *out, uint64_t *masks, uint64_t cap, uint64_t *n)
{
    if (!c || !n) return GROOT_E_INVALID;
    Slot *s = c->waited;
    if (!s) return fail(c, GROOT_E_STATE, "no finished batch");
    HIP_TRY(c, hipSetDevice(c->device));
    *n = s->n_trav;
    const uint64_t m = std::min<uint64_t>(cap, s->n_trav);
    if (s->host_results) {
        if (m && out) memcpy(out, s->h_trav.p, m * sizeof(groot_trav));
        if (m && masks) {        // compact path sets back to path_words words per traversal
            memset(masks, 0, m * c->pw_view * sizeof(uint64_t));
            uint64_t o = 0;
            for (uint64_t i = 0; i < m; i++) {
                const uint32_t w = c->h_graph_words[s->h_trav.p[i].graph_id];
                memcpy(masks + i * c->pw_view, s->h_mask.p + o, (size_t)w);     // (w bytes)
                o += w;
            }
        }
    } else {
        if (m && out) HIP_TRY(c, hipMemcpy(out, s->d_trav.p, m * sizeof(groot_trav), hipMemcpyDeviceToHost));
        if (m && masks) HIP_TRY(c, hipMemcpy(masks, s->d_mask.p, m * c->pw_view * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return GROOT_OK;
}

// seeds and sketches stay in the batch's work set: they are the waited batch's only until a newer batch runs through that set
static int work_buffers_of_waited(groot_ctx *c)
{
    Slot *s = c->waited;
    if (!s) return fail(c, GROOT_E_STATE, "no finished batch");
    if (s->n_reads && (c->ws[s->set].owner != s || c->ws[s->set].ticket != s->ticket))
        return fail(c, GROOT_E_STATE, "a newer batch has been submitted: the seeds / sketches of the waited batch are gone");
    return GROOT_OK;
}

int groot_hip_read_seeds(groot_ctx *c, groot_seed *out, uint64_t cap, uint64_t *n)
{
    if (!c || !n) return GROOT_E_INVALID;
    if (int rc = work_buffers_of_waited(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const Slot *s = c->waited;
    const uint32_t R = s->n_reads;
    std::vector<uint32_t> cnt(R), win((size_t)c->seed_slots * R);
    if (R) {
        HIP_TRY(c, hipMemcpy(cnt.data(), c->ws[s->set].seed_count.p, (size_t)R * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(win.data(), c->ws[s->set].seed_win.p, (size_t)c->seed_slots * R * 4, hipMemcpyDeviceToHost));   // [slot][R], R = this batch
    }
    // reads the text lookup answered have their seed windows in the outcome table, not in the seed slots
    std::vector<uint32_t> tidx;
    if (R && c->dix.out_tab && !c->h_out_tab.empty()) {
        tidx.resize(R);
        HIP_TRY(c, hipMemcpy(tidx.data(), c->ws[s->set].tab_idx.p, (size_t)R * 4, hipMemcpyDeviceToHost));
    }
    const size_t ed = (size_t)c->dix.out_stride_q * 4;       // dwords per entry
    uint64_t total = 0;
    std::vector<uint32_t> tmp;
    for (uint32_t r = 0; r < R; r++) {
        tmp.clear();
        if (!tidx.empty() && tidx[r] != kEmpty && (tidx[r] & kTabSeedsHere)) {
            const uint32_t *e0 = &c->h_out_tab[(size_t)(tidx[r] & ((1u << kOutIdxBits) - 1u)) * ed];
            const uint32_t n_ent = std::max(e0[3] >> 16, 1u) + (e0[2] >> 20);
            for (uint32_t e = 0; e < n_ent; e++)
                for (uint32_t x = 0; x < kOutSeedDw; x++)
                    if (e0[e * ed + ed - kOutSeedDw + x] != kEmpty) tmp.push_back(e0[e * ed + ed - kOutSeedDw + x]);
        } else {
            const uint32_t m = std::min(cnt[r] & 0x7FFFFFFFu, c->seed_slots);
            for (uint32_t j = 0; j < m; j++) tmp.push_back(win[(size_t)j * R + r]);
        }
        std::sort(tmp.begin(), tmp.end());
        for (uint32_t w : tmp) {
            if (out && total < cap) out[total] = groot_seed{s->first_read_id + r, w};
            total++;
        }
    }
    *n = total;
    return GROOT_OK;
}

int groot_hip_read_sketches(groot_ctx *c, uint64_t *out, uint64_t cap_reads, uint64_t *n_reads)
{
    if (!c || !n_reads) return GROOT_E_INVALID;
    if (int rc = work_buffers_of_waited(c)) return rc;
    if (!c->prm.keep_sketches) return fail(c, GROOT_E_STATE, "ctx was opened without keep_sketches");
    HIP_TRY(c, hipSetDevice(c->device));
    *n_reads = c->waited->n_reads;
    const uint64_t m = std::min<uint64_t>(cap_reads, c->waited->n_reads);
    if (m && out) HIP_TRY(c, hipMemcpy(out, c->ws[c->waited->set].sketches.p, m * c->s * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return GROOT_OK;
}

int groot_hip_stage_ms(groot_ctx *c, groot_stage_ms *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    if (c->waited) *out = c->waited->ms;
    else memset(out, 0, sizeof *out);
    return GROOT_OK;
}

int groot_hip_path_pass_stats(groot_ctx *c, uint32_t *ran, uint64_t *reads, float *ms)
{
    if (!c || !ran || !reads || !ms) return GROOT_E_INVALID;
    const Slot *s = c->waited;
    *ran = s && s->path_used ? 1u : 0u;
    *reads = *ran ? s->path_reads : 0;
    *ms = *ran ? s->path_ms : 0.0f;
    return GROOT_OK;
}

// ---- call counts ----------------------------------------------------------------------------------------------------
static int table_rows(groot_ctx *c, std::vector<uint32_t> &q_of_row)     // device sync + the current row -> kmerCount map
{
    if (int rc = drain(c)) return rc;
    uint32_t n = 0;
    HIP_TRY(c, hipMemcpy(&n, c->q_nrows.p, 4, hipMemcpyDeviceToHost));
    q_of_row.resize(n);
    if (n) HIP_TRY(c, hipMemcpy(q_of_row.data(), c->q_of_row.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return GROOT_OK;
}

int groot_hip_attempts_export(groot_ctx *c, uint32_t *q_values, uint32_t *counts, uint32_t cap_rows, uint32_t *n_rows, uint32_t *n_windows)
{
    if (!c || !n_rows) return GROOT_E_INVALID;
    std::vector<uint32_t> qs;
    if (int rc = table_rows(c, qs)) return rc;
    *n_rows = (uint32_t)qs.size();
    if (n_windows) *n_windows = c->n_windows;
    std::vector<uint32_t> order(qs.size());
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return qs[a] < qs[b]; });
    for (uint32_t i = 0; i < order.size() && i < cap_rows; i++) {
        if (q_values) q_values[i] = qs[order[i]];
        if (counts && c->n_windows)
            HIP_TRY(c, hipMemcpy(counts + (size_t)i * c->n_windows, c->attempts_ptr + (size_t)order[i] * c->n_windows, (size_t)c->n_windows * 4,
                                 hipMemcpyDeviceToHost));
    }
    return GROOT_OK;
}

int groot_hip_attempts_layout(groot_ctx *c, const uint32_t *q_values, uint32_t n_q, void *d_table)
{
    if (!c || (n_q && !q_values)) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "a batch is in flight");
    for (uint32_t i = 0; i < n_q; i++) {
        if (q_values[i] > c->max_q) return fail(c, GROOT_E_INVALID, "kmerCount %u exceeds max_read_len-k+1=%u", q_values[i], c->max_q);
        if (i && q_values[i] <= q_values[i - 1]) return fail(c, GROOT_E_INVALID, "kmerCounts must be strictly ascending");
    }
    std::vector<uint32_t> qs;
    if (int rc = table_rows(c, qs)) return rc;
    std::vector<uint32_t> new_row(qs.size());
    for (size_t r = 0; r < qs.size(); r++) {
        const uint32_t *p = std::lower_bound(q_values, q_values + n_q, qs[r]);
        if (p == q_values + n_q || *p != qs[r]) return fail(c, GROOT_E_INVALID, "the layout lacks kmerCount %u, which has counts", qs[r]);
        new_row[r] = (uint32_t)(p - q_values);
    }
    const uint32_t cap = std::max<uint32_t>(n_q, 1);
    DevBuf<uint32_t> own;
    uint32_t *dst = (uint32_t *)d_table;
    if (!dst) { HIP_TRY(c, own.alloc((size_t)cap * c->n_windows)); dst = own.p; }
    // (a caller re-laying out the buffer the table already lives in: its rows are staged first, or the memset below would wipe
    // them and the row moves could overlap)
    DevBuf<uint32_t> stage;
    const uint32_t *src = c->attempts_ptr;
    if (dst == c->attempts_ptr && !qs.empty()) {
        HIP_TRY(c, stage.alloc(qs.size() * (size_t)c->n_windows));
        HIP_TRY(c, hipMemcpy(stage.p, c->attempts_ptr, qs.size() * (size_t)c->n_windows * 4, hipMemcpyDeviceToDevice));
        src = stage.p;
    }
    if (n_q) HIP_TRY(c, hipMemset(dst, 0, (size_t)n_q * c->n_windows * 4));
    for (size_t r = 0; r < qs.size(); r++)
        HIP_TRY(c, hipMemcpy(dst + (size_t)new_row[r] * c->n_windows, src + r * c->n_windows, (size_t)c->n_windows * 4, hipMemcpyDeviceToDevice));
    std::vector<uint32_t> rowmap(c->max_q + 2, kEmpty);
    for (uint32_t i = 0; i < n_q; i++) rowmap[q_values[i]] = i;
    HIP_TRY(c, hipMemcpy(c->q_row.p, rowmap.data(), rowmap.size() * 4, hipMemcpyHostToDevice));
    if (n_q) HIP_TRY(c, hipMemcpy(c->q_of_row.p, q_values, (size_t)n_q * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->q_nrows.p, &n_q, 4, hipMemcpyHostToDevice));
    if (d_table) {
        c->attempts.release();
        c->attempts_ptr = dst; c->att_external = true; c->att_cap = n_q;
    } else {
        std::swap(c->attempts.p, own.p); std::swap(c->attempts.n, own.n);
        c->attempts_ptr = c->attempts.p; c->att_external = false; c->att_cap = cap;
    }
    return GROOT_OK;
}

int groot_hip_attempts_import(groot_ctx *c, const uint32_t *q_values, const uint32_t *counts, uint32_t n_rows)
{
    if (!c || (n_rows && (!q_values || !counts))) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "a batch is in flight");
    if (c->att_external) return fail(c, GROOT_E_STATE, "the table lives in a caller-owned buffer");
    std::vector<uint32_t> qs;
    if (int rc = table_rows(c, qs)) return rc;
    std::vector<uint32_t> all(qs);
    all.insert(all.end(), q_values, q_values + n_rows);
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    if (int rc = groot_hip_attempts_layout(c, all.data(), (uint32_t)all.size(), nullptr)) return rc;
    if (!n_rows || !c->n_windows) return GROOT_OK;
    DevBuf<uint32_t> tmp;
    HIP_TRY(c, tmp.alloc(c->n_windows));
    for (uint32_t r = 0; r < n_rows; r++) {
        const uint32_t row = (uint32_t)(std::lower_bound(all.begin(), all.end(), q_values[r]) - all.begin());
        HIP_TRY(c, hipMemcpy(tmp.p, counts + (size_t)r * c->n_windows, (size_t)c->n_windows * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(add_u32_kernel, dim3((unsigned)std::min<size_t>((c->n_windows + kBlock - 1) / kBlock, 65535)), dim3(kBlock), 0, c->stream,
                           c->attempts_ptr + (size_t)row * c->n_windows, tmp.p, (size_t)c->n_windows);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return GROOT_OK;
}

int groot_hip_attempts_device(groot_ctx *c, void **d_table, uint32_t *n_rows, uint32_t *n_windows)
{
    if (!c || !d_table) return GROOT_E_INVALID;
    std::vector<uint32_t> qs;
    if (int rc = table_rows(c, qs)) return rc;
    *d_table = c->attempts_ptr;
    if (n_rows) *n_rows = (uint32_t)qs.size();
    if (n_windows) *n_windows = c->n_windows;
    return GROOT_OK;
}

int groot_hip_attempts_reset(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    if (int rc = drain(c)) return rc;
    if (c->att_cap) HIP_TRY(c, hipMemset(c->attempts_ptr, 0, (size_t)c->att_cap * c->n_windows * sizeof(uint32_t)));
    return GROOT_OK;
}

int groot_hip_attempts_shape(groot_ctx *c, uint32_t *n_q, uint32_t *n_windows)
{
    if (!c) return GROOT_E_INVALID;
    if (n_q) *n_q = c->max_q + 1;
    if (n_windows) *n_windows = c->n_windows;
    return GROOT_OK;
}

int groot_hip_attempts_read(groot_ctx *c, uint32_t *out, uint64_t n_elems)
{
    if (!c || !out) return GROOT_E_INVALID;
    const uint64_t have = (uint64_t)(c->max_q + 1) * c->n_windows;
    if (n_elems < have) return fail(c, GROOT_E_NOSPACE, "need room for %llu counts", (unsigned long long)have);
    std::vector<uint32_t> qs;
    if (int rc = table_rows(c, qs)) return rc;
    memset(out, 0, have * sizeof(uint32_t));
    for (size_t r = 0; r < qs.size(); r++)
        if (c->n_windows)
            HIP_TRY(c, hipMemcpy(out + (size_t)qs[r] * c->n_windows, c->attempts_ptr + r * c->n_windows, (size_t)c->n_windows * 4, hipMemcpyDeviceToHost));
    return GROOT_OK;
}

// ---- the one exchange of a multi-GPU run ----------------------------------------------------------------------------
namespace {
// RCCL is loaded on first use: a single-GPU run never touches it
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool load()
    {
        if (lib) return true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) return false;
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        AllReduce = (decltype(AllReduce))dlsym(lib, "ncclAllReduce");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        return CommInitAll && CommDestroy && GroupStart && GroupEnd && AllReduce;
    }
};
Rccl g_rccl;
constexpr int kNcclUint32 = 3, kNcclSum = 0;    // ncclDataType_t / ncclRedOp_t values of rccl.h
} // namespace

int groot_hip_attempts_allreduce(groot_ctx *const *ctxs, int n_ctx)
{
    if (!ctxs || n_ctx <= 0) return GROOT_E_INVALID;
    groot_ctx *c0 = ctxs[0];
    for (int i = 0; i < n_ctx; i++) {
        if (!ctxs[i]) return GROOT_E_INVALID;
        if (ctxs[i]->n_windows != c0->n_windows || ctxs[i]->max_q != c0->max_q) return fail(c0, GROOT_E_INVALID, "ctxs were opened on different indexes / read length limits");
        if (ctxs[i]->att_external) return fail(c0, GROOT_E_STATE, "ctx %d keeps its table in a caller-owned buffer", i);
    }
    // GROOT_FORCE_RCCL=1: take the RCCL branch even when all ctxs share one device (a communicator over a single device is legal):
    // the one way to run dlopen, the symbol lookups, the enum values and the grouped in-place ncclAllReduce on a one-GPU box
    const bool force_rccl = c0->kn.force_rccl;
    if (n_ctx == 1 && !force_rccl) return drain(c0);
    // union row layout (ascending kmerCount) on every ctx
    std::vector<uint32_t> all;
    for (int i = 0; i < n_ctx; i++) {
        std::vector<uint32_t> qs;
        if (int rc = table_rows(ctxs[i], qs)) return fail(c0, rc, "%s", ctxs[i]->err.c_str());
        all.insert(all.end(), qs.begin(), qs.end());
    }
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    for (int i = 0; i < n_ctx; i++) {
        HIP_TRY(c0, hipSetDevice(ctxs[i]->device));
        if (int rc = groot_hip_attempts_layout(ctxs[i], all.data(), (uint32_t)all.size(), nullptr)) return fail(c0, rc, "%s", ctxs[i]->err.c_str());
    }
    const size_t count = all.size() * (size_t)c0->n_windows;
    if (!count) return GROOT_OK;
    // ctxs sharing a device (tests; several ctxs per GPU): fold them into the first ctx of that device with a kernel
    std::vector<int> lead;                       // one ctx index per distinct device
    for (int i = 0; i < n_ctx; i++) {
        int l = -1;
        for (int j : lead) if (ctxs[j]->device == ctxs[i]->device) l = j;
        if (l < 0) { lead.push_back(i); continue; }
        HIP_TRY(c0, hipSetDevice(ctxs[i]->device));
        hipLaunchKernelGGL(add_u32_kernel, dim3((unsigned)std::min<size_t>((count + kBlock - 1) / kBlock, 65535)), dim3(kBlock), 0, ctxs[l]->stream,
                           ctxs[l]->attempts_ptr, ctxs[i]->attempts_ptr, count);
        HIP_TRY(c0, hipGetLastError());
        HIP_TRY(c0, hipStreamSynchronize(ctxs[l]->stream));
    }
    if (lead.size() > 1 || force_rccl) {
        // one RCCL communicator over the distinct devices, one in-place ncclAllReduce(sum, uint32) per device: ring over xGMI
        if (!g_rccl.load()) return fail(c0, GROOT_E_DEVICE, "librccl.so could not be loaded: %s", dlerror());
        std::vector<int> devs;
        for (int j : lead) devs.push_back(ctxs[j]->device);
        std::vector<void *> comms(lead.size(), nullptr);
        int nrc = g_rccl.CommInitAll(comms.data(), (int)devs.size(), devs.data());
        if (nrc) return fail(c0, GROOT_E_DEVICE, "ncclCommInitAll: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(nrc) : "error");
        nrc = g_rccl.GroupStart();
        for (size_t j = 0; j < lead.size() && !nrc; j++) {
            groot_ctx *c = ctxs[lead[j]];
            (void)hipSetDevice(c->device);
            nrc = g_rccl.AllReduce(c->attempts_ptr, c->attempts_ptr, count, kNcclUint32, kNcclSum, comms[j], c->stream);
        }
        const int erc = g_rccl.GroupEnd();
        if (!nrc) nrc = erc;
        for (size_t j = 0; j < lead.size(); j++) {
            (void)hipSetDevice(ctxs[lead[j]]->device);
            (void)hipStreamSynchronize(ctxs[lead[j]]->stream);
        }
        for (void *cm : comms) if (cm) (void)g_rccl.CommDestroy(cm);
        if (nrc) return fail(c0, GROOT_E_DEVICE, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(nrc) : "error");
    }
    // every ctx ends up with the totals
    for (int i = 0; i < n_ctx; i++) {
        int l = -1;
        for (int j : lead) if (ctxs[j]->device == ctxs[i]->device) l = j;
        if (l == i) continue;
        HIP_TRY(c0, hipSetDevice(ctxs[i]->device));
        HIP_TRY(c0, hipMemcpy(ctxs[i]->attempts_ptr, ctxs[l]->attempts_ptr, count * 4, hipMemcpyDeviceToDevice));
    }
    return GROOT_OK;
}

int groot_hip_sketch(groot_ctx *c, const uint8_t *seq_concat, const uint64_t *seq_off, uint32_t n, uint64_t *out)
{
    if (!c || !out || (n && (!seq_concat || !seq_off))) return GROOT_E_INVALID;
    if (!idle(c)) return fail(c, GROOT_E_STATE, "a batch is in flight");
    if (!n) return GROOT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (n > c->prm.max_batch_reads) return fail(c, GROOT_E_NOSPACE, "more sequences than max_batch_reads");
    const uint64_t total = seq_off[n];
    uint32_t max_len = 0;
    for (uint32_t i = 0; i < n; i++) max_len = std::max<uint32_t>(max_len, (uint32_t)(seq_off[i + 1] - seq_off[i]));
    DevBuf<uint64_t> sk, off;
    DevBuf<uint8_t> seq;
    DevBuf<DeviceCounters> ctr;
    HIP_TRY(c, sk.alloc((size_t)n * c->s));
    HIP_TRY(c, off.alloc((size_t)n + 1));
    HIP_TRY(c, seq.alloc(total + 64));
    HIP_TRY(c, ctr.alloc(1));
    HIP_TRY(c, hipMemcpyAsync(seq.p, seq_concat, total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(off.p, seq_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(ctr.p, 0, sizeof(DeviceCounters), c->stream));
    SeedArgs a{};
    a.ix = c->dix;
    a.ix.max_q = 0;   // no lookup: every read gets min_eq = S+1
    a.seq = seq.p; a.seq_off = off.p; a.n_reads = n; a.max_read_len = c->prm.max_read_len;
    a.lds_read_bytes = (uint32_t)std::min<uint64_t>((uint64_t)kBlock * std::min(max_len, c->prm.max_read_len) + 32, kMaxLdsReadBytes);
    a.seed_slots = c->seed_slots; a.seed_count = c->ws[0].seed_count.p; a.seed_win = c->ws[0].seed_win.p;
    a.sketch_out = sk.p; a.sort_key = nullptr; a.read_rec = nullptr; a.q_seen = nullptr; a.ctr = ctr.p; a.shards = c->seed_shards.p;
    launch_seed(c->s, c->max_k, a, true, dim3((n + kBlock - 1) / kBlock), kLdsReads + ((a.lds_read_bytes + 15) & ~15u), c->stream);
    HIP_TRY(c, hipGetLastError());
    DeviceCounters h{};
    HIP_TRY(c, hipMemcpyAsync(&h, ctr.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out, sk.p, (size_t)n * c->s * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->ws[0].owner = nullptr;      // its seed slots were used as scratch
    if (h.flags & kFlagShortRead) return fail(c, GROOT_E_SHORT_READ, "k size is greater than sequence length");
    if (h.flags & kFlagLongRead) return fail(c, GROOT_E_NOSPACE, "a sequence is longer than max_read_len=%u", c->prm.max_read_len);
    return GROOT_OK;
}

} // extern "C"
