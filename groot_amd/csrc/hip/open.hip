// open.hip -- groot_hip_open*: a new ctx's streams and slots, the device tables (built on the host by index_tables.hpp, uploaded here), the work
// buffers, and what is built with the device's help: prefix tables, signature index, the memo (outcome table + text table), in the
// foreground or on the ctx's background thread.  One of the seven translation units of libgroot_hip.so (launch.hpp); the calls between
// this unit and the pipeline (groot_hip.hip) are open.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../common/cpus.hpp"
#include "../common/view_check.hpp"
#include "counters.hpp"
#include "ctx.hpp"
#include "index_tables.hpp"
#include "kernels_open.hpp"
#include "kernels_path.hpp"   // kPathHold
#include "launch.hpp"
#include "open.hpp"

using namespace groot;

// ---------------------------------------------------------------------------------------------
// sketch_sig_kernel's side of the index: window texts, proven against Key.Sketch, and the signature table
// ---------------------------------------------------------------------------------------------
// n WindowSize-mers of window texts (concatenated; owner[j] = their window) through the full-width kernel twice on one upload:
// sketches (compared with Key.Sketch on the device: differs[j]) and the whole seed stage (per read the record's cnt_flags word and the scheduling key without
// span bits: first seed window << 2 | dead-orientation class)
static int text_pass(groot_ctx *c, const uint8_t *seqs, const uint32_t *owner, uint32_t n, uint32_t len, uint8_t *differs, uint32_t *cnt_flags,
                     uint32_t *keys)
{
    DevBuf<uint64_t> off, sk;
    DevBuf<uint8_t> seq, bad;
    DevBuf<DeviceCounters> ctr;
    DevBuf<uint32_t> cnt, win, key, own;
    DevBuf<ReadRec> rec;
    const uint64_t total = (uint64_t)n * len;
    HIP_TRY(c, off.alloc((size_t)n + 1));
    HIP_TRY(c, sk.alloc((size_t)n * c->s));
    HIP_TRY(c, seq.alloc(total + 64));
    HIP_TRY(c, bad.alloc(n));
    HIP_TRY(c, ctr.alloc(1));
    HIP_TRY(c, cnt.alloc(n));
    HIP_TRY(c, own.alloc(n));
    // (one read of the ctx's seed slots: on the background builder's thread the caller's thread may grow them meanwhile -- finish_counters)
    const bool bg = on_background_thread();
    const uint32_t seed_slots = bg ? c->bg_seed_slots : c->seed_slots;
    HIP_TRY(c, win.alloc((size_t)seed_slots * n));
    HIP_TRY(c, key.alloc(n));
    HIP_TRY(c, rec.alloc(n));
    HIP_TRY(c, hipMemcpyAsync(seq.p, seqs, total, hipMemcpyHostToDevice, c->build_stream));
    HIP_TRY(c, hipMemcpyAsync(own.p, owner, (size_t)n * 4, hipMemcpyHostToDevice, c->build_stream));
    HIP_TRY(c, hipMemsetAsync(ctr.p, 0, sizeof(DeviceCounters), c->build_stream));
    const dim3 grid((n + kBlock - 1) / kBlock);
    launch_uniform_offsets(off.p, n, len, c->build_stream);
    SeedArgs a{};
    a.ix = *c->build_dix;
    a.seq = seq.p; a.seq_off = off.p; a.n_reads = n; a.max_read_len = std::max(len, bg ? c->bg_max_read_len : c->prm.max_read_len);
    a.lds_read_bytes = (uint32_t)std::min<uint64_t>((uint64_t)kBlock * len + 32, kMaxLdsReadBytes);
    a.seed_slots = seed_slots; a.seed_count = cnt.p; a.seed_win = win.p;
    a.ctr = ctr.p; a.shards = c->build_shards;
    const size_t lds = kLdsReads + ((a.lds_read_bytes + 15) & ~15u);
    SeedArgs d = a;                                         // sketches only: no lookup
    d.ix.max_q = 0; d.sketch_out = sk.p;
    launch_seed(c->s, c->max_k, d, true, grid, lds, c->build_stream);
    hipLaunchKernelGGL(sketch_equal_kernel, grid, dim3(kBlock), 0, c->build_stream, sk.p, own.p, c->win_sketch.p, c->s, n, bad.p);
    a.sort_key = key.p; a.sort_span_bits = 0; a.read_rec = rec.p;
    launch_seed(c->s, c->max_k, a, false, grid, lds, c->build_stream);
    HIP_TRY(c, hipGetLastError());
    std::vector<ReadRec> h(n);
    HIP_TRY(c, hipMemcpyAsync(h.data(), rec.p, (size_t)n * sizeof(ReadRec), hipMemcpyDeviceToHost, c->build_stream));
    HIP_TRY(c, hipMemcpyAsync(keys, key.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->build_stream));
    HIP_TRY(c, hipMemcpyAsync(differs, bad.p, n, hipMemcpyDeviceToHost, c->build_stream));
    HIP_TRY(c, hipStreamSynchronize(c->build_stream));
    HIP_TRY(c, hipMemsetAsync(c->build_shards, 0, (size_t)kSeedShards * kSeedShardStride * sizeof(unsigned long long), c->build_stream));
    HIP_TRY(c, hipStreamSynchronize(c->build_stream));   // (nobody folds them here)
    for (uint32_t i = 0; i < n; i++) cnt_flags[i] = h[i].cnt_flags;
    return GROOT_OK;
}

// Outcome table (DeviceIndex::out_tab, device_types.hpp OutEntry) and text table (DeviceIndex::text_tab).
// What this ctx does with a read -- which windows ContainmentIndex.Query returns, which of them get IncrementSubPath, which
// traversals AlignRead reports, in which order (lshe.go:153-175, graphminion.go:46-102, alignment.go:13-159) -- is a function of
// the read's bases alone.  So the strings real reads are most likely to BE, every WindowSize-mer of every indexed sequence path on
// both strands, go through the ctx's own pipeline once, as ordinary batches (signature kernel -> full-width kernel -> sort ->
// align_kernel -> ordering), the align stage additionally noting the windows it counted, and every string with 1..16 traversals gets
// its records stored: a memo of the pipeline's own results, nothing else.  At run time a read that equals such a string is
// answered by text_lookup_kernel (keyed by the bases) or by the signature kernel (sig_info of the window-text strings, which are
// path strings too) and never reaches the align stage.
static int build_outcome_table(groot_ctx *c, const groot_index_view *v, const std::vector<uint8_t> &text, const std::vector<uint32_t> &tlen,
                               std::vector<uint32_t> &info, uint32_t w, uint32_t vstride)
{
    const bool stats = c->kn.open_stats;
    auto t_lap = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!stats) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[groot open]     memo: %-22s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_lap).count());
        t_lap = now;
    };
    const uint32_t n = c->n_windows, pw = c->pw_view;
    const uint32_t sq = out_stride_q(pw);
    const uint32_t tw = (w + 15) / 16;
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(c->prm.max_batch_reads, 1u << 20), c->prm.max_batch_bases / w);
    if (!chunk) return GROOT_OK;
    // ---- 1. the strings: every WindowSize-mer of every path, both strands, each once ----
    // (the text table serves reads of exactly WindowSize bases whose kmerCount puts Query on the every-slot-equal branch)
    const uint32_t q_w = w - c->k + 1;
    const bool text_ok = w <= 224 && q_w < c->h_q_min_eq.size() && !c->kn.no_text_table;
    // strings with a few bytes other than ACGT (a path through an N): bases with code 0 at those positions, then the bytes and their
    // positions as the text table keeps them (device_types.hpp text_exc_dwords) -- only the text lookup can find these
    const uint32_t twk = text_key_dwords(tw);               // dwords of bases in a text-table entry (zero-padded)
    const uint32_t xw = text_ok ? text_exc_dwords(twk) : 0;
    StringSet set, xset;
    {
        uint64_t expect = 0;
        for (uint32_t p = 0; p < v->n_paths; p++) expect += v->path_len[p] >= w ? 2 * (uint64_t)(v->path_len[p] - w + 1) : 0;
        // The memo's budget (groot_params.memo_budget_mb): per string at most one outcome entry (16 * stride bytes; strings with
        // several traversals are few), one text-table entry at load factor 1/2 (128 bytes), and -- while it is built -- the string
        // set on the host (4 tw + 8 bytes).  An index whose path strings need more is opened without the memo.
        const uint64_t budget = (uint64_t)(c->prm.memo_budget_mb ? c->prm.memo_budget_mb : GROOT_MEMO_DEFAULT_MB) << 20;
        const uint64_t need = expect * ((uint64_t)sq * 16 + 128 + 4 * tw + 8);
        if (need > budget || expect >= (1ull << 30)) {
            if (stats) fprintf(stderr, "[groot open]     memo: skipped, %llu path strings need about %llu MiB (budget %llu MiB)\n", (unsigned long long)expect,
                               (unsigned long long)(need >> 20), (unsigned long long)(budget >> 20));
            return GROOT_OK;
        }
        set.init(tw, (size_t)expect);
        xset.init(twk + xw, 4096);
        std::vector<uint8_t> seq, strand[2];
        std::vector<uint32_t> pk[2];
        std::vector<uint32_t> bad_before[2];                // number of bytes other than ACGT before position i
        std::vector<uint32_t> high_before[2];               // ... of bytes above 'T': RevComplement panics on such a read (seqio.go:126) -- a string holding
                                                            // one stays out of the memo (its batch status would drop the whole capture chunk with it)
        uint32_t buf[16 + 4];
        for (uint32_t g = 0; g < v->n_graphs; g++)
            for (uint32_t lp = 0; lp < v->graph_path_off[g + 1] - v->graph_path_off[g]; lp++) {
                seq.clear();
                for (uint32_t node = v->graph_node_off[g]; node < v->graph_node_off[g + 1]; node++) {   // a path visits its nodes in ascending order (graph.go:243-262)
                    if (!((v->node_mask[(size_t)node * v->path_words + (lp >> 6)] >> (lp & 63)) & 1ULL)) continue;
                    seq.insert(seq.end(), v->bases + v->node_seq_off[node], v->bases + v->node_seq_off[node + 1]);
                }
                const size_t L = seq.size();
                if (L < w) continue;
                for (int st = 0; st < 2; st++) {
                    pk[st].assign(L / 16 + tw + 3, 0);
                    bad_before[st].assign(L + 1, 0);
                    high_before[st].assign(L + 1, 0);
                    strand[st].resize(L);
                    for (size_t i = 0; i < L; i++) {
                        uint8_t b = st ? seq[L - 1 - i] : seq[i];       // (reverse strand: ACGT complemented, any other byte as it is)
                        const bool acgt = b == 'A' || b == 'C' || b == 'G' || b == 'T';
                        if (st && acgt) b = b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : 'A';
                        strand[st][i] = b;
                        bad_before[st][i + 1] = bad_before[st][i] + (acgt ? 0 : 1);
                        high_before[st][i + 1] = high_before[st][i] + (b > 'T' ? 1 : 0);
                        if (acgt) put2(pk[st].data(), i, (uint32_t)code_of(b));
                    }
                    for (size_t i = 0; i + w <= L; i++) {
                        const uint32_t nb = bad_before[st][i + w] - bad_before[st][i];
                        if (nb > 2 * xw || high_before[st][i + w] != high_before[st][i]) continue;
                        pack_at(pk[st], i, w, tw, buf);
                        if (!nb) { (void)set.find(buf, true); continue; }
                        for (uint32_t x = tw; x < twk + xw; x++) buf[x] = 0;
                        for (uint32_t x = 0, np = 0; x < w; x++)
                            if (bad_before[st][i + x + 1] != bad_before[st][i + x]) {
                                buf[twk + (np >> 1)] |= (((x + 1) << 8) | strand[st][i + x]) << (16 * (np & 1));
                                np++;
                            }
                        (void)xset.find(buf, true);
                    }
                }
            }
    }
    lap("path strings");
    const size_t NS = set.n, NX = xset.n, NT = NS + NX;     // string ids: the ACGT strings, then the ones with exceptions
    if (!NT) return GROOT_OK;
    // ---- 2. the pipeline, once per string ----
    DevBuf<uint8_t> d_seq;
    DevBuf<uint64_t> d_off;
    HIP_TRY(c, d_seq.alloc((size_t)chunk * w + 64));
    HIP_TRY(c, d_off.alloc((size_t)chunk + 1));
    std::vector<uint32_t> tab;                              // entries, sq * 4 dwords each
    std::vector<uint32_t> sinfo(NT, 0);                     // sig_info word per string (0 = not tabulated)
    std::vector<uint8_t> in_text(NT, 0);                    // ... and it may go into the text table
    std::vector<uint8_t> seqs((size_t)chunk * w);
    std::vector<uint64_t> offs((size_t)chunk + 1);
    for (uint32_t i = 0; i <= chunk; i++) offs[i] = (uint64_t)i * w;
    HIP_TRY(c, hipMemcpy(d_off.p, offs.data(), ((size_t)chunk + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    std::vector<groot_trav> travs;
    std::vector<uint64_t> masks;
    std::vector<uint32_t> icnt, iwin, nseeds, seedw;
    std::vector<size_t> big;                                // strings with more calls / seeds than the first pass keeps: second pass
    c->out_strings = NT; c->out_tabulated = c->out_entries = 0;
    int rc_all = GROOT_OK;
    c->tab_capture = true;
    static const char kBase[4] = {'A', 'C', 'T', 'G'};
    // one batch: strings ids[0..m) through the pipeline; incr_cap call-count windows and up to seed_rows seed windows kept per string
    auto run = [&](const size_t *ids, uint32_t m, uint32_t incr_cap, bool second_pass) -> int {
        {
            const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(32u, granted_cpus()), m / 4096));
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t]() {
                for (uint32_t j = (uint32_t)((uint64_t)m * t / nt); j < (uint32_t)((uint64_t)m * (t + 1) / nt); j++) {
                    const uint32_t *pwd = ids[j] < NS ? &set.words[ids[j] * tw] : &xset.words[(ids[j] - NS) * (twk + xw)];
                    uint8_t *dst = &seqs[(size_t)j * w];
                    for (uint32_t x = 0; x < w; x++) dst[x] = (uint8_t)kBase[(pwd[x >> 4] >> (2 * (x & 15))) & 3u];
                    if (ids[j] >= NS)
                        for (uint32_t np = 0; np < 2 * xw; np++) {
                            const uint32_t pair = (pwd[twk + (np >> 1)] >> (16 * (np & 1))) & 0xFFFFu;
                            if (pair) dst[(pair >> 8) - 1] = (uint8_t)pair;
                        }
                }
            });
            for (auto &x : th) x.join();
        }
        c->incr_cap = incr_cap;
        HIP_TRY(c, c->incr_cnt.reserve(m));
        HIP_TRY(c, c->incr_win.reserve((size_t)m * incr_cap));
        Slot *s = nullptr;
        if (int rc = take_slot(c, m, &s)) return rc;
        if (int rc = ensure_slot(c, s, Slot::IN_DEVICE, 0)) return rc;      // (resident input: no staging is allocated for this)
        HIP_TRY(c, hipMemcpy(d_seq.p, seqs.data(), (size_t)m * w, hipMemcpyHostToDevice));
        s->input = Slot::IN_DEVICE; s->n_reads = m; s->first_read_id = 0; s->mixed_len = false; s->one_len = true;
        s->n_bases = 0; s->n_exc = 0; s->max_len = w; s->uniform_len = 0;
        s->ext_seq = d_seq.p; s->ext_off = d_off.p;
        if (int rc = enqueue(c, s)) return rc;
        Slot *done = nullptr;
        if (int rc = collect_impl(c, &done)) return rc;
        const bool ok = done->status == GROOT_OK;
        const uint32_t nt = done->n_trav;
        const uint32_t seed_rows = second_pass ? c->seed_slots : std::min<uint32_t>(4 * kOutSeedDw, c->seed_slots);
        travs.resize(nt); masks.resize((size_t)nt * pw); icnt.resize(m); iwin.resize((size_t)m * incr_cap);
        nseeds.resize(m); seedw.resize((size_t)seed_rows * m);
        if (ok) {
            if (nt) {
                HIP_TRY(c, hipMemcpy(travs.data(), done->d_trav.p, (size_t)nt * sizeof(groot_trav), hipMemcpyDeviceToHost));
                HIP_TRY(c, hipMemcpy(masks.data(), done->d_mask.p, (size_t)nt * pw * sizeof(uint64_t), hipMemcpyDeviceToHost));
            }
            HIP_TRY(c, hipMemcpy(nseeds.data(), c->ws[done->set].seed_count.p, (size_t)m * 4, hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy2D(seedw.data(), (size_t)m * 4, c->ws[done->set].seed_win.p, (size_t)m * 4, (size_t)m * 4, seed_rows, hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(icnt.data(), c->incr_cnt.p, (size_t)m * 4, hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(iwin.data(), c->incr_win.p, (size_t)m * incr_cap * 4, hipMemcpyDeviceToHost));
        }
        release_slot(c, done);
        if (!ok) return GROOT_OK;
        size_t t0 = 0;
        for (uint32_t j = 0; j < m; j++) {                  // records come in (read, ord) order
            size_t t1 = t0;
            while (t1 < nt && travs[t1].read_id == j) t1++;
            const size_t sid = ids[j];
            const uint32_t cnt = (uint32_t)(t1 - t0), ni = icnt[j] & 0x7FFFFFFFu, nsd = nseeds[j] & 0x7FFFFFFFu;
            if (!second_pass && (ni > incr_cap || nsd > seed_rows)) { big.push_back(sid); t0 = t1; continue; }
            const size_t first = tab.size() / (sq * 4);
            // entries: one per traversal (at least one), and as many more -- without a record -- as the string's IncrementSubPath calls
            // (two per entry) and seed windows (four per entry) need: at lower containment thresholds a read brings several windows
            // of one graph and one traversal
            const bool seeds_fit = nsd <= c->seed_slots && nsd <= seed_rows;
            const uint32_t n_ent = std::max(std::max(cnt, 1u), std::max((ni + 1) / 2, seeds_fit ? (nsd + kOutSeedDw - 1) / kOutSeedDw : 0u));
            const uint32_t n_extra = n_ent - std::max(cnt, 1u);
            if (cnt <= kOutMaxTrav && ni <= incr_cap && n_extra < (1u << 12) && first + n_ent < (1u << kOutIdxBits)) {
                for (uint32_t e = 0; e < n_ent; e++) {
                    const size_t b = tab.size();
                    tab.resize(b + sq * 4, 0);
                    if (e < cnt) {
                        const groot_trav &t = travs[t0 + e];
                        tab[b] = t.node; tab[b + 1] = t.offset; tab[b + 2] = t.graph_id; tab[b + 3] = (uint32_t)t.flags;
                    } else tab[b] = kEmpty;
                    if (e == 0) tab[b + 2] = (tab[b + 2] & 0xFFFFFu) | (n_extra << 20);   // (graph ids stay below 2^20: checked at open)
                    // multimapped / mapped as the align stage counts them (boss.go:195-200): a read with seeds is mapped
                    if (e == 0) tab[b + 3] |= ((icnt[j] >> 31) ? 0x100u : 0u) | (nsd ? 0x200u : 0u) | (cnt << 16);
                    tab[b + 4] = 2 * e < ni ? iwin[(size_t)j * incr_cap + 2 * e] : kEmpty;
                    tab[b + 5] = 2 * e + 1 < ni ? iwin[(size_t)j * incr_cap + 2 * e + 1] : kEmpty;
                    uint32_t here = 0;                      // seed windows in this entry: bits 10..12 of [3]
                    for (uint32_t x = 0; x < kOutSeedDw; x++) {
                        const bool has = seeds_fit && kOutSeedDw * e + x < nsd;
                        tab[b + sq * 4 - kOutSeedDw + x] = has ? seedw[(size_t)(kOutSeedDw * e + x) * m + j] : kEmpty;
                        here += has;
                    }
                    tab[b + 3] |= here << 10;
                    for (uint32_t x = 0; x < pw; x++) {
                        tab[b + kOutHdrDw + 2 * x] = e < cnt ? (uint32_t)masks[(t0 + e) * pw + x] : 0u;
                        tab[b + kOutHdrDw + 2 * x + 1] = e < cnt ? (uint32_t)(masks[(t0 + e) * pw + x] >> 32) : 0u;
                    }
                }
                // are the IncrementSubPath calls exactly the string's seed windows, once each?  (then the signature kernel counts them itself)
                bool all_seeds = ni == nsd && ni <= 4 && ni <= c->seed_slots;
                if (all_seeds) {
                    uint32_t a4[4], b4[4];
                    for (uint32_t x = 0; x < ni; x++) { a4[x] = iwin[(size_t)j * incr_cap + x]; b4[x] = seedw[(size_t)x * m + j]; }
                    std::sort(a4, a4 + ni); std::sort(b4, b4 + ni);
                    all_seeds = std::equal(a4, a4 + ni, b4) && std::adjacent_find(a4, a4 + ni) == a4 + ni;
                }
                sinfo[sid] = kOutTab | (cnt ? std::min(cnt - 1, kOutTravLong) << kOutTravShift : kOutNoRec) | (all_seeds ? kOutAllSeeds : 0u) | (uint32_t)first;
                in_text[sid] = seeds_fit && text_ok;
                c->out_tabulated++;
            }
            t0 = t1;
        }
        return GROOT_OK;
    };
    {
        std::vector<size_t> ids(chunk);
        for (size_t s0 = 0; s0 < NT && !rc_all; s0 += chunk) {
            const uint32_t m = (uint32_t)std::min<size_t>(chunk, NT - s0);
            std::iota(ids.begin(), ids.begin() + m, s0);
            rc_all = run(ids.data(), m, kIncrCap, false);
        }
        // second pass: the few strings whose reads bring dozens of seed windows (a sequence shared by many graphs): everything kept
        const uint32_t chunk2 = std::min<uint32_t>(chunk, 4096);
        for (size_t s0 = 0; s0 < big.size() && !rc_all; s0 += chunk2)
            rc_all = run(big.data() + s0, (uint32_t)std::min<size_t>(chunk2, big.size() - s0), kIncrCapBig, true);
    }
    c->tab_capture = false;
    c->incr_cnt.release(); c->incr_win.release();
    // the capture batches counted IncrementSubPath calls and claimed rows of the call-count table: back to the state of a fresh ctx
    {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::vector<uint32_t> none(c->max_q + 2, kEmpty);
        HIP_TRY(c, hipMemcpy(c->q_row.p, none.data(), none.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemset(c->q_seen.p, 0, (size_t)(c->max_q + 2) * 4));
        HIP_TRY(c, hipMemset(c->q_nrows.p, 0, 4));
        if (c->att_cap) HIP_TRY(c, hipMemset(c->attempts_ptr, 0, (size_t)c->att_cap * c->n_windows * sizeof(uint32_t)));
        for (WorkSet &w : c->ws) w.owner = nullptr;
        c->trav_per_read = 1.25; c->bytes_per_trav = 0; c->dfs_frac = 1.0; c->todo_frac = 1.0; c->lsh_frac = -1.0; c->long_frac = -1.0;
    }
    if (rc_all) return rc_all;
    lap("pipeline on the strings");
    c->out_entries = tab.size() / (sq * 4);
    if (!c->out_entries) return GROOT_OK;
    // ---- 3. sig_info of the window-text strings (the signature kernel's way into the table): they are path strings ----
    {
        const unsigned nt = std::min(32u, granted_cpus());
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t]() {
        uint32_t buf[16];
        std::vector<uint32_t> pk;
        for (uint32_t i = t; i < n; i += nt) {                  // (the set is only read here)
            if (!tlen[i]) continue;
            for (uint32_t row = 0; row < 2; row++) {
                const uint8_t *src = &text[(size_t)i * 2 * kTextMax + row * kTextMax];
                pk.assign(tlen[i] / 16 + tw + 3, 0);
                for (uint32_t x = 0; x < tlen[i]; x++) put2(pk.data(), x, (uint32_t)code_of(src[x]));   // (text rows hold ACGT only)
                for (uint32_t o = 0; o + w <= tlen[i]; o++) {
                    pack_at(pk, o, w, tw, buf);
                    const long j = set.find(buf, false);
                    if (j >= 0 && sinfo[(size_t)j]) info[((size_t)i * 2 + row) * vstride + o] = sinfo[(size_t)j];
                }
            }
        }
        });
        for (auto &x : th) x.join();
    }
    lap("sig_info");
    tab.resize(tab.size() + 16, 0);
    HIP_TRY(c, c->out_tab.alloc(c->out_entries * sq + 4));
    HIP_TRY(c, hipMemcpy(c->out_tab.p, tab.data(), (c->out_entries * sq + 4) * sizeof(uint4), hipMemcpyHostToDevice));
    c->h_out_tab = std::move(tab);
    HIP_TRY(c, hipMemcpy(c->sig_info.p, info.data(), info.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sig_inline_off_kernel, dim3((unsigned)((c->sig.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, c->sig.p, (uint32_t)c->sig.n);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (WorkSet &w : c->ws) HIP_TRY(c, w.tab_idx.alloc(c->prm.max_batch_reads));
    HIP_TRY(c, c->tab_hist.alloc(c->n_windows));
    HIP_TRY(c, hipMemset(c->tab_hist.p, 0, (size_t)c->n_windows * sizeof(uint32_t)));
    c->dix.out_tab = c->out_tab.p;
    c->dix.out_stride_q = sq;
    // ---- 4. text table: 64-byte entries {tag, sig_info word, bases}, keyed by the bases ----
    // (at ANY containment threshold: the memo is the pipeline's own output for the string under this ctx's parameters, whichever
    // branch of Query produced its seeds)
    if (text_ok) {
        size_t ns = 0;
        for (size_t j = 0; j < NT; j++) ns += in_text[j];
        uint32_t cap = 1024;
        while (cap < 2 * ns) cap <<= 1;
        // filled on the device: the strings are uploaded as they sit in the set, every thread claims a slot for its string with a
        // compare-and-swap on the entry's sig_info word (0 = free) and writes tag and bases behind it
        DevBuf<uint32_t> d_words, d_xwords, d_info;
        for (size_t j = 0; j < NT; j++) if (!in_text[j]) sinfo[j] = 0;      // (sinfo is not needed past this point)
        HIP_TRY(c, upload(d_words, set.words.data(), NS * tw));
        HIP_TRY(c, upload(d_xwords, xset.words.data(), NX * (twk + xw)));
        HIP_TRY(c, upload(d_info, sinfo.data(), NT));
        HIP_TRY(c, c->text_tab.alloc((size_t)cap * 4));
        HIP_TRY(c, hipMemsetAsync(c->text_tab.p, 0, (size_t)cap * 64, c->stream));
        if (NS) hipLaunchKernelGGL(text_table_fill_kernel, dim3((unsigned)((NS + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, d_words.p, d_info.p, (uint32_t)NS, tw,
                                   tw, twk, reinterpret_cast<uint32_t *>(c->text_tab.p), cap - 1);
        if (NX) hipLaunchKernelGGL(text_table_fill_kernel, dim3((unsigned)((NX + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, d_xwords.p, d_info.p + NS, (uint32_t)NX, twk,
                                   twk + xw, twk, reinterpret_cast<uint32_t *>(c->text_tab.p), cap - 1);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->dix.text_tab = c->text_tab.p;
        c->dix.text_mask = cap - 1;
        c->text_entries = ns;
    }
    lap("text table");
    if (stats)
        fprintf(stderr, "[groot open]   memo: %llu of %llu distinct path strings tabulated (%llu in the second pass), %llu entries of %u bytes; text table: %llu strings in %u slots of 64 bytes\n",
                (unsigned long long)c->out_tabulated, (unsigned long long)c->out_strings, (unsigned long long)big.size(), (unsigned long long)c->out_entries, sq * 16,
                (unsigned long long)c->text_entries, c->dix.text_tab ? c->dix.text_mask + 1 : 0u);
    return GROOT_OK;
}

static int build_signature_index(groot_ctx *c, const groot_index_view *v, const std::vector<uint32_t> &sketch_class)
{
    const uint32_t n = v->n_windows, s = v->sketch_size, w = v->window_size, k = v->kmer_size;
    if (c->kn.no_sig || !sig_supported(s, v->max_k, k) || w > kTextMax || w < k || !n || n >= (1u << 24)) return GROOT_OK;   // (SigEntry::group: 24 bits)
    const bool open_stats = c->kn.open_stats;
    auto t_lap = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!open_stats) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[groot open]   sig: %-22s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_lap).count());
        t_lap = now;
    };
    // 1. the bases every window was sketched from, forward and reverse complement
    WindowTexts wt = build_window_texts(v, std::min(32u, granted_cpus()));
    std::vector<uint8_t> &text = wt.text;
    std::vector<uint32_t> &tlen = wt.tlen;
    lap("texts");
    if (c->bg_cancel) return GROOT_OK;   // (background build abandoned: nothing of it is installed)
    // 2. proof and verdicts, one pass: every WindowSize-mer of both rows must reproduce Key.Sketch through the full-width kernel
    //    (a window whose text does not is left without one: its reads take the full-width kernel), and what the full-width
    //    seed stage's epilogue says about the same strings (the reads the signature kernel confirms ARE these strings) --
    //    verdict bits and dead-orientation class, one byte each.  A text whose own bases do not come back with a seed is dropped.
    const uint32_t vstride = kTextMax - w + 1;
    std::vector<uint32_t> verdict((size_t)n * 2 * vstride + 16, 0);   // DeviceIndex::sig_info (verdict bytes first, tabulated outcomes in step 5)
    {
        const uint32_t chunk = 1u << 20;
        std::vector<uint8_t> seqs, differs;
        std::vector<uint32_t> owner, flags, keys;
        std::vector<size_t> where;
        auto flush = [&]() -> int {
            if (owner.empty()) return GROOT_OK;
            flags.resize(owner.size()); keys.resize(owner.size()); differs.resize(owner.size());
            if (int rc = text_pass(c, seqs.data(), owner.data(), (uint32_t)owner.size(), w, differs.data(), flags.data(), keys.data())) return rc;
            for (size_t j = 0; j < owner.size(); j++) {
                if (differs[j] || !(flags[j] & kRecCountMask) || keys[j] == kEmpty) { tlen[owner[j]] = 0; continue; }
                verdict[where[j]] = ((flags[j] >> 24) & 0x3Fu) | ((keys[j] & 3u) << 6);
            }
            seqs.clear(); owner.clear(); where.clear();
            return GROOT_OK;
        };
        for (uint32_t i = 0; i < n; i++) {
            if (!tlen[i]) continue;
            for (uint32_t row = 0; row < 2; row++)
                for (uint32_t o = 0; o + w <= tlen[i]; o++) {
                    const uint8_t *src = &text[(size_t)i * 2 * kTextMax + row * kTextMax + o];
                    seqs.insert(seqs.end(), src, src + w);
                    owner.push_back(i);
                    where.push_back(((size_t)i * 2 + row) * vstride + o);
                }
            if (owner.size() >= chunk)
                if (int rc = flush()) return rc;
        }
        if (int rc = flush()) return rc;
        for (uint32_t i = 0; i < n; i++)
            if (!tlen[i]) memset(&text[(size_t)i * 2 * kTextMax], 0, 2 * kTextMax);
    }
    lap("proof + verdicts");
    if (c->bg_cancel) return GROOT_OK;   // (background build abandoned: nothing of it is installed)
    // 3. where the smallest k-mer of every text row is (first occurrence), and the rows at 2 bits per base
    std::vector<uint8_t> argmin((size_t)n * 2, 0);
    {
        DevBuf<uint8_t> d_text, d_pos;
        DevBuf<uint32_t> d_len;
        HIP_TRY(c, upload(d_text, text.data(), text.size()));
        HIP_TRY(c, upload(d_len, tlen.data(), tlen.size()));
        HIP_TRY(c, d_pos.alloc((size_t)n * 2));
        hipLaunchKernelGGL(text_argmin_kernel, dim3((2 * n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->build_stream, d_text.p, d_len.p, 2 * n, k, d_pos.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(argmin.data(), d_pos.p, argmin.size(), hipMemcpyDeviceToHost, c->build_stream));
        HIP_TRY(c, hipStreamSynchronize(c->build_stream));
    }
    std::vector<uint8_t> packed((size_t)n * 2 * (kTextMax / 4) + 64, 0);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t row = 0; row < 2; row++) {
            const uint8_t *src = &text[((size_t)i * 2 + row) * kTextMax];
            uint8_t *dst = &packed[((size_t)i * 2 + row) * (kTextMax / 4)];
            for (uint32_t j = 0; j < tlen[i]; j++) dst[j >> 2] |= (uint8_t)(((src[j] >> 1) & 3u) << (2 * (j & 3)));
        }
    c->sig_disabled = 0;
    for (uint32_t i = 0; i < n; i++) c->sig_disabled += tlen[i] == 0;
    const std::vector<uint8_t> nodes = build_win_nodes(v);
    lap("argmin + packing");
    if (c->bg_cancel) return GROOT_OK;   // (background build abandoned: nothing of it is installed)
    // 4. signature index: entries grouped by signature + the directory over the distinct signatures
    const SigTables sg = build_sig_tables(v, sketch_class, tlen, argmin, verdict, nodes, vstride);
    const std::vector<SigEntry> &ent = sg.ent;
    const uint32_t cap = (uint32_t)(sg.dir.size() / 4);
    HIP_TRY(c, upload(c->sig, ent.data(), ent.size()));
    HIP_TRY(c, upload(c->sig_dir, reinterpret_cast<const uint4 *>(sg.dir.data()), (size_t)cap));
    HIP_TRY(c, upload(c->win_text, packed.data(), packed.size()));
    HIP_TRY(c, upload(c->sig_info, verdict.data(), verdict.size()));
    HIP_TRY(c, upload(c->win_nodes, nodes.data(), nodes.size(), 4));
    c->build_dix->sig_info = c->sig_info.p;
    c->build_dix->sig_verdict_stride = vstride;
    c->build_dix->win_nodes = c->win_nodes.p;
    lap("tables + uploads");
    c->build_dix->sig = c->sig.p;
    c->build_dix->sig_dir = c->sig_dir.p;
    c->build_dix->sig_mask = cap - 1;
    c->build_dix->win_text = c->win_text.p;
    // 5. outcome table: the align stage itself, once, on every string that confirms reads
    if (c->build_dix == &c->dix && c->dix.sig_info && !c->kn.no_outcome_table && c->prm.memo_budget_mb != GROOT_MEMO_OFF && !c->prm.no_exact_align && !c->prm.keep_sketches && w <= c->prm.max_read_len && v->n_graphs < (1u << 20)) {
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = build_outcome_table(c, v, text, tlen, verdict, w, vstride)) return rc;
        c->out_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        lap("outcome table");
    }
    return GROOT_OK;
}

// DeviceIndex::win_prefix: per window, which 6-mers its level-1 / level-2 start positions can spell as read bases [0, 6) and [6, 12)
// (kernels_open.hpp prefix_positions_kernel / prefix_windows_kernel; on the host this took three core-seconds for arg-annot.90)
static int build_prefix_tables(groot_ctx *c, const groot_index_view *v)
{
    if (!v->n_windows || !v->n_nodes || !v->n_bases) return GROOT_OK;      // (an index without windows: groot_hip_sketch only)
    DevBuf<uint32_t> d_seq_off, d_edge_off, pos_bits;
    HIP_TRY(c, upload(d_seq_off, v->node_seq_off, (size_t)v->n_nodes + 1));
    HIP_TRY(c, upload(d_edge_off, v->node_edge_off, (size_t)v->n_nodes + 1));
    HIP_TRY(c, c->win_prefix.alloc((size_t)v->n_windows * kPrefixWords));
    static_assert(kPrefixWords == kBlock, "a thread per word of a window's two tables");
    // a pass per run of whole graphs holding up to 2 M bases (1 KB of sets per base position): the windows of a graph only start in its
    // own nodes, and nodes and windows are stored graph by graph (else: one pass over everything)
    bool grouped = true;
    for (uint32_t w = 1; w < v->n_windows; w++) grouped &= v->win_graph[w] >= v->win_graph[w - 1];
    const uint64_t kPassBases = 2u << 20;
    uint32_t g0 = 0, w0 = 0;
    while (g0 < v->n_graphs) {
        uint32_t g1 = g0 + 1;
        const uint32_t p0 = v->node_seq_off[v->graph_node_off[g0]];
        if (!grouped) g1 = v->n_graphs;
        else while (g1 < v->n_graphs && (uint64_t)v->node_seq_off[v->graph_node_off[g1 + 1]] - p0 <= kPassBases) g1++;
        const uint32_t p1 = v->node_seq_off[v->graph_node_off[g1]];
        uint32_t w1 = w0;
        if (!grouped) w1 = v->n_windows;
        else while (w1 < v->n_windows && v->win_graph[w1] < g1) w1++;
        if (p1 > p0 && w1 > w0) {
            const size_t words = (size_t)(p1 - p0) * 256 + 256;
            HIP_TRY(c, pos_bits.reserve(words));
            HIP_TRY(c, hipMemsetAsync(pos_bits.p, 0, words * sizeof(uint32_t), c->build_stream));
            PrefixBuildArgs a{};
            a.bases = c->bases.p; a.seq_off = d_seq_off.p; a.edge_off = d_edge_off.p; a.edges = c->edges.p;
            a.n_nodes = v->n_nodes; a.p0 = p0; a.p1 = p1; a.pos_bits = pos_bits.p;
            hipLaunchKernelGGL(prefix_positions_kernel, dim3((unsigned)((2 * (uint64_t)(p1 - p0) + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->build_stream, a);
            hipLaunchKernelGGL(prefix_windows_kernel, dim3(w1 - w0), dim3(kBlock), 0, c->build_stream, c->win_rec.p, c->cn_pre.p, d_seq_off.p, pos_bits.p, p0, w0, w1, c->win_prefix.p);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(c->build_stream));
        } else if (w1 > w0) HIP_TRY(c, hipMemsetAsync(c->win_prefix.p + (size_t)w0 * kPrefixWords, 0, (size_t)(w1 - w0) * kPrefixWords * sizeof(uint32_t), c->build_stream));
        g0 = g1; w0 = w1;
    }
    HIP_TRY(c, hipStreamSynchronize(c->build_stream));
    c->build_dix->win_prefix = c->win_prefix.p;
    return GROOT_OK;
}

// what a background open has finished moves into the ctx's index description: between two batches, on the caller's thread
int groot::install_background(groot_ctx *c, bool wait)
{
    const int st0 = c->bg_state.load(std::memory_order_acquire);
    if (st0 == 0 || (st0 == 1 && !wait)) return GROOT_OK;
    if (c->bg.joinable()) c->bg.join();
    const int st = c->bg_state.load(std::memory_order_acquire);
    c->bg_state.store(0);
    c->build_dix = &c->dix; c->build_stream = c->stream; c->build_shards = c->seed_shards.p;
    if (st == 3) return fail(c, c->bg_rc ? c->bg_rc : GROOT_E_DEVICE, "background part of groot_hip_open: %s", c->bg_err.c_str());
    if (st == 4) return GROOT_OK;         // abandoned: the ctx goes on with the full-width kernels (same results)
    const DeviceIndex &b = c->bg_dix;
    c->dix.win_prefix = b.win_prefix;
    c->dix.sig = b.sig; c->dix.sig_dir = b.sig_dir; c->dix.sig_mask = b.sig_mask; c->dix.win_text = b.win_text;
    c->dix.sig_info = b.sig_info; c->dix.sig_verdict_stride = b.sig_verdict_stride; c->dix.win_nodes = b.win_nodes;
    return GROOT_OK;
}

// the ctx's five streams, the work sets' events and the pipeline's slots with theirs
static int create_streams_and_slots(groot_ctx *c)
{
    HIP_TRY(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    {
        // the align stream gets a priority of its own (the lowest): streams of different priorities never share a hardware queue -- two
        // streams on one queue run their kernels in turn, seen once as a headline of 5.3 instead of 9 Greads/s -- and the hashing
        // kernels, which are the longer stage on most workloads, get their workgroups placed first
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&c->astream, hipStreamNonBlocking, lo) != hipSuccess)
            HIP_TRY(c, hipStreamCreateWithFlags(&c->astream, hipStreamNonBlocking));
        // the tail stream, at the same priority: the tail of batch b beside the first pass of batch b+1 (GROOT_SERIAL_TAIL=1: one stream for both, as
        // before the split -- every "tail stream" below is then the walk stream)
        if (c->kn.serial_tail) c->tstream = c->astream;
        else {
            if (hipStreamCreateWithPriority(&c->own_tstream, hipStreamNonBlocking, lo) != hipSuccess)
                HIP_TRY(c, hipStreamCreateWithFlags(&c->own_tstream, hipStreamNonBlocking));
            c->tstream = c->own_tstream;
        }
    }
    for (WorkSet &w : c->ws) HIP_TRY(c, hipEventCreateWithFlags(&w.ev_free, hipEventDisableTiming));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->h2d_stream, hipStreamNonBlocking));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    c->build_dix = &c->dix; c->build_stream = c->stream;
    for (uint32_t i = 0; i < c->prm.pipeline_depth; i++) {
        std::unique_ptr<Slot> s(new Slot());
        for (hipEvent_t *e : {&s->ev_seed, &s->ev_walk, &s->ev_h2d0, &s->ev_h2d, &s->ev_compute, &s->ev_ctr, &s->ev_d2h0, &s->ev_d2h}) HIP_TRY(c, hipEventCreate(e));
        for (auto &e : s->ev) HIP_TRY(c, hipEventCreate(&e));
        c->slots.push_back(std::move(s));
    }
    return GROOT_OK;
}

// shared work buffers (inputs / outputs are per pipeline slot, allocated at their first use)
static int alloc_work_buffers(groot_ctx *c)
{
    const uint32_t R = c->prm.max_batch_reads, s = c->s;
    HIP_TRY(c, c->sort_key.alloc(R));
    HIP_TRY(c, c->sort_key_out.alloc(R));
    HIP_TRY(c, c->long_list.alloc(kLongListCap));
    HIP_TRY(c, c->long_count.alloc(4));
    HIP_TRY(c, hipMemset(c->long_count.p, 0, 4 * sizeof(uint32_t)));
    {
        std::vector<uint32_t> iota(R);
        std::iota(iota.begin(), iota.end(), 0u);
        HIP_TRY(c, upload(c->perm_in, iota.data(), iota.size()));
    }
    if (int rc = alloc_seed_slots(c, c->prm.max_seeds_per_read)) return rc;
    // (+ vcap slots behind the reads: the items of split reads, AlignArgs::vitem)
    c->vcap = c->kn.small_buffers ? 8u : std::max<uint32_t>(4096, R / 4);   // (small: most split reads find no room for their items and are handled whole)
    for (WorkSet &w : c->ws) {     // what a batch's seed stage hands to its align and order stages: two sets, taken in turn
        HIP_TRY(c, w.seed_count.alloc(R));
        HIP_TRY(c, w.read_rec.alloc(R));
        HIP_TRY(c, w.perm.alloc(R));
        HIP_TRY(c, w.perm_count.alloc(4));
        if (c->lean || c->path) {
            HIP_TRY(c, w.perm2.alloc(R));
            HIP_TRY(c, w.packed.alloc((size_t)R * (c->prm.max_read_len <= 128 ? 2 : 4)));
        }
        if (c->prm.keep_sketches) HIP_TRY(c, w.sketches.alloc((size_t)R * s));
        HIP_TRY(c, w.trav_first.alloc((size_t)R + c->vcap));
        HIP_TRY(c, w.mask_first.alloc(((size_t)R + c->vcap) * c->pw));
        HIP_TRY(c, w.trav_cnt.alloc((size_t)R + c->vcap));
        HIP_TRY(c, w.vitem.alloc(std::max<uint32_t>(c->vcap, 1)));
        HIP_TRY(c, w.split_list.alloc(kLongListCap));
        HIP_TRY(c, w.vcount.alloc(4));
        HIP_TRY(c, hipMemset(w.vcount.p, 0, 4 * sizeof(uint32_t)));
    }
    HIP_TRY(c, c->trav_off.alloc(R));
    if (c->lean || c->path) HIP_TRY(c, c->lean_stk.alloc((size_t)R * 4));
    if (c->path) HIP_TRY(c, c->path_hold.alloc((size_t)R * 3 * kPathHold));
    for (WorkSet &w : c->ws) {
        HIP_TRY(c, w.ovf_cnt.alloc(kOvfShards + 3));
        HIP_TRY(c, hipMemset(w.ovf_cnt.p, 0, (kOvfShards + 3) * sizeof(uint32_t)));
    }
    if (int rc = alloc_ovf(c, c->kn.small_buffers ? 2u : std::max<uint32_t>(256, R / kOvfShards / 4))) return rc;
    // the align kernel is persistent: exactly the workgroups that are resident at once (GROOT_ALIGN_WAVES per SIMD = per CU)
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
    c->n_cu = (uint32_t)std::max(n_cu, 1);
    uint32_t per_cu = c->pw > 3 ? kAlignWavesWide : kAlignWaves;
    // (3 or 2 workgroups of the persistent grid per CU instead of 4, so that the next batch's hashing kernels find free registers from the start: measured in
    // round 4 -- 3: no difference on any kernel-path workload, 2: mixed 8 M 1 022 -> 983, configs[2] through the kernels 1 861 -> 1 740 Mreads/s)
    c->align_threads = std::min<uint32_t>(((R + kBlock - 1) / kBlock) * kBlock, (uint32_t)std::max(n_cu, 1) * per_cu * kBlock);
    c->stk_depth = c->prm.max_read_len;
    HIP_TRY(c, c->stk_hdr.alloc((size_t)c->stk_depth * c->align_threads));
    HIP_TRY(c, c->stk_mask.alloc((size_t)c->stk_depth * c->align_threads * c->pw));
    // LSH-Forest branch of Query: the hashing kernels query in place (a lane per read) and hand the reads with more than lsh_defer_rows
    // candidate rows to lsh_heavy_kernel (a wavefront per read).  Two alternatives were built, measured slower on every workload
    // and removed in round 4 ("Removed"): a kernel dealing the rows of 64 reads over a wavefront, and a query launch of its own.
    if (c->l_max <= kLshMaxBands) {
#ifndef GROOT_LSH_DEFER_ROWS
#define GROOT_LSH_DEFER_ROWS 64    // (round 5, mixed 75..150-base reads, 8 M per batch, t = 0.99 / 0.90: 8 -> 813 / 404, 16 -> 980 / 512, 32 -> 1 120 / 618, 64 -> 1 203 / 656 Mreads/s)
#endif
        c->lsh_defer_rows = GROOT_LSH_DEFER_ROWS;
        c->lsh_cap = c->kn.small_buffers ? 4u : std::max<uint32_t>(4096, R / 4);   // (small: most heavy reads find the list full and walk their own rows)
        HIP_TRY(c, c->lsh_list.alloc(c->lsh_cap));
        HIP_TRY(c, c->lsh_count.alloc(4));
        HIP_TRY(c, hipMemset(c->lsh_count.p, 0, 4 * sizeof(uint32_t)));
        HIP_TRY(c, c->lsh_sketch.alloc((size_t)c->lsh_cap * s));
    }
    HIP_TRY(c, c->todo_list.alloc(R));
    HIP_TRY(c, c->todo_count.alloc(1));
    HIP_TRY(c, hipMemset(c->todo_count.p, 0, sizeof(uint32_t)));
    HIP_TRY(c, c->seed_shards.alloc((size_t)kSeedShards * kSeedShardStride));
    HIP_TRY(c, hipMemset(c->seed_shards.p, 0, (size_t)kSeedShards * kSeedShardStride * sizeof(unsigned long long)));
    HIP_TRY(c, hipDeviceSynchronize());
    return GROOT_OK;
}

// the LSH forest band tables, joined and uploaded before anything can take the LSH-Forest branch (once: later calls do nothing)
static int finish_lsh(groot_ctx *c, LshTables &lsh)
{
    if (lsh.job.joinable()) lsh.job.join();
    if (c->band_keys.p) return GROOT_OK;
    HIP_TRY(c, upload(c->band_keys, lsh.keys.data(), lsh.keys.size()));
    HIP_TRY(c, upload(c->band_ids, lsh.ids.data(), lsh.ids.size()));
    HIP_TRY(c, upload(c->band_hash, lsh.tab.data(), lsh.tab.size()));
    HIP_TRY(c, upload(c->band_sig, lsh.sig.data(), lsh.sig.size(), 32));
    HIP_TRY(c, upload(c->band_run, lsh.run.data(), lsh.run.size()));
    c->dix.band_keys = c->band_keys.p; c->dix.band_ids = c->band_ids.p; c->dix.band_hash = c->band_hash.p;
    c->dix.band_sig = c->band_sig.p; c->dix.band_run = c->band_run.p;
    lsh.keys = {}; lsh.ids = {}; lsh.run = {}; lsh.tab = {}; lsh.sig = {};
    return GROOT_OK;
}

// prefix tables (0.2 s on arg-annot.90) and signature index (0.4 s) on a thread of their own: the ctx takes batches at once --
// through the full-width kernel and without the seed stage's verdicts until they are there (same results)
static int start_background(groot_ctx *c, const groot_index_view *v, std::vector<uint32_t> &&sketch_class)
{
    c->bg_dix = c->dix;
    HIP_TRY(c, hipStreamCreateWithFlags(&c->bg_stream, hipStreamNonBlocking));
    HIP_TRY(c, c->bg_shards.alloc((size_t)kSeedShards * kSeedShardStride));
    HIP_TRY(c, hipMemset(c->bg_shards.p, 0, (size_t)kSeedShards * kSeedShardStride * sizeof(unsigned long long)));
    c->build_dix = &c->bg_dix; c->build_stream = c->bg_stream; c->build_shards = c->bg_shards.p;
    c->bg_seed_slots = c->seed_slots; c->bg_max_read_len = c->prm.max_read_len;
    c->bg_state.store(1);
    c->bg = std::thread([c, v, sc = std::move(sketch_class)]() {
        enter_background_thread();
        int rc = GROOT_OK;
        try {
            if (hipSetDevice(c->device) != hipSuccess) rc = fail(c, GROOT_E_DEVICE, "hipSetDevice");
            if (!rc && !c->bg_cancel) rc = build_prefix_tables(c, v);
            if (!rc && !c->bg_cancel) rc = build_signature_index(c, v, sc);
        } catch (const std::exception &e) {
            rc = fail(c, GROOT_E_NOSPACE, "%s", e.what());
        }
        c->bg_rc = rc;
        c->bg_state.store(rc ? 3 : (c->bg_cancel ? 4 : 2), std::memory_order_release);
    });
    return GROOT_OK;
}

// the device, the parameters (0 = default) and the view are usable; the ctx's scalars
static int check_and_set_params(groot_ctx *c, int device_id, const groot_index_view *v, const groot_params *p)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(c, GROOT_E_DEVICE, "no HIP device available (libgroot_hip has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(c, GROOT_E_INVALID, "device %d out of range (%d devices)", device_id, ndev);
    if (!v) return fail(c, GROOT_E_INVALID, "null index view");
    c->device = device_id;
    c->kn = Knobs::read();
    HIP_TRY(c, hipSetDevice(device_id));
    groot_params d;
    groot_params_default(&d);
    c->prm = p ? *p : d;
    if (!c->prm.max_read_len) c->prm.max_read_len = d.max_read_len;
    if (!c->prm.max_batch_reads) c->prm.max_batch_reads = d.max_batch_reads;
    if (!c->prm.max_seeds_per_read) c->prm.max_seeds_per_read = d.max_seeds_per_read;
    if (!c->prm.max_batch_bases) c->prm.max_batch_bases = (uint64_t)c->prm.max_batch_reads * c->prm.max_read_len;
    if (!c->prm.pipeline_depth) c->prm.pipeline_depth = d.pipeline_depth;
    if (c->prm.pipeline_depth > 16) return fail(c, GROOT_E_INVALID, "pipeline_depth must be <= 16");
    if (c->prm.max_read_len > 65535) return fail(c, GROOT_E_UNSUPPORTED, "max_read_len must be <= 65535");
    if (v->kmer_size == 0 || v->kmer_size > 64) return fail(c, GROOT_E_UNSUPPORTED, "k-mer size %u not in [1,64]", v->kmer_size);
    if (c->prm.max_read_len < v->kmer_size) return fail(c, GROOT_E_INVALID, "max_read_len smaller than the k-mer size");
    {   // never upload a view whose indices do not resolve (truncated / corrupt index, wrong file)
        const std::string why = check_index_view(v);
        if (!why.empty()) return fail(c, GROOT_E_FORMAT, "inconsistent index view: %s", why.c_str());
    }
    if (!seed_supported(v->sketch_size, v->max_k))
        return fail(c, GROOT_E_UNSUPPORTED, "sketch size %u with maxK %u is outside what the kernels handle (1 <= maxK <= sketch size <= %d)", v->sketch_size,
                    v->max_k, kGenericMaxS);
    c->s = v->sketch_size; c->k = v->kmer_size; c->max_k = v->max_k; c->l_max = v->sketch_size / v->max_k;
    c->pw_view = v->path_words; c->pw = round_pw(v->path_words);
    if (!c->pw) return fail(c, GROOT_E_UNSUPPORTED, "graphs with more than 704 paths are not supported (path_words=%u)", v->path_words);
    c->n_windows = v->n_windows;
    c->max_q = c->prm.max_read_len - c->k + 1;
    return GROOT_OK;
}

// call-count table: rows appear as kmerCounts do
static int alloc_call_counts(groot_ctx *c)
{
    std::vector<uint32_t> none(c->max_q + 2, kEmpty);
    HIP_TRY(c, upload(c->q_row, none.data(), none.size()));
    HIP_TRY(c, c->q_seen.alloc(c->max_q + 2));
    HIP_TRY(c, hipMemset(c->q_seen.p, 0, (size_t)(c->max_q + 2) * 4));
    HIP_TRY(c, c->q_of_row.alloc(c->max_q + 2));
    HIP_TRY(c, c->q_nrows.alloc(1));
    HIP_TRY(c, hipMemset(c->q_nrows.p, 0, 4));
    if (int rc = grow_attempts(c, std::min<uint32_t>(4, c->max_q + 1))) return rc;
    return GROOT_OK;
}

static int open_impl(groot_ctx *c, int device_id, const groot_index_view *v, const groot_params *p, uint32_t flags)
{
    // ---- 1. checks ----
    if (int rc = check_and_set_params(c, device_id, v, p)) return rc;
    const uint32_t n = v->n_windows, s = v->sketch_size;

    // ---- 2. streams and slots ----
    if (int rc = create_streams_and_slots(c)) return rc;
    const bool open_stats = c->kn.open_stats;
    auto t_open = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!open_stats) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[groot open] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_open).count());
        t_open = now;
    };
    lap("device + streams");

    // ---- 3. the index in HBM: per table build (index_tables.hpp), upload, DeviceIndex field (those without a line here: the block at the end) ----
    const unsigned nt = std::min(32u, granted_cpus());
    HIP_TRY(c, upload(c->edges, v->edges, v->n_edges));
    HIP_TRY(c, upload(c->bases, v->bases, v->n_bases, 64));   // kernels read 8-byte windows up to 24 bytes past a node start
    {
        const std::vector<unsigned char> recs = build_node_records(v, c->pw);
        HIP_TRY(c, upload(c->node_rec, recs.data(), recs.size()));
    }
    c->h_node_graph = build_node_graph(v);
    // first pass of the align stage (kernels_lean.hpp, kernels_path.hpp): texts at 2 bits per base behind 32-bit bit offsets; an index too
    // large for those goes without one (align_kernel alone: correct at any size)
    const bool first_pass = c->pw == 3 && !c->prm.no_exact_align && bit_addressable32(v->n_bases);
    c->lean = first_pass && c->kn.lean;
    c->path = first_pass && !c->kn.lean && !c->kn.no_path;
    if (c->path) {
        PathTables pt;
        c->path = build_path_tables(v, c->h_node_graph, pt);
        if (c->path) {
            HIP_TRY(c, upload(c->path_node, pt.node.data(), pt.node.size()));
            HIP_TRY(c, upload(c->path_text, pt.text.data(), pt.text.size()));
            HIP_TRY(c, upload(c->path_tag, pt.tag.data(), pt.tag.size()));
            HIP_TRY(c, upload(c->path_nodes, pt.nodes.data(), pt.nodes.size()));
            HIP_TRY(c, upload(c->path_tab, pt.tab.data(), pt.tab.size()));
            if (open_stats)
                fprintf(stderr, "[groot open] path tables: %u of %u paths with a text, %zu bases; node records %.2f MB, text + tags %.2f MB, node lists %.2f MB, sparse tables %.2f MB\n",
                        pt.n_text_paths, v->n_paths, pt.n_bases, pt.node.size() * 16 / 1e6, (pt.text.size() + pt.tag.size()) * 4 / 1e6, pt.nodes.size() * 4 / 1e6, pt.tab.size() * 8 / 1e6);
        }
    }
    if (c->lean || c->path) {
        const LeanTables lt = build_lean_tables(v);
        HIP_TRY(c, upload(c->bases2, lt.bases2.data(), lt.bases2.size()));
        HIP_TRY(c, upload(c->lean_nodes, lt.nodes.data(), lt.nodes.size()));
        HIP_TRY(c, upload(c->lean_ext, lt.ext.data(), lt.ext.size()));
        HIP_TRY(c, upload(c->cn_pre2, reinterpret_cast<const uint4 *>(lt.cn_pre2.data()), lt.cn_pre2.size() / 4));
        HIP_TRY(c, upload(c->win_ok, lt.win_ok.data(), lt.win_ok.size()));
    }
    {
        const std::vector<uint32_t> pre = build_cn_pre(v);
        HIP_TRY(c, upload(c->cn_pre, reinterpret_cast<const uint4 *>(pre.data()), pre.size() / 4));
        c->dix.cn_pre = c->cn_pre.p;
    }
    {
        const std::vector<uint64_t> sets = build_node_l2b(v, nt);
        HIP_TRY(c, upload(c->node_l2b, sets.data(), sets.size(), 2));
        c->dix.node_l2b = c->node_l2b.p;
    }
    lap("node records + prefix tables");
    HIP_TRY(c, upload(c->win_graph, v->win_graph, n));
    counters_init(c, v);
    c->packed_travs = !c->prm.results_on_device && c->prm.max_batch_reads <= (1u << 24);
    {
        const std::vector<uint32_t> end = build_graph_win_end(v);
        if (!end.empty()) {
            HIP_TRY(c, upload(c->graph_win_end, end.data(), end.size()));
            c->dix.graph_win_end = c->graph_win_end.p;
        }
    }
    c->h_graph_words = build_graph_words(v);
    HIP_TRY(c, upload(c->graph_words, c->h_graph_words.data(), c->h_graph_words.size()));
    {
        const std::vector<WinRec> wr = build_win_rec(v);
        HIP_TRY(c, upload(c->win_rec, wr.data(), wr.size()));
    }
    HIP_TRY(c, upload(c->cn_node, v->cn_node, v->n_cn));
    HIP_TRY(c, upload(c->win_sketch, v->win_sketch, (size_t)n * s, 2));
    lap("window arrays");
    // lookup structures (the reference bootstraps its LSH forests at load too, lshe.go:95-147)
    std::vector<uint32_t> sketch_class;      // smallest window id with the same 64-bit sketch
    {
        ExactTable ex = build_exact_table(v);
        HIP_TRY(c, upload(c->exact, ex.tab.data(), ex.tab.size()));
        c->dix.exact_mask = (uint32_t)ex.tab.size() - 1;
        sketch_class = std::move(ex.sketch_class);
    }
    lap("exact table");
    // the band tables are sorted on threads of their own while the main thread goes on building what the window-sized strings of the
    // signature index / memo need first (finish_lsh)
    LshTables lsh;
    start_lsh_tables(lsh, v, c->l_max, std::min(16u, granted_cpus()));
    c->band_hash_bits = lsh.hash_bits;
    lap("LSH forest tables");
    {
        const QTables qt = build_q_tables(v, c->max_q, c->l_max, c->prm.containment_threshold);
        HIP_TRY(c, upload(c->q_k, qt.k.data(), qt.k.size()));
        HIP_TRY(c, upload(c->q_l, qt.l.data(), qt.l.size()));
        HIP_TRY(c, upload(c->q_min_eq, qt.min_eq.data(), qt.min_eq.size()));
        c->h_q_min_eq = qt.min_eq;
    }
    if (int rc = alloc_call_counts(c)) return rc;
    DeviceIndex &x = c->dix;
    x.k = v->kmer_size; x.s = s; x.w = v->window_size; x.num_window_kmers = v->num_window_kmers;
    x.n_windows = n; x.n_nodes = v->n_nodes; x.pw = c->pw;
    x.edges = c->edges.p; x.bases = c->bases.p;
    x.win_prefix = c->win_prefix.p; x.win_graph = c->win_graph.p; x.win_rec = c->win_rec.p; x.cn_node = c->cn_node.p;
    x.win_sketch = c->win_sketch.p; x.exact = c->exact.p; x.band_keys = c->band_keys.p; x.band_ids = c->band_ids.p;
    x.band_hash = c->band_hash.p; x.band_hash_bits = c->band_hash_bits; x.band_sig = c->band_sig.p; x.band_run = c->band_run.p;
    x.max_k = v->max_k; x.l_max = c->l_max; x.q_k = c->q_k.p; x.q_l = c->q_l.p; x.q_min_eq = c->q_min_eq.p; x.max_q = c->max_q;
    x.q_row = c->q_row.p;
    lap("per-kmerCount tables");

    // ---- 4. work buffers ----
    if (int rc = alloc_work_buffers(c)) return rc;
    lap("work buffers");
    c->build_shards = c->seed_shards.p;

    // ---- 5. what the device helps to build: prefix tables, signature index, memo -- here and now, or on the background thread ----
    // WindowSize-mers on the every-slot-equal branch of Query never touch the LSH-Forest tables: the signature index and the memo
    // (both run window-sized strings through the kernels) are built while the band tables are still being sorted
    const uint32_t q_w = v->window_size >= v->kmer_size ? v->window_size - v->kmer_size + 1 : 0;
    const bool w_exact = q_w && q_w < c->h_q_min_eq.size() && c->h_q_min_eq[q_w] == s;
    // The memo needs the signature index and the ctx's whole pipeline: with it everything is built here and now.
    const bool memo_wanted = !c->kn.no_outcome_table && c->prm.memo_budget_mb != GROOT_MEMO_OFF && !c->prm.no_exact_align && !c->prm.keep_sketches;
    if ((flags & GROOT_OPEN_BACKGROUND) && !memo_wanted) {
        if (int rc = finish_lsh(c, lsh)) return rc;
        lap("LSH forest tables (waited for)");
        return start_background(c, v, std::move(sketch_class));
    }
    if (int rc = build_prefix_tables(c, v)) return rc;
    lap("prefix tables");
    if (!w_exact) { if (int rc = finish_lsh(c, lsh)) return rc; lap("LSH forest tables (waited for)"); }
    if (int rc = build_signature_index(c, v, sketch_class)) return rc;
    if (int rc = finish_lsh(c, lsh)) return rc;
    lap("signature index");
    return GROOT_OK;
}

extern "C" {

int groot_hip_open_stats(const groot_ctx *c, groot_open_stats *out)
{
    if (!c || !out) return GROOT_E_INVALID;
    memset(out, 0, sizeof *out);
    out->open_ms = c->open_ms; out->memo_ms = c->out_build_ms;
    out->memo_strings = c->out_strings; out->memo_tabulated = c->out_tabulated; out->memo_entries = c->out_entries; out->text_entries = c->text_entries;
    out->memo_hbm_bytes = c->out_tab.n * sizeof(uint4) + c->text_tab.n * sizeof(uint4) + c->sig_info.n * sizeof(uint32_t);
    return GROOT_OK;
}

int groot_hip_open(groot_ctx **out, int device_id, const groot_index_view *idx, const groot_params *p)
{
    return groot_hip_open_flags(out, device_id, idx, p, 0);
}

int groot_hip_open_abandon(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    if (c->bg_state.load(std::memory_order_acquire) == 1) c->bg_cancel = true;   // (a finished build is installed by the next submit as usual)
    return GROOT_OK;
}

int groot_hip_open_wait(groot_ctx *c)
{
    if (!c) return GROOT_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    return install_background(c, true);
}

int groot_hip_open_flags(groot_ctx **out, int device_id, const groot_index_view *idx, const groot_params *p, uint32_t flags)
{
    if (!out) return fail(nullptr, GROOT_E_INVALID, "null out pointer");
    *out = nullptr;
    groot_ctx *c = new groot_ctx();
    const auto t_open0 = std::chrono::steady_clock::now();
    int rc;
    try {
        rc = open_impl(c, device_id, idx, p, flags);
    } catch (const std::bad_alloc &) {      // (host tables of the index / the memo: nothing may unwind through the C boundary)
        rc = fail(c, GROOT_E_NOSPACE, "out of host memory while building the device tables");
    } catch (const std::exception &e) {
        rc = fail(c, GROOT_E_INVALID, "groot_hip_open: %s", e.what());
    }
    c->open_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_open0).count();
    if (rc) {
        (void)fail(nullptr, rc, "%s", c->err.c_str());   // (the ctx goes: groot_hip_last_error(NULL) keeps its text)
        groot_hip_close(c);
        return rc;
    }
    *out = c;
    return GROOT_OK;
}

} // extern "C"
