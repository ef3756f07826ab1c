// open.hpp -- what the pipeline (groot_hip.hip) and groot_hip_open* (open.hip: the device tables of index_tables.hpp, streams, work
// buffers, the memo, the background builder) need of each other.
#pragma once

#include "ctx.hpp"

namespace groot {

constexpr uint32_t kMaxLdsReadBytes = 64 * 1024;   // SeedArgs::lds_read_bytes at most (launch_seed_stage; open's text_pass)

// ---- open.hip, called by groot_hip.hip ----
int install_background(groot_ctx *c, bool wait);                // enqueue (wait = false) and the calls that need the whole index: what a background open has finished moves into c->dix

// ---- groot_hip.hip, called by open.hip ----
void enter_background_thread();                                 // the ctx's background builder, first thing: fail() on this thread writes groot_ctx::bg_err from now on
bool on_background_thread();                                    // text_pass: the builder reads its own copies of the ctx's mutable state (bg_seed_slots, bg_max_read_len)
int alloc_seed_slots(groot_ctx *c, uint32_t slots);             // alloc_work_buffers: the work sets' seed windows (finish_counters grows them)
int alloc_ovf(groot_ctx *c, uint32_t cap_per_shard);            // alloc_work_buffers: the work sets' overflow lists (finish_counters grows them)
int grow_attempts(groot_ctx *c, uint32_t rows);                 // open_impl: the first rows of the call-count table (finish_counters adds rows)
int take_slot(groot_ctx *c, uint32_t n_reads, Slot **out);      // build_outcome_table: a free slot for a capture batch, as the submit calls do
int ensure_slot(groot_ctx *c, Slot *s, Slot::Input in, uint64_t n_exc);   // ... its buffers
int enqueue(groot_ctx *c, Slot *s);                             // ... the batch through the ctx's own pipeline
int collect_impl(groot_ctx *c, Slot **out);                     // ... its results, still on the device
void release_slot(groot_ctx *c, Slot *s);                       // ... and the slot is free again
void launch_uniform_offsets(uint64_t *off, uint32_t n, uint32_t len, hipStream_t st);   // text_pass: uniform_offsets_kernel (kernels_misc.hpp: one unit per __global__ function)

} // namespace groot
