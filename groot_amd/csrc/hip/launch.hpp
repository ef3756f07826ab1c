// launch.hpp -- kernel dispatch by (sketch size, maxK, k) and path words.  libgroot_hip.so is built from seven translation units
// (groot_hip.hip: ctx + batch pipeline + C ABI + the small kernels; open.hip: groot_hip_open* -- device tables (index_tables.hpp), work buffers, memo -- reached through open.hpp; counters.hip: the counters behind the order stage, reached through counters.hpp; rescue.hip: the rescue family among them -- mismatch and gapped rescue, their reads in the classes and in assigned coverage, their records -- reached through rescue.hpp; seed_full.hip: the full-width hashing kernel; seed_fast.hip: signature kernel,
// text lookup, list pass; align.hip: the graph-walk kernels) so that they compile side by side; these are the calls between them.
#pragma once

#include "device_types.hpp"

namespace groot {

// K1+K2 full width (sketch_seed_kernel): any `groot index -s / -y` -- sizes without a compiled instance run the run-time-sized kernel
bool seed_supported(uint32_t s, uint32_t max_k);
void launch_seed(uint32_t s, uint32_t max_k, const SeedArgs &a, bool dump, dim3 grid, size_t lds, hipStream_t st);

// signature kernel; the list pass of the full-width kernel (behind it, or behind the text lookup); the text lookup
bool sig_supported(uint32_t s, uint32_t max_k, uint32_t k);
void launch_sig(uint32_t s, const SeedArgs &a, uint32_t max_len, hipStream_t st);
void launch_list(uint32_t s, const SeedArgs &a, dim3 list_grid, hipStream_t st);
void launch_text_lookup(uint32_t key_dwords, const SeedArgs &a, dim3 grid, size_t lds, hipStream_t st);

// K3
void launch_align(uint32_t pw, const AlignArgs &a, dim3 grid, hipStream_t st);
void launch_align_lean(uint32_t pw, const LeanArgs &a, dim3 grid, hipStream_t st);   // first pass (pw == 3 only)
void launch_align_path(uint32_t pw, const LeanArgs &a, dim3 grid, hipStream_t st);   // first pass against path text (pw == 3 only)

} // namespace groot
