// kernels_rare.hpp -- the draw without replacement behind the rarefaction curves (groot_hip_em_rarefy; the contract is in
// include/groot_host.h, "rarefaction curves").
//
// rare_draw_kernel: a thread per draw, grid = (chunks of draws, replicates x depths).  Workgroup row y = (replicate, depth d) takes the
// draws j of the depth interval [m[d-1], m[d]) (m[-1] = 0) and nothing else, so no histogram mixes two depths.  Draw j of replicate b is
// the unit pi_b(j) of the permutation in ../common/rare_perm.hpp (six Feistel rounds, walked back into [0, N)), looked up in the
// cumulative table of the EC counts exactly as boot_resample_kernel looks up its draw: cum and a u32 histogram in LDS when they fit
// (kLds), one global u64 atomic per non-zero bin at the end; otherwise cum is searched in global memory and every draw is one global
// atomic.  Only integers: the counts do not depend on the launch shape.  The lanes of a wavefront walk different lengths (below 4 on
// average, the domain being smaller than 4 N); the wavefront waits for its longest walk.
//
// rare_cumsum_kernel: the increments [replicate][depth][EC] into the cumulative rare_count, in place: a thread per (replicate, EC)
// adds along the depths.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../common/rare_perm.hpp"
#include "kernels_boot.hpp"

namespace groot {

struct RareDrawArgs {
    const uint64_t *cum;              // [n_ec + 1]
    const uint64_t *depths;           // [n_depths] ascending, 1 <= m <= total
    unsigned long long *inc;          // [replicates of this launch][n_depths][n_ec], zeroed
    uint64_t total;                   // N = cum[n_ec], 1 <= N < 2^62
    uint64_t seed;
    uint32_t n_ec;                    // > 0
    uint32_t n_depths;                // > 0
    uint32_t b0;                      // the launch's first replicate
    uint32_t half_bits;               // h
};

template <bool kLds> __global__ void __launch_bounds__(kBootDrawBlock) rare_draw_kernel(RareDrawArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rare_lds[];
    uint64_t *lcum = reinterpret_cast<uint64_t *>(rare_lds);                         // [n_ec + 1]
    uint32_t *hist = reinterpret_cast<uint32_t *>(lcum + (size_t)a.n_ec + 1);        // [n_ec]
    const uint32_t tid = threadIdx.x;
    const uint32_t rep = blockIdx.y / a.n_depths, d = blockIdx.y % a.n_depths;
    const uint64_t j0 = d ? a.depths[d - 1] : 0, j1 = a.depths[d];                   // this row's draws
    constexpr uint64_t kChunk = (uint64_t)kBootDrawBlock * kBootDrawsPerThread;
    if (j0 + (uint64_t)blockIdx.x * kChunk >= j1) return;                            // (the whole workgroup: an interval shorter than the grid)
    unsigned long long *out = a.inc + (size_t)blockIdx.y * a.n_ec;
    const uint64_t key = rare_key(a.seed, (uint64_t)a.b0 + rep);
    if (kLds) {
        for (uint32_t e = tid; e <= a.n_ec; e += kBootDrawBlock) lcum[e] = a.cum[e];
        for (uint32_t e = tid; e < a.n_ec; e += kBootDrawBlock) hist[e] = 0;
        __syncthreads();
    }
    uint64_t since = 0;               // draws in the histogram (uniform over the workgroup): flushed before a u32 bin could wrap
    for (uint64_t c0 = j0 + (uint64_t)blockIdx.x * kChunk; c0 < j1; c0 += (uint64_t)gridDim.x * kChunk) {
        for (uint32_t i = 0; i < kBootDrawsPerThread; i++) {
            const uint64_t j = c0 + (uint64_t)i * kBootDrawBlock + tid;
            if (j >= j1) break;
            const uint64_t t = rare_pi(key, a.half_bits, a.total, j);
            if (kLds) atomicAdd(&hist[boot_find(lcum, a.n_ec, t)], 1u);
            else atomicAdd(&out[boot_find(a.cum, a.n_ec, t)], 1ull);
        }
        if (kLds) {
            since += kChunk;
            if (since >= (1ull << 31)) {
                __syncthreads();
                for (uint32_t e = tid; e < a.n_ec; e += kBootDrawBlock) {
                    const uint32_t h = hist[e];
                    if (h) { atomicAdd(&out[e], (unsigned long long)h); hist[e] = 0; }
                }
                __syncthreads();
                since = 0;
            }
        }
    }
    if (kLds) {
        __syncthreads();
        for (uint32_t e = tid; e < a.n_ec; e += kBootDrawBlock) {
            const uint32_t h = hist[e];
            if (h) atomicAdd(&out[e], (unsigned long long)h);
        }
    }
}

// inc[r][d][e] += inc[r][d-1][e] along d, for the n_rep replicates of a launch
__global__ void __launch_bounds__(256) rare_cumsum_kernel(unsigned long long *inc, uint32_t n_rep, uint32_t n_depths, uint32_t n_ec)
{
    const uint64_t n = (uint64_t)n_rep * n_ec;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / n_ec, e = i % n_ec;
        unsigned long long *p = inc + r * n_depths * n_ec + e;
        unsigned long long sum = 0;
        for (uint32_t d = 0; d < n_depths; d++, p += n_ec) { sum += *p; *p = sum; }
    }
}

} // namespace groot
