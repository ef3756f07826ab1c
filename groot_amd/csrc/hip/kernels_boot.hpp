// kernels_boot.hpp -- bootstrap replicates of the abundance EM on the device (groot_hip_em_bootstrap; the contract is in
// include/groot_host.h, "bootstrap intervals").
//
// boot_resample_kernel: a thread per draw, grid = (chunks of draws, replicates).  Draw j of replicate b is a splitmix64 value of
// (seed, b * n_draws + j), scaled to [0, N) by the high half of a 64 x 64 product and looked up in the cumulative table of the EC
// counts.  Only integers: the counts do not depend on the launch shape.  When the table fits (kLds), cum lies in LDS and the
// workgroup counts into an LDS histogram that it flushes with one global atomic per non-zero bin -- the EC sizes are very skewed,
// a few bins take most draws; otherwise cum is searched in global memory (L2-resident) and every draw is one global u64 atomic.
//
// boot_em_kernel: one workgroup per replicate (looping when there are more replicates than workgroups), each running
// groot_host_em (report.cpp) on its own counts to its own stop.  The host's scatter loop over ECs is restated as two gathers:
//   (1) a thread per EC:   denom = the sum of alpha[ids] in ID order; norm[e] = count / denom, or 0.0 when the host skips the EC
//                          (count 0, or denom < 2^-52);
//   (2) a thread per path: next = the sum over the ECs that hold p, in ascending EC order (a path -> EC CSR built once on the host),
//                          of alpha[p] * norm[e]; the `changed` test; alpha[p] = next.
// For every path these are the host's additions in the host's order, and alpha * 0.0 for a skipped EC leaves a non-negative sum as
// it is, so alpha and the iteration count equal the host's bit for bit.  Phase (2) reads no alpha but its own path's, so `next`
// needs no array: alpha and norm, (n_paths + n_ec) doubles, lie in LDS when they fit (kLds) and in per-workgroup global scratch
// otherwise.  Both kernels' floating point is compiled without contraction: a fused multiply-add would round once where the host
// rounds twice.  f64 denormals are on (the target's default), the quotient is the correctly rounded v_div_* sequence.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace groot {

constexpr int kBootDrawBlock = 256;
constexpr uint32_t kBootDrawsPerThread = 64;     // a workgroup takes chunks of 16 384 draws
constexpr int kBootEmBlock = 1024;               // one replicate per workgroup: all 16 waves of it on one CU

struct BootDrawArgs {
    const uint64_t *cum;              // [n_ec + 1]
    unsigned long long *boot_count;   // [replicates of this launch][n_ec], zeroed
    uint64_t total;                   // N = cum[n_ec] > 0
    uint64_t n_draws, seed;
    uint32_t n_ec;                    // > 0
    uint32_t b0;                      // the launch's first replicate
};

__device__ __forceinline__ uint64_t boot_draw(uint64_t seed, uint64_t index, uint64_t total)
{
    uint64_t z = seed + (index + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return __umul64hi(z, total);
}

// the EC e with cum[e] <= t < cum[e + 1] (cum[0] = 0 <= t < cum[n_ec]: an EC with count 0 is never the answer)
template <class P> __device__ __forceinline__ uint32_t boot_find(P cum, uint32_t n_ec, uint64_t t)
{
    uint32_t lo = 0, hi = n_ec;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cum[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

template <bool kLds> __global__ void __launch_bounds__(kBootDrawBlock) boot_resample_kernel(BootDrawArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char boot_lds[];
    uint64_t *lcum = reinterpret_cast<uint64_t *>(boot_lds);                         // [n_ec + 1]
    uint32_t *hist = reinterpret_cast<uint32_t *>(lcum + (size_t)a.n_ec + 1);        // [n_ec]
    const uint32_t tid = threadIdx.x;
    const uint32_t rep = blockIdx.y;
    unsigned long long *out = a.boot_count + (size_t)rep * a.n_ec;
    const uint64_t base = (uint64_t)(a.b0 + rep) * a.n_draws;
    constexpr uint64_t kChunk = (uint64_t)kBootDrawBlock * kBootDrawsPerThread;
    if (kLds) {
        for (uint32_t e = tid; e <= a.n_ec; e += kBootDrawBlock) lcum[e] = a.cum[e];
        for (uint32_t e = tid; e < a.n_ec; e += kBootDrawBlock) hist[e] = 0;
        __syncthreads();
    }
    uint64_t since = 0;               // draws in the histogram (uniform over the workgroup): flushed before a u32 bin could wrap
    for (uint64_t c0 = (uint64_t)blockIdx.x * kChunk; c0 < a.n_draws; c0 += (uint64_t)gridDim.x * kChunk) {
        for (uint32_t i = 0; i < kBootDrawsPerThread; i++) {
            const uint64_t j = c0 + (uint64_t)i * kBootDrawBlock + tid;
            if (j >= a.n_draws) break;
            const uint64_t t = boot_draw(a.seed, base + j, a.total);
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

struct BootEmArgs {
    const uint32_t *ec_off;           // [n_ec + 1] the ECs' IDs, CSR (as given: ID order)
    const uint32_t *ec_ids;
    const uint32_t *path_off;         // [n_paths + 1] the ECs of every path in ascending EC order, CSR (one entry per occurrence)
    const uint32_t *path_ecs;
    const unsigned long long *boot_count;   // [n_rep][n_ec]
    double *alpha_out;                // [n_rep][n_paths]
    uint32_t *iterations;             // [n_rep]
    double *scratch;                  // !kLds: [gridDim.x][n_paths + n_ec]
    double alpha0;                    // 1 / n_paths, divided on the host
    uint32_t n_paths, n_ec, n_rep, min_iter, max_iter;
};

// sum of x[idx[i]] (kScale: of scale * x[idx[i]]) over i in [begin, end), added one after the other in the order of i, as the host adds
// them.  Eight indices and eight values are fetched at a time: the index loads come from global memory, and a loop that waits for each
// of them before the next add spends the iteration on their latency (84 us an iteration at configs[2], where a path lies in up to 175 ECs).
template <bool kScale> __device__ __forceinline__ double boot_sum_in_order(const double *x, const uint32_t *__restrict__ idx, uint32_t begin, uint32_t end,
                                                                         double scale)
{
#pragma clang fp contract(off)
    double sum = 0.0;
    uint32_t i = begin;
    for (; i + 8 <= end; i += 8) {
        uint32_t k[8];
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) k[u] = idx[i + u];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = x[k[u]];
#pragma unroll
        for (int u = 0; u < 8; u++) sum += kScale ? scale * v[u] : v[u];
    }
    for (; i < end; i++) sum += kScale ? scale * x[idx[i]] : x[idx[i]];
    return sum;
}

template <bool kLds> __global__ void __launch_bounds__(kBootEmBlock) boot_em_kernel(BootEmArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char boot_lds[];
    double *alpha = kLds ? reinterpret_cast<double *>(boot_lds) : a.scratch + (size_t)blockIdx.x * ((size_t)a.n_paths + a.n_ec);
    double *norm = alpha + a.n_paths;
    const uint32_t tid = threadIdx.x;
    const double tolerance = 2.220446049250313e-16;            // nextafter(1, 2) - 1 = 2^-52
    const double alpha_limit = 1e-7, alpha_change = 1e-2, alpha_change_limit = 1e-2;
    for (uint32_t rep = blockIdx.x; rep < a.n_rep; rep += gridDim.x) {
        const unsigned long long *count = a.boot_count + (size_t)rep * a.n_ec;
        __syncthreads();                                        // (the previous replicate's alpha has been copied out)
        for (uint32_t p = tid; p < a.n_paths; p += kBootEmBlock) alpha[p] = a.alpha0;
        __syncthreads();
        bool final_round = false;
        uint32_t it = 0;
        for (; it < a.max_iter; it++) {
            for (uint32_t e = tid; e < a.n_ec; e += kBootEmBlock) {
                const unsigned long long c = count[e];
                double nm = 0.0;
                if (c != 0) {
                    const double denom = boot_sum_in_order<false>(alpha, a.ec_ids, a.ec_off[e], a.ec_off[e + 1], 1.0);
                    if (!(denom < tolerance)) nm = (double)c / denom;
                }
                norm[e] = nm;
            }
            __syncthreads();
            int changed = 0;
            for (uint32_t p = tid; p < a.n_paths; p += kBootEmBlock) {
                const double al = alpha[p];
                const double next = boot_sum_in_order<true>(norm, a.path_ecs, a.path_off[p], a.path_off[p + 1], al);
                if (next > alpha_change_limit && fabs(next - al) / next > alpha_change) changed = 1;
                alpha[p] = next;
            }
            changed = __syncthreads_or(changed);
            const bool stop = changed == 0 && it > a.min_iter;
            if (final_round) break;
            if (stop) {                       // one more round after this one, from alpha with its tiny values zeroed
                final_round = true;
                for (uint32_t p = tid; p < a.n_paths; p += kBootEmBlock)
                    if (alpha[p] < alpha_limit / 10.0) alpha[p] = 0.0;
                __syncthreads();
            }
        }
        __syncthreads();
        for (uint32_t p = tid; p < a.n_paths; p += kBootEmBlock) a.alpha_out[(size_t)rep * a.n_paths + p] = alpha[p];
        if (tid == 0) a.iterations[rep] = it;
    }
}

} // namespace groot
