// kernels_csup.hpp -- bootstrap support for the calls on the device (groot_hip_call_support; the contract is in include/groot_host.h,
// "bootstrap support for the calls").
//
// The host groups the tuples of the assigned-coverage table by (EC, path) into rows: row r is path_len + 1 integers at d[row_base[r]],
// the rows of a path lie one behind the other in canonical EC order.  Rows are replicate-independent and are made once per chunk of paths:
//
// csup_fill_kernel<T>: a thread per tuple, +n at Pos and -n at last + 1 of its row with integer atomics modulo 2^w (T = u32 while every
//   row's record sum is below 2^32, else u64): the order of the atomics does not matter.
// csup_scan_kernel<T>: a wavefront per row, 64 entries at a time: a wave-level inclusive scan plus the carry of the entries before turns
//   the differences into d_e[x], in place.
// csup_weight_kernel: a thread per (replicate, EC): denom_b(e) added in ID order, then f_b(e,p) = s_b(e) * w_b(e,p) for every listed ID.
// csup_cover_kernel<T, R>: a workgroup per (path, group of R replicates).  The f_b of the path's rows for the R replicates are staged in
//   LDS (kCsupTile rows at a time) and read as broadcasts; a thread takes the bases x = tid, tid + 256, ..: each d value is loaded once,
//   coalesced over x, and feeds R accumulators D = D + (double)d * f, the rows strictly in list order.  The covered bases are counted
//   with a ballot and a popcount per wavefront, and one atomic add per wavefront and replicate goes into covered[b][p].
//
// Everything in floating point is compiled without contraction: the host rounds the product and the sum separately.  The quotients are
// the correctly rounded v_div_* sequence, f64 denormals are on (the target's default), (double) of an integer below 2^53 .. 2^64 rounds
// to nearest as the host's conversion does.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.hpp"

namespace groot {

constexpr uint32_t kCsupTile = 256;      // rows of one path staged in LDS at a time: 256 x R = 8 replicates x 8 B = 16 KB
constexpr int kCsupReps = 8;             // R: replicates per workgroup of csup_cover_kernel

template <class T> struct CsupAtomic;
template <> struct CsupAtomic<uint32_t> { using type = unsigned int; };
template <> struct CsupAtomic<uint64_t> { using type = unsigned long long; };

struct CsupFillArgs {
    const uint32_t *t_row;            // [n_tuples] the tuple's row
    const uint32_t *t_pos, *t_last;   // Pos <= last < path_len (the host has checked; a tuple with Pos > last covers nothing)
    const uint64_t *t_n;
    const uint64_t *row_base;         // [n_rows + 1] offsets of the rows in entries, over all chunks
    uint64_t chunk_base;              // row_base of the chunk's first row
    uint32_t t0, t1;                  // the chunk's tuples
};

template <class T> __global__ void __launch_bounds__(kBlock) csup_fill_kernel(CsupFillArgs a, T *d)
{
    using A = typename CsupAtomic<T>::type;
    for (uint64_t i = (uint64_t)a.t0 + (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.t1; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t pos = a.t_pos[i], last = a.t_last[i];
        if (pos > last) continue;
        A *row = reinterpret_cast<A *>(d) + (a.row_base[a.t_row[i]] - a.chunk_base);
        const A n = (A)a.t_n[i];
        atomicAdd(row + pos, n);
        atomicAdd(row + (size_t)last + 1, (A)0 - n);
    }
}

__device__ __forceinline__ uint32_t csup_shfl_up(uint32_t v, int k) { return (uint32_t)__shfl_up((int)v, k, 64); }
__device__ __forceinline__ uint64_t csup_shfl_up(uint64_t v, int k)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, k, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), k, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t csup_shfl(uint32_t v, int l) { return (uint32_t)__shfl((int)v, l, 64); }
__device__ __forceinline__ uint64_t csup_shfl(uint64_t v, int l)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, l, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), l, 64);
    return ((uint64_t)hi << 32) | lo;
}

// rows [r0, r1): entry x becomes the sum of the entries 0 .. x (modulo 2^w); the entry at path_len is not read again and stays
template <class T> __global__ void __launch_bounds__(kBlock) csup_scan_kernel(const uint64_t *row_base, uint64_t chunk_base, uint32_t r0, uint32_t r1, T *d)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = kBlock / 64;
    for (uint64_t r = (uint64_t)r0 + (uint64_t)blockIdx.x * waves + wave; r < r1; r += (uint64_t)gridDim.x * waves) {
        T *row = d + (row_base[r] - chunk_base);
        const uint64_t len = row_base[r + 1] - row_base[r] - 1;
        T carry = 0;
        for (uint64_t x0 = 0; x0 < len; x0 += 64) {        // (uniform over the wavefront: every lane takes part in the shuffles)
            const uint64_t x = x0 + lane;
            T v = x < len ? row[x] : (T)0;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                const T up = csup_shfl_up(v, k);
                if ((int)lane >= k) v += up;
            }
            v += carry;
            if (x < len) row[x] = v;
            carry = csup_shfl(v, 63);
        }
    }
}

struct CsupWeightArgs {
    const uint32_t *ec_off;                 // [n_ec + 1] the ECs' IDs, CSR
    const uint32_t *ec_ids;
    const uint64_t *count;                  // [n_ec], > 0
    const unsigned long long *boot_count;   // [n_rep][n_ec]
    const double *alpha;                    // [n_rep][n_paths]
    double *f;                              // [n_rep][listed IDs]
    uint32_t n_ec, n_paths, n_rep;
};

__global__ void __launch_bounds__(kBlock) csup_weight_kernel(CsupWeightArgs a)
{
#pragma clang fp contract(off)
    const double tolerance = 2.220446049250313e-16;            // nextafter(1, 2) - 1 = 2^-52
    const uint64_t total = (uint64_t)a.n_rep * a.n_ec, listed = a.ec_off[a.n_ec];
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t b = (uint32_t)(i / a.n_ec), e = (uint32_t)(i % a.n_ec);
        const double *alpha = a.alpha + (size_t)b * a.n_paths;
        const uint32_t lo = a.ec_off[e], hi = a.ec_off[e + 1];
        double denom = 0.0;
        for (uint32_t j = lo; j < hi; j++) denom = denom + alpha[a.ec_ids[j]];
        const unsigned long long bc = a.boot_count[i];
        const bool skip = bc == 0 || denom < tolerance;
        const double s = (double)bc / (double)a.count[e];
        double *f = a.f + (size_t)b * listed;
        for (uint32_t j = lo; j < hi; j++) {
            const double w = skip ? 0.0 : alpha[a.ec_ids[j]] / denom;
            f[j] = s * w;
        }
    }
}

struct CsupCoverArgs {
    const uint32_t *path_row;         // [paths of the selection + 1] the rows of every selected path, over all chunks
    const uint32_t *path_len;         // [paths of the selection]
    const uint32_t *row_listed;       // [n_rows] the row's index among the listed IDs
    const uint64_t *row_base;         // [n_rows + 1]
    const double *f;                  // [n_rep][listed]
    uint32_t *covered;                // [n_rep][n_sel], zeroed
    uint64_t chunk_base;
    uint64_t listed;
    double call_depth;
    uint32_t s0;                      // the chunk's first selected path (blockIdx.x counts from it)
    uint32_t n_sel, n_rep;
    uint32_t g0;                      // the launch's first group of R replicates (blockIdx.y counts from it)
};

template <class T, int R> __global__ void __launch_bounds__(kBlock) csup_cover_kernel(CsupCoverArgs a, const T *d)
{
#pragma clang fp contract(off)
    __shared__ double lf[kCsupTile * R];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t s = a.s0 + blockIdx.x, b0 = (a.g0 + blockIdx.y) * R;
    const uint32_t r0 = a.path_row[s], r1 = a.path_row[s + 1], len = a.path_len[s];
    const bool one_tile = r1 - r0 <= kCsupTile;
    uint32_t mine[R];                 // lane 0 of each wavefront: the covered bases its wavefront has seen
#pragma unroll
    for (int k = 0; k < R; k++) mine[k] = 0;
    for (uint32_t x0 = 0; x0 < len; x0 += kBlock) {       // (uniform over the workgroup: the barriers below)
        const uint32_t x = x0 + tid;
        const bool in = x < len;
        double D[R];
#pragma unroll
        for (int k = 0; k < R; k++) D[k] = 0.0;
        for (uint32_t t0 = r0; t0 < r1; t0 += kCsupTile) {
            const uint32_t nt = min(kCsupTile, r1 - t0);
            if (!(one_tile && x0)) {                      // a path of at most kCsupTile rows is staged once
                __syncthreads();
                for (uint32_t i = tid; i < nt * R; i += kBlock) {
                    const uint32_t b = b0 + i % R;
                    lf[i] = b < a.n_rep ? a.f[(size_t)b * a.listed + a.row_listed[t0 + i / R]] : 0.0;
                }
                __syncthreads();
            }
            if (in)
                for (uint32_t i = 0; i < nt; i++) {
                    const double dv = (double)d[a.row_base[t0 + i] - a.chunk_base + x];
#pragma unroll
                    for (int k = 0; k < R; k++) {
                        const double term = dv * lf[i * R + k];
                        D[k] = D[k] + term;
                    }
                }
        }
#pragma unroll
        for (int k = 0; k < R; k++) mine[k] += (uint32_t)__popcll(__ballot(in && D[k] >= a.call_depth));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < R; k++)
            if (b0 + k < a.n_rep && mine[k]) atomicAdd(&a.covered[(size_t)(b0 + k) * a.n_sel + s], mine[k]);
    }
}

} // namespace groot
