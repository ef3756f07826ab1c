// rare_perm.hpp -- the permutation pi_b of the rarefaction draw (include/groot_host.h, "rarefaction curves"), one text for the host
// library (report.cpp) and the device kernel (kernels_rare.hpp): only 64-bit integer arithmetic modulo 2^64, so both give the same x.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GROOT_RARE_HD __host__ __device__ __forceinline__
#else
#define GROOT_RARE_HD inline
#endif

namespace groot {

constexpr uint64_t kRareGolden = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kRareMaxUnits = 1ull << 62;         // N below this: h <= 31, the Feistel domain 2^(2h) fits 64 bits

// sm(z): the mixing steps of the bootstrap's draw
GROOT_RARE_HD uint64_t rare_sm(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// h = the smallest integer >= 1 with 2^(2h) >= N (1 <= N < 2^62)
GROOT_RARE_HD uint32_t rare_half_bits(uint64_t n)
{
    uint32_t h = 1;
    while (h < 31 && (1ull << (2 * h)) < n) h++;
    return h;
}

// k_b
GROOT_RARE_HD uint64_t rare_key(uint64_t seed, uint64_t b) { return rare_sm(seed + (b + 1) * kRareGolden); }

// pi_b(j), 0 <= j < n: six Feistel rounds over [0, 2^(2h)), walked until the value is back inside [0, n).  The network is a bijection
// of its domain, so the walk from a j < n returns to [0, n) and pi_b is a bijection of it.
GROOT_RARE_HD uint64_t rare_pi(uint64_t key, uint32_t h, uint64_t n, uint64_t j)
{
    const uint64_t mask = (1ull << h) - 1;
    uint64_t x = j;
    do {
        uint64_t l = x >> h, r = x & mask;
        for (uint64_t t = 0; t < 6; t++) {
            const uint64_t f = rare_sm(key + (((t << 32) | r) + 1) * kRareGolden) >> (64 - h);
            const uint64_t nl = r;
            r = l ^ f;
            l = nl;
        }
        x = (l << h) | r;
    } while (x >= n);
    return x;
}

} // namespace groot
