// bn_rng_dev.hpp -- the device side of the library's random streams (oracle/lw_oracle.c states them): a stream is xoshiro128++
// seeded by ONE Philox4x32-10 block keyed by (seed, stream id).  Shared by the sampler (bn_lw_kernels.hip) and the annealing
// chains (bn_learn_anneal.hip); device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bnmi {

__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = uint64_t(0xD2511F53u) * c0, p1 = uint64_t(0xCD9E8D57u) * c2;
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = uint32_t(p1); c2 = n2; c3 = uint32_t(p0);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// xoshiro128++ 1.0 (Blackman & Vigna): one 32-bit output, state in x/y/z/w
__device__ __forceinline__ uint32_t xoshiro_next(uint4& g) {
    const uint32_t sum = g.x + g.w;
    const uint32_t result = ((sum << 7) | (sum >> 25)) + g.x;
    const uint32_t t = g.y << 9;
    g.z ^= g.x; g.w ^= g.y; g.y ^= g.z; g.x ^= g.w;
    g.z ^= t;
    g.w = (g.w << 11) | (g.w >> 21);
    return result;
}

}  // namespace bnmi
