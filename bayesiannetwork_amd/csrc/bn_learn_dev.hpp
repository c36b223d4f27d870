// bn_learn_dev.hpp -- device functions the searches over a term table share (bn_learn_anneal.hip, bn_learn_hc.hip): lane reads,
// the wave-level LDS ordering, the stream's integer draw, the term lookup and the learner's evaluation.  One wave per chain or run,
// lane v = node v.
#pragma once

#include <hip/hip_runtime.h>

#include "bn_learn_anneal.hpp"
#include "bn_rng_dev.hpp"

namespace bnmi {
namespace {

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t lane_u32(uint32_t x, int l) { return uint32_t(__builtin_amdgcn_readlane(int(x), l)); }
__device__ __forceinline__ uint64_t lane_u64(uint64_t x, int l) {
    return (uint64_t(lane_u32(uint32_t(x >> 32), l)) << 32) | lane_u32(uint32_t(x), l);
}
__device__ __forceinline__ double lane_f64(double x, int l) { return __longlong_as_double((long long)lane_u64(uint64_t(__double_as_longlong(x)), l)); }

// the lanes of a wave run in step, and its LDS operations complete in order: what is left is to keep the compiler from moving them
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t draw_below(uint4& g, uint32_t m) { return uint32_t((uint64_t(xoshiro_next(g)) * m) >> 32); }

// the index of parent set `mask` in child c's row of the term table; mask has at most q bits, all below n, and not bit c
__device__ __forceinline__ uint32_t rank_of(const uint32_t* tab, int c, uint64_t mask) {
    uint32_t rank = 0;
    int j = 0;
    while (mask) {
        const int s = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        ++j;
        rank += tab[kAnnealTabBinom + j * 64 + (s - (s > c ? 1 : 0))];
    }
    return rank + tab[j];
}

// ll(c, mask) from the term table
__device__ __forceinline__ double term_of(const double* __restrict__ terms, int64_t T, const uint32_t* tab, int c, uint64_t mask) {
    return terms[int64_t(c) * T + rank_of(tab, c, mask)];
}

// the learner's score of the graph whose family terms the lanes hold in x: likelihood -= ll[v] in node order through lane reads (no
// tree), then the AIC / MDL penalty from the exact parameter count -- the bits of bn_learn_score.  Criteria 2 and 3 (BDeu, K2) have
// no penalty: the likelihood alone.
__device__ __forceinline__ double evaluate_terms(double x, int64_t params, int n, int criterion, double penalty) {
    double likelihood = 0.0;
    for (int v = 0; v < n; ++v) likelihood -= lane_f64(x, v);
    if (criterion >= 2) return likelihood;
    return criterion == 0 ? likelihood + double(params) : likelihood + double(params) * penalty;
}

// log Gamma(x) for finite x > 0 as a stated function (include/bn_mi355x.h, "Bayesian-Dirichlet scores"): the argument is shifted
// to x >= 16 by the recurrence, then Stirling's series with six terms; every operation is a plain fp64 one (no contraction) and the
// only library call is the device's log.
constexpr double kLgC0 = 1.0 / 12.0, kLgC1 = -1.0 / 360.0, kLgC2 = 1.0 / 1260.0, kLgC3 = -1.0 / 1680.0, kLgC4 = 1.0 / 1188.0,
                 kLgC5 = -691.0 / 360360.0;
constexpr uint64_t kHalfLog2PiBits = 0x3FED67F1C864BEB4ull;   // 0.9189385332046727

__device__ inline double lgamma_pos(double x) {
    double p = 1.0;
    bool shifted = false;
    while (x < 16.0) {   // at most 16 steps
        p = p * x;
        x = x + 1.0;
        shifted = true;
    }
    const double r = 1.0 / x, r2 = r * r;
    double s = kLgC5;
    s = s * r2 + kLgC4;
    s = s * r2 + kLgC3;
    s = s * r2 + kLgC2;
    s = s * r2 + kLgC1;
    s = s * r2 + kLgC0;
    s = s * r;
    const double v = (((x - 0.5) * log(x)) - x) + __longlong_as_double((long long)kHalfLog2PiBits) + s;
    return shifted ? v - log(p) : v;
}

}  // namespace
}  // namespace bnmi
