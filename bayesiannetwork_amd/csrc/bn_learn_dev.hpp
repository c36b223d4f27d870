// bn_learn_dev.hpp -- device functions the searches over a term table share (bn_learn_anneal.hip, bn_learn_hc.hip,
// bn_learn_climb.hip): lane reads, the wave-level LDS ordering, the run frame (entry, stream, family state, closing store, launch),
// the stream's integer draw, the term lookup and the learner's evaluation.  One wave per run, lane v = node v.
#pragma once

#include <hip/hip_runtime.h>

#include "bn_learn_search.hpp"
#include "bn_rng_dev.hpp"

namespace bnmi {
namespace {

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t lane_u32(uint32_t x, int l) { return uint32_t(__builtin_amdgcn_readlane(int(x), l)); }
__device__ __forceinline__ uint64_t lane_u64(uint64_t x, int l) {
    return (uint64_t(lane_u32(uint32_t(x >> 32), l)) << 32) | lane_u32(uint32_t(x), l);
}
__device__ __forceinline__ double lane_f64(double x, int l) { return __longlong_as_double((long long)lane_u64(uint64_t(__double_as_longlong(x)), l)); }
// (the same reads where the source lane differs per lane)
__device__ __forceinline__ uint32_t from_lane_u32(uint32_t x, int src) { return uint32_t(__builtin_amdgcn_ds_bpermute(src << 2, int(x))); }
__device__ __forceinline__ uint64_t from_lane_u64(uint64_t x, int src) {
    return (uint64_t(from_lane_u32(uint32_t(x >> 32), src)) << 32) | from_lane_u32(uint32_t(x), src);
}

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
        rank += tab[kTermTabBinom + j * 64 + (s - (s > c ? 1 : 0))];
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

// ---- the run frame: what the kernel of every search does alike around its loop ---------------------------------------------------

struct SearchWave {
    int wave, lane, run;   // wave and run are wave-uniform
    bool surplus;          // a wave past the last run (of the last workgroup): the kernel returns; no workgroup barrier follows
};

// the rank tables into LDS, the workgroup's one barrier, then who this wave is
template <int Waves>
__device__ __forceinline__ SearchWave search_enter(uint32_t* s_tab, const SearchArgs& a) {
    for (int i = int(threadIdx.x); i < kTermTabBinom + (a.q + 1) * 64; i += Waves * 64) s_tab[i] = a.tab[i];
    __syncthreads();
    const int wave = uni(int(threadIdx.x >> 6)), run = int(blockIdx.x) * Waves + wave;
    return SearchWave{wave, int(threadIdx.x & 63), run, run >= a.runs};
}

// run j's stream: xoshiro128++ seeded by Philox4x32-10({j_lo, j_hi, 0, 0}, {seed_lo, seed_hi}), wave-uniform
__device__ __forceinline__ uint4 seed_stream(int run, uint32_t seed_lo, uint32_t seed_hi) {
    uint4 g = philox4x32_10(uint32_t(run), 0u, 0u, 0u, seed_lo, seed_hi);
    g.x = uint32_t(uni(int(g.x))); g.y = uint32_t(uni(int(g.y))); g.z = uint32_t(uni(int(g.z))); g.w = uint32_t(uni(int(g.w)));
    if ((g.x | g.y | g.z | g.w) == 0) g.x = 1;
    return g;
}

// Lane v's family state: the parent mask pm, the exact int64 row product rows (for the parameter count), the family term ll and the
// arity kk.  A lane past n holds no parents, one row, term 0 and arity 1.
__device__ __forceinline__ void load_family(const StartGraph& g, const int32_t* k, int n, int lane, uint64_t& pm, int64_t& rows, double& ll,
                                            int32_t& kk) {
    const bool node = lane < n;
    pm = node ? g.pmask0[lane] : 0;
    rows = node ? g.rows0[lane] : 1;
    ll = node ? g.ll0[lane] : 0.0;
    kk = node ? k[lane] : 1;
}
// the family with parent p (of arity k_p) added ...
__device__ __forceinline__ void with_parent(uint64_t pm, int64_t rows, int p, uint32_t k_p, uint64_t& pm_new, int64_t& rows_new) {
    pm_new = pm | (uint64_t(1) << p);
    rows_new = rows * k_p;
}
// ... and removed (an eligible family has at most 2^20 entries: the divide is exact in 32 bits)
__device__ __forceinline__ int64_t rows_without(int64_t rows, uint32_t k_p) { return int64_t(uint32_t(rows) / k_p); }
__device__ __forceinline__ void without_parent(uint64_t pm, int64_t rows, int p, uint32_t k_p, uint64_t& pm_new, int64_t& rows_new) {
    pm_new = pm & ~(uint64_t(1) << p);
    rows_new = rows_without(rows, k_p);
}
// the change of the parameter count when the lanes' row products go from rows to rows_new: lane `to`'s part and, for a reversal,
// lane `from`'s (a lane whose family stays has rows_new == rows)
__device__ __forceinline__ int64_t params_delta(int32_t kk, int64_t rows, int64_t rows_new, int to, int from, bool reversal) {
    const int64_t delta = int64_t(kk - 1) * (rows_new - rows);
    int64_t sum = int64_t(lane_u64(uint64_t(delta), to));
    if (reversal) sum += int64_t(lane_u64(uint64_t(delta), from));
    return sum;
}

// the graph a run ends with
__device__ __forceinline__ void store_graph(const SearchArgs& a, int run, int lane, uint64_t pm, double ll) {
    if (lane < a.n) {
        a.masks[int64_t(run) * a.n + lane] = pm;
        a.ll[int64_t(run) * a.n + lane] = ll;
    }
}

// one wave per run, Waves runs per workgroup; returns a hipError_t value (0: success)
template <int Waves, class Args>
int launch_search(void (*kernel)(Args), const Args& a, void* stream) {
    const int blocks = (a.runs + Waves - 1) / Waves;
    hipLaunchKernelGGL(kernel, dim3(unsigned(blocks)), dim3(Waves * 64), 0, hipStream_t(stream), a);
    return int(hipGetLastError());
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
