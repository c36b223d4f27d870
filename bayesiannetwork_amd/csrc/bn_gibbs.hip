// bn_gibbs.hip -- the kernel of Gibbs sampling with coloured parallel chains; bn_gibbs.hpp states the contract and the shape.
#include <hip/hip_runtime.h>

#include "bn_gibbs.hpp"
#include "bn_launch.hpp"
#include "bn_rng_dev.hpp"

namespace bnmi {
namespace {

constexpr int kRegStates = 8;   // arities up to this keep a node's weights in registers

// where child c's entries for x = 0, 1, ... stand in the flat array: *at + x * *step (the other parents and c's own state fixed)
__device__ __forceinline__ void child_entries(const GibbsArgs& a, const GibbsChild& c, const uint8_t* st, int64_t* at, int64_t* step) {
    int64_t row = 0;
    for (int32_t q = 0; q < c.term_n; ++q) {
        const GibbsTerm t = a.terms[c.term_lo + q];
        row += int64_t(st[t.node]) * t.stride;
    }
    *at = c.cpt_off + row * c.k + st[c.node];
    *step = c.stride * c.k;
}

// w[x] of one update, by itself: the node's own entry, times one entry per child in ascending child index
__device__ __forceinline__ double gibbs_weight(const GibbsArgs& a, const GibbsSlot& s, const uint8_t* st, int64_t own, int32_t x) {
    double w = a.cpt[own + x];
    for (int32_t j = 0; j < s.child_n; ++j) {
        int64_t at, step;
        child_entries(a, a.children[s.child_lo + j], st, &at, &step);
        w *= a.cpt[at + x * step];
    }
    return w;
}

__device__ __forceinline__ double gibbs_uniform(uint64_t seed, uint64_t chain, uint64_t g, int32_t v) {
    const uint4 r = philox4x32_10(uint32_t(v), uint32_t(g), uint32_t(chain), uint32_t(chain >> 32), uint32_t(seed),
                                  uint32_t(seed >> 32) ^ kGibbsKeyTag);
    const uint64_t U = (uint64_t(r.x) << 21) | uint64_t(r.y >> 11);
    return double(U) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ bool finite_above_zero(double T) { return T > 0.0 && T <= 1.7976931348623157e308; }

// One update of slot s's node in the chain whose states are st; false: stuck.  Arities up to kRegStates: the weights stay in
// registers and the children are the outer loop -- a child's descriptor and its other parents are read once, and its entries
// for all x are loads that do not wait for each other.  Larger arities: every weight is computed twice, once for T and once for
// the choice.  The operations on each w[x] and their order are the same in both.
__device__ __forceinline__ bool gibbs_update(const GibbsArgs& a, const GibbsSlot& s, uint8_t* st, uint64_t chain, uint64_t g) {
    int64_t row = 0;
    for (int32_t j = 0; j < s.term_n; ++j) {
        const GibbsTerm t = a.terms[s.term_lo + j];
        row += int64_t(st[t.node]) * t.stride;
    }
    const int64_t own = s.cpt_off + row * s.k;
    int32_t pick = -1, last = -1;
    if (s.k <= kRegStates) {
        double w[kRegStates];
#pragma unroll
        for (int32_t x = 0; x < kRegStates; ++x) w[x] = x < s.k ? a.cpt[own + x] : 0.0;
        for (int32_t j = 0; j < s.child_n; ++j) {
            int64_t at, step;
            child_entries(a, a.children[s.child_lo + j], st, &at, &step);
#pragma unroll
            for (int32_t x = 0; x < kRegStates; ++x)
                if (x < s.k) w[x] *= a.cpt[at + x * step];
        }
        double T = 0.0;
#pragma unroll
        for (int32_t x = 0; x < kRegStates; ++x)
            if (x < s.k) T += w[x];
        if (!finite_above_zero(T)) return false;
        const double t = gibbs_uniform(a.seed, chain, g, s.node) * T;
        double c = 0.0;
#pragma unroll
        for (int32_t x = 0; x < kRegStates; ++x)
            if (x < s.k) {
                c += w[x];
                if (w[x] > 0.0) last = x;
                if (pick < 0 && t < c) pick = x;
            }
    } else {
        double T = 0.0;
        for (int32_t x = 0; x < s.k; ++x) T += gibbs_weight(a, s, st, own, x);
        if (!finite_above_zero(T)) return false;
        const double t = gibbs_uniform(a.seed, chain, g, s.node) * T;
        double c = 0.0;
        for (int32_t x = 0; x < s.k; ++x) {
            const double w = gibbs_weight(a, s, st, own, x);
            c += w;
            if (w > 0.0) last = x;
            if (t < c) { pick = x; break; }
        }
    }
    if (pick < 0) pick = last;
    if (pick >= 0) st[s.node] = uint8_t(pick);
    return true;
}

__global__ __launch_bounds__(kGibbsThreads) void gibbs_kernel(const GibbsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gibbs_lds[];
    uint32_t* const hist = reinterpret_cast<uint32_t*>(gibbs_lds);
    // a chain is a group of `lanes` = 8 .. 64 neighbouring lanes of a wave
    const int32_t lanes = 1 << a.lanes_log2, group = int32_t(threadIdx.x) >> a.lanes_log2, lane = int32_t(threadIdx.x) & (lanes - 1);
    uint8_t* const st = gibbs_lds + ((a.cells * 4 + 15) & ~15) + group * a.state_stride;
    const uint64_t idx = uint64_t(blockIdx.x) * uint64_t(kGibbsThreads >> a.lanes_log2) + uint64_t(group);   // the group's chain inside the launch
    const bool active = idx < a.n_chains;
    const uint64_t chain = a.chain_begin + idx;
    uint8_t* const mine = a.states + (active ? idx : 0) * uint64_t(a.n);

    for (int32_t q = int32_t(threadIdx.x); q < a.cells; q += kGibbsThreads) hist[q] = 0u;
    if (active)
        for (int32_t v = lane; v < a.n; v += lanes) st[v] = mine[v];
    __syncthreads();

    unsigned long long stuck = 0;
    for (uint32_t i = 0; i < a.n_sweeps; ++i) {
        const uint64_t g = a.sweep_begin + i;
        for (int32_t col = 0; col < a.n_colours; ++col) {
            if (active) {
                const int32_t hi = a.colour_ptr[col + 1];
                for (int32_t q = a.colour_ptr[col] + lane; q < hi; q += lanes) {
                    const GibbsSlot s = a.slots[q];
                    if (a.clamp[s.node] >= 0) continue;
                    if (!gibbs_update(a, s, st, chain, g)) ++stuck;
                }
            }
            __syncthreads();   // the next colour reads what this one wrote
        }
        if (g >= a.burn_in && (g - a.burn_in) % a.thin == 0) {
            if (active)
                for (int32_t q = lane; q < a.n; q += lanes) {
                    const GibbsSlot& s = a.slots[q];
                    atomicAdd(&hist[s.hist_off + st[s.node]], 1u);
                }
            __syncthreads();   // (the next sweep writes the states this one counted)
        }
    }

    // (the last colour's barrier, or the count's, stands between the last write and these reads)
    if (active)
        for (int32_t v = lane; v < a.n; v += lanes) mine[v] = st[v];
    for (int32_t q = int32_t(threadIdx.x); q < a.cells; q += kGibbsThreads)
        if (hist[q]) atomicAdd(&a.counts[q], static_cast<unsigned long long>(hist[q]));
    if (stuck) atomicAdd(a.stuck, stuck);
}

}  // namespace

int launch_gibbs(const GibbsArgs& a, int64_t blocks, int32_t lds_bytes, void* stream) {
    return launched([&] {
        if (blocks > 0) hipLaunchKernelGGL(gibbs_kernel, dim3(uint32_t(blocks)), dim3(kGibbsThreads), size_t(lds_bytes), (hipStream_t)stream, a);
    });
}

}  // namespace bnmi
