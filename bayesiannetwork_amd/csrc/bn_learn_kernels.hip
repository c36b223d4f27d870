// bn_learn_kernels.hip -- the two kernels under structure learning (reference bayesian/learning/greedy.hpp, k2_algorithm.hpp):
// exact family counts of MANY candidate families of a child in one pass over the table, and per family the maximum-likelihood
// log-likelihood term  sum over entries with N != 0 of double(N) * log(double(N) / double(row total)).
//
// Counting.  A chunk is a child c, its base parents and a run of candidates u.  The table is [node][pattern] bytes, so a lane takes
// kLearnLanePatterns consecutive patterns (one 8-byte load of a node's row; a wave load is 512 contiguous bytes).  Everything about
// the chunk -- child, parents, arities, candidates -- is the same in every lane and is read through uniform addresses (scalar
// loads).  Per pattern the weight and the base index B = mixed radix over the base parents are loaded / computed ONCE and reused
// for every candidate: cell of candidate u = (B * k_u + s_u) * k_c + s_c, two multiply-adds, no division.  The counters live in LDS
// while the chunk's block has <= kLearnLdsCells cells, else in device memory; both are uint64 integer atomics, so the counts do not
// depend on the grouping, the chunking, the split or the order of the patterns.  No floating-point atomics anywhere.
//
// Scoring.  One workgroup per family; the additions are bn_score_nodes' (bn_score_kernels.hip): thread t adds the terms of the
// entries r = t, t + 256, ... of the FITTED layout in increasing r from +0.0, then the 256 partial sums are folded by halves.  The
// counted cell of entry r is found by division per entry (bn_learn.hpp, LearnFamily).
#include <hip/hip_runtime.h>

#include "bn_learn.hpp"

namespace bnmi {

__device__ __forceinline__ uint32_t state_of(const uint2& x, int i) {
    return ((i < 4 ? x.x : x.y) >> (8 * (i & 3))) & 255u;
}

__global__ __launch_bounds__(kLearnBlock) void learn_count_kernel(LearnArgs a, int32_t chunk0) {
    constexpr int LP = kLearnLanePatterns;
    __shared__ unsigned long long sh[kLearnLdsCells];
    const LearnChunk* __restrict__ cp = a.chunks + (chunk0 + int32_t(blockIdx.x));
    const int32_t* __restrict__ par_id = a.par_id + cp->base_at;
    const int32_t* __restrict__ par_k = a.par_k + cp->base_at;
    const int32_t* __restrict__ cand_id = a.cand_id + cp->cand_at;
    const int32_t* __restrict__ cand_k = a.cand_k + cp->cand_at;
    const int32_t* __restrict__ cand_cell = a.cand_cell + cp->cand_at;
    const int n_base = cp->n_base, n_cand = cp->n_cand, cells = cp->cells, base_cell = cp->base_cell;
    const uint32_t kc = uint32_t(cp->kc);
    const bool in_lds = cp->in_lds != 0;
    unsigned long long* __restrict__ blockN = a.N + cp->count_at;
    const uint8_t* __restrict__ Tc = a.T + int64_t(cp->child) * a.Ppad;
    if (in_lds)
        for (int q = threadIdx.x; q < cells; q += kLearnBlock) sh[q] = 0ull;
    __syncthreads();
    const int64_t tiles = (a.P + kLearnTile - 1) / kLearnTile;
    const int64_t share = (tiles + gridDim.y - 1) / gridDim.y;
    const int64_t t_end = min(tiles, share * (int64_t(blockIdx.y) + 1));
    for (int64_t t = share * blockIdx.y; t < t_end; ++t) {
        const int64_t p0 = (t * kLearnBlock + threadIdx.x) * LP;
        if (p0 >= a.P) continue;   // (p0 < P <= Ppad, both multiples of 8 apart from P: the lane's 8 bytes are inside the row)
        unsigned long long w[LP];
#pragma unroll
        for (int i = 0; i < LP; ++i) w[i] = p0 + i < a.P ? a.w[p0 + i] : 0ull;
        uint32_t B[LP];   // base parents' assignment, first parent most significant, then the child's state
#pragma unroll
        for (int i = 0; i < LP; ++i) B[i] = 0u;
        for (int j = 0; j < n_base; ++j) {
            const uint32_t ku = uint32_t(par_k[j]);
            const uint2 x = *reinterpret_cast<const uint2*>(a.T + int64_t(par_id[j]) * a.Ppad + p0);
#pragma unroll
            for (int i = 0; i < LP; ++i) B[i] = B[i] * ku + state_of(x, i);
        }
        const uint2 xc = *reinterpret_cast<const uint2*>(Tc + p0);
        if (base_cell >= 0) {
#pragma unroll
            for (int i = 0; i < LP; ++i) {
                if (!w[i]) continue;
                const uint32_t cell = uint32_t(base_cell) + B[i] * kc + state_of(xc, i);
                if (in_lds) atomicAdd(&sh[cell], w[i]);
                else atomicAdd(&blockN[cell], w[i]);
            }
        }
        for (int g = 0; g < n_cand; ++g) {
            const uint32_t ku = uint32_t(cand_k[g]), at = uint32_t(cand_cell[g]);
            const uint2 x = *reinterpret_cast<const uint2*>(a.T + int64_t(cand_id[g]) * a.Ppad + p0);
#pragma unroll
            for (int i = 0; i < LP; ++i) {
                if (!w[i]) continue;
                const uint32_t cell = at + (B[i] * ku + state_of(x, i)) * kc + state_of(xc, i);
                if (in_lds) atomicAdd(&sh[cell], w[i]);
                else atomicAdd(&blockN[cell], w[i]);
            }
        }
    }
    __syncthreads();
    if (in_lds)
        for (int q = threadIdx.x; q < cells; q += kLearnBlock) {
            if (gridDim.y == 1) blockN[q] = sh[q];
            else if (sh[q]) atomicAdd(&blockN[q], sh[q]);
        }
}

__global__ __launch_bounds__(kLearnLanes) void learn_score_kernel(LearnArgs a, int32_t fam0) {
    __shared__ double sh[kLearnLanes];
    __shared__ unsigned long long tot[kLearnLanes];   // totals of the rows that the 256 entries in hand touch (<= 256 rows)
    const LearnFamily* __restrict__ f = a.fams + (fam0 + int32_t(blockIdx.x));
    const unsigned long long* __restrict__ N = a.N + f->count_at;
    unsigned long long* __restrict__ out = a.counts_out ? a.counts_out + f->out_at : nullptr;
    const uint32_t entries = uint32_t(f->entries), kc = uint32_t(f->kc), ku = uint32_t(f->ku), low = uint32_t(f->low);
    const uint32_t tid = threadIdx.x;
    // first counted cell of the fitted row `row`
    auto row_cell = [&](uint32_t row) {
        const uint32_t t = row / low, lo = row - t * low;
        const uint32_t hi = t / ku, su = t - hi * ku;
        return ((hi * low + lo) * ku + su) * kc;
    };
    double acc = 0.0;
    for (uint32_t r0 = 0; r0 < entries; r0 += kLearnLanes) {
        const uint32_t row0 = r0 / kc, row1 = min(r0 + kLearnLanes - 1, entries - 1) / kc;
        if (row0 + tid <= row1) {
            const uint32_t c0 = row_cell(row0 + tid);
            unsigned long long total = 0;
            for (uint32_t s = 0; s < kc; ++s) total += N[c0 + s];
            tot[tid] = total;
        }
        __syncthreads();
        const uint32_t r = r0 + tid;
        if (r < entries) {
            const uint32_t row = r / kc, s = r - row * kc;
            const unsigned long long c = N[row_cell(row) + s];
            if (out) out[r] = c;
            if (c) acc += double(c) * log(double(c) / double(tot[row - row0]));   // the division is fit_normalize_kernel's
        }
        __syncthreads();
    }
    sh[tid] = acc;
    __syncthreads();
    for (int s = kLearnLanes / 2; s > 0; s >>= 1) {
        if (int(tid) < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.ll[fam0 + blockIdx.x] = sh[0];
}

int learn_launch_count(const LearnArgs& a, int32_t chunk0, int32_t n_chunks, int splits, void* stream) {
    (void)hipGetLastError();
    if (n_chunks > 0)
        hipLaunchKernelGGL(learn_count_kernel, dim3(unsigned(n_chunks), unsigned(splits)), dim3(kLearnBlock), 0, (hipStream_t)stream, a, chunk0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

int learn_launch_score(const LearnArgs& a, int32_t fam0, int32_t n_fams, void* stream) {
    (void)hipGetLastError();
    if (n_fams > 0)
        hipLaunchKernelGGL(learn_score_kernel, dim3(unsigned(n_fams)), dim3(kLearnLanes), 0, (hipStream_t)stream, a, fam0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace bnmi
