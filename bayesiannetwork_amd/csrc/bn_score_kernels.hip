// bn_score_kernels.hip -- log-likelihood of a pattern table under a network, reference
// bayesian/evaluation/basic_info_criteria.hpp:44-78 (calc_likelihood): per distinct pattern the sum over the
// nodes of log P(state | parents' states), and per node the sum over its CPT entries of count x log entry.
// The logarithms come from the host (L = std::log of the flat CPT, bn_score.cpp): the device gathers and adds,
// in the orders include/bn_mi355x.h states, so every result can be restated bit for bit.
//
// Row kernel: the table is [node][pattern] bytes, so a lane takes kScoreLanePatterns consecutive patterns (two dwords
// of a node's row in one load: a wave load is 512 contiguous bytes) and the wave walks the nodes of a segment.  Everything about
// a node -- selected or not, parents, arities, table offset -- is the same in every lane and is read through
// uniform addresses (kernel arguments, blockIdx, loop counters): scalar loads, no vector load but the state
// dwords and the gathers from L.  The table is zero from P to Ppad and state 0 is valid for every node, so lanes
// in the padding compute like any other; a lane whose bytes would start beyond Ppad reads the last ones of the
// row instead and stores nothing.  No floating-point atomics: segment sums go to `part`, a second kernel adds
// them in segment order (or, on a long table, the workgroup walks the segments itself: the same additions).
#include <hip/hip_runtime.h>

#include "bn_score.hpp"

namespace bnmi {

// LP consecutive state bytes of a row as LP / 4 dwords, one load of 4, 8 or 16 bytes (p is a multiple of LP, the row base of 64)
template <int W>
__device__ __forceinline__ void load_states(const uint8_t* p, uint32_t (&w)[W]) {
    static_assert(W == 1 || W == 2 || W == 4, "4, 8 or 16 patterns per lane");
    if constexpr (W == 1) {
        w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else if constexpr (W == 2) {
        const uint2 x = *reinterpret_cast<const uint2*>(p);
        w[0] = x.x; w[1] = x.y;
    } else {
        const uint4 x = *reinterpret_cast<const uint4*>(p);
        w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
    }
}

template <typename Idx, bool kLoop>
__global__ __launch_bounds__(kScoreBlock) void score_rows_kernel(ScoreRowsArgs a) {
    constexpr int LP = kScoreLanePatterns;
    const int32_t* __restrict__ k = a.m.k;
    const int32_t* __restrict__ in_ptr = a.m.in_ptr;
    const int32_t* __restrict__ in_idx = a.m.in_idx;
    const int64_t* __restrict__ cpt_off = a.m.cpt_off;
    const uint32_t* __restrict__ selw = a.sel;
    const int64_t p0 = (int64_t(blockIdx.x) * kScoreBlock + threadIdx.x) * LP;
    const int64_t pl = min(p0, a.Ppad - LP);   // (Ppad is a multiple of 64: a lane's LP bytes are inside the row or beyond it, never across)
    const int s_begin = kLoop ? 0 : int(blockIdx.y), s_end = kLoop ? a.n_segs : int(blockIdx.y) + 1;
    double total[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) total[i] = 0.0;
    for (int s = s_begin; s < s_end; ++s) {
        const int v0 = a.segs[s] << kScoreSegShift;
        const int v1 = min(a.m.n, v0 + (1 << kScoreSegShift));
        double acc[LP];
#pragma unroll
        for (int i = 0; i < LP; ++i) acc[i] = 0.0;
        for (int v = v0; v < v1; ++v) {
            if (!((selw[v >> 5] >> (v & 31)) & 1u)) continue;   // wave-uniform
            const int e0 = in_ptr[v], e1 = in_ptr[v + 1];
            Idx row[LP];   // parent assignment, first parent most significant
#pragma unroll
            for (int i = 0; i < LP; ++i) row[i] = 0;
            for (int e = e0; e < e1; ++e) {
                const int u = in_idx[e];
                const uint32_t ku = uint32_t(k[u]);
                uint32_t w[LP / 4];
                load_states(a.T + int64_t(u) * a.Ppad + pl, w);
#pragma unroll
                for (int i = 0; i < LP; ++i) row[i] = row[i] * ku + ((w[i / 4] >> (8 * (i % 4))) & 255u);
            }
            const uint32_t kv = uint32_t(k[v]);
            uint32_t w[LP / 4];
            load_states(a.T + int64_t(v) * a.Ppad + pl, w);
            const double* __restrict__ Lv = a.m.L + cpt_off[v];
#pragma unroll
            for (int i = 0; i < LP; ++i) acc[i] += Lv[row[i] * kv + ((w[i / 4] >> (8 * (i % 4))) & 255u)];
        }
        if (kLoop) {
#pragma unroll
            for (int i = 0; i < LP; ++i) total[i] += acc[i];
        } else if (p0 < a.Ppad) {
            double* dst = a.part + int64_t(s) * a.Ppad + p0;
#pragma unroll
            for (int i = 0; i < LP; ++i) dst[i] = acc[i];
        }
    }
    if (kLoop && p0 < a.Ppad) {
#pragma unroll
        for (int i = 0; i < LP; ++i) a.out[p0 + i] = total[i];
    }
}

// out[p] = the segment sums of pattern p added in increasing segment order, from +0.0
__global__ __launch_bounds__(kScoreBlock) void score_rows_reduce_kernel(const double* __restrict__ part, int32_t n_segs, int64_t Ppad,
                                                                       double* __restrict__ out) {
    const int64_t p = int64_t(blockIdx.x) * kScoreBlock + threadIdx.x;
    if (p >= Ppad) return;
    double t = 0.0;
    for (int s = 0; s < n_segs; ++s) t += part[int64_t(s) * Ppad + p];
    out[p] = t;
}

// One workgroup per node.  Thread t adds the terms double(N) * L of the node's entries r = t, t + 256, ... (r counted
// from the node's first entry) in increasing r from +0.0, skipping N == 0; the 256 partial sums are then folded
// by halves: for s = 128, 64, ..., 1: partial[t] += partial[t + s] (t < s).
__global__ __launch_bounds__(kScoreNodeLanes) void score_nodes_kernel(ScoreModel m, const unsigned long long* __restrict__ N,
                                                                      double* __restrict__ ll_node) {
    __shared__ double sh[kScoreNodeLanes];
    const int v = blockIdx.x;
    const int64_t o0 = m.cpt_off[v], csz = m.cpt_off[v + 1] - o0;
    double acc = 0.0;
    for (int64_t r = threadIdx.x; r < csz; r += kScoreNodeLanes) {
        const unsigned long long c = N[o0 + r];
        if (c) acc += double(c) * m.L[o0 + r];
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kScoreNodeLanes / 2; s > 0; s >>= 1) {
        if (int(threadIdx.x) < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) ll_node[v] = sh[0];
}

int score_launch_rows(const ScoreRowsArgs& a, bool wide, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    const int64_t tiles = (a.Ppad + kScoreTile - 1) / kScoreTile;
    if (score_rows_loop(a.n_segs, a.Ppad)) {
        if (wide) hipLaunchKernelGGL((score_rows_kernel<uint64_t, true>), dim3(unsigned(tiles)), dim3(kScoreBlock), 0, s, a);
        else hipLaunchKernelGGL((score_rows_kernel<uint32_t, true>), dim3(unsigned(tiles)), dim3(kScoreBlock), 0, s, a);
    } else {
        if (wide) hipLaunchKernelGGL((score_rows_kernel<uint64_t, false>), dim3(unsigned(tiles), a.n_segs), dim3(kScoreBlock), 0, s, a);
        else hipLaunchKernelGGL((score_rows_kernel<uint32_t, false>), dim3(unsigned(tiles), a.n_segs), dim3(kScoreBlock), 0, s, a);
        hipLaunchKernelGGL(score_rows_reduce_kernel, dim3(unsigned((a.Ppad + kScoreBlock - 1) / kScoreBlock)), dim3(kScoreBlock), 0, s,
                           a.part, a.n_segs, a.Ppad, a.out);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

int score_launch_nodes(const ScoreModel& m, const unsigned long long* N, double* ll_node, void* stream) {
    (void)hipGetLastError();
    if (m.n > 0) hipLaunchKernelGGL(score_nodes_kernel, dim3(m.n), dim3(kScoreNodeLanes), 0, (hipStream_t)stream, m, N, ll_node);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace bnmi
