// bn_learn_lattice.hip -- the subset lattice under exhaustive parent-set search (reference bayesian/learning/brute_force.hpp,
// stepwise_structure.hpp): the exact counts of  base + S  for EVERY subset S of m candidates, made from the counts of the one top
// family  base + all candidates  that learn_count_kernel counted.  A family's counts are the top family's with the absent
// candidates summed out; uint64 sums are exact, so every family has the counts -- and through learn_score_kernel the bits --
// it has when it is counted from the pattern table by itself.  Integer adds only; no atomics at all (every output cell has one
// writer).
//
// Summing a variable x out of a table laid out [variables above x][x][variables below x, child state]:
//     out[h * inner + l] = sum over s < k_x of in[(h * k_x + s) * inner + l],     inner = cells below x.
// Consecutive threads take consecutive output cells, so a wave reads k_x runs of `inner`-long contiguous cells.  Both forms sum
// the absent candidate with the SMALLEST id (the most significant one) first: that is the choice with the largest `inner`.
//
// One-launch form (top family <= kLearnLdsCells cells).  A workgroup copies the top table into LDS once (32 KiB) and then makes the
// families mask = blockIdx.x, + gridDim.x, ...: per family it sums the absent candidates out one after another, the steps
// separated by workgroup barriers.  The first step reads the top table and writes at most half of it, every step at most half of
// the one before, so the steps alternate between two LDS buffers of 2 048 and 1 024 cells and the last step writes the family in
// device memory.  A candidate of arity 1 changes nothing in the layout and is passed over.  A family costs at most 2 x 4 096
// cell reads from LDS whatever m is; the alternative -- deriving each family from a neighbour one level up -- would need the
// level (up to C(m, m/2) tables) in LDS or one launch per level, and at this size the launches are what costs.
//
// Per-level form (larger top families).  One launch per number of absent candidates; family S is derived from S + x, x the absent
// candidate with the smallest id, which the level before wrote in device memory (L2-resident at these sizes: all 2^m tables fit
// kLearnMaxScratchCells).  Grid = (blocks over the cells, families of the level).
#include <hip/hip_runtime.h>

#include "bn_learn.hpp"

namespace bnmi {

constexpr int kLatticeBufA = kLearnLdsCells / 2, kLatticeBufB = kLearnLdsCells / 4;

__global__ __launch_bounds__(kLearnBlock) void learn_lattice_lds_kernel(LatticeLds a) {
    __shared__ unsigned long long top[kLearnLdsCells];
    __shared__ unsigned long long buf_a[kLatticeBufA];
    __shared__ unsigned long long buf_b[kLatticeBufB];
    const uint32_t tid = threadIdx.x, top_cells = uint32_t(a.top_cells);
    const int32_t full = a.n_fams - 1;
    {
        const unsigned long long* __restrict__ src = a.N + a.fams[full].count_at;
        for (uint32_t q = tid; q < top_cells; q += kLearnBlock) top[q] = src[q];
    }
    __syncthreads();
    for (int32_t mask = int32_t(blockIdx.x); mask < full; mask += int32_t(gridDim.x)) {   // (the top family is in place)
        unsigned long long* __restrict__ out = a.N + a.fams[mask].count_at;
        int left = 0;   // steps to take: absent candidates of arity > 1
        for (int p = 0; p < a.nv; ++p)
            if (a.bit[p] >= 0 && !((mask >> a.bit[p]) & 1) && a.k[p] > 1) ++left;
        if (left == 0) {   // the top family itself, up to variables with one state
            for (uint32_t q = tid; q < top_cells; q += kLearnBlock) out[q] = top[q];
            continue;
        }
        const unsigned long long* src = top;
        uint32_t outer = 1, inner = top_cells;
        int step = 0;
        for (int p = 0; p < a.nv; ++p) {
            const uint32_t kx = uint32_t(a.k[p]);
            inner /= kx;   // cells below position p: every variable there is still in the table
            const bool absent = a.bit[p] >= 0 && !((mask >> a.bit[p]) & 1);
            if (!absent) outer *= kx;
            if (!absent || kx == 1) continue;
            const uint32_t cells = outer * inner;   // (<= the source's cells / 2)
            --left;
            unsigned long long* dst = left == 0 ? out : (step & 1) ? buf_b : buf_a;
            for (uint32_t o = tid; o < cells; o += kLearnBlock) {
                const uint32_t h = o / inner, l = o - h * inner;
                const unsigned long long* in = src + (h * kx) * inner + l;
                unsigned long long sum = 0;
                for (uint32_t s = 0; s < kx; ++s) sum += in[s * inner];
                dst[o] = sum;
            }
            __syncthreads();   // the next step reads what this one wrote; the next family overwrites what this one read
            src = dst;
            ++step;
        }
    }
}

__global__ __launch_bounds__(kLearnBlock) void learn_lattice_level_kernel(unsigned long long* __restrict__ N, const LatticeStep* __restrict__ steps,
                                                                          int32_t step0) {
    const LatticeStep* __restrict__ st = steps + (step0 + int32_t(blockIdx.y));
    const uint32_t cells = uint32_t(st->cells), inner = uint32_t(st->inner), kx = uint32_t(st->kx);
    const unsigned long long* __restrict__ in = N + st->in_at;
    unsigned long long* __restrict__ out = N + st->out_at;
    for (uint32_t o = blockIdx.x * kLearnBlock + threadIdx.x; o < cells; o += gridDim.x * kLearnBlock) {
        const uint32_t h = o / inner, l = o - h * inner;
        const unsigned long long* __restrict__ p = in + size_t(h * kx) * inner + l;
        unsigned long long sum = 0;
        for (uint32_t s = 0; s < kx; ++s) sum += p[size_t(s) * inner];
        out[o] = sum;
    }
}

int learn_launch_lattice_lds(const LatticeLds& a, int blocks, void* stream) {
    (void)hipGetLastError();
    if (a.n_fams > 1 && blocks > 0)
        hipLaunchKernelGGL(learn_lattice_lds_kernel, dim3(unsigned(blocks)), dim3(kLearnBlock), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

int learn_launch_lattice_level(unsigned long long* N, const LatticeStep* steps, int32_t step0, int32_t n_steps, int32_t max_cells, void* stream) {
    (void)hipGetLastError();
    if (n_steps > 0) {
        // four cells per thread where the tables are large; a level has at most C(16, 8) = 12 870 families (grid y <= 65 535)
        const unsigned bx = unsigned(std::max(1, std::min(1024, (max_cells + 4 * kLearnBlock - 1) / (4 * kLearnBlock))));
        hipLaunchKernelGGL(learn_lattice_level_kernel, dim3(bx, unsigned(n_steps)), dim3(kLearnBlock), 0, (hipStream_t)stream, N, steps, step0);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace bnmi
