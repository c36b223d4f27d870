// bn_learn_bd.hip -- the Bayesian-Dirichlet form of learn_score_kernel (bn_learn_kernels.hip): per family the log marginal
// likelihood of its counts under a Dirichlet prior, BDeu (kind 2, equivalent sample size ess) or K2 (kind 3, Cooper-Herskovits).
//
// For a family of child arity kc with R parent configurations (all of them, observed or not) and E = R * kc entries:
//   BDeu: a_r = ess / double(R), a_c = ess / double(E);   K2: a_c = 1.0, a_r = double(kc)
//   G_r = lgamma_pos(a_r), G_c = lgamma_pos(a_c), once per family
//   entry r (row j, state s, count N, row total tot): t_r = 0.0; N != 0: t_r = lgamma_pos(a_c + double(N)) - G_c;
//                                                     s == 0 and tot != 0: t_r = t_r + (G_r - lgamma_pos(a_r + double(tot)))
//   bd = the sum of t_r in learn_score_kernel's order: thread t adds r = t, t + 256, ... from +0.0, the 256 partial sums folded by halves.
// lgamma_pos is the stated function of bn_learn_dev.hpp; the result depends on the family's counts and (kind, ess) alone.  Same
// shape as learn_score_kernel: one workgroup per family, row totals of the 256 entries in hand in LDS, the optional fitted-layout
// copy of the counts, no floating-point atomics.
#include <hip/hip_runtime.h>

#include "bn_learn.hpp"
#include "bn_learn_dev.hpp"

namespace bnmi {

__global__ __launch_bounds__(kLearnLanes) void learn_score_bd_kernel(LearnArgs a, int32_t fam0, int32_t kind, double ess) {
    __shared__ double sh[kLearnLanes];
    __shared__ unsigned long long tot[kLearnLanes];   // totals of the rows that the 256 entries in hand touch (<= 256 rows)
    __shared__ double prior[4];                       // a_r, a_c, G_r, G_c
    const LearnFamily* __restrict__ f = a.fams + (fam0 + int32_t(blockIdx.x));
    const unsigned long long* __restrict__ N = a.N + f->count_at;
    unsigned long long* __restrict__ out = a.counts_out ? a.counts_out + f->out_at : nullptr;
    const uint32_t entries = uint32_t(f->entries), kc = uint32_t(f->kc), ku = uint32_t(f->ku), low = uint32_t(f->low);
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        double a_r, a_c;
        if (kind == 2) {
            a_r = ess / double(entries / kc);
            a_c = ess / double(entries);
        } else {
            a_c = 1.0;
            a_r = double(kc);
        }
        prior[0] = a_r;
        prior[1] = a_c;
        prior[2] = lgamma_pos(a_r);
        prior[3] = lgamma_pos(a_c);
    }
    __syncthreads();
    const double a_r = prior[0], a_c = prior[1], G_r = prior[2], G_c = prior[3];
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
            double t = 0.0;
            if (c) t = lgamma_pos(a_c + double(c)) - G_c;
            if (s == 0) {
                const unsigned long long total = tot[row - row0];
                if (total) t = t + (G_r - lgamma_pos(a_r + double(total)));
            }
            acc += t;
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

int learn_launch_score_bd(const LearnArgs& a, int32_t fam0, int32_t n_fams, int32_t kind, double ess, void* stream) {
    (void)hipGetLastError();
    if (n_fams > 0)
        hipLaunchKernelGGL(learn_score_bd_kernel, dim3(unsigned(n_fams)), dim3(kLearnLanes), 0, (hipStream_t)stream, a, fam0, kind, ess);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace bnmi
