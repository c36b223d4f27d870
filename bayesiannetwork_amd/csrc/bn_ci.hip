// bn_ci.hip -- the statistic / p-value / decision kernel of the conditional-independence tests (include/bn_mi355x.h, bn_ci_tests and
// bn_learn_pc), and the chi-square tail alone (bn_ci_chisq_sf).
//
// One workgroup per test.  The test's table N[s][b][a] (s the stratum over the sorted conditioning set, b the state of y, a the state
// of x, least significant) lies in the count scratch as learn_count_kernel left it.  The strata are taken in runs whose row and
// column sums fit kCiMargCells of LDS: thread-per-sum integer additions (exact, no atomics), then the stratum totals and the
// adjusted degrees of freedom, then the terms.  Thread t adds the terms of the cells r = t, t + 256, ... in increasing r from +0.0
// whatever the runs are (a run's first cell need not be a multiple of 256), and the 256 partial sums are folded by halves:
// bn_score_nodes' order, so G is a function of the counts alone.  Thread 0 then takes the tail (bn_ci_dev.hpp) and, for
// bn_learn_pc, lowers the edge's rank by an integer atomicMin when the test is independent.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include "bn_ci.hpp"
#include "bn_ci_dev.hpp"

namespace bnmi {

__global__ __launch_bounds__(kCiLanes) void ci_stat_kernel(CiArgs a, int32_t test0) {
    __shared__ unsigned long long marg[kCiMargCells];   // per stratum in hand: ky row sums R[b], then kx column sums C[a]
    __shared__ unsigned long long tot[kCiMaxStrata];    // N_s
    __shared__ double part[kCiLanes];
    __shared__ long long dfs[kCiLanes];
    const CiTest* __restrict__ t = a.tests + (test0 + int32_t(blockIdx.x));
    const unsigned long long* __restrict__ N = a.N + t->count_at;
    unsigned long long* __restrict__ out = a.counts_out ? a.counts_out + t->out_at : nullptr;
    const uint32_t kx = uint32_t(t->kx), ky = uint32_t(t->ky), kxy = kx * ky, per = kx + ky;
    const uint32_t strata = uint32_t(t->cells) / kxy;
    const uint32_t run = min(strata, uint32_t(kCiMargCells) / per);   // (per <= 510: at least 8 strata; at most kCiMaxStrata)
    const uint32_t tid = threadIdx.x;
    double acc = 0.0;
    long long dfa = 0;
    for (uint32_t s0 = 0; s0 < strata; s0 += run) {
        const uint32_t g = min(run, strata - s0);
        for (uint32_t m = tid; m < g * per; m += kCiLanes) {
            const uint32_t sl = m / per, j = m - sl * per;
            const unsigned long long* __restrict__ cell = N + (s0 + sl) * kxy;
            unsigned long long sum = 0;
            if (j < ky)
                for (uint32_t x = 0; x < kx; ++x) sum += cell[j * kx + x];
            else
                for (uint32_t y = 0; y < ky; ++y) sum += cell[y * kx + (j - ky)];
            marg[m] = sum;
        }
        __syncthreads();
        for (uint32_t sl = tid; sl < g; sl += kCiLanes) {
            unsigned long long total = 0;
            int rows = 0, cols = 0;
            for (uint32_t y = 0; y < ky; ++y) {
                const unsigned long long v = marg[sl * per + y];
                total += v;
                rows += v != 0;
            }
            for (uint32_t x = 0; x < kx; ++x) cols += marg[sl * per + ky + x] != 0;
            tot[sl] = total;
            if (total) dfa += (long long)(rows - 1) * (cols - 1);
        }
        __syncthreads();
        const uint32_t r_lo = s0 * kxy, r_hi = (s0 + g) * kxy;
        for (uint32_t r = r_lo + ((tid - r_lo) & (kCiLanes - 1)); r < r_hi; r += kCiLanes) {
            const uint32_t s = r / kxy, rem = r - s * kxy, y = rem / kx, x = rem - y * kx, sl = s - s0;
            const unsigned long long c = N[r];
            if (out) out[r] = c;
            if (c) {
                const double num = double(c) * double(tot[sl]);
                const double den = double(marg[sl * per + y]) * double(marg[sl * per + ky + x]);
                acc += double(c) * log(num / den);
            }
        }
        __syncthreads();
    }
    part[tid] = acc;
    dfs[tid] = dfa;
    __syncthreads();
    for (int s = kCiLanes / 2; s > 0; s >>= 1) {
        if (int(tid) < s) {
            part[tid] += part[tid + s];
            dfs[tid] += dfs[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double stat = 2.0 * part[0];
        if (!(stat > 0.0)) stat = 0.0;   // (a rounding below zero, and -0.0)
        const long long df = a.df_rule == 0 ? (long long)(kx - 1) * (long long)(ky - 1) * (long long)strata : dfs[0];
        const double p = chisq_sf(stat, df);
        a.stat[t->slot] = stat;
        a.df[t->slot] = df;
        a.p[t->slot] = p;
        if (a.edge_rank && t->edge >= 0 && p > a.alpha) atomicMin(&a.edge_rank[t->edge], t->rank);
    }
}

__global__ __launch_bounds__(kCiLanes) void ci_sf_kernel(int64_t n, const double* __restrict__ g, const long long* __restrict__ df,
                                                        double* __restrict__ p) {
    const int64_t i = int64_t(blockIdx.x) * kCiLanes + threadIdx.x;
    if (i < n) p[i] = chisq_sf(g[i], df[i]);
}

int ci_launch_stat(const CiArgs& a, int32_t test0, int32_t n_tests, void* stream) {
    (void)hipGetLastError();
    if (n_tests > 0) hipLaunchKernelGGL(ci_stat_kernel, dim3(unsigned(n_tests)), dim3(kCiLanes), 0, (hipStream_t)stream, a, test0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

int ci_launch_sf(int64_t n, const double* g, const long long* df, double* p, void* stream) {
    (void)hipGetLastError();
    if (n > 0)
        hipLaunchKernelGGL(ci_sf_kernel, dim3(unsigned((n + kCiLanes - 1) / kCiLanes)), dim3(kCiLanes), 0, (hipStream_t)stream, n, g, df, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace bnmi
