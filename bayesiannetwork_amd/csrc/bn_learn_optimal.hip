// bn_learn_optimal.hip -- the kernels of exact structure learning (bn_learn_optimal of include/bn_mi355x.h; NOT IN THE REFERENCE):
//   optimal_bps_kernel   step 1, one pass of the min-zeta transform: a workgroup takes a tile of at most 2^12 cells of one child
//                        into LDS (32 KiB of costs, 16 KiB of ranks), does the butterflies of the pass's bits there and writes the
//                        tile back.  The first pass makes the cells from the term table instead of loading them.
//   optimal_sink_kernel  step 2, one popcount level: a thread per mask, the masks of another level leave at once.
//   optimal_back_kernel  step 3, one thread walks the sinks back from V and unranks the parent sets.
// Every fp64 operation is a plain one (-ffp-contract=off); min does not round and (cost, rank) is a total order, so no result
// depends on the order of the passes or of the lanes.
#include <hip/hip_runtime.h>

#include "bn_learn_optimal.hpp"

namespace bnmi {
namespace {

// does (cb, rb) come before (ca, ra)?  smaller cost first, among equal costs the smaller rank
__device__ __forceinline__ bool before(double cb, uint32_t rb, double ca, uint32_t ra) { return cb < ca || (cb == ca && rb < ra); }

// The cell of parent set c (child v's squeezed mask) before any pass: (f(v, S), rank(v, S)) where |S| <= mp, else (+inf, no rank).
// f is +inf where the term is NaN or S leaves allowed[v].  The squeezed bit positions are the rank tables' relabelled nodes.
__device__ __forceinline__ void first_cell(const OptimalBpsArgs& a, const uint32_t* s_tab, int v, int32_t kv, uint64_t allow, uint32_t c,
                                           double& cost, uint32_t& rank) {
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    if (__popc(c) > a.mp) {
        cost = inf;
        rank = kOptimalNoRank;
        return;
    }
    uint32_t r = 0, left = c;
    uint64_t pm = 0;
    int64_t rows = 1;
    int j = 0;
    while (left) {
        const int s = __ffs(int(left)) - 1;
        left &= left - 1;
        ++j;
        r += s_tab[kTermTabBinom + j * 64 + s];
        const int u = s + (s >= v ? 1 : 0);
        pm |= uint64_t(1) << u;
        if (rows <= (int64_t(1) << 20)) rows *= a.k[u];   // (a family over 2^20 entries has a NaN term: its count is not read)
    }
    r += s_tab[j];
    const double term = a.terms[int64_t(v) * a.T + r];
    double f = 0.0 - term;
    if (a.penalised) f = f + double(int64_t(kv - 1) * rows) * a.penalty;
    if (term != term || (pm & ~allow) != 0) f = inf;
    cost = f;
    rank = r;
}

__global__ __launch_bounds__(kOptimalThreads) void optimal_bps_kernel(OptimalBpsArgs a) {
    __shared__ double s_cost[1 << kOptimalTileBits];
    __shared__ uint32_t s_rank[1 << kOptimalTileBits];
    __shared__ uint32_t s_tab[kTermTabWords];
    const OptimalPass p = a.pass;
    const int v = int(blockIdx.y), tid = int(threadIdx.x);
    const uint32_t t = blockIdx.x;
    const int m = a.n - 1;
    const bool first = p.b0 == 0;
    const uint32_t cells = 1u << (p.low + p.nb);
    // the cell index of tile entry i: i's lowest `low` bits stay, the others are the cell's bits from b0; the tile number fills the rest
    const uint32_t mid_bits = uint32_t(p.b0 - p.low);
    const uint32_t fixed = ((t & ((1u << mid_bits) - 1u)) << p.low) | ((t >> mid_bits) << (p.b0 + p.nb));
    const uint32_t low_mask = (1u << p.low) - 1u;
    const size_t row = size_t(v) << m;
    if (first) {
        for (int i = tid; i < kTermTabBinom + (a.q + 1) * 64; i += kOptimalThreads) s_tab[i] = a.tab[i];
        __syncthreads();
        const int32_t kv = a.k[v];
        const uint64_t allow = a.allowed[v];
        for (uint32_t i = uint32_t(tid); i < cells; i += kOptimalThreads) first_cell(a, s_tab, v, kv, allow, fixed | i, s_cost[i], s_rank[i]);
    } else {
        for (uint32_t i = uint32_t(tid); i < cells; i += kOptimalThreads) {
            const size_t c = row + (fixed | (i & low_mask) | ((i >> p.low) << p.b0));
            s_cost[i] = a.cost[c];
            s_rank[i] = a.rank[c];
        }
    }
    // bit b of the tile index: entry i with the bit set takes the smaller of itself and i with the bit clear.  Lanes take
    // consecutive pairs, so from bit 5 up a half-wave reads 32 consecutive doubles (every bank once); below, two runs share banks.
    for (int b = p.low; b < p.low + p.nb; ++b) {
        __syncthreads();
        const uint32_t bit = 1u << b;
        for (uint32_t pr = uint32_t(tid); pr < (cells >> 1); pr += kOptimalThreads) {
            const uint32_t i = ((pr >> b) << (b + 1)) | bit | (pr & (bit - 1u));
            const double ca = s_cost[i], cb = s_cost[i ^ bit];
            const uint32_t ra = s_rank[i], rb = s_rank[i ^ bit];
            if (before(cb, rb, ca, ra)) {
                s_cost[i] = cb;
                s_rank[i] = rb;
            }
        }
    }
    __syncthreads();
    for (uint32_t i = uint32_t(tid); i < cells; i += kOptimalThreads) {
        const size_t c = row + (fixed | (i & low_mask) | ((i >> p.low) << p.b0));
        a.cost[c] = s_cost[i];
        a.rank[c] = s_rank[i];
    }
}

// R[W] = min over v in W, v ascending, of R[W \ v] + bps[v][squeeze(W \ v)].cost: one add per term, a strictly smaller value
// replaces the current one (the lowest v stays among equals); sink[W] = that v
__global__ __launch_bounds__(kOptimalThreads) void optimal_sink_kernel(OptimalSinkArgs a) {
    const uint32_t sets = 1u << a.n;
    const int m = a.n - 1;
    for (uint32_t W = blockIdx.x * kOptimalThreads + threadIdx.x; W < sets; W += gridDim.x * kOptimalThreads) {
        if (__popc(W) != a.level) continue;
        double best = 0.0;
        int sink = -1;
        uint32_t left = W;
        while (left) {
            const int v = __ffs(int(left)) - 1;
            left &= left - 1;
            const uint32_t rest = W ^ (1u << v);
            const double val = a.R[rest] + a.cost[(size_t(v) << m) + optimal_squeeze(rest, v)];
            if (sink < 0 || val < best) {
                best = val;
                sink = v;
            }
        }
        a.R[W] = best;
        a.sink[W] = uint8_t(sink);
    }
}

// the parent set of rank r among child c's, as a mask over the nodes: the size j is the last with offset[j] <= r, then the
// relabelled members from the largest down, each the largest s' with C(s', i) <= what is left
__device__ uint64_t unrank_mask(const uint32_t* tab, int n, int q, int c, uint32_t r) {
    int j = 0;
    while (j < q && tab[j + 1] <= r) ++j;
    r -= tab[j];
    uint32_t squeezed = 0;
    int s = n - 2;
    for (int i = j; i >= 1; --i) {
        while (s > i - 1 && tab[kTermTabBinom + i * 64 + s] > r) --s;
        r -= tab[kTermTabBinom + i * 64 + s];
        squeezed |= 1u << s;
        --s;
    }
    return optimal_unsqueeze(squeezed, c);
}

__global__ void optimal_back_kernel(OptimalBackArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int n = a.n, m = n - 1;
    uint32_t W = (1u << n) - 1u;
    a.value[0] = a.R[W];
    for (int i = n - 1; i >= 0; --i) {
        const int s = int(a.sink[W]);
        W ^= 1u << s;
        uint32_t r = a.rank[(size_t(s) << m) + optimal_squeeze(W, s)];
        if (int64_t(r) >= a.T) r = 0;   // (never: the empty set, rank 0, is inside every candidate set and comes before "no rank")
        a.order[i] = s;
        a.masks[s] = unrank_mask(a.tab, n, a.q, s, r);
        a.ll[s] = a.terms[int64_t(s) * a.T + r];
    }
}

}  // namespace

int learn_launch_optimal_bps(const OptimalBpsArgs& a, void* stream) {
    hipLaunchKernelGGL(optimal_bps_kernel, dim3(unsigned(a.pass.tiles), unsigned(a.n)), dim3(kOptimalThreads), 0, hipStream_t(stream), a);
    return int(hipGetLastError());
}

int learn_launch_optimal_sink(const OptimalSinkArgs& a, void* stream) {
    const unsigned blocks = unsigned(((size_t(1) << a.n) + kOptimalThreads - 1) / kOptimalThreads);
    hipLaunchKernelGGL(optimal_sink_kernel, dim3(blocks), dim3(kOptimalThreads), 0, hipStream_t(stream), a);
    return int(hipGetLastError());
}

int learn_launch_optimal_back(const OptimalBackArgs& a, void* stream) {
    hipLaunchKernelGGL(optimal_back_kernel, dim3(1), dim3(64), 0, hipStream_t(stream), a);
    return int(hipGetLastError());
}

}  // namespace bnmi
