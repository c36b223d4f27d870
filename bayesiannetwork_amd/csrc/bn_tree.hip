// bn_tree.hip -- maximum spanning tree of a dense symmetric weight matrix: Prim's algorithm in one workgroup (bn_tree_max_spanning,
// bn_learn_tree).  DESIGN.md "Chow-Liu and TAN trees".
//
// Edge order (include/bn_mi355x.h): weight descending, then (min(u, v), max(u, v)) ascending; -0.0 == 0.0.  The order is total and
// strict over distinct edges, so the maximum spanning tree is unique and Prim -- which adds, at every step, the first edge under that
// order that leaves the tree -- finds it from any root.
//
// key[x] / from[x]: the first edge under the order from the tree to the non-tree node x.  Node x belongs to thread x mod blockDim:
// that thread alone reads and writes key[x], from[x] and in_tree[x], so a step needs one barrier, the one of the argmax.
#include <hip/hip_runtime.h>

#include <climits>

#include "bn_tree.hpp"

namespace bnmi {

namespace {

// an edge's rank among equal weights, and which end is outside the tree: ((lo << 12 | hi) << 1) | (outside == hi)
__device__ __forceinline__ int edge_code(int in, int out) {
    const int lo = in < out ? in : out, hi = in < out ? out : in;
    return (((lo << 12) | hi) << 1) | int(out == hi);
}

__device__ __forceinline__ bool edge_before(double wa, int ca, double wb, int cb) { return wa > wb || (wa == wb && ca < cb); }

__global__ __launch_bounds__(kTreeMaxThreads) void tree_prim(const double* __restrict__ w, int32_t m, int32_t root,
                                                             int32_t* __restrict__ parent, double* __restrict__ weight) {
    __shared__ double key[kTreeMaxNodes];
    __shared__ int32_t from[kTreeMaxNodes];
    __shared__ uint8_t in_tree[kTreeMaxNodes];
    __shared__ double red_w[2][kTreeMaxThreads / 64];
    __shared__ int red_c[2][kTreeMaxThreads / 64];
    const int nt = int(blockDim.x), tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6, nwaves = nt >> 6;
    const double ninf = -__builtin_huge_val();

    for (int x = tid; x < m; x += nt) {
        key[x] = x == root ? 0.0 : w[int64_t(root) * m + x];
        from[x] = root;
        in_tree[x] = uint8_t(x == root);
    }
    if (tid == 0) {
        parent[root] = -1;
        if (weight) weight[root] = 0.0;
    }
    for (int step = 1; step < m; ++step) {
        double bw = ninf;   // (a real edge of weight -inf has a code below INT_MAX)
        int bc = INT_MAX;
        for (int x = tid; x < m; x += nt) {
            if (in_tree[x]) continue;
            const double kw = key[x];
            const int c = edge_code(from[x], x);
            if (edge_before(kw, c, bw, bc)) { bw = kw; bc = c; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double ow = __shfl_xor(bw, off, 64);
            const int oc = __shfl_xor(bc, off, 64);
            if (edge_before(ow, oc, bw, bc)) { bw = ow; bc = oc; }
        }
        const int slot = step & 1;   // (two sets of slots: a wave may write step + 1's while another still reads step's)
        if (lane == 0) { red_w[slot][wave] = bw; red_c[slot][wave] = bc; }
        __syncthreads();
        bw = red_w[slot][0];
        bc = red_c[slot][0];
        for (int i = 1; i < nwaves; ++i) {
            const double ow = red_w[slot][i];
            const int oc = red_c[slot][i];
            if (edge_before(ow, oc, bw, bc)) { bw = ow; bc = oc; }
        }
        if (bc == INT_MAX) break;   // (no node left: cannot happen in m - 1 steps)
        const int hi = (bc >> 1) & (kTreeMaxNodes - 1), lo = bc >> 13;
        const int v = (bc & 1) ? hi : lo;
        if (tid == v % nt) {
            in_tree[v] = 1;
            parent[v] = from[v];
            if (weight) weight[v] = key[v];
        }
        const double* __restrict__ row = w + int64_t(v) * m;
        for (int x = tid; x < m; x += nt) {
            if (in_tree[x]) continue;   // (v itself: its owner has just marked it)
            const double nw = row[x];
            if (edge_before(nw, edge_code(v, x), key[x], edge_code(from[x], x))) {
                key[x] = nw;
                from[x] = v;
            }
        }
    }
}

}  // namespace

int tree_launch_prim(const double* w, int32_t m, int32_t root, int32_t* parent, double* weight, void* stream) {
    hipLaunchKernelGGL(tree_prim, dim3(1), dim3(unsigned(tree_threads(m))), 0, hipStream_t(stream), w, m, root, parent, weight);
    return int(hipGetLastError());
}

}  // namespace bnmi
