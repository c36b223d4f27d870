// bn_tree.hpp -- maximum spanning tree of a dense weight matrix on the device (bn_tree_max_spanning and bn_learn_tree of
// include/bn_mi355x.h, which states the edge order).  Host-side view of the kernel in bn_tree.hip; the C ABI is in bn_learn_tree.cpp.
#pragma once

#include <cstdint>

namespace bnmi {

constexpr int32_t kTreeMaxNodes = 4096;        // key / from / in_tree of every node in one workgroup's LDS
constexpr int kTreeMaxThreads = 1024;

// threads of the one workgroup for m nodes: whole waves, at most kTreeMaxThreads
inline int tree_threads(int32_t m) {
    const int t = (m + 63) / 64 * 64;
    return t < 64 ? 64 : (t > kTreeMaxThreads ? kTreeMaxThreads : t);
}

// Prim from `root` over w [m][m] (device, symmetric: row u is read for u's edges), 2 <= m <= kTreeMaxNodes, 0 <= root < m, no NaN.
// parent [m] (device): the neighbour on the path to root, -1 at root; weight [m] (device, may be null): w[v][parent[v]], 0.0 at root.
// Returns a hipError_t value (0: success).
int tree_launch_prim(const double* w, int32_t m, int32_t root, int32_t* parent, double* weight, void* stream);

}  // namespace bnmi
