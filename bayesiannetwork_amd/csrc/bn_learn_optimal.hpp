// bn_learn_optimal.hpp -- exact structure learning by dynamic programming over node subsets (Silander & Myllymaki 2006): the
// limits, the index of a candidate set, the pass schedule's record and the argument structs of the three kernels in
// bn_learn_optimal.hip.  The C ABI (bn_learn_optimal of include/bn_mi355x.h) is in bn_learn_search.cpp, the host-only planning in
// bn_learn_optimal_plan.cpp.  No HIP include: the planner and its stand-alone test read this file too.
#pragma once

#include <cstdint>

#include "bn_learn_terms.hpp"

#if defined(__HIPCC__)
#define BN_OPT_HD __host__ __device__
#else
#define BN_OPT_HD
#endif

namespace bnmi {

constexpr int kOptimalMaxNodes = 24;    // 24 * 2^23 cells of 12 bytes and 2^24 sets of 9: 2.4 GB
constexpr int kOptimalTileBits = 12;    // a tile: 2^12 cells, 32 KiB of costs and 16 KiB of ranks in LDS
constexpr int kOptimalLowBits = 4;      // a strided tile keeps the 2^4 lowest cells together: 128 bytes of costs per row
constexpr int kOptimalThreads = 256;
constexpr uint32_t kOptimalNoRank = 0xFFFFFFFFu;

// the candidate set C (a mask over the nodes, bit v clear) as child v's cell index: bit v squeezed out, s' = s - (s > v)
BN_OPT_HD inline uint32_t optimal_squeeze(uint32_t C, int v) { return (C & ((1u << v) - 1u)) | ((C >> (v + 1)) << v); }
// ... and back: the mask over the nodes of cell c of child v
BN_OPT_HD inline uint32_t optimal_unsqueeze(uint32_t c, int v) { return (c & ((1u << v) - 1u)) | ((c >> v) << (v + 1)); }

// One pass of the min-zeta transform over a child's 2^m cells (m = n - 1): a workgroup takes a tile of 2^(low + nb) cells, all
// combinations of the cell index's bits [0, low) and [b0, b0 + nb), and does the butterflies of the nb bits from b0 there.  The
// first pass (low 0, b0 0) also initialises the cells.  Tile t of a child: the bits [low, b0) of the cell index are t's lowest
// b0 - low bits, the bits from b0 + nb up are the rest of t.
struct OptimalPass {
    int32_t low, b0, nb;
    int32_t tiles;        // per child: 2^(m - low - nb)
};

struct OptimalBpsArgs {
    const double* terms;        // [n][T]
    const uint32_t* tab;        // [kTermTabWords]
    int64_t T;
    const int32_t* k;           // [n] arities
    const uint64_t* allowed;    // [n]: bit u of allowed[v]: u may be a parent of v (all ones where the call gave none)
    int32_t n, q, mp;
    int32_t penalised;          // AIC / MDL: the cost carries double(dp) * penalty
    double penalty;
    double* cost;               // [n][2^(n - 1)]
    uint32_t* rank;             // [n][2^(n - 1)]
    OptimalPass pass;
};

struct OptimalSinkArgs {
    const double* cost;         // [n][2^(n - 1)]
    double* R;                  // [2^n]
    uint8_t* sink;              // [2^n]
    int32_t n, level;           // the sets of `level` nodes
};

struct OptimalBackArgs {
    const double* terms;
    const uint32_t* tab;
    int64_t T;
    const uint32_t* rank;       // [n][2^(n - 1)]
    const double* R;
    const uint8_t* sink;
    int32_t n, q;
    int32_t* order;             // [n] parents first
    uint64_t* masks;            // [n] parent masks
    double* ll;                 // [n] family terms
    double* value;              // [1] R[V]
};

// each returns a hipError_t value (0: success)
int learn_launch_optimal_bps(const OptimalBpsArgs& a, void* stream);
int learn_launch_optimal_sink(const OptimalSinkArgs& a, void* stream);
int learn_launch_optimal_back(const OptimalBackArgs& a, void* stream);

}  // namespace bnmi
