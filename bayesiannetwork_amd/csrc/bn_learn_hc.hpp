// bn_learn_hc.hpp -- hierarchical-clustering stepwise structure search over a precomputed table of family terms (reference
// bayesian/learning/stepwise_structure_hc.hpp).  Host-side view of the kernel in bn_learn_hc.hip; the C ABI (bn_learn_hc of
// include/bn_mi355x.h) is in bn_learn_search.cpp.  The term table and its rank tables are bn_learn_terms.hpp's.
#pragma once

#include "bn_learn_search.hpp"

namespace bnmi {

constexpr int kHcWaves = 2;                  // runs per workgroup (the LDS budget: DESIGN 4.14)
constexpr int kHcMaxSims = 2016;             // C(64, 2): the similarity list never holds more than C(live clusters, 2) entries
constexpr int kHcMaxIds = 128;               // cluster ids 0 .. 2n - 2 <= 126
// node lists of every cluster ever made: n singletons, then per merge the merged list; the sum over the merges of the merged
// sizes is largest when one cluster takes a singleton at a time: 2 + 3 + ... + 64 = 2 079
constexpr int kHcNodeBytes = 64 + 2079 + 33; // = 2 176

constexpr uint32_t kHcOneCluster = 1, kHcNoSimilarity = 2;

struct HcRecord {         // per run
    double score;         // the learner's score of the final graph
    uint32_t merges, tried, kept, pruned, pairs_kept, flags;
    uint32_t visits, pad_;
};

struct HcTrace {          // per merge (kind 0) and per pruning visit (kind 1) of the traced run, in the order they happen
    uint64_t value_bits;  // merge: the similarity of the merged pair; visit: make_similarity(new, cluster)
    uint8_t kind, a, b, c;   // merge: parent id, child id, coin; visit: cluster id, connections, pruned
    uint32_t pad_;
};

struct HcArgs : SearchArgs {    // (params0: of the empty graph)
    const double* S;            // [n][n] similarities, read as S[l][r]: l from make_similarity's first cluster
    double alpha, average;
    HcRecord* rec;              // [runs]
    HcTrace* trace;             // null, or [trace_cap]
};

// returns a hipError_t value (0: success)
int learn_launch_hc(const HcArgs& a, void* stream);

}  // namespace bnmi
