// bn_ci.hpp -- conditional-independence tests "x _||_ y | S" from exact counts (include/bn_mi355x.h, bn_ci_tests / bn_learn_pc): the
// host-side view of the kernels in bn_ci.hip.  The counts are learn_count_kernel's (bn_learn_kernels.hip): the candidate family
// "child x, base S, candidate y" is counted candidate-last, cell (s * k_y + b) * k_x + a -- the table N[s][b][a] of the test.
#pragma once

#include <cstdint>

namespace bnmi {

constexpr int kCiLanes = 256;            // partial sums of the statistic: bn_score_nodes' order
constexpr int kCiMargCells = 4096;       // LDS: row and column sums of the strata in hand
constexpr int kCiMaxStrata = 2048;       // LDS: their totals (k_x + k_y >= 2, so strata in hand <= kCiMargCells / 2)
constexpr int kCiMaxCond = 8;            // |S|
constexpr uint32_t kCiNoRank = 0xFFFFFFFFu;

// One test as the statistic kernel reads it.
struct CiTest {
    int64_t count_at;     // first cell of N[s][b][a] in the count scratch of the pass
    int64_t out_at;       // first cell in counts_out
    int32_t cells;        // strata * ky * kx
    int32_t kx, ky;
    int32_t slot;         // where stat / df / p go
    int32_t edge;         // bn_learn_pc: the edge whose rank an independent test lowers; -1: none
    uint32_t rank;        // the test's rank among the edge's tests
};

struct CiArgs {
    const unsigned long long* N;
    const CiTest* tests;
    double* stat;                        // [slots]
    long long* df;
    double* p;
    unsigned long long* counts_out;      // or null
    uint32_t* edge_rank;                 // or null: per edge the lowest rank of an independent test (integer atomicMin)
    int32_t df_rule;                     // 0 nominal, 1 adjusted
    int32_t pad_;
    double alpha;
};

// each returns a hipError_t value (0: success)
int ci_launch_stat(const CiArgs& a, int32_t test0, int32_t n_tests, void* stream);
int ci_launch_sf(int64_t n, const double* g, const long long* df, double* p, void* stream);

}  // namespace bnmi
