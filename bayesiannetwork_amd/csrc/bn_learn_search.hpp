// bn_learn_search.hpp -- the run frame of the searches over a term table (annealing, hierarchical clustering, hill climbing): what
// every kernel is given and every host entry fills alike (SearchRun, bn_learn_search.cpp).  One wave per run, lane v = node v; each
// search's own header builds its argument struct on these.
#pragma once

#include <cstdint>

#include "bn_learn_terms.hpp"

namespace bnmi {

constexpr int kSearchMaxRuns = 1 << 16;

struct SearchArgs {
    const double* terms;        // [n][T]
    const uint32_t* tab;        // [kTermTabWords]
    int64_t T;
    const int32_t* k;           // [n] arities
    int32_t n, q, max_parents;  // q: the table's bound (the rank tables); max_parents <= q: what a run refuses at
    int32_t criterion;
    int64_t params0;            // parameters of the starting graph
    double penalty;
    uint32_t seed_lo, seed_hi;
    int32_t runs;
    int32_t trace_run;          // -1: none
    uint32_t trace_cap;
    uint64_t* masks;            // [runs][n] parent masks of the graph a run ends with
    double* ll;                 // [runs][n] its family terms
};

struct StartGraph {             // [n] each: parent masks, row products, family terms
    const uint64_t* pmask0;
    const int64_t* rows0;
    const double* ll0;
};

}  // namespace bnmi
