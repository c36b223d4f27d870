// bn_learn_optimal_plan.hpp -- what bn_learn_optimal decides before it touches the device, as pure functions of (n, the bounds, the
// allowed masks): the limit checks and their texts, the in-degree bound, the cell and byte counts and the schedule of the min-zeta
// passes.  No HIP: bn_learn_optimal_plan.cpp is also compiled alone by tests/cpp/test_optimal_plan.cpp.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bn_learn_optimal.hpp"

namespace bn_eng __attribute__((visibility("hidden"))) {
int fail(int code, const std::string& msg);   // bn_last_error (bn_engine.cpp; the stand-alone test has its own)
}  // namespace bn_eng

#pragma GCC visibility push(hidden)   // (internal to the library: nothing here is part of its surface)
namespace bnmi {

struct OptimalPlan {
    int32_t n = 0, mp = 0;
    int64_t cells = 0;            // n * 2^(n - 1): the best-parent-set cells
    int64_t sets = 0;             // 2^n
    int64_t cost_bytes = 0, rank_bytes = 0, r_bytes = 0, sink_bytes = 0;
    int64_t bytes = 0;            // their sum: 12 per cell and 9 per set
    std::vector<OptimalPass> passes;   // every bit of [0, n - 1) in exactly one pass, in increasing order
};

// The checks, in this order: 1 <= n <= 24; max_parents >= 1; no bit at or above n in allowed[v] (allowed: NULL or [n]).  mp =
// min(max_parents, q, learner_max_parents).  BN_OK, or what bn_eng::fail returned (BN_ERR_ARG): nothing of `out` is then to be used.
int plan_optimal(int32_t n, int32_t max_parents, int32_t q, int32_t learner_max_parents, const uint64_t* allowed, OptimalPlan& out);

}  // namespace bnmi
#pragma GCC visibility pop
