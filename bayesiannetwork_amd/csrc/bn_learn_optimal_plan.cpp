// bn_learn_optimal_plan.cpp -- the host-only planning of bn_learn_optimal_plan.hpp.  Pure functions: no HIP call, no device state.
// The error texts and the order of the checks are the C ABI's (include/bn_mi355x.h, bn_learn_optimal).
#include "bn_learn_optimal_plan.hpp"

#include <algorithm>

#include "../../include/bn_mi355x.h"

namespace bnmi {

int plan_optimal(int32_t n, int32_t max_parents, int32_t q, int32_t learner_max_parents, const uint64_t* allowed, OptimalPlan& out) {
    using bn_eng::fail;
    if (n < 1 || n > kOptimalMaxNodes)
        return fail(BN_ERR_ARG, "optimal: " + std::to_string(n) + " nodes (1 .. " + std::to_string(kOptimalMaxNodes) +
                                    ": the tables hold n * 2^(n - 1) cells of 12 bytes and 2^n sets of 9)");
    if (max_parents < 1) return fail(BN_ERR_ARG, "optimal: max_parents " + std::to_string(max_parents) + " (at least 1)");
    for (int32_t v = 0; allowed && v < n; ++v)
        if (n < 64 && (allowed[v] >> n) != 0)
            return fail(BN_ERR_ARG, "optimal: allowed[" + std::to_string(v) + "] names a node at or above " + std::to_string(n));
    out = OptimalPlan{};
    out.n = n;
    out.mp = std::min(max_parents, std::min(q, learner_max_parents));
    const int32_t m = n - 1;
    out.cells = int64_t(n) << m;
    out.sets = int64_t(1) << n;
    out.cost_bytes = out.cells * 8;
    out.rank_bytes = out.cells * 4;
    out.r_bytes = out.sets * 8;
    out.sink_bytes = out.sets;
    out.bytes = out.cost_bytes + out.rank_bytes + out.r_bytes + out.sink_bytes;
    // the first pass makes the cells and does the bits of one contiguous tile; a later pass gathers up to 12 - 4 higher bits into a
    // tile whose rows are the 2^4 lowest cells
    const int32_t nb0 = std::min(m, kOptimalTileBits);
    out.passes.push_back(OptimalPass{0, 0, nb0, int32_t(1) << (m - nb0)});
    for (int32_t b = nb0; b < m;) {
        const int32_t nb = std::min(kOptimalTileBits - kOptimalLowBits, m - b);
        out.passes.push_back(OptimalPass{kOptimalLowBits, b, nb, int32_t(1) << (m - kOptimalLowBits - nb)});
        b += nb;
    }
    return BN_OK;
}

}  // namespace bnmi
