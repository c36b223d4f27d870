// test_optimal_plan.cpp -- the host-only planner of the exact search (bayesiannetwork_amd/csrc/bn_learn_optimal_plan.cpp),
// stand-alone: compiled together with the planner by plain g++ (tests/test_optimal_refs.py adds -fsanitize=address,undefined), no
// HIP and no library.  The limits on both sides, squeeze and its inverse, the byte counts and the pass schedule: every bit of a
// child's cell index is done by exactly one pass, and the tiles of a pass cover every cell exactly once.  Exit status 0 and "ok ..."
// on success, the first violated property otherwise.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bn_learn_optimal_plan.hpp"
#include "bn_mi355x.h"

using namespace bnmi;

static std::string g_msg;   // the last error text
namespace bn_eng {
int fail(int code, const std::string& msg) {
    g_msg = msg;
    return code;
}
}  // namespace bn_eng

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// the cell index of entry i of tile t of a pass, as the kernel forms it
static uint32_t cell_of(const OptimalPass& p, uint32_t t, uint32_t i) {
    const uint32_t mid_bits = uint32_t(p.b0 - p.low);
    const uint32_t fixed = ((t & ((1u << mid_bits) - 1u)) << p.low) | ((t >> mid_bits) << (p.b0 + p.nb));
    return fixed | (i & ((1u << p.low) - 1u)) | ((i >> p.low) << p.b0);
}

int main() {
    OptimalPlan plan;
    // the limits, on both sides of each
    CHECK(plan_optimal(0, 3, 3, 16, nullptr, plan) == BN_ERR_ARG && has(g_msg, "0 nodes") && has(g_msg, "1 .. 24"));
    CHECK(plan_optimal(25, 3, 3, 16, nullptr, plan) == BN_ERR_ARG && has(g_msg, "25 nodes") && has(g_msg, "1 .. 24"));
    CHECK(plan_optimal(1, 3, 3, 16, nullptr, plan) == BN_OK && plan.n == 1 && plan.cells == 1 && plan.sets == 2);
    CHECK(plan_optimal(24, 3, 3, 16, nullptr, plan) == BN_OK);
    CHECK(plan_optimal(5, 0, 3, 16, nullptr, plan) == BN_ERR_ARG && has(g_msg, "max_parents 0"));
    CHECK(plan_optimal(5, -1, 3, 16, nullptr, plan) == BN_ERR_ARG);
    CHECK(plan_optimal(5, 1, 3, 16, nullptr, plan) == BN_OK && plan.mp == 1);
    // mp: the smallest of the three bounds
    CHECK(plan_optimal(5, 7, 3, 16, nullptr, plan) == BN_OK && plan.mp == 3);
    CHECK(plan_optimal(5, 7, 3, 2, nullptr, plan) == BN_OK && plan.mp == 2);
    // allowed: bits below n pass (a node's own bit too), a bit at n or above does not
    std::vector<uint64_t> allowed(5, 0x1F);
    CHECK(plan_optimal(5, 3, 3, 16, allowed.data(), plan) == BN_OK);
    allowed[3] = 0x20;
    CHECK(plan_optimal(5, 3, 3, 16, allowed.data(), plan) == BN_ERR_ARG && has(g_msg, "allowed[3]"));
    allowed[3] = uint64_t(1) << 63;
    CHECK(plan_optimal(5, 3, 3, 16, allowed.data(), plan) == BN_ERR_ARG);
    // the order of the checks: the nodes first
    CHECK(plan_optimal(25, 0, 3, 16, allowed.data(), plan) == BN_ERR_ARG && has(g_msg, "25 nodes"));

    // squeeze and its inverse for every child of five nodes
    for (int v = 0; v < 5; ++v) {
        std::vector<int> seen(16, 0);
        for (uint32_t C = 0; C < 32; ++C) {
            if ((C >> v) & 1) continue;
            const uint32_t c = optimal_squeeze(C, v);
            CHECK(c < 16 && optimal_unsqueeze(c, v) == C);
            ++seen[c];
            for (int s = 0; s < 5; ++s)   // node s sits at bit s - (s > v)
                if (s != v) CHECK(((C >> s) & 1) == ((c >> (s - (s > v ? 1 : 0))) & 1));
        }
        for (int x : seen) CHECK(x == 1);
    }

    // the byte counts at the limit: 24 * 2^23 cells of 8 + 4 bytes, 2^24 sets of 8 + 1
    CHECK(plan_optimal(24, 3, 3, 16, nullptr, plan) == BN_OK);
    CHECK(plan.cells == int64_t(24) << 23 && plan.sets == int64_t(1) << 24);
    CHECK(plan.cost_bytes == 1610612736ll && plan.rank_bytes == 805306368ll && plan.r_bytes == 134217728ll && plan.sink_bytes == 16777216ll);
    CHECK(plan.bytes == 2566914048ll);

    // the schedule
    long passes_total = 0;
    for (int n : {1, 2, 3, 12, 13, 14, 16, 20, 21, 22, 24}) {
        CHECK(plan_optimal(n, 3, 3, 16, nullptr, plan) == BN_OK);
        const int m = n - 1;
        std::vector<int> done(size_t(m), 0);
        CHECK(!plan.passes.empty() && plan.passes[0].low == 0 && plan.passes[0].b0 == 0);   // the first pass makes the cells
        for (size_t j = 0; j < plan.passes.size(); ++j) {
            const OptimalPass& p = plan.passes[j];
            CHECK(p.low >= 0 && p.nb >= 0 && p.low + p.nb <= kOptimalTileBits && p.b0 + p.nb <= m);
            CHECK(j == 0 ? true : (p.low <= p.b0 && p.nb >= 1 && p.b0 > 0));
            CHECK(int64_t(p.tiles) << (p.low + p.nb) == int64_t(1) << m);
            for (int b = p.b0; b < p.b0 + p.nb; ++b) ++done[size_t(b)];
            if (m <= 16) {   // the tiles cover every cell once
                std::vector<uint8_t> hit(size_t(1) << m, 0);
                for (uint32_t t = 0; t < uint32_t(p.tiles); ++t)
                    for (uint32_t i = 0; i < (1u << (p.low + p.nb)); ++i) {
                        const uint32_t c = cell_of(p, t, i);
                        CHECK(c < (1u << m));
                        ++hit[c];
                    }
                for (uint8_t x : hit) CHECK(x == 1);
            } else {         // the largest tile and entry stay inside the row
                CHECK(cell_of(p, uint32_t(p.tiles) - 1, (1u << (p.low + p.nb)) - 1) == (1u << m) - 1);
            }
        }
        for (int x : done) CHECK(x == 1);
        CHECK(plan.passes.size() == size_t(m <= 12 ? 1 : 1 + (m - 12 + 7) / 8));
        passes_total += long(plan.passes.size());
    }
    std::printf("ok: limits, squeeze, bytes at n = 24, %ld passes over 11 sizes\n", passes_total);
    return 0;
}
