// test_memo1_policy.cpp -- the host decisions of the resident path's second-sweep image (bn_policy::memo1_*, bayesiannetwork_amd/csrc/
// bn_engine_policy.cpp), stand-alone: compiled together with bn_engine_policy.cpp by plain g++ (tests/test_cpp_memo1_policy.py builds
// it with -fsanitize=address,undefined), no HIP and no library.  Four questions: does a run start at sweep 2; what is the node-level
// adjacency; what is the seed of sweep 1's residual -- the contribution of the first node, by descending contribution, whose closed
// neighbourhood holds no evidence node; and what does a set do to the image and to the image's own list of what it holds, across a
// set that is over the work limit.  The expected values are written out from the rules, not from running the functions.
// Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "bn_engine_policy.hpp"

using namespace bn_policy;

static long g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static Memo1Run run(bool on0, bool valid0, bool flow, int32_t max_sweeps, double eps, double c0, bool on1, bool valid1, double seed) {
    Memo1Run r;
    r.level0.enabled = on0; r.level0.image_valid = valid0; r.level0.flow = flow; r.level0.max_sweeps = max_sweeps; r.level0.eps = eps;
    r.level0.const_residual = c0;
    r.enabled = on1; r.image_valid = valid1; r.seed = seed;
    return r;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- whether a run starts at sweep 2
    CHECK(memo1_applies(run(true, true, false, 0, 1e-3, 0.75, true, true, 0.2)));
    CHECK(!memo1_applies(run(false, true, false, 0, 1e-3, 0.75, true, true, 0.2)));   // option "memo0" off
    CHECK(!memo1_applies(run(true, false, false, 0, 1e-3, 0.75, true, true, 0.2)));   // no first-sweep image
    CHECK(!memo1_applies(run(true, true, true, 0, 1e-3, 0.75, true, true, 0.2)));     // dataflow form
    CHECK(!memo1_applies(run(true, true, false, 0, 1e-3, 0.75, false, true, 0.2)));   // option "memo1" off
    CHECK(!memo1_applies(run(true, true, false, 0, 1e-3, 0.75, true, false, 0.2)));   // the image does not hold the set in force
    CHECK(!memo1_applies(run(true, true, false, 1, 1e-3, 0.75, true, true, 0.2)));    // the run ends behind sweep 0
    CHECK(!memo1_applies(run(true, true, false, 2, 1e-3, 0.75, true, true, 0.2)));    // ... behind sweep 1
    CHECK(memo1_applies(run(true, true, false, 3, 1e-3, 0.75, true, true, 0.2)));
    CHECK(memo1_applies(run(true, true, false, 1030, 0.0, 0.75, true, true, 0.2)));
    CHECK(memo1_applies(run(true, true, false, 0, 0.2, 0.75, true, true, 0.2)));      // residual < eps stops: eps == the seed does not
    CHECK(!memo1_applies(run(true, true, false, 0, std::nextafter(0.2, 1.0), 0.75, true, true, 0.2)));
    CHECK(!memo1_applies(run(true, true, false, 0, 0.5, 0.75, true, true, 0.2)));     // sweep 1 may end the run (sweep 0 may not)
    CHECK(memo0_applies(run(true, true, false, 0, 0.5, 0.75, true, true, 0.2).level0));
    CHECK(!memo1_applies(run(true, true, false, 0, 0.1, 0.05, true, true, 0.2)));     // sweep 0 may end the run
    CHECK(!memo1_applies(run(true, true, false, 0, 1e-3, 0.75, true, true, 0.0)));    // every node inside the ring
    CHECK(!memo1_applies(run(true, true, false, 0, 1e-3, 0.75, true, true, -1.0)));
    CHECK(!memo1_applies(run(true, true, false, 0, 1e-3, 0.75, true, true, inf)));
    CHECK(!memo1_applies(run(true, true, false, 0, 1e-3, 0.75, true, true, nan)));
    CHECK(!memo1_applies(run(true, true, false, 0, nan, 0.75, true, true, 0.2)));
    CHECK(memo1_applies(run(true, true, false, 0, -1.0, 0.75, true, true, 0.2)));     // (eps <= 0 never stops a run)

    // ---- adjacency of a hand-made graph: 0 -> 1 -> 2 -> 3 -> 4, 5 -> 4, 6 alone, 7 -> 8 (parents' CSR)
    //      node:     0   1   2   3   4      5   6   7   8
    const std::vector<int32_t> in_ptr = {0, 0, 1, 2, 3, 5, 5, 5, 5, 6};
    const std::vector<int32_t> in_idx = {0, 1, 2, 3, 5, 7};
    std::vector<int32_t> adj_off, adj;
    CHECK(memo1_adjacency(9, in_ptr, in_idx, adj_off, adj) == 2);
    CHECK(adj_off.size() == 10 && adj_off[9] == 12 && adj.size() == 12);
    auto nb = [&](int v) { return std::vector<int32_t>(adj.begin() + adj_off[size_t(v)], adj.begin() + adj_off[size_t(v) + 1]); };
    CHECK((nb(0) == std::vector<int32_t>{1}));
    CHECK((nb(1) == std::vector<int32_t>{0, 2}));                    // parents first, then children
    CHECK((nb(4) == std::vector<int32_t>{3, 5}));
    CHECK((nb(5) == std::vector<int32_t>{4}));
    CHECK(nb(6).empty());
    CHECK((nb(8) == std::vector<int32_t>{7}));
    std::vector<int32_t> eo, ea;
    CHECK(memo1_adjacency(0, {}, {}, eo, ea) == 0 && eo.size() == 1 && ea.empty());

    // ---- the seed walk: contributions descend along `order`
    const std::vector<double> cv1 = {0.9, 0.1, 0.8, 0.2, 0.7, 0.3, 0.6, 0.5, 0.4};
    const std::vector<int32_t> order = {0, 2, 4, 6, 7, 8, 5, 3, 1};
    std::vector<uint32_t> st;
    uint32_t ep = 0;
    memo0_stamp(nullptr, 0, 9, st, ep);
    CHECK(memo1_seed(order, cv1, adj_off, adj, st, ep) == 0.9);       // no evidence: the first candidate
    const int32_t e1[] = {1};                                         // N[1] = {0, 1, 2}: the first and second candidates are inside
    memo0_stamp(e1, 1, 9, st, ep);
    CHECK(memo1_seed(order, cv1, adj_off, adj, st, ep) == 0.7);       // node 4 (N[4] = {3, 4, 5})
    const int32_t e2[] = {0};                                         // the first candidate carries the evidence itself
    memo0_stamp(e2, 1, 9, st, ep);
    CHECK(memo1_seed(order, cv1, adj_off, adj, st, ep) == 0.8);       // node 2 (N[2] = {1, 2, 3})
    const int32_t e3[] = {1, 5};                                      // first three candidates inside: 0, 2 through 1; 4 through 5
    memo0_stamp(e3, 2, 9, st, ep);
    CHECK(memo1_seed(order, cv1, adj_off, adj, st, ep) == 0.6);       // node 6, which has no neighbour at all
    const int32_t e4[] = {1, 5, 6};
    memo0_stamp(e4, 3, 9, st, ep);
    CHECK(memo1_seed(order, cv1, adj_off, adj, st, ep) == 0.5);       // node 7
    const int32_t e5[] = {1, 3, 6, 8};                                // the ring is {0..4} + {6} + {7, 8}; N[5] = {4, 5} holds no
    memo0_stamp(e5, 4, 9, st, ep);                                    // evidence node: the seventh candidate decides
    CHECK(memo1_seed(order, cv1, adj_off, adj, st, ep) == 0.3);
    const int32_t e6[] = {1, 4, 6, 8};                                // every node inside the ring
    memo0_stamp(e6, 4, 9, st, ep);
    CHECK(memo1_seed(order, cv1, adj_off, adj, st, ep) == 0.0);
    CHECK(!memo1_applies(run(true, true, false, 0, 1e-3, 0.75, true, true, memo1_seed(order, cv1, adj_off, adj, st, ep))));

    // ---- the work limit
    CHECK(memo1_patch_fits(10, 5, 4, 75));                            // (10 + 5) x (1 + 4) = 75
    CHECK(!memo1_patch_fits(10, 5, 4, 74));
    CHECK(memo1_patch_fits(0, 0, 8, 0));
    CHECK(!memo1_patch_fits(1, 0, 0, 0));
    CHECK(memo1_patch_fits(1 << 30, 1 << 30, 8, int64_t(1) << 40));   // (no 32-bit overflow)

    // ---- what a set does to the image and its own list, across a skipped set
    std::vector<int32_t> applied, list;
    const int32_t limit = 12, deg = 2;                                // at most 4 listed nodes
    memo0_stamp(nullptr, 0, 9, st, ep);
    Memo1Plan p = memo1_plan_set(nullptr, 0, st, ep, true, deg, limit, applied, list);
    CHECK(!p.patch && p.holds && list.empty() && applied.empty());    // nothing to apply, nothing to restore: the pristine image
    const int32_t A[] = {1, 4, 7};
    memo0_stamp(A, 3, 9, st, ep);
    p = memo1_plan_set(A, 3, st, ep, true, deg, limit, applied, list);
    CHECK(p.patch && p.holds && (list == std::vector<int32_t>{1, 4, 7}) && (applied == std::vector<int32_t>{1, 4, 7}));
    const int32_t B[] = {4, 2};                                       // keeps 4, drops 1 and 7, adds 2: E then R
    memo0_stamp(B, 2, 9, st, ep);
    p = memo1_plan_set(B, 2, st, ep, true, deg, limit, applied, list);
    CHECK(p.patch && p.holds && (list == std::vector<int32_t>{4, 2, 1, 7}) && (applied == std::vector<int32_t>{4, 2}));
    const int32_t D[] = {0, 2, 3, 5, 8};                              // 5 + 1 restored (4) = 6 listed nodes x 3 = 18 > 12: no patch
    memo0_stamp(D, 5, 9, st, ep);
    p = memo1_plan_set(D, 5, st, ep, true, deg, limit, applied, list);
    CHECK(!p.patch && !p.holds && list.empty() && (applied == std::vector<int32_t>{4, 2}));   // the image still holds B
    const int32_t F[] = {2, 6};                                       // the sparse set behind it restores what B left, not what D held
    memo0_stamp(F, 2, 9, st, ep);
    p = memo1_plan_set(F, 2, st, ep, true, deg, limit, applied, list);
    CHECK(p.patch && p.holds && (list == std::vector<int32_t>{2, 6, 4}) && (applied == std::vector<int32_t>{2, 6}));
    memo0_stamp(F, 2, 9, st, ep);                                     // a one-shot call that does not want the launch: as over the limit
    p = memo1_plan_set(F, 2, st, ep, false, deg, limit, applied, list);
    CHECK(!p.patch && !p.holds && (applied == std::vector<int32_t>{2, 6}));
    memo0_stamp(nullptr, 0, 9, st, ep);                               // the empty set behind a non-empty image: everything goes back
    p = memo1_plan_set(nullptr, 0, st, ep, true, deg, limit, applied, list);
    CHECK(p.patch && p.holds && (list == std::vector<int32_t>{2, 6}) && applied.empty());
    memo0_stamp(nullptr, 0, 9, st, ep);                               // ... and again: nothing left to do, even where no launch is wanted
    p = memo1_plan_set(nullptr, 0, st, ep, false, deg, limit, applied, list);
    CHECK(!p.patch && p.holds && list.empty());
    memo0_stamp(A, 3, 9, st, ep);                                     // a limit of 0 never patches a non-empty set
    p = memo1_plan_set(A, 3, st, ep, true, deg, 0, applied, list);
    CHECK(!p.patch && !p.holds && applied.empty());
    std::printf("ok: %ld checks\n", g_checks);
    return 0;
}
