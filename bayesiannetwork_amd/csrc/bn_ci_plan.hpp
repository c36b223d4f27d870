// bn_ci_plan.hpp -- what conditional-independence tests and a level of PC-stable do before they touch the device, as pure functions
// of the arities and the adjacency: the checks and the grouping of a batch of tests by (x, S) (ci_group_tests); the tests of a level,
// their groups, edges and ranks (pc_plan_level); the chunks of groups handed to the device (pc_chunks); a separating set back from
// its rank (pc_unrank).  No HIP: bn_ci_plan.cpp is also compiled alone by tests/cpp/test_ci_plan.cpp.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace bn_eng __attribute__((visibility("hidden"))) {
int fail(int code, const std::string& msg);   // bn_last_error (bn_engine.cpp; the stand-alone test has its own)
}  // namespace bn_eng

#pragma GCC visibility push(hidden)
namespace bnmi {

constexpr int32_t kCiPlanMaxCond = 8;                          // |S|
constexpr int64_t kCiPlanMaxCells = int64_t(1) << 20;          // k_x * k_y * prod k_S: bn_learn_score_groups' family limit
constexpr int32_t kPcMaxNodes = 1024;
constexpr int64_t kPcDefaultMaxTests = int64_t(1) << 22;       // per level
constexpr int64_t kPcMaxMaxTests = int64_t(1) << 26;
constexpr int32_t kPcChunkTests = 1 << 16;                     // tests per chunk at most

// groups in CSR form, as bn_learn_score_groups takes them: child x, base S (increasing), candidates y
struct CiGroups {
    std::vector<int32_t> child, base_ptr{0}, base_idx, cand_ptr{0}, cand_idx;
    int32_t groups() const { return int32_t(child.size()); }
    int32_t tests() const { return int32_t(cand_idx.size()); }
};

struct CiTestIn {
    int32_t x, y;
    const int32_t* s;   // any order
    int32_t n_s;
};

// Groups the tests by (x, sorted S), groups and candidates in order of first appearance; slot[i]: the place of test i among the
// candidates (group-major).  The same test listed twice takes one slot.  BN_OK, or what bn_eng::fail returned (the text names the test).
int ci_group_tests(const int32_t* k, int32_t n, const std::vector<CiTestIn>& tests, CiGroups& out, std::vector<int32_t>& slot);

// One level of PC-stable over the adjacency A (adj[v] increasing, symmetric).
struct PcLevel {
    int32_t level = 0;
    bool any = false;                        // some ordered pair (x, y) has |A(x) \ {y}| >= level: else the search stops
    std::vector<int32_t> edge_a, edge_b;     // the edges of A, a < b, in increasing (a, b)
    CiGroups g;                              // groups in increasing (x, S lexicographic); candidates increasing
    std::vector<int32_t> edge;               // per test (candidate): its edge ...
    std::vector<uint32_t> rank;              // ... and its rank among the edge's tests: side * C(|A(min)| - 1, level) + the index of S
    std::vector<int64_t> group_cells;        // count-scratch cells of a group: base family + every candidate family
    int64_t tests = 0;                       // tests handed to the device
    int64_t skipped = 0;                     // tests over kCiPlanMaxCells: not run, dependent
};

// number of tests the level asks for (over-limit tests included), saturating at 2^62
int64_t pc_level_tests(const std::vector<std::vector<int32_t>>& adj, int32_t level);
// BN_ERR_STATE naming the level and the number when that passes max_tests; nothing is trimmed
int pc_plan_level(const int32_t* k, const std::vector<std::vector<int32_t>>& adj, int32_t level, int64_t max_tests, PcLevel& out);
// runs of whole groups [first, second) whose cells fit max_cells (a group larger than that is a chunk of its own) and whose tests
// number at most max_chunk_tests (likewise)
void pc_chunks(const PcLevel& lv, int64_t max_cells, int32_t max_chunk_tests, std::vector<std::pair<int32_t, int32_t>>& chunks);
// the S of the test of rank `rank` of the edge a < b at `level`
std::vector<int32_t> pc_unrank(const std::vector<std::vector<int32_t>>& adj, int32_t a, int32_t b, int32_t level, uint32_t rank);
// C(m, r) saturating at 2^62
int64_t pc_binom(int64_t m, int32_t r);

}  // namespace bnmi
#pragma GCC visibility pop
