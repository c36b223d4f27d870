// test_ci_plan.cpp -- the host-only planner of conditional-independence tests and PC-stable levels
// (bayesiannetwork_amd/csrc/bn_ci_plan.cpp) on seeded random graphs, stand-alone: compiled together with bn_ci_plan.cpp by plain g++
// (tests/test_cpp_pc.py adds -fsanitize=address,undefined), no HIP and no library.  Every property is checked against a
// recomputation from the adjacency; exit status 0 and "ok ..." on success, the first violated property otherwise.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <tuple>

#include "bn_ci_plan.hpp"
#include "bn_mi355x.h"

using namespace bnmi;

static std::string g_msg;   // the last error text
namespace bn_eng {
int fail(int code, const std::string& msg) {
    g_msg = msg;
    return code;
}
}  // namespace bn_eng

static long g_case = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::printf("FAILED %s:%d: %s  (case %ld)\n", __FILE__, __LINE__, #cond, g_case); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

using Adj = std::vector<std::vector<int32_t>>;
using Test = std::tuple<int32_t, int32_t, std::vector<int32_t>>;   // x, y, S

static int rnd(std::mt19937_64& r, int lo, int hi) { return lo + int(r() % uint64_t(hi - lo + 1)); }

// every l-subset of `list` in lexicographic order
static void subsets(const std::vector<int32_t>& list, int l, std::vector<std::vector<int32_t>>& out) {
    out.clear();
    std::vector<int32_t> cur;
    std::vector<size_t> idx(static_cast<size_t>(l));
    if (int(list.size()) < l) return;
    for (int i = 0; i < l; ++i) idx[size_t(i)] = size_t(i);
    for (;;) {
        cur.clear();
        for (size_t i : idx) cur.push_back(list[i]);
        out.push_back(cur);
        int i = l - 1;
        while (i >= 0 && idx[size_t(i)] == list.size() - size_t(l - i)) --i;
        if (i < 0) break;
        ++idx[size_t(i)];
        for (int j = i + 1; j < l; ++j) idx[size_t(j)] = idx[size_t(j) - 1] + 1;
    }
}

// the tests of edge a < b in the stated order: side 0 (S from A(a) \ {b}) then side 1, S lexicographic
static std::vector<Test> edge_tests(const Adj& adj, int32_t a, int32_t b, int level) {
    std::vector<Test> seq;
    std::vector<std::vector<int32_t>> ss;
    for (int side = 0; side < 2; ++side) {
        const int32_t x = side ? b : a, y = side ? a : b;
        if (level == 0 && side == 1) continue;
        std::vector<int32_t> rest;
        for (int32_t v : adj[size_t(x)])
            if (v != y) rest.push_back(v);
        subsets(rest, level, ss);
        for (const auto& s : ss) seq.emplace_back(x, y, s);
    }
    return seq;
}

static void check_level(const std::vector<int32_t>& k, const Adj& adj, int level, int64_t cell_limit) {
    PcLevel lv;
    CHECK(pc_plan_level(k.data(), adj, level, int64_t(1) << 26, lv) == BN_OK);
    const int32_t n = int32_t(adj.size());
    bool any = false;
    for (int32_t x = 0; x < n; ++x) any = any || (!adj[size_t(x)].empty() && int(adj[size_t(x)].size()) - 1 >= level);
    CHECK(lv.any == any);   // the level stops exactly when no ordered pair qualifies
    if (!any) {
        CHECK(lv.tests == 0 && lv.g.groups() == 0);
        return;
    }
    // what the level must run, per edge, with ranks 0, 1, ... in the stated order
    std::map<Test, std::pair<int32_t, uint32_t>> want;   // test -> (edge, rank)
    int64_t asked = 0, over = 0;
    size_t e = 0;
    for (int32_t a = 0; a < n; ++a)
        for (int32_t b : adj[size_t(a)]) {
            if (b < a) continue;
            CHECK(e < lv.edge_a.size() && lv.edge_a[e] == a && lv.edge_b[e] == b);
            const std::vector<Test> seq = edge_tests(adj, a, b, level);
            for (size_t r = 0; r < seq.size(); ++r) {
                ++asked;
                int64_t cells = int64_t(k[size_t(std::get<0>(seq[r]))]) * k[size_t(std::get<1>(seq[r]))];
                for (int32_t v : std::get<2>(seq[r])) cells *= k[size_t(v)];
                CHECK(pc_unrank(adj, a, b, level, uint32_t(r)) == std::get<2>(seq[r]));   // the rank names the set
                if (cells > kCiPlanMaxCells) ++over;
                else want.emplace(seq[r], std::make_pair(int32_t(e), uint32_t(r)));
            }
            ++e;
        }
    CHECK(e == lv.edge_a.size());
    CHECK(pc_level_tests(adj, level) == asked && lv.skipped == over && lv.tests == int64_t(want.size()));
    // the groups: (x, S) with S increasing, every test once, its edge and rank as stated
    std::set<Test> seen;
    std::set<std::vector<int32_t>> keys;
    CHECK(lv.g.base_ptr.size() == size_t(lv.g.groups()) + 1 && lv.g.cand_ptr.size() == size_t(lv.g.groups()) + 1);
    CHECK(lv.edge.size() == size_t(lv.tests) && lv.rank.size() == size_t(lv.tests) && lv.group_cells.size() == size_t(lv.g.groups()));
    for (int32_t g = 0; g < lv.g.groups(); ++g) {
        const int32_t x = lv.g.child[size_t(g)];
        std::vector<int32_t> s(lv.g.base_idx.begin() + lv.g.base_ptr[size_t(g)], lv.g.base_idx.begin() + lv.g.base_ptr[size_t(g) + 1]);
        CHECK(int(s.size()) == level && std::is_sorted(s.begin(), s.end()));
        std::vector<int32_t> key = s;
        key.insert(key.begin(), x);
        CHECK(keys.insert(key).second);   // one group per (x, S)
        int64_t base = k[size_t(x)], cells = 0;
        for (int32_t v : s) base *= k[size_t(v)];
        cells = base;
        CHECK(lv.g.cand_ptr[size_t(g) + 1] > lv.g.cand_ptr[size_t(g)]);
        for (int32_t c = lv.g.cand_ptr[size_t(g)]; c < lv.g.cand_ptr[size_t(g) + 1]; ++c) {
            const Test t(x, lv.g.cand_idx[size_t(c)], s);
            auto it = want.find(t);
            CHECK(it != want.end() && seen.insert(t).second);
            CHECK(lv.edge[size_t(c)] == it->second.first && lv.rank[size_t(c)] == it->second.second);
            cells += base * k[size_t(lv.g.cand_idx[size_t(c)])];
        }
        CHECK(lv.group_cells[size_t(g)] == cells);
    }
    CHECK(seen.size() == want.size());
    // chunks: consecutive, every group once, within the limits unless a single group
    std::vector<std::pair<int32_t, int32_t>> chunks;
    for (int32_t max_tests : {1 << 16, 7}) {
        pc_chunks(lv, cell_limit, max_tests, chunks);
        int32_t at = 0;
        for (const auto& c : chunks) {
            CHECK(c.first == at && c.second > c.first);
            int64_t cells = 0, tests = 0;
            for (int32_t g = c.first; g < c.second; ++g) {
                cells += lv.group_cells[size_t(g)];
                tests += lv.g.cand_ptr[size_t(g) + 1] - lv.g.cand_ptr[size_t(g)];
            }
            CHECK(c.second - c.first == 1 || (cells <= cell_limit && tests <= max_tests));
            at = c.second;
        }
        CHECK(at == lv.g.groups());
    }
}

static void check_grouping(std::mt19937_64& r, const std::vector<int32_t>& k) {
    const int32_t n = int32_t(k.size());
    std::vector<Test> tests;
    for (int i = 0, m = rnd(r, 1, 40); i < m; ++i) {
        if (!tests.empty() && rnd(r, 0, 4) == 0) {   // a test listed again, its S in another order
            Test t = tests[size_t(rnd(r, 0, int(tests.size()) - 1))];
            std::shuffle(std::get<2>(t).begin(), std::get<2>(t).end(), r);
            tests.push_back(t);
            continue;
        }
        std::vector<int32_t> ids(static_cast<size_t>(n));
        for (int32_t v = 0; v < n; ++v) ids[size_t(v)] = v;
        std::shuffle(ids.begin(), ids.end(), r);
        const int ns = rnd(r, 0, std::min(n - 2, 3));
        tests.emplace_back(ids[0], ids[1], std::vector<int32_t>(ids.begin() + 2, ids.begin() + 2 + ns));
    }
    std::vector<CiTestIn> in;
    for (const Test& t : tests) in.push_back(CiTestIn{std::get<0>(t), std::get<1>(t), std::get<2>(t).data(), int32_t(std::get<2>(t).size())});
    CiGroups g;
    std::vector<int32_t> slot;
    CHECK(ci_group_tests(k.data(), n, in, g, slot) == BN_OK);
    std::vector<Test> by_slot;   // what every slot stands for
    std::set<std::vector<int32_t>> keys;
    for (int32_t i = 0; i < g.groups(); ++i) {
        std::vector<int32_t> s(g.base_idx.begin() + g.base_ptr[size_t(i)], g.base_idx.begin() + g.base_ptr[size_t(i) + 1]);
        CHECK(std::is_sorted(s.begin(), s.end()));
        std::vector<int32_t> key = s;
        key.insert(key.begin(), g.child[size_t(i)]);
        CHECK(keys.insert(key).second);
        for (int32_t c = g.cand_ptr[size_t(i)]; c < g.cand_ptr[size_t(i) + 1]; ++c) by_slot.emplace_back(g.child[size_t(i)], g.cand_idx[size_t(c)], s);
    }
    std::set<Test> distinct;
    for (size_t i = 0; i < tests.size(); ++i) {
        Test t = tests[i];
        std::sort(std::get<2>(t).begin(), std::get<2>(t).end());
        distinct.insert(t);
        CHECK(slot[i] >= 0 && size_t(slot[i]) < by_slot.size() && by_slot[size_t(slot[i])] == t);   // no test lost
    }
    CHECK(std::set<Test>(by_slot.begin(), by_slot.end()).size() == by_slot.size() && by_slot.size() == distinct.size());   // none duplicated
}

static void check_refusals() {
    const std::vector<int32_t> k{2, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 255, 255, 255};
    const int32_t n = int32_t(k.size());
    CiGroups g;
    std::vector<int32_t> slot;
    auto run = [&](int32_t x, int32_t y, std::vector<int32_t> s) {
        std::vector<int32_t> ok{2};
        std::vector<CiTestIn> in{CiTestIn{0, 1, ok.data(), 1}, CiTestIn{x, y, s.data(), int32_t(s.size())}};
        g_msg.clear();
        return ci_group_tests(k.data(), n, in, g, slot);
    };
    CHECK(run(3, 3, {}) == BN_ERR_ARG && g_msg.find("test 1") == 0 && g_msg.find("same variable") != std::string::npos);
    CHECK(run(3, 4, {5, 3}) == BN_ERR_ARG && g_msg.find("test 1") == 0 && g_msg.find("x (3) is in the conditioning set") != std::string::npos);
    CHECK(run(3, 4, {5, 4}) == BN_ERR_ARG && g_msg.find("y (4) is in the conditioning set") != std::string::npos);
    CHECK(run(3, 4, {5, 6, 5}) == BN_ERR_ARG && g_msg.find("listed twice") != std::string::npos);
    CHECK(run(0, 1, {2, 3, 4, 5, 6, 7, 8, 9, 10}) == BN_ERR_ARG && g_msg.find("9 variables") != std::string::npos);
    CHECK(run(0, 1, {12, 13, 14}) == BN_ERR_ARG && g_msg.find("cells") != std::string::npos);
    CHECK(run(0, n, {}) == BN_ERR_ARG && run(0, 1, {-1}) == BN_ERR_ARG);
    CHECK(run(0, 1, {2, 3, 4, 5, 6, 7, 8, 9}) == BN_OK && g.groups() == 2);
    // a level over max_tests is refused, naming the level and the number
    Adj full(6);
    for (int32_t a = 0; a < 6; ++a)
        for (int32_t b = 0; b < 6; ++b)
            if (a != b) full[size_t(a)].push_back(b);
    PcLevel lv;
    g_msg.clear();
    CHECK(pc_plan_level(k.data(), full, 2, 179, lv) == BN_ERR_STATE && g_msg.find("level 2 needs 180 tests") != std::string::npos);
    CHECK(pc_plan_level(k.data(), full, 2, 180, lv) == BN_OK && lv.tests == 180);   // 6 nodes x 5 neighbours x C(4, 2) sets
    CHECK(pc_binom(5, 2) == 10 && pc_binom(4, 5) == 0 && pc_binom(1023, 8) == (int64_t(1) << 62));
}

int main() {
    std::mt19937_64 r(20260117);
    long levels = 0;
    for (g_case = 0; g_case < 120; ++g_case) {
        const int32_t n = rnd(r, 2, 9);
        std::vector<int32_t> k(static_cast<size_t>(n));
        const bool wide = g_case % 10 == 9;   // arities that push tests over 2^20 cells
        for (auto& x : k) x = wide ? rnd(r, 30, 255) : rnd(r, 1, 4);
        Adj adj(static_cast<size_t>(n));
        const int dens = rnd(r, 20, 100);
        for (int32_t a = 0; a < n; ++a)
            for (int32_t b = a + 1; b < n; ++b)
                if (rnd(r, 1, 100) <= dens) {
                    adj[size_t(a)].push_back(b);
                    adj[size_t(b)].push_back(a);
                }
        for (auto& l : adj) std::sort(l.begin(), l.end());
        for (int level = 0; level <= std::min(n, 5); ++level, ++levels) check_level(k, adj, level, rnd(r, 100, 400));
        if (n >= 3 && !wide) check_grouping(r, k);   // (wide arities: over the cell limit, refused -- check_refusals)
    }
    check_refusals();
    std::printf("ok: %ld levels, ranks, groups, chunks and refusals\n", levels);
    return 0;
}
