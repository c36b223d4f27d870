// bn_ci_plan.cpp -- the host-only planning of bn_ci_plan.hpp: the checks and grouping of a batch of conditional-independence tests,
// and the tests, groups, ranks and chunks of one level of PC-stable.  Pure functions of the arities and the adjacency: no HIP call,
// no device state.  The error texts are the C ABI's (include/bn_mi355x.h, bn_ci_tests / bn_learn_pc).
#include "bn_ci_plan.hpp"

#include <algorithm>
#include <map>

#include "../../include/bn_mi355x.h"

namespace bnmi {
namespace {

using bn_eng::fail;

constexpr int64_t kSat = int64_t(1) << 62;

int64_t sat_mul(int64_t a, int64_t b) { return (a != 0 && b > kSat / a) ? kSat : std::min(a * b, kSat); }

std::string tname(size_t i) { return "test " + std::to_string(i) + ": "; }

}  // namespace

int64_t pc_binom(int64_t m, int32_t r) {
    if (r < 0 || m < r) return 0;
    int64_t c = 1;
    for (int32_t i = 1; i <= r; ++i) {
        // c = c * (m - r + i) / i, exact at every step; saturating
        const int64_t f = m - r + i;
        if (c >= kSat / f) return kSat;
        c = c * f / i;
    }
    return c;
}

int ci_group_tests(const int32_t* k, int32_t n, const std::vector<CiTestIn>& tests, CiGroups& out, std::vector<int32_t>& slot) {
    out = CiGroups{};
    slot.assign(tests.size(), -1);
    struct Group {
        std::vector<int32_t> cand;   // in order of first appearance
    };
    std::map<std::vector<int32_t>, int32_t> index;   // (x, S...) -> group
    std::vector<std::vector<int32_t>> keys;
    std::vector<Group> groups;
    std::vector<std::pair<int32_t, int32_t>> where(tests.size());   // (group, candidate) of every test
    for (size_t i = 0; i < tests.size(); ++i) {
        const CiTestIn& t = tests[i];
        if (t.x < 0 || t.x >= n || t.y < 0 || t.y >= n) return fail(BN_ERR_ARG, tname(i) + "variable id out of range");
        if (t.x == t.y) return fail(BN_ERR_ARG, tname(i) + "x and y are the same variable (" + std::to_string(t.x) + ")");
        if (t.n_s < 0 || (t.n_s > 0 && !t.s)) return fail(BN_ERR_ARG, tname(i) + "bad conditioning set");
        if (t.n_s > kCiPlanMaxCond)
            return fail(BN_ERR_ARG, tname(i) + "a conditioning set of " + std::to_string(t.n_s) + " variables (at most " +
                                        std::to_string(kCiPlanMaxCond) + ")");
        std::vector<int32_t> key(size_t(t.n_s) + 1);
        key[0] = t.x;
        std::copy(t.s, t.s + t.n_s, key.begin() + 1);
        std::sort(key.begin() + 1, key.end());
        int64_t cells = int64_t(k[t.x]) * k[t.y];
        for (int32_t j = 1; j <= t.n_s; ++j) {
            const int32_t u = key[size_t(j)];
            if (u < 0 || u >= n) return fail(BN_ERR_ARG, tname(i) + "conditioning variable id " + std::to_string(u) + " out of range");
            if (u == t.x || u == t.y)
                return fail(BN_ERR_ARG, tname(i) + (u == t.x ? "x" : "y") + " (" + std::to_string(u) + ") is in the conditioning set");
            if (j > 1 && u == key[size_t(j) - 1])
                return fail(BN_ERR_ARG, tname(i) + "variable " + std::to_string(u) + " is listed twice in the conditioning set");
            cells = std::min(cells * k[u], kSat);   // (<= 255^10 < 2^62 anyway)
        }
        if (cells > kCiPlanMaxCells)
            return fail(BN_ERR_ARG, tname(i) + "a table of " + std::to_string(cells) + " cells (k_x * k_y * prod k_S at most 2^20)");
        auto it = index.find(key);
        if (it == index.end()) {
            it = index.emplace(key, int32_t(groups.size())).first;
            keys.push_back(key);
            groups.emplace_back();
        }
        Group& g = groups[size_t(it->second)];
        size_t c = std::find(g.cand.begin(), g.cand.end(), t.y) - g.cand.begin();
        if (c == g.cand.size()) g.cand.push_back(t.y);
        where[i] = {it->second, int32_t(c)};
    }
    std::vector<int32_t> first(groups.size());
    for (size_t g = 0; g < groups.size(); ++g) {
        first[g] = int32_t(out.cand_idx.size());
        out.child.push_back(keys[g][0]);
        out.base_idx.insert(out.base_idx.end(), keys[g].begin() + 1, keys[g].end());
        out.base_ptr.push_back(int32_t(out.base_idx.size()));
        out.cand_idx.insert(out.cand_idx.end(), groups[g].cand.begin(), groups[g].cand.end());
        out.cand_ptr.push_back(int32_t(out.cand_idx.size()));
    }
    for (size_t i = 0; i < tests.size(); ++i) slot[i] = first[size_t(where[i].first)] + where[i].second;
    return BN_OK;
}

int64_t pc_level_tests(const std::vector<std::vector<int32_t>>& adj, int32_t level) {
    int64_t total = 0;
    for (size_t x = 0; x < adj.size(); ++x) {
        const int64_t deg = int64_t(adj[x].size());
        if (level == 0) {
            for (int32_t y : adj[x]) total += y > int32_t(x);
        } else if (deg - 1 >= level) {
            total = std::min(total + sat_mul(deg, pc_binom(deg - 1, level)), kSat);   // deg neighbours y, C(deg - 1, level) sets each
        }
    }
    return total;
}

int pc_plan_level(const int32_t* k, const std::vector<std::vector<int32_t>>& adj, int32_t level, int64_t max_tests, PcLevel& out) {
    out = PcLevel{};
    out.level = level;
    const int32_t n = int32_t(adj.size());
    for (int32_t x = 0; x < n; ++x)
        if (!adj[size_t(x)].empty() && int32_t(adj[size_t(x)].size()) - 1 >= level) out.any = true;
    if (!out.any) return BN_OK;
    const int64_t asked = pc_level_tests(adj, level);
    if (asked > max_tests)
        return fail(BN_ERR_STATE, "bn_learn_pc: level " + std::to_string(level) + " needs " + std::to_string(asked) + " tests (max_tests " +
                                      std::to_string(max_tests) + "); nothing was changed");
    // the edges, and per neighbour entry its edge
    std::vector<std::vector<int32_t>> eid(adj.size());
    for (int32_t a = 0; a < n; ++a) eid[size_t(a)].resize(adj[size_t(a)].size());
    for (int32_t a = 0; a < n; ++a)
        for (size_t j = 0; j < adj[size_t(a)].size(); ++j) {
            const int32_t b = adj[size_t(a)][j];
            if (b < a) continue;
            const int32_t e = int32_t(out.edge_a.size());
            out.edge_a.push_back(a);
            out.edge_b.push_back(b);
            eid[size_t(a)][j] = e;
            const std::vector<int32_t>& nb = adj[size_t(b)];
            eid[size_t(b)][size_t(std::lower_bound(nb.begin(), nb.end(), a) - nb.begin())] = e;
        }
    std::vector<int32_t> pick(static_cast<size_t>(level)), kept, kept_j;
    for (int32_t x = 0; x < n; ++x) {
        const std::vector<int32_t>& A = adj[size_t(x)];
        const int32_t deg = int32_t(A.size());
        if (deg == 0 || deg - 1 < level) continue;
        const int64_t m = deg - 1;   // |A(x) \ {y}|
        for (int32_t i = 0; i < level; ++i) pick[size_t(i)] = i;
        for (;;) {   // every level-subset of A(x) by positions, lexicographic
            int64_t base = k[x];
            for (int32_t i = 0; i < level; ++i) base = std::min(base * k[A[size_t(pick[size_t(i)])]], kSat);
            kept.clear();
            kept_j.clear();
            for (int32_t j = 0, i = 0; j < deg; ++j) {
                if (i < level && pick[size_t(i)] == j) { ++i; continue; }   // y in S
                const int32_t y = A[size_t(j)];
                if (level == 0 && y < x) continue;                          // level 0: x < y only
                if (base > kCiPlanMaxCells || base * k[y] > kCiPlanMaxCells) { ++out.skipped; continue; }
                kept.push_back(y);
                kept_j.push_back(j);
            }
            if (!kept.empty()) {
                int64_t cells = base;
                for (size_t c = 0; c < kept.size(); ++c) {
                    const int32_t y = kept[c], jy = kept_j[c];
                    cells += base * k[y];
                    // the index of S among the level-subsets of A(x) \ {y}: positions shift down past y
                    int64_t idx = pc_binom(m, level) - 1;
                    for (int32_t i = 0; i < level; ++i) {
                        const int32_t p = pick[size_t(i)] - (pick[size_t(i)] > jy ? 1 : 0);
                        idx -= pc_binom(m - 1 - p, level - i);
                    }
                    const int32_t lo = std::min(x, y);
                    const int64_t side0 = x == lo ? 0 : pc_binom(int64_t(adj[size_t(lo)].size()) - 1, level);
                    out.edge.push_back(eid[size_t(x)][size_t(jy)]);
                    out.rank.push_back(uint32_t(side0 + idx));
                    out.g.cand_idx.push_back(y);
                }
                out.g.child.push_back(x);
                for (int32_t i = 0; i < level; ++i) out.g.base_idx.push_back(A[size_t(pick[size_t(i)])]);
                out.g.base_ptr.push_back(int32_t(out.g.base_idx.size()));
                out.g.cand_ptr.push_back(int32_t(out.g.cand_idx.size()));
                out.group_cells.push_back(cells);
            }
            int32_t i = level - 1;   // the next subset
            while (i >= 0 && pick[size_t(i)] == deg - level + i) --i;
            if (i < 0) break;
            ++pick[size_t(i)];
            for (int32_t j = i + 1; j < level; ++j) pick[size_t(j)] = pick[size_t(j) - 1] + 1;
        }
    }
    out.tests = int64_t(out.g.cand_idx.size());
    return BN_OK;
}

void pc_chunks(const PcLevel& lv, int64_t max_cells, int32_t max_chunk_tests, std::vector<std::pair<int32_t, int32_t>>& chunks) {
    chunks.clear();
    const int32_t groups = lv.g.groups();
    int32_t first = 0;
    int64_t cells = 0, tests = 0;
    for (int32_t g = 0; g < groups; ++g) {
        const int64_t gt = lv.g.cand_ptr[size_t(g) + 1] - lv.g.cand_ptr[size_t(g)];
        if (g > first && (cells + lv.group_cells[size_t(g)] > max_cells || tests + gt > max_chunk_tests)) {
            chunks.emplace_back(first, g);
            first = g;
            cells = tests = 0;
        }
        cells += lv.group_cells[size_t(g)];
        tests += gt;
    }
    if (groups > first) chunks.emplace_back(first, groups);
}

std::vector<int32_t> pc_unrank(const std::vector<std::vector<int32_t>>& adj, int32_t a, int32_t b, int32_t level, uint32_t rank) {
    const int64_t side0 = pc_binom(int64_t(adj[size_t(a)].size()) - 1, level);
    const bool from_b = int64_t(rank) >= side0;
    const int32_t x = from_b ? b : a, y = from_b ? a : b;
    int64_t r = int64_t(rank) - (from_b ? side0 : 0);
    std::vector<int32_t> list;   // A(x) \ {y}
    for (int32_t v : adj[size_t(x)])
        if (v != y) list.push_back(v);
    const int64_t m = int64_t(list.size());
    std::vector<int32_t> s;
    int64_t p = 0;
    for (int32_t i = 0; i < level; ++i) {
        // position p is taken when fewer than C(m - 1 - p, level - 1 - i) subsets are left to skip
        for (;; ++p) {
            const int64_t with_p = pc_binom(m - 1 - p, level - 1 - i);
            if (r < with_p) break;
            r -= with_p;
        }
        s.push_back(list[size_t(p)]);
        ++p;
    }
    return s;
}

}  // namespace bnmi
