// test_learn_plan.cpp -- the host-only planner of structure learning (bayesiannetwork_amd/csrc/bn_learn_plan.cpp) on seeded random
// batches, stand-alone: compiled together with bn_learn_plan.cpp by plain g++ (tests/test_cpp_learn_plan.py adds
// -fsanitize=address,undefined), no HIP and no library.  The scratch limit is the planner's parameter, so a few hundred cells give
// batches of many passes.  Every property is checked against a recomputation from the input lists; exit status 0 and "ok ..." on
// success, the first violated property otherwise.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "bn_learn_plan.hpp"
#include "bn_mi355x.h"

using namespace bnmi;

static std::string g_msg;   // the last error text
namespace bn_eng {
int fail(int code, const std::string& msg) {
    g_msg = msg;
    return code;
}
}  // namespace bn_eng

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::printf("FAILED %s:%d: %s  (case %ld)\n", __FILE__, __LINE__, #cond, g_case); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)
static long g_case = 0;

struct Group {
    int32_t child;
    std::vector<int32_t> base, cand;
};

static int rnd(std::mt19937_64& r, int lo, int hi) { return lo + int(r() % uint64_t(hi - lo + 1)); }

static std::vector<GroupIn> views(const std::vector<Group>& gs) {
    std::vector<GroupIn> v;
    for (const Group& g : gs) v.push_back(GroupIn{g.child, g.base.data(), int32_t(g.base.size()), g.cand.data(), int32_t(g.cand.size())});
    return v;
}

// every property of one plan; returns the number of passes
static size_t check_group_plan(const std::vector<int32_t>& k, const std::vector<Group>& gs, int64_t limit, const GroupPlan& p) {
    // the families in input order, from the lists alone
    struct Want { int32_t entries, kc, ku, low; int64_t out_at; size_t group; };
    std::vector<Want> want;
    std::vector<size_t> base_of_group;
    int64_t out_at = 0;
    for (size_t g = 0; g < gs.size(); ++g) {
        const int32_t kc = k[size_t(gs[g].child)];
        base_of_group.push_back(want.size());
        for (int j = -1; j < int(gs[g].cand.size()); ++j) {
            std::vector<int32_t> par = gs[g].base;
            if (j >= 0) par.push_back(gs[g].cand[size_t(j)]);
            std::sort(par.begin(), par.end());
            int64_t entries = kc, low = 1;
            bool after = false;
            for (int32_t u : par) {
                entries *= k[size_t(u)];
                if (after) low *= k[size_t(u)];
                if (j >= 0 && u == gs[g].cand[size_t(j)]) after = true;
            }
            want.push_back(Want{int32_t(entries), kc, j < 0 ? 1 : k[size_t(gs[g].cand[size_t(j)])], j < 0 ? 1 : int32_t(low), out_at, g});
            out_at += entries;
        }
    }
    const size_t F = want.size(), C = p.chunks.size();
    CHECK(p.out_cells == out_at && p.fams.size() == F && p.order.size() == F);
    if (F == 0) {
        CHECK(C == 0 && p.passes.empty() && p.scratch_cells == 0);
        return 0;
    }
    // order: a permutation; fams[i] is input family order[i], with its shape and its place in the fitted-layout copy
    std::vector<int32_t> launch_of(F, -1);
    for (size_t i = 0; i < F; ++i) {
        CHECK(p.order[i] >= 0 && size_t(p.order[i]) < F && launch_of[size_t(p.order[i])] < 0);
        launch_of[size_t(p.order[i])] = int32_t(i);
        const Want& w = want[size_t(p.order[i])];
        const LearnFamily& f = p.fams[i];
        CHECK(f.entries == w.entries && f.kc == w.kc && f.ku == w.ku && f.low == w.low && f.out_at == w.out_at);
    }
    // chunks: every family in exactly one; the kinds' limits; the uploaded id / arity arrays
    CHECK(p.base_fam.size() == C && p.cand_fam.size() == p.cand_id.size() && p.cand_k.size() == p.cand_id.size() && p.cand_cell.size() == p.cand_id.size());
    std::vector<int32_t> chunk_of(F, -1), cell_in_chunk(F, 0), bases_counted(gs.size(), 0);
    size_t cand_seen = 0;
    for (size_t c = 0; c < C; ++c) {
        const LearnChunk& ch = p.chunks[c];
        std::vector<int32_t> members;
        CHECK((ch.base_cell >= 0) == (p.base_fam[c] >= 0));
        if (ch.base_cell >= 0) {
            members.push_back(p.base_fam[c]);
            cell_in_chunk[size_t(p.base_fam[c])] = ch.base_cell;
        }
        CHECK(ch.cand_at == int32_t(cand_seen) && ch.n_cand >= 0 && size_t(ch.cand_at + ch.n_cand) <= p.cand_id.size());
        cand_seen += size_t(ch.n_cand);
        for (int32_t j = 0; j < ch.n_cand; ++j) {
            members.push_back(p.cand_fam[size_t(ch.cand_at + j)]);
            cell_in_chunk[size_t(members.back())] = p.cand_cell[size_t(ch.cand_at + j)];
        }
        CHECK(!members.empty());
        const size_t g = want[size_t(members[0])].group;
        CHECK(ch.child == gs[g].child && ch.kc == k[size_t(ch.child)] && ch.n_base == int32_t(gs[g].base.size()));
        for (int32_t j = 0; j < ch.n_base; ++j)
            CHECK(p.par_id[size_t(ch.base_at + j)] == gs[g].base[size_t(j)] && p.par_k[size_t(ch.base_at + j)] == k[size_t(gs[g].base[size_t(j)])]);
        int64_t cells = 0;
        for (size_t mi = 0; mi < members.size(); ++mi) {
            const int32_t f = members[mi];
            CHECK(f >= 0 && size_t(f) < F && chunk_of[size_t(f)] < 0 && want[size_t(f)].group == g);
            chunk_of[size_t(f)] = int32_t(c);
            CHECK(cell_in_chunk[size_t(f)] == cells);   // back to back inside the block
            cells += want[size_t(f)].entries;
            CHECK((want[size_t(f)].entries <= kLearnLdsCells) == (ch.in_lds == 1));
            if (size_t(f) == base_of_group[g]) {
                CHECK(ch.base_cell >= 0 && f == p.base_fam[c]);
                ++bases_counted[g];
            } else {
                const size_t at = size_t(ch.cand_at) + mi - (ch.base_cell >= 0 ? 1 : 0);
                const int32_t u = gs[g].cand[size_t(f) - base_of_group[g] - 1];
                CHECK(p.cand_id[at] == u && p.cand_k[at] == k[size_t(u)]);
            }
        }
        CHECK(ch.cells == cells && (ch.in_lds == 0 || ch.in_lds == 1));
        if (ch.in_lds) CHECK(ch.cells <= kLearnLdsCells && ch.n_cand <= kLearnMaxLdsCand);
        else CHECK(ch.n_cand <= kLearnMaxGlobalCand);
    }
    CHECK(cand_seen == p.cand_id.size());
    for (size_t f = 0; f < F; ++f) CHECK(chunk_of[f] >= 0);
    for (size_t g = 0; g < gs.size(); ++g) CHECK(bases_counted[g] == 1);
    // passes: a partition of the chunks and of the launch order; blocks back to back from 0; within the limit unless one chunk; greedy
    int32_t chunk_at = 0, fam_at = 0;
    int64_t largest = 0;
    std::vector<int32_t> pass_of_chunk(C, -1);
    for (size_t pi = 0; pi < p.passes.size(); ++pi) {
        const LearnPass& ps = p.passes[pi];
        CHECK(ps.chunk0 == chunk_at && ps.n_chunks >= 1 && ps.fam0 == fam_at && ps.n_fams >= 1);
        int64_t at = 0;
        for (int32_t c = ps.chunk0; c < ps.chunk0 + ps.n_chunks; ++c) {
            CHECK(size_t(c) < C && p.chunks[size_t(c)].count_at == at);
            pass_of_chunk[size_t(c)] = int32_t(pi);
            at += p.chunks[size_t(c)].cells;
        }
        CHECK(ps.cells == at && (at <= limit || ps.n_chunks == 1));
        chunk_at += ps.n_chunks;
        if (size_t(chunk_at) < C) CHECK(at + p.chunks[size_t(chunk_at)].cells > limit);   // the next chunk did not fit
        largest = std::max(largest, at);
        // the pass's families: those of its chunks, in input order, each range inside the pass and disjoint from the others
        std::vector<std::pair<int64_t, int64_t>> ranges;
        for (int32_t i = ps.fam0; i < ps.fam0 + ps.n_fams; ++i) {
            CHECK(size_t(i) < F);
            const int32_t f = p.order[size_t(i)];
            CHECK(pass_of_chunk[size_t(chunk_of[size_t(f)])] == int32_t(pi));
            if (i > ps.fam0) CHECK(p.order[size_t(i) - 1] < f);   // stable
            const int64_t c0 = p.fams[size_t(i)].count_at;
            CHECK(c0 == p.chunks[size_t(chunk_of[size_t(f)])].count_at + cell_in_chunk[size_t(f)]);
            CHECK(c0 >= 0 && c0 + p.fams[size_t(i)].entries <= ps.cells);
            ranges.emplace_back(c0, c0 + p.fams[size_t(i)].entries);
        }
        std::sort(ranges.begin(), ranges.end());
        for (size_t i = 1; i < ranges.size(); ++i) CHECK(ranges[i - 1].second <= ranges[i].first);
        fam_at += ps.n_fams;
    }
    CHECK(size_t(chunk_at) == C && size_t(fam_at) == F && p.scratch_cells == largest);
    return p.passes.size();
}

static void random_groups(uint64_t seed, long& plans, long& multi, long& cut, long& reordered) {
    std::mt19937_64 r(seed);
    const int32_t n = 48;
    std::vector<int32_t> k(static_cast<size_t>(n));
    const int kmax = rnd(r, 2, 6);
    for (int32_t& x : k) x = rnd(r, 1, kmax);
    std::vector<Group> gs(size_t(rnd(r, 0, 5)));
    for (size_t g = 0; g < gs.size(); ++g) {
        std::vector<int32_t> ids(size_t(n), 0);
        for (int32_t v = 0; v < n; ++v) ids[size_t(v)] = v;
        std::shuffle(ids.begin(), ids.end(), r);
        gs[g].child = g > 0 && rnd(r, 0, 2) == 0 ? gs[g - 1].child : ids[0];
        ids.erase(std::find(ids.begin(), ids.end(), gs[g].child));
        gs[g].base.assign(ids.begin(), ids.begin() + rnd(r, 0, 5));
        std::sort(gs[g].base.begin(), gs[g].base.end());
        const int n_cand = rnd(r, 0, 3) == 0 ? 0 : rnd(r, 0, 40);
        gs[g].cand.assign(ids.begin() + 5, ids.begin() + 5 + n_cand);
    }
    const std::vector<GroupIn> in = views(gs);
    GroupPlan whole;
    CHECK(plan_groups(k.data(), n, in, std::numeric_limits<int64_t>::max(), whole) == BN_OK);
    CHECK(check_group_plan(k, gs, std::numeric_limits<int64_t>::max(), whole) <= 1);
    int64_t total = 0, biggest = 1;
    for (const LearnChunk& c : whole.chunks) {
        total += c.cells;
        biggest = std::max<int64_t>(biggest, c.cells);
    }
    for (int64_t limit : {int64_t(1), biggest, biggest + int64_t(r() % uint64_t(total + 1)), (total + 1) / 2, total - 1, total}) {
        GroupPlan p;
        CHECK(plan_groups(k.data(), n, in, limit, p) == BN_OK);
        const size_t passes = check_group_plan(k, gs, limit, p);
        ++plans;
        if (limit >= total) CHECK(passes <= 1);
        if (limit == 1) CHECK(passes == p.chunks.size());
        if (passes > 1) ++multi;
        // a group whose families lie in more than one pass; a launch order that is not the input order
        std::vector<int32_t> first_pass(gs.size(), -1);
        bool any_cut = false;
        for (size_t pi = 0; pi < passes; ++pi)
            for (int32_t i = p.passes[pi].fam0; i < p.passes[pi].fam0 + p.passes[pi].n_fams; ++i) {
                size_t g = 0;
                int64_t at = 0;
                while (at + 1 + int64_t(gs[g].cand.size()) <= p.order[size_t(i)]) at += 1 + int64_t(gs[g++].cand.size());
                if (first_pass[g] < 0) first_pass[g] = int32_t(pi);
                any_cut = any_cut || first_pass[g] != int32_t(pi);
            }
        cut += any_cut;
        reordered += !std::is_sorted(p.order.begin(), p.order.end());
    }
}

static void random_subsets(uint64_t seed, long& plans, long& level_form) {
    std::mt19937_64 r(seed);
    const int32_t n = 16;
    std::vector<int32_t> k(static_cast<size_t>(n));
    const int kmax = rnd(r, 2, 6);
    for (int32_t& x : k) x = rnd(r, 1, kmax);
    std::vector<int32_t> ids(size_t(n), 0);
    for (int32_t v = 0; v < n; ++v) ids[size_t(v)] = v;
    std::shuffle(ids.begin(), ids.end(), r);
    const int32_t child = ids[0], n_base = rnd(r, 0, 4), m = rnd(r, 0, 6);
    const std::vector<int32_t> base(ids.begin() + 1, ids.begin() + 1 + n_base), cand(ids.begin() + 5, ids.begin() + 5 + m);   // (any order)
    // the top family's variables in increasing id
    std::vector<int32_t> var = base;
    var.insert(var.end(), cand.begin(), cand.end());
    std::sort(var.begin(), var.end());
    int64_t top = k[size_t(child)], all = top;
    for (int32_t u : var) {
        top *= k[size_t(u)];
        all *= std::find(cand.begin(), cand.end(), u) == cand.end() ? k[size_t(u)] : k[size_t(u)] + 1;
    }
    SubsetPlan p;
    const int status = plan_subsets(k.data(), n, child, n_base, base.data(), m, cand.data(), kLearnMaxScratchCells, p);
    CHECK((status == BN_OK) == (top <= kLearnMaxEntries && all <= kLearnMaxScratchCells));
    if (status != BN_OK) return;
    ++plans;
    const int32_t nv = n_base + m, n_fams = 1 << m, full = n_fams - 1, kc = k[size_t(child)];
    CHECK(p.nv == nv && p.n_fams == n_fams && p.kc == kc && p.id == var && int32_t(p.fams.size()) == n_fams);
    auto bit_of = [&](int32_t u) {
        const auto it = std::find(cand.begin(), cand.end(), u);
        return it == cand.end() ? -1 : int32_t(it - cand.begin());
    };
    auto kept = [&](int32_t mask, int32_t u) { return bit_of(u) < 0 || ((mask >> bit_of(u)) & 1); };
    int64_t at = 0;
    for (int32_t mask = 0; mask < n_fams; ++mask) {
        int64_t cells = kc;
        for (int32_t u : var)
            if (kept(mask, u)) cells *= k[size_t(u)];
        const LearnFamily& f = p.fams[size_t(mask)];
        CHECK(f.entries == cells && f.count_at == at && f.out_at == at && f.kc == kc && f.ku == 1 && f.low == 1);
        at += cells;
    }
    for (int32_t q = 0; q < nv; ++q) CHECK(p.k[size_t(q)] == k[size_t(var[size_t(q)])] && p.bit[size_t(q)] == bit_of(var[size_t(q)]));
    CHECK(p.all_cells == at && p.top_cells == p.fams[size_t(full)].entries && p.lds == (p.top_cells <= kLearnLdsCells));
    CHECK(p.chunks.size() == 1);
    const LearnChunk& ch = p.chunks[0];
    CHECK(ch.count_at == p.fams[size_t(full)].count_at && ch.child == child && ch.kc == kc && ch.base_at == 0 && ch.n_base == nv && ch.n_cand == 0 &&
          ch.base_cell == 0 && ch.cells == p.top_cells && ch.in_lds == (p.lds ? 1 : 0));
    CHECK(int32_t(p.level_at.size()) == m + 2 && int32_t(p.level_max.size()) == m + 1);
    if (p.lds) {
        CHECK(p.steps.empty());
        return;
    }
    ++level_form;
    // every non-top mask exactly once, in the level of its absent candidates, from the superset with the absent candidate of smallest id
    CHECK(int32_t(p.steps.size()) == full && p.level_at[size_t(m) + 1] == full);
    std::vector<int> made(size_t(n_fams), 0);
    for (int32_t l = 1; l <= m; ++l) {
        int32_t largest = 0;
        CHECK(p.level_at[size_t(l)] <= p.level_at[size_t(l) + 1]);
        for (int32_t i = p.level_at[size_t(l)]; i < p.level_at[size_t(l) + 1]; ++i) {
            const LatticeStep& st = p.steps[size_t(i)];
            int32_t mask = -1;
            for (int32_t x = 0; x < n_fams; ++x)
                if (p.fams[size_t(x)].count_at == st.out_at) mask = x;
            CHECK(mask >= 0 && mask != full && m - __builtin_popcount(unsigned(mask)) == l);
            ++made[size_t(mask)];
            int32_t x = -1;   // the absent candidate with the smallest id
            for (int32_t u : var)
                if (x < 0 && !kept(mask, u)) x = u;
            const int32_t sup = mask | (1 << bit_of(x));
            int64_t inner = kc;
            for (int32_t u : var)
                if (u > x && kept(mask, u)) inner *= k[size_t(u)];
            CHECK(st.in_at == p.fams[size_t(sup)].count_at && st.cells == p.fams[size_t(mask)].entries && st.kx == k[size_t(x)] && st.inner == inner);
            CHECK(int64_t(st.cells) * st.kx == p.fams[size_t(sup)].entries && st.cells % st.inner == 0);
            largest = std::max(largest, st.cells);
        }
        CHECK(p.level_max[size_t(l)] == largest);
    }
    for (int32_t mask = 0; mask < full; ++mask) CHECK(made[size_t(mask)] == 1);
}

// each limit: accepted at the boundary, refused one past it, with the ABI's text
static void limits() {
    auto refused = [](int r, const char* text) { return r == BN_ERR_ARG && g_msg.find(text) != std::string::npos; };
    std::vector<int32_t> ones(20, 1), ids(20, 0);
    for (int32_t v = 0; v < 20; ++v) ids[size_t(v)] = v;
    GroupPlan gp;
    SubsetPlan sp;
    const int64_t big = kLearnMaxScratchCells;
    // parents per family: 16
    CHECK(plan_groups(ones.data(), 20, {GroupIn{0, ids.data() + 1, 15, ids.data() + 16, 1}}, big, gp) == BN_OK && gp.fams.size() == 2);
    CHECK(refused(plan_groups(ones.data(), 20, {GroupIn{0, ids.data() + 1, 16, ids.data() + 17, 1}}, big, gp), "group 0: a family of 17 parents (at most 16)"));
    CHECK(plan_groups(ones.data(), 20, {GroupIn{0, ids.data() + 1, 16, nullptr, 0}}, big, gp) == BN_OK);
    CHECK(refused(plan_groups(ones.data(), 20, {GroupIn{0, ids.data() + 1, 17, nullptr, 0}}, big, gp), "a family of 17 parents"));
    CHECK(plan_subsets(ones.data(), 20, 0, 10, ids.data() + 1, 6, ids.data() + 11, big, sp) == BN_OK);
    CHECK(refused(plan_subsets(ones.data(), 20, 0, 10, ids.data() + 1, 7, ids.data() + 11, big, sp), "the top family has 17 parents (n_base + m at most 16)"));
    // entries per family: 2^20 = 4^10
    std::vector<int32_t> k(20, 4);
    k[10] = 1;
    k[11] = 2;
    CHECK(plan_groups(k.data(), 20, {GroupIn{0, ids.data() + 1, 9, ids.data() + 10, 1}}, big, gp) == BN_OK && gp.fams[1].entries == kLearnMaxEntries);
    CHECK(refused(plan_groups(k.data(), 20, {GroupIn{0, ids.data() + 1, 9, ids.data() + 10, 2}}, big, gp), "group 0: a family table of more than 2^20 entries"));
    CHECK(refused(plan_groups(k.data(), 20, {GroupIn{0, ids.data() + 1, 9, nullptr, 0}, GroupIn{0, ids.data() + 1, 11, nullptr, 0}}, big, gp), "group 1: a family table"));
    CHECK(plan_subsets(k.data(), 20, 0, 8, ids.data() + 1, 2, ids.data() + 9, big, sp) == BN_OK && sp.top_cells == kLearnMaxEntries);
    CHECK(refused(plan_subsets(k.data(), 20, 0, 8, ids.data() + 1, 3, ids.data() + 9, big, sp), "the top family's table has more than 2^20 (1048576) entries"));
    // cells of the 2^m tables of a subset call: the scratch limit (child 4, two candidates of arity 4: 4 * 5 * 5 = 100)
    CHECK(plan_subsets(k.data(), 20, 0, 0, nullptr, 2, ids.data() + 1, 100, sp) == BN_OK && sp.all_cells == 100);
    CHECK(refused(plan_subsets(k.data(), 20, 0, 0, nullptr, 2, ids.data() + 1, 99, sp), "the 2^2 count tables need 100 cells"));
    // and an empty batch is an empty plan
    CHECK(plan_groups(k.data(), 20, {}, big, gp) == BN_OK && gp.fams.empty() && gp.passes.empty());
}

int main() {
    long plans = 0, multi = 0, cut = 0, reordered = 0, subset_plans = 0, level_form = 0;
    for (g_case = 0; g_case < 300; ++g_case) random_groups(uint64_t(1000 + g_case), plans, multi, cut, reordered);
    for (g_case = 0; g_case < 400; ++g_case) random_subsets(uint64_t(5000 + g_case), subset_plans, level_form);
    g_case = -1;
    limits();
    // the cases the device never sees in one piece must have been there
    CHECK(multi > 300 && cut > 100 && reordered > 50 && level_form > 20);
    std::printf("ok: %ld group plans (%ld of several passes, %ld with a group cut by a pass, %ld reordered), %ld subset plans (%ld per level)\n", plans, multi,
                cut, reordered, subset_plans, level_form);
    return 0;
}
