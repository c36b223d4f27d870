// test_jt_plan.cpp -- the junction-tree planner (bayesiannetwork_amd/csrc/bn_jt_plan.cpp) stand-alone: compiled with that file alone
// by plain g++ (tests/test_cpp_jt_plan.py also builds it with -fsanitize=address,undefined), no HIP and no library.  Every case
// checks the tree (families inside their cliques, running intersection, separators, levels) and walks the ITEM TABLES the way the
// kernel does -- every index through a bounds-checked access -- and compares the marginals with the enumeration of the joint.
// Cases: one node, two unconnected nodes, a chain, a collider, a 3 x 3 grid, a 13-variable clique, the scratch budget at exactly
// the plan's size and one cell below, a clique of exactly 2^20 entries and the next size up.
// Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>

#include "bn_jt_plan.hpp"

using namespace bnmi;

static long g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

struct Model {
    std::vector<int32_t> k, in_ptr{0}, in_idx;
    std::vector<int64_t> cpt_off{0};
    std::vector<double> cpt;
    int32_t n() const { return int32_t(k.size()); }
    void add(int32_t arity, std::vector<int32_t> parents, bool values = true) {
        int64_t rows = 1;
        for (int32_t p : parents) { in_idx.push_back(p); rows *= k[size_t(p)]; }
        in_ptr.push_back(int32_t(in_idx.size()));
        k.push_back(arity);
        cpt_off.push_back(cpt_off.back() + rows * arity);
        if (!values) return;
        for (int64_t r = 0; r < rows; ++r) {
            std::vector<double> row(size_t(arity), 0.0);
            double s = 0;
            for (double& x : row) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; x = 0.05 + double(seed >> 40) / double(1 << 24); s += x; }
            for (double x : row) cpt.push_back(x / s);
        }
    }
    unsigned long long seed = 12345;
};

static JtPlan plan_of(const Model& m, int64_t budget = kJtScratchCells) {
    JtPlan p;
    build_jt_plan(m.n(), m.k.data(), m.in_ptr.data(), m.in_idx.data(), m.cpt_off.data(), budget, p);
    return p;
}

static std::vector<int32_t> slice(const std::vector<int32_t>& v, const std::vector<int32_t>& ptr, int32_t c) {
    return std::vector<int32_t>(v.begin() + ptr.at(size_t(c)), v.begin() + ptr.at(size_t(c) + 1));
}

// the properties of a junction tree
static void check_tree(const Model& m, const JtPlan& P) {
    CHECK(P.built && P.nc >= 1 && int32_t(P.parent.size()) == P.nc);
    for (int32_t c = 0; c < P.nc; ++c) {
        const std::vector<int32_t> vs = slice(P.vars, P.var_ptr, c), ss = slice(P.sep_vars, P.sep_ptr, c);
        CHECK(!vs.empty() && std::is_sorted(vs.begin(), vs.end()) && std::adjacent_find(vs.begin(), vs.end()) == vs.end());
        const int32_t p = P.parent[size_t(c)];
        if (p < 0) { CHECK(P.level[size_t(c)] == 0 && ss.empty()); continue; }
        CHECK(p < c && P.level[size_t(c)] == P.level[size_t(p)] + 1);
        const std::vector<int32_t> ps = slice(P.vars, P.var_ptr, p);
        std::vector<int32_t> both;
        std::set_intersection(vs.begin(), vs.end(), ps.begin(), ps.end(), std::back_inserter(both));
        CHECK(both == ss && !ss.empty());
        CHECK(!std::includes(ps.begin(), ps.end(), vs.begin(), vs.end()));   // maximal cliques only
    }
    for (int32_t v = 0; v < m.n(); ++v) {
        const std::vector<int32_t> cs = slice(P.vars, P.var_ptr, P.cpt_clique.at(size_t(v))), hs = slice(P.vars, P.var_ptr, P.home.at(size_t(v)));
        CHECK(std::binary_search(cs.begin(), cs.end(), v) && std::binary_search(hs.begin(), hs.end(), v));
        for (int32_t a = m.in_ptr[size_t(v)]; a < m.in_ptr[size_t(v) + 1]; ++a) CHECK(std::binary_search(cs.begin(), cs.end(), m.in_idx[size_t(a)]));
        int tops = 0;   // running intersection: exactly one clique that holds v has no parent holding v
        for (int32_t c = 0; c < P.nc; ++c) {
            const std::vector<int32_t> vs = slice(P.vars, P.var_ptr, c);
            if (!std::binary_search(vs.begin(), vs.end(), v)) continue;
            const int32_t p = P.parent[size_t(c)];
            const std::vector<int32_t> ps = p < 0 ? std::vector<int32_t>() : slice(P.vars, P.var_ptr, p);
            tops += std::binary_search(ps.begin(), ps.end(), v) ? 0 : 1;
        }
        CHECK(tops == 1);
    }
}

static double two_level(const std::vector<double>& st, int64_t base, const std::vector<int32_t>& res, int32_t off, int32_t cnt) {
    double total = 0.0;
    for (int32_t r = 0; r < cnt; r += kJtRun) {
        double run = 0.0;
        for (int32_t t = r; t < std::min(r + kJtRun, cnt); ++t) run += st.at(size_t(base + res.at(size_t(off + t))));
        total += run;
    }
    return total;
}

// the kernel's phases over the item tables, one lane after the other
static std::vector<double> emulate(const Model& m, const JtPlan& P, const std::vector<std::vector<double>>& ev, double* p_e) {
    std::vector<double> st(size_t(P.state_cells), -1.0);
    const int64_t sep0 = P.pot_cells, marg0 = sep0 + P.sep_cells, scl0 = marg0 + P.N;
    for (int64_t g = 0; g < P.pot_cells; ++g) {   // base potential x evidence
        const JtClique& q = P.cliques.at(size_t(P.ent_clique.at(size_t(g))));
        const int32_t e = int32_t(g) - q.pot_off;
        CHECK(e >= 0 && e < q.size);
        double v = 1.0;
        const int32_t c = P.ent_clique[size_t(g)];
        for (int32_t t = P.asg_ptr.at(size_t(c)); t < P.asg_ptr.at(size_t(c) + 1); ++t) {
            const JtAsg& s = P.asg.at(size_t(t));
            int64_t at = s.cpt_off;
            for (int32_t f = s.fam_lo; f < s.fam_hi; ++f) at += int64_t((e / P.fam.at(size_t(f)).stride) % P.fam[size_t(f)].k) * P.fam[size_t(f)].cstride;
            CHECK(at >= m.cpt_off[size_t(s.node)] && at < m.cpt_off[size_t(s.node) + 1]);
            v *= m.cpt.at(size_t(at));
        }
        for (int32_t h = q.home_lo; h < q.home_hi; ++h) {
            const int32_t node = P.home_nodes.at(size_t(h));
            const JtNode& nd = P.nodes.at(size_t(node));
            if (!ev[size_t(node)].empty()) v *= ev[size_t(node)].at(size_t((e / nd.stride) % nd.k));
        }
        st.at(size_t(g)) = v;
    }
    for (int32_t l = P.nlev - 1; l >= 0; --l) {
        const JtLevel& L = P.levels.at(size_t(l));
        for (int32_t gs = L.sep_lo; gs < L.sep_hi; ++gs) {
            const JtClique& q = P.cliques.at(size_t(P.sep_clique.at(size_t(gs))));
            CHECK(q.level == l);
            st.at(size_t(sep0 + gs)) = two_level(st, q.pot_off + P.c_base.at(size_t(gs)), P.c_res, q.cres_off, q.cres_cnt);
        }
        for (int32_t c = L.c_lo; c < L.c_hi; ++c) {
            double s = 0.0;
            for (int32_t j = 0; j < P.cliques.at(size_t(c)).sep_size; ++j) s += st.at(size_t(sep0 + P.cliques[size_t(c)].sep_off + j));
            st.at(size_t(scl0 + c)) = s;
        }
        if (l == 0) break;
        const JtLevel& U = P.levels.at(size_t(l) - 1);
        for (int32_t g = U.pot_lo; g < U.pot_hi; ++g) {
            const JtClique& q = P.cliques.at(size_t(P.ent_clique.at(size_t(g))));
            double v = st.at(size_t(g));
            for (int32_t c = q.child_lo; c < q.child_hi; ++c) {
                const JtClique& ch = P.cliques.at(size_t(c));
                CHECK(ch.parent == P.ent_clique[size_t(g)]);
                const int32_t j = P.up_map.at(size_t(ch.up_off + (g - q.pot_off)));
                CHECK(j >= 0 && j < ch.sep_size);
                double msg = st.at(size_t(sep0 + ch.sep_off + j));
                const double s = st.at(size_t(scl0 + c));
                if (s > 0.0) msg = msg / s;
                v *= msg;
            }
            st.at(size_t(g)) = v;
        }
    }
    for (int32_t l = 1; l < P.nlev; ++l) {
        const JtLevel& L = P.levels.at(size_t(l));
        for (int32_t gs = L.sep_lo; gs < L.sep_hi; ++gs) {
            const int32_t c = P.sep_clique.at(size_t(gs));
            const JtClique& q = P.cliques.at(size_t(c));
            const double nw = two_level(st, P.cliques.at(size_t(q.parent)).pot_off + P.p_base.at(size_t(gs)), P.p_res, q.pres_off, q.pres_cnt);
            double msg = st.at(size_t(sep0 + gs));
            const double s = st.at(size_t(scl0 + c));
            if (s > 0.0) msg = msg / s;
            st.at(size_t(sep0 + gs)) = msg == 0.0 ? 0.0 : nw / msg;
        }
        for (int32_t g = L.pot_lo; g < L.pot_hi; ++g) {
            const JtClique& q = P.cliques.at(size_t(P.ent_clique.at(size_t(g))));
            const int32_t j = P.dn_map.at(size_t(g));
            CHECK(j >= 0 && j < q.sep_size);
            st.at(size_t(g)) *= st.at(size_t(sep0 + q.sep_off + j));
        }
    }
    std::vector<double> bel(size_t(P.N), 0.0);
    for (int32_t i = 0; i < P.N; ++i) {
        const JtNode& nd = P.nodes.at(size_t(P.elem_node.at(size_t(i))));
        const JtClique& q = P.cliques.at(size_t(nd.home));
        const int32_t cnt = q.size / nd.k, span = nd.stride * nd.k;
        double total = 0.0;
        for (int32_t r = 0; r < cnt; r += kJtRun) {
            double run = 0.0;
            for (int32_t t = r; t < std::min(r + kJtRun, cnt); ++t)
                run += st.at(size_t(q.pot_off + (i - nd.bel_off) * nd.stride + (t / nd.stride) * span + t % nd.stride));
            total += run;
        }
        st.at(size_t(marg0 + i)) = total;
    }
    for (int32_t i = 0; i < P.N; ++i) {
        const JtNode& nd = P.nodes[size_t(P.elem_node[size_t(i)])];
        double tot = 0.0;
        for (int32_t x = 0; x < nd.k; ++x) tot += st.at(size_t(marg0 + nd.bel_off + x));
        bel[size_t(i)] = st[size_t(marg0 + i)] / tot;
    }
    *p_e = 1.0;
    for (int32_t c = 0; c < P.nc; ++c) *p_e *= st.at(size_t(scl0 + c));
    return bel;
}

// P(x_v, e) for every node by enumeration of the joint
static std::vector<double> enumerate(const Model& m, const std::vector<std::vector<double>>& ev, double* p_e) {
    const int32_t n = m.n();
    std::vector<int64_t> off(size_t(n) + 1, 0);
    for (int32_t v = 0; v < n; ++v) off[size_t(v) + 1] = off[size_t(v)] + m.k[size_t(v)];
    std::vector<double> acc(static_cast<size_t>(off[size_t(n)]), 0.0);
    std::vector<int32_t> x(size_t(n), 0);
    double total = 0.0;
    for (;;) {
        double w = 1.0;
        for (int32_t v = 0; v < n; ++v) {
            int64_t row = 0;
            for (int32_t a = m.in_ptr[size_t(v)]; a < m.in_ptr[size_t(v) + 1]; ++a) row = row * m.k[size_t(m.in_idx[size_t(a)])] + x[size_t(m.in_idx[size_t(a)])];
            w *= m.cpt[size_t(m.cpt_off[size_t(v)] + row * m.k[size_t(v)] + x[size_t(v)])];
            if (!ev[size_t(v)].empty()) w *= ev[size_t(v)][size_t(x[size_t(v)])];
        }
        total += w;
        for (int32_t v = 0; v < n; ++v) acc[size_t(off[size_t(v)] + x[size_t(v)])] += w;
        int32_t v = n - 1;
        while (v >= 0 && ++x[size_t(v)] == m.k[size_t(v)]) x[size_t(v--)] = 0;
        if (v < 0) break;
    }
    for (double& a : acc) a /= total;
    *p_e = total;
    return acc;
}

static void check_case(const Model& m, int32_t want_cliques, int64_t want_max) {
    const JtPlan P = plan_of(m);
    CHECK(P.ok);
    check_tree(m, P);
    if (want_cliques > 0) CHECK(P.nc == want_cliques);
    if (want_max > 0) CHECK(P.max_clique == want_max);
    std::vector<std::vector<double>> none(size_t(m.n())), some(size_t(m.n()));
    for (int32_t v = 0; v < m.n(); v += 3) {   // hard on node 0, soft with a zero on the others
        some[size_t(v)].assign(size_t(m.k[size_t(v)]), v == 0 ? 0.0 : 0.7);
        some[size_t(v)][size_t(m.k[size_t(v)]) - 1] = v == 0 ? 1.0 : 0.0;
        if (v != 0) some[size_t(v)][0] = 0.3;
    }
    for (const auto& ev : {none, some}) {
        double pe = 0, want_pe = 0;
        const std::vector<double> got = emulate(m, P, ev, &pe), want = enumerate(m, ev, &want_pe);
        CHECK(got.size() == want.size());
        for (size_t i = 0; i < got.size(); ++i) CHECK(std::fabs(got[i] - want[i]) <= 1e-12);
        CHECK(std::fabs(pe - want_pe) <= 1e-12 * want_pe);
    }
}

int main() {
    { Model m; m.add(3, {}); check_case(m, 1, 3); }
    { Model m; m.add(2, {}); m.add(3, {}); check_case(m, 2, 3); CHECK(plan_of(m).nlev == 1); }   // two roots
    { Model m; m.add(3, {}); for (int32_t v = 1; v < 7; ++v) m.add(2 + v % 2, {v - 1}); check_case(m, 6, 9); CHECK(plan_of(m).nlev == 4); }   // rooted at its centre
    { Model m; m.add(2, {}); m.add(3, {}); m.add(2, {0, 1}); check_case(m, 1, 12); }              // collider: one clique
    {   // 3 x 3 grid, parents left and up
        Model m;
        for (int32_t r = 0; r < 3; ++r)
            for (int32_t c = 0; c < 3; ++c) {
                std::vector<int32_t> ps;
                if (r) ps.push_back((r - 1) * 3 + c);
                if (c) ps.push_back(r * 3 + c - 1);
                m.add(2 + (r + c) % 2, ps);
            }
        check_case(m, 0, 0);
        CHECK(plan_of(m).max_clique_vars <= 4);   // (the moralised grid has treewidth 3, and min-fill finds it)
    }
    {   // a 13-variable clique: twelve binary roots, their common child, its child
        Model m;
        std::vector<int32_t> roots;
        for (int32_t v = 0; v < 12; ++v) { m.add(2, {}); roots.push_back(v); }
        m.add(2, roots);
        m.add(3, {12});
        check_case(m, 2, 8192);
        const JtPlan P = plan_of(m);
        CHECK(P.max_clique_vars == 13 && jt_form(P, 0) == 2 && jt_form(P, 1) == 0 && jt_form(P, 2) == 2);
        // the scratch budget at exactly the plan's size, and one cell below
        const JtPlan fits = plan_of(m, P.state_cells);
        CHECK(fits.ok && !fits.cliques.empty());
        JtPlan tight = plan_of(m, P.state_cells - 1);
        CHECK(tight.built && !tight.ok && tight.cliques.empty() && tight.why.find("scratch budget of " + std::to_string(P.state_cells - 1)) != std::string::npos);
        CHECK(jt_form(tight, 0) == 0 && jt_form(tight, 2) == 0);
        jt_apply_budget(tight, P.state_cells);
        CHECK(tight.ok && tight.why.empty());
        jt_apply_budget(tight, P.state_cells - 1);
        CHECK(!tight.ok);
    }
    { Model m; m.add(2, {}); m.add(2, {0}); const JtPlan P = plan_of(m); CHECK(jt_form(P, 0) == 1 && jt_form(P, 1) == 1 && jt_form(P, 2) == 2); }
    for (int32_t roots : {19, 20}) {   // a clique of exactly 2^20 entries, and the next size up
        Model m;
        std::vector<int32_t> ps;
        for (int32_t v = 0; v < roots; ++v) { m.add(2, {}, false); ps.push_back(v); }
        m.add(2, ps, false);
        const JtPlan P = plan_of(m);
        if (roots == 19) {
            CHECK(P.ok && P.nc == 1 && P.max_clique == kJtMaxClique && P.max_clique_vars == 20 && int64_t(P.ent_clique.size()) == kJtMaxClique);
            check_tree(m, P);
            CHECK(*std::max_element(P.c_res.begin(), P.c_res.end()) == kJtMaxClique - 1);
        } else {
            CHECK(!P.built && !P.ok && P.cliques.empty());
            CHECK(P.why.find("21 variables and 2097152 entries") != std::string::npos && P.why.find("limit of 1048576") != std::string::npos);
        }
    }
    std::printf("ok: %ld checks\n", g_checks);
    return 0;
}
