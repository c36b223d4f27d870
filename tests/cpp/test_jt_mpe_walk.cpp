// test_jt_mpe_walk.cpp -- exact MPE on the junction tree (bn_jt.hpp, "Exact MPE") as a HOST WALK of the planner's item tables, stand-alone:
// compiled with bayesiannetwork_amd/csrc/bn_jt_plan.cpp alone by plain g++ (tests/test_cpp_jt_mpe_walk.py also builds it with
// -fsanitize=address,undefined), no HIP and no library.  The walk does collect, pick, distribute, read-out and states THE WAY
// jt_mpe_kernel INDEXES THEM -- the picks within the N doubles of the unnormalised marginals, every index through a bounds-checked access -- and is
// compared with the enumeration of the joint on Pearl's network (no evidence, H = 0, a soft vector), the two-node tie network
// (decoded to (0, 1), which per-node decoding cannot give) and a 3 x 3 grid.
// Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "bn_jt.hpp"   // (the rules this walk follows; the header is plain C++)
#include "bn_jt_plan.hpp"

using namespace bnmi;

static_assert(kJtMax == 2 && kJtSum == 1, "bn_get_info \"jt_last_kind\": 1 a sum run, 2 a max run");

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
    // rows empty: random strictly positive rows
    void add(int32_t arity, std::vector<int32_t> parents, std::vector<double> rows = {}) {
        int64_t nrows = 1;
        for (int32_t p : parents) { in_idx.push_back(p); nrows *= k.at(size_t(p)); }
        in_ptr.push_back(int32_t(in_idx.size()));
        k.push_back(arity);
        cpt_off.push_back(cpt_off.back() + nrows * arity);
        if (!rows.empty()) { CHECK(int64_t(rows.size()) == nrows * arity); cpt.insert(cpt.end(), rows.begin(), rows.end()); return; }
        for (int64_t r = 0; r < nrows; ++r) {
            std::vector<double> row(size_t(arity), 0.0);
            double s = 0;
            for (double& x : row) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; x = 0.05 + double(seed >> 40) / double(1 << 24); s += x; }
            for (double x : row) cpt.push_back(x / s);
        }
    }
    unsigned long long seed = 2024;
};

struct Result {
    std::vector<double> mm;        // [N] normalised max-marginals
    std::vector<int32_t> states;   // [n]
    double best = 1.0;             // the product of the scales
};

static double max_fold(const std::vector<double>& st, int64_t base, const std::vector<int32_t>& res, int32_t off, int32_t cnt) {
    double acc = 0.0;
    for (int32_t t = 0; t < cnt; ++t) {
        const double x = st.at(size_t(base + res.at(size_t(off + t))));
        acc = acc < x ? x : acc;
    }
    return acc;
}

// jt_mpe_kernel's phases over the item tables, one lane after the other
static Result walk(const Model& m, const JtPlan& P, const std::vector<std::vector<double>>& ev) {
    std::vector<double> st(size_t(P.state_cells), -1.0);
    CHECK(P.nc <= P.n && P.n <= P.N);             // the picks, nc int32, fit the region of the unnormalised marginals, N doubles
    std::vector<int32_t> pick(size_t(P.nc), -1);
    const int64_t sep0 = P.pot_cells, marg0 = sep0 + P.sep_cells, scl0 = marg0 + P.N;
    for (int64_t g = 0; g < P.pot_cells; ++g) {   // base potential x evidence
        const int32_t c = P.ent_clique.at(size_t(g));
        const JtClique& q = P.cliques.at(size_t(c));
        const int32_t e = int32_t(g) - q.pot_off;
        CHECK(e >= 0 && e < q.size);
        double v = 1.0;
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
    // ---- collect
    for (int32_t l = P.nlev - 1; l >= 0; --l) {
        const JtLevel& L = P.levels.at(size_t(l));
        for (int32_t gs = L.sep_lo; gs < L.sep_hi; ++gs) {
            const JtClique& q = P.cliques.at(size_t(P.sep_clique.at(size_t(gs))));
            CHECK(q.level == l);
            st.at(size_t(sep0 + gs)) = max_fold(st, q.pot_off + P.c_base.at(size_t(gs)), P.c_res, q.cres_off, q.cres_cnt);
        }
        for (int32_t c = L.c_lo; c < L.c_hi; ++c) {
            const JtClique& q = P.cliques.at(size_t(c));
            double s = 0.0;
            for (int32_t j = 0; j < q.sep_size; ++j) {
                const double x = st.at(size_t(sep0 + q.sep_off + j));
                s = s < x ? x : s;
            }
            st.at(size_t(scl0 + c)) = s;
            if (l == 0) {   // a root's entries are final
                CHECK(q.parent < 0 && q.size >= 1);
                int32_t at = 0;
                double best = st.at(size_t(q.pot_off));
                for (int32_t i = 1; i < q.size; ++i) {
                    const double x = st.at(size_t(q.pot_off + i));
                    if (x > best) { best = x; at = i; }
                }
                pick.at(size_t(c)) = at;
            }
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
    // ---- distribute, the picks of a level in the phase of its ratios
    for (int32_t l = 1; l < P.nlev; ++l) {
        const JtLevel& L = P.levels.at(size_t(l));
        for (int32_t gs = L.sep_lo; gs < L.sep_hi; ++gs) {
            const int32_t c = P.sep_clique.at(size_t(gs));
            const JtClique& q = P.cliques.at(size_t(c));
            const double nw = max_fold(st, P.cliques.at(size_t(q.parent)).pot_off + P.p_base.at(size_t(gs)), P.p_res, q.pres_off, q.pres_cnt);
            double msg = st.at(size_t(sep0 + gs));
            const double s = st.at(size_t(scl0 + c));
            if (s > 0.0) msg = msg / s;
            st.at(size_t(sep0 + gs)) = msg == 0.0 ? 0.0 : nw / msg;
        }
        for (int32_t c = L.c_hi - 1; c >= L.c_lo; --c) {
            const JtClique& q = P.cliques.at(size_t(c));
            const int32_t up = pick.at(size_t(q.parent));
            CHECK(up >= 0 && up < P.cliques.at(size_t(q.parent)).size);   // written by the level above
            const int32_t j = P.up_map.at(size_t(q.up_off + up));
            CHECK(j >= 0 && j < q.sep_size);
            const int32_t base = P.c_base.at(size_t(q.sep_off + j));
            CHECK(q.cres_cnt >= 1);
            int32_t at = P.c_res.at(size_t(q.cres_off));
            double best = st.at(size_t(q.pot_off + base + at));
            for (int32_t t = 1; t < q.cres_cnt; ++t) {
                const int32_t r = P.c_res.at(size_t(q.cres_off + t));
                CHECK(r > P.c_res[size_t(q.cres_off + t - 1)]);   // ascending entry index
                CHECK(base + r < q.size);
                const double x = st.at(size_t(q.pot_off + base + r));
                if (x > best) { best = x; at = r; }
            }
            CHECK(P.dn_map.at(size_t(q.pot_off + base + at)) == j);   // the pick lies in the separator entry its parent chose
            pick.at(size_t(c)) = base + at;
        }
        for (int32_t g = L.pot_lo; g < L.pot_hi; ++g) {
            const JtClique& q = P.cliques.at(size_t(P.ent_clique.at(size_t(g))));
            const int32_t j = P.dn_map.at(size_t(g));
            CHECK(j >= 0 && j < q.sep_size);
            st.at(size_t(g)) *= st.at(size_t(sep0 + q.sep_off + j));
        }
    }
    // ---- read-out, states
    Result out;
    out.mm.assign(size_t(P.N), 0.0);
    out.states.assign(size_t(P.n), -1);
    for (int32_t i = 0; i < P.N; ++i) {
        const JtNode& nd = P.nodes.at(size_t(P.elem_node.at(size_t(i))));
        const JtClique& q = P.cliques.at(size_t(nd.home));
        const int32_t cnt = q.size / nd.k, span = nd.stride * nd.k;
        double acc = 0.0;
        for (int32_t t = 0; t < cnt; ++t) {
            const int32_t at = (i - nd.bel_off) * nd.stride + (t / nd.stride) * span + t % nd.stride;
            CHECK(at >= 0 && at < q.size);
            const double x = st.at(size_t(q.pot_off + at));
            acc = acc < x ? x : acc;
        }
        st.at(size_t(marg0 + i)) = acc;
    }
    for (int32_t i = 0; i < P.N; ++i) {
        const JtNode& nd = P.nodes[size_t(P.elem_node[size_t(i)])];
        double tot = 0.0;
        for (int32_t x = 0; x < nd.k; ++x) tot += st.at(size_t(marg0 + nd.bel_off + x));
        out.mm[size_t(i)] = st[size_t(marg0 + i)] / tot;
    }
    for (int32_t v = 0; v < P.n; ++v) {
        const JtNode& nd = P.nodes.at(size_t(v));
        const int32_t at = pick.at(size_t(nd.home));
        CHECK(at >= 0 && at < P.cliques.at(size_t(nd.home)).size);
        out.states[size_t(v)] = (at / nd.stride) % nd.k;
    }
    for (int32_t c = 0; c < P.nc; ++c) out.best *= st.at(size_t(scl0 + c));
    return out;
}

struct Brute {
    std::vector<double> mm;
    std::vector<int32_t> states;
    double best = -1.0, second = -1.0;
};

// max-marginals (normalised), the first maximiser in ascending assignment order, the best and second-best weights
static Brute enumerate(const Model& m, const std::vector<std::vector<double>>& ev) {
    const int32_t n = m.n();
    std::vector<int64_t> off(size_t(n) + 1, 0);
    for (int32_t v = 0; v < n; ++v) off[size_t(v) + 1] = off[size_t(v)] + m.k[size_t(v)];
    Brute b;
    b.mm.assign(size_t(off[size_t(n)]), 0.0);
    std::vector<int32_t> x(size_t(n), 0);
    for (;;) {
        double w = 1.0;
        for (int32_t v = 0; v < n; ++v) {
            int64_t row = 0;
            for (int32_t a = m.in_ptr[size_t(v)]; a < m.in_ptr[size_t(v) + 1]; ++a) row = row * m.k[size_t(m.in_idx[size_t(a)])] + x[size_t(m.in_idx[size_t(a)])];
            w *= m.cpt[size_t(m.cpt_off[size_t(v)] + row * m.k[size_t(v)] + x[size_t(v)])];
            if (!ev[size_t(v)].empty()) w *= ev[size_t(v)][size_t(x[size_t(v)])];
        }
        if (w > b.best) { b.second = b.best; b.best = w; b.states = x; }
        else if (w > b.second) b.second = w;
        for (int32_t v = 0; v < n; ++v) b.mm[size_t(off[size_t(v)] + x[size_t(v)])] = std::max(b.mm[size_t(off[size_t(v)] + x[size_t(v)])], w);
        int32_t v = n - 1;
        while (v >= 0 && ++x[size_t(v)] == m.k[size_t(v)]) x[size_t(v--)] = 0;
        if (v < 0) break;
    }
    for (int32_t v = 0; v < n; ++v) {
        double tot = 0.0;
        for (int64_t i = off[size_t(v)]; i < off[size_t(v) + 1]; ++i) tot += b.mm[size_t(i)];
        for (int64_t i = off[size_t(v)]; i < off[size_t(v) + 1]; ++i) b.mm[size_t(i)] /= tot;
    }
    return b;
}

static Result check_case(const Model& m, const std::vector<std::vector<double>>& ev, bool decided) {
    JtPlan P;
    build_jt_plan(m.n(), m.k.data(), m.in_ptr.data(), m.in_idx.data(), m.cpt_off.data(), kJtScratchCells, P);
    CHECK(P.ok);
    const Result got = walk(m, P, ev);
    const Brute want = enumerate(m, ev);
    CHECK(got.mm.size() == want.mm.size());
    for (size_t i = 0; i < got.mm.size(); ++i) CHECK(std::fabs(got.mm[i] - want.mm[i]) <= 1e-12);
    CHECK(std::fabs(got.best - want.best) <= 1e-12 * want.best);
    if (decided) {   // one maximiser, by a margin: the decoded assignment is it
        CHECK(want.second < want.best * (1 - 1e-9));
        CHECK(got.states == want.states);
    }
    return got;
}

int main() {
    {   // Pearl's network: R, S, W <- R, H <- R, S
        Model m;
        m.add(2, {}, {0.2, 0.8});
        m.add(2, {}, {0.1, 0.9});
        m.add(2, {0}, {1.0, 0.0, 0.2, 0.8});
        m.add(2, {0, 1}, {1.0, 0.0, 1.0, 0.0, 0.9, 0.1, 0.0, 1.0});
        std::vector<std::vector<double>> ev(4);
        check_case(m, ev, true);
        ev[3] = {1.0, 0.0};                       // H = 0
        check_case(m, ev, true);
        ev[3].clear();
        ev[2] = {0.3, 0.9};                       // a soft vector on W
        check_case(m, ev, true);
    }
    {   // the tie network: node 0 uniform, node 1 = "not node 0"
        Model m;
        m.add(2, {}, {0.5, 0.5});
        m.add(2, {0}, {0.0, 1.0, 1.0, 0.0});
        const Result r = check_case(m, std::vector<std::vector<double>>(2), false);
        CHECK(r.mm == std::vector<double>({0.5, 0.5, 0.5, 0.5}));
        CHECK(r.states == std::vector<int32_t>({0, 1}));   // per-node argmax would give (0, 0), probability 0
        CHECK(r.best == 0.5);
    }
    {   // 3 x 3 grid, parents left and up, mixed arities; also with evidence
        Model m;
        for (int32_t r = 0; r < 3; ++r)
            for (int32_t c = 0; c < 3; ++c) {
                std::vector<int32_t> ps;
                if (r) ps.push_back((r - 1) * 3 + c);
                if (c) ps.push_back(r * 3 + c - 1);
                m.add(2 + (r + c) % 2, ps);
            }
        std::vector<std::vector<double>> ev(9);
        check_case(m, ev, true);
        ev[0] = {0.0, 1.0};
        ev[4] = {0.7, 0.2};
        ev[8] = {0.0, 1.0};
        check_case(m, ev, true);
    }
    std::printf("ok: %ld checks\n", g_checks);
    return 0;
}
