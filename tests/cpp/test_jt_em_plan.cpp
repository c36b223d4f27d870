// test_jt_em_plan.cpp -- the family tables of exact expectation-maximisation (bn_jt_plan.hpp: families, f_node, f_base, f_res) and the
// rows of a launch (bn_policy::jt_em_plan), stand-alone: compiled with bayesiannetwork_amd/csrc/bn_jt_plan.cpp and
// bn_engine_policy.cpp alone by plain g++ (tests/test_cpp_jt_em_plan.py also builds it with -fsanitize=address,undefined), no HIP and
// no library.  The walk does potentials, collect, distribute and the family read-out THE WAY jt_em_kernel INDEXES THEM -- the rows'
// posteriors in a `b` slice, the family totals in the first n cells of the region of the unnormalised marginals, every index through
// a bounds-checked access -- and is compared with the enumeration of the joint on Pearl's network and a 3 x 3 grid, rows with
// unobserved cells.  The rows-per-launch function is checked on both sides of each of its limits.
// Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "bn_engine_policy.hpp"
#include "bn_jt.hpp"   // (the rules this walk follows; the header is plain C++)
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
    unsigned long long seed = 2025;
};

constexpr int kMissing = kJtEmMissing;

static double two_level(const std::vector<double>& tab, int64_t base, const std::vector<int32_t>& res, int32_t off, int32_t cnt) {
    double total = 0.0;
    for (int32_t r = 0; r < cnt; r += kJtRun) {
        const int32_t hi = std::min(r + kJtRun, cnt);
        double run = 0.0;
        for (int32_t t = r; t < hi; ++t) run += tab.at(size_t(base + res.at(size_t(off + t))));
        total += run;
    }
    return total;
}

struct Row {
    std::vector<double> b;   // [S]
    int32_t skipped = 0;
    double p = 1.0;          // the product of the scales
};

// jt_em_kernel's phases over the item tables, one lane after the other
static Row walk(const Model& m, const JtPlan& P, const std::vector<uint8_t>& cells) {
    const int64_t S = m.cpt_off.back();
    std::vector<double> st(size_t(P.state_cells), -1.0);
    const int64_t sep0 = P.pot_cells, tot0 = sep0 + P.sep_cells, scl0 = tot0 + P.N;
    CHECK(P.n <= P.N);   // the n family totals fit the region of the unnormalised marginals
    CHECK(int64_t(P.families.size()) == P.n && int64_t(P.f_node.size()) == S && int64_t(P.f_base.size()) == S);
    for (int64_t g = 0; g < P.pot_cells; ++g) {   // base potential x the one-hot vectors of the observed home nodes
        const int32_t c = P.ent_clique.at(size_t(g));
        const JtClique& q = P.cliques.at(size_t(c));
        const int32_t e = int32_t(g) - q.pot_off;
        double v = 1.0;
        for (int32_t t = P.asg_ptr.at(size_t(c)); t < P.asg_ptr.at(size_t(c) + 1); ++t) {
            const JtAsg& s = P.asg.at(size_t(t));
            int64_t at = s.cpt_off;
            for (int32_t f = s.fam_lo; f < s.fam_hi; ++f) at += int64_t((e / P.fam.at(size_t(f)).stride) % P.fam[size_t(f)].k) * P.fam[size_t(f)].cstride;
            v *= m.cpt.at(size_t(at));
        }
        for (int32_t h = q.home_lo; h < q.home_hi; ++h) {
            const int32_t node = P.home_nodes.at(size_t(h));
            const JtNode& nd = P.nodes.at(size_t(node));
            const int cell = cells.at(size_t(node));
            if (cell != kMissing) v *= (e / nd.stride) % nd.k == cell ? 1.0 : 0.0;
        }
        st.at(size_t(g)) = v;
    }
    for (int32_t l = P.nlev - 1; l >= 0; --l) {   // collect
        const JtLevel& L = P.levels.at(size_t(l));
        for (int32_t gs = L.sep_lo; gs < L.sep_hi; ++gs) {
            const JtClique& q = P.cliques.at(size_t(P.sep_clique.at(size_t(gs))));
            st.at(size_t(sep0 + gs)) = two_level(st, q.pot_off + P.c_base.at(size_t(gs)), P.c_res, q.cres_off, q.cres_cnt);
        }
        for (int32_t c = L.c_lo; c < L.c_hi; ++c) {
            const JtClique& q = P.cliques.at(size_t(c));
            double s = 0.0;
            for (int32_t j = 0; j < q.sep_size; ++j) s += st.at(size_t(sep0 + q.sep_off + j));
            st.at(size_t(scl0 + c)) = s;
        }
        if (l == 0) break;
        const JtLevel& U = P.levels.at(size_t(l) - 1);
        for (int32_t g = U.pot_lo; g < U.pot_hi; ++g) {
            const JtClique& q = P.cliques.at(size_t(P.ent_clique.at(size_t(g))));
            double v = st.at(size_t(g));
            for (int32_t c = q.child_lo; c < q.child_hi; ++c) {
                const JtClique& ch = P.cliques.at(size_t(c));
                double msg = st.at(size_t(sep0 + ch.sep_off + P.up_map.at(size_t(ch.up_off + (g - q.pot_off)))));
                const double s = st.at(size_t(scl0 + c));
                if (s > 0.0) msg = msg / s;
                v *= msg;
            }
            st.at(size_t(g)) = v;
        }
    }
    for (int32_t l = 1; l < P.nlev; ++l) {   // distribute
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
            st.at(size_t(g)) *= st.at(size_t(sep0 + q.sep_off + P.dn_map.at(size_t(g))));
        }
    }
    // ---- the family read-out
    Row out;
    out.b.assign(size_t(S), -1.0);
    for (int64_t q = 0; q < S; ++q) {
        const int32_t v = P.f_node.at(size_t(q));
        const JtFamily& F = P.families.at(size_t(v));
        const JtClique& cq = P.cliques.at(size_t(P.cpt_clique.at(size_t(v))));
        CHECK(F.pot_off == cq.pot_off && q >= F.cpt_lo && q < F.cpt_lo + F.cpt_cnt);
        CHECK(F.cpt_lo == m.cpt_off[size_t(v)] && F.cpt_cnt == m.cpt_off[size_t(v) + 1] - m.cpt_off[size_t(v)]);
        CHECK(int64_t(F.cpt_cnt) * F.res_cnt == cq.size && F.res_cnt >= 1 && P.f_res.at(size_t(F.res_off)) == 0);
        const int32_t base = P.f_base.at(size_t(q));
        for (int32_t t = 0; t < F.res_cnt; ++t) {
            const int32_t r = P.f_res.at(size_t(F.res_off + t));
            CHECK(t == 0 || r > P.f_res[size_t(F.res_off + t - 1)]);   // ascending entry index
            CHECK(base + r >= 0 && base + r < cq.size);
            // the entry's digits are those of the flat CPT entry: own state last, first parent most significant
            const int32_t e = base + r;
            int64_t flat = 0;
            for (int32_t a = m.in_ptr[size_t(v)]; a < m.in_ptr[size_t(v) + 1]; ++a) {
                const int32_t u = m.in_idx[size_t(a)];
                const auto vs = P.vars.begin() + P.var_ptr[size_t(P.cpt_clique[size_t(v)])], ve = P.vars.begin() + P.var_ptr[size_t(P.cpt_clique[size_t(v)]) + 1];
                int32_t stride = 1;
                for (auto it = ve; it-- > vs && *it != u;) stride *= m.k[size_t(*it)];
                flat = flat * m.k[size_t(u)] + (e / stride) % m.k[size_t(u)];
            }
            {
                const auto vs = P.vars.begin() + P.var_ptr[size_t(P.cpt_clique[size_t(v)])], ve = P.vars.begin() + P.var_ptr[size_t(P.cpt_clique[size_t(v)]) + 1];
                int32_t stride = 1;
                for (auto it = ve; it-- > vs && *it != v;) stride *= m.k[size_t(*it)];
                flat = flat * m.k[size_t(v)] + (e / stride) % m.k[size_t(v)];
            }
            CHECK(F.cpt_lo + flat == q);
        }
        out.b.at(size_t(q)) = two_level(st, int64_t(F.pot_off) + base, P.f_res, F.res_off, F.res_cnt);
    }
    for (int32_t v = 0; v < P.n; ++v) {   // s_v into the first n cells of the marginals' region
        const JtFamily& F = P.families.at(size_t(v));
        double total = 0.0;
        for (int32_t r = 0; r < F.cpt_cnt; r += kJtRun) {
            double run = 0.0;
            for (int32_t t = r; t < std::min(r + kJtRun, F.cpt_cnt); ++t) run += out.b.at(size_t(F.cpt_lo + t));
            total += run;
        }
        CHECK(tot0 + v < scl0);
        st.at(size_t(tot0 + v)) = total;
    }
    for (int64_t q = 0; q < S; ++q) {
        const double s = st.at(size_t(tot0 + P.f_node.at(size_t(q))));
        out.b[size_t(q)] = s > 0.0 ? out.b[size_t(q)] / s : 0.0;
    }
    for (int32_t v = 0; v < P.n; ++v) out.skipped += st.at(size_t(tot0 + v)) > 0.0 ? 0 : 1;
    for (int32_t c = 0; c < P.nc; ++c) out.p *= st.at(size_t(scl0 + c));
    return out;
}

// P(x_v, pa(v) | e) in the flat CPT layout and P(e), by enumeration
static Row enumerate(const Model& m, const std::vector<uint8_t>& cells) {
    const int32_t n = m.n();
    Row out;
    out.b.assign(size_t(m.cpt_off.back()), 0.0);
    out.p = 0.0;
    std::vector<int32_t> x(size_t(n), 0);
    for (;;) {
        double w = 1.0;
        std::vector<int64_t> at(size_t(n), 0);
        for (int32_t v = 0; v < n; ++v) {
            int64_t row = 0;
            for (int32_t a = m.in_ptr[size_t(v)]; a < m.in_ptr[size_t(v) + 1]; ++a) row = row * m.k[size_t(m.in_idx[size_t(a)])] + x[size_t(m.in_idx[size_t(a)])];
            at[size_t(v)] = m.cpt_off[size_t(v)] + row * m.k[size_t(v)] + x[size_t(v)];
            w *= m.cpt[size_t(at[size_t(v)])];
            if (cells[size_t(v)] != kMissing && cells[size_t(v)] != x[size_t(v)]) w = 0.0;
        }
        out.p += w;
        for (int32_t v = 0; v < n; ++v) out.b[size_t(at[size_t(v)])] += w;
        int32_t v = n - 1;
        while (v >= 0 && ++x[size_t(v)] == m.k[size_t(v)]) x[size_t(v--)] = 0;
        if (v < 0) break;
    }
    if (out.p > 0.0)
        for (double& y : out.b) y /= out.p;
    return out;
}

static void check_case(const Model& m, const std::vector<uint8_t>& cells, int32_t skipped) {
    JtPlan P;
    build_jt_plan(m.n(), m.k.data(), m.in_ptr.data(), m.in_idx.data(), m.cpt_off.data(), kJtScratchCells, P);
    CHECK(P.ok);
    const Row got = walk(m, P, cells);
    const Row want = enumerate(m, cells);
    CHECK(got.skipped == skipped);
    CHECK(std::fabs(got.p - want.p) <= 1e-12 * std::max(want.p, 1e-300));
    if (skipped) return;
    for (size_t q = 0; q < got.b.size(); ++q) CHECK(std::fabs(got.b[q] - want.b[q]) <= 1e-12);
}

static void check_rows_per_launch() {
    using bn_policy::EmPlan;
    using bn_policy::jt_em_plan;
    const int32_t S = 100;
    // form 1: em_plan's rows -- the b scratch, the table, the launch's workgroup limit
    CHECK(jt_em_plan(1000, S, 100 * S, 1, 5000, 1).chunk == 100);
    CHECK(jt_em_plan(1000, S, 100 * S - 1, 1, 5000, 1).chunk == 99);
    CHECK(jt_em_plan(1000, S, S - 1, 1, 5000, 1).chunk == 1);          // below one row: still one
    CHECK(jt_em_plan(50, S, 100 * S, 1, 5000, 1).chunk == 50);         // the table
    CHECK(jt_em_plan(1 << 20, 1, int64_t(1) << 40, 1, 5000, 1).chunk == bn_policy::kEmMaxChunk);
    // form 2: also the state slices the junction tree's scratch holds
    CHECK(jt_em_plan(1000, S, 100 * S, 2, 5000, 7 * 5000).chunk == 7);
    CHECK(jt_em_plan(1000, S, 100 * S, 2, 5000, 7 * 5000 - 1).chunk == 6);
    CHECK(jt_em_plan(1000, S, 100 * S, 2, 5000, 4999).chunk == 1);     // below one slice: still one
    CHECK(jt_em_plan(1000, S, 100 * S, 2, 5000, 100 * 5000).chunk == 100);
    CHECK(jt_em_plan(1000, S, 100 * S, 2, 5000, 101 * 5000).chunk == 100);   // the b scratch binds
    CHECK(jt_em_plan(1000, S, 100 * S, 2, 5000, 99 * 5000).chunk == 99);
    // the cut covers the table once, in order, and closes every block once whatever the chunk
    for (int form = 1; form <= 2; ++form)
        for (int64_t rows : {1, 255, 256, 257, 513, 1000}) {
            const EmPlan p = jt_em_plan(rows, S, 100 * S, form, 5000, 37 * 5000);
            CHECK(p.chunk == std::min<int64_t>(rows, form == 2 ? 37 : 100));
            CHECK(p.scratch == int64_t(p.chunk) * S && p.n_blocks == (rows + 255) / 256);
            int64_t next = 0, closes = 0;
            for (int64_t c = 0; c < p.n_chunks; ++c) {
                const bn_policy::EmChunk k = bn_policy::em_chunk(p, rows, c);
                CHECK(k.first == next && k.count >= 1 && k.count <= p.chunk);
                next += k.count;
                closes += k.closes;
            }
            CHECK(next == rows && closes == p.n_blocks);
        }
}

int main() {
    const uint8_t X = uint8_t(kMissing);
    {   // Pearl's network: R, S, W <- R, H <- R, S
        Model m;
        m.add(2, {}, {0.2, 0.8});
        m.add(2, {}, {0.1, 0.9});
        m.add(2, {0}, {1.0, 0.0, 0.2, 0.8});
        m.add(2, {0, 1}, {1.0, 0.0, 1.0, 0.0, 0.9, 0.1, 0.0, 1.0});
        check_case(m, {X, X, X, X}, 0);
        check_case(m, {X, X, X, 0}, 0);
        check_case(m, {1, X, 1, X}, 0);
        check_case(m, {1, 0, 1, 0}, 0);      // fully observed: every b is 0 or 1
        check_case(m, {0, X, 1, X}, 4);      // probability 0: every family of the tree is skipped
    }
    {   // 3 x 3 grid, parents UP then LEFT (not ascending for the inner nodes' flat order to differ from the clique's), mixed arities
        Model m;
        for (int32_t r = 0; r < 3; ++r)
            for (int32_t c = 0; c < 3; ++c) {
                std::vector<int32_t> ps;
                if (c) ps.push_back(r * 3 + c - 1);
                if (r) ps.push_back((r - 1) * 3 + c);
                m.add(2 + (r + c) % 2, ps);
            }
        check_case(m, {X, X, X, X, X, X, X, X, X}, 0);
        check_case(m, {1, X, X, X, 0, X, X, X, 1}, 0);
        check_case(m, {X, 2, X, 1, X, X, 0, X, X}, 0);
        check_case(m, {0, 1, 1, 2, 0, 1, 1, 0, 1}, 0);
    }
    check_rows_per_launch();
    std::printf("ok: %ld checks\n", g_checks);
    return 0;
}
