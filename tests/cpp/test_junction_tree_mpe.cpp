// test_junction_tree_mpe.cpp -- bn::inference::junction_tree::mpe (include/bayesian/inference/junction_tree.hpp), the C++ face of
// bn_jt_mpe_run, over the repository's stand-in data model (include/compat): built and run by tests/test_cpp_jt_mpe.py, needs a GPU.
// Prints one JSON object; exit status = failures.
//   Pearl's network with H = 0: the decoded assignment is the argmax of the enumeration of the eight joint assignments, its log
//   probability log of the best to 1e-12 relative, the max-marginals equal the enumeration's to 1e-12; mpe() without evidence; the
//   marginals of operator() are not disturbed by an mpe() between two calls; malformed evidence throws.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/inference/junction_tree.hpp>

namespace {

struct node_spec {
    int arity;
    std::vector<int> parents;
    std::vector<double> rows;   // row-major, first parent slowest
};

bn::graph_t build(std::vector<node_spec> const& spec)
{
    bn::graph_t g;
    for(std::size_t i = 0; i < spec.size(); ++i)
    {
        auto v = g.add_vertex();
        v->id = static_cast<int>(i) + 1;
        v->selectable_num = spec[i].arity;
    }
    auto const vl = g.vertex_list();
    for(std::size_t i = 0; i < spec.size(); ++i)
        for(int p : spec[i].parents)
            if(!g.add_edge(vl[p], vl[i])) std::printf("add_edge failed\n");
    for(std::size_t i = 0; i < spec.size(); ++i)
    {
        std::vector<bn::vertex_type> ps;
        for(int p : spec[i].parents) ps.push_back(vl[p]);
        vl[i]->cpt.assign(ps, vl[i]);
        std::vector<int> st(ps.size(), 0);
        std::size_t const k = spec[i].arity;
        for(std::size_t r = 0; r * k < spec[i].rows.size(); ++r)
        {
            bn::condition_t cond;
            for(std::size_t j = 0; j < ps.size(); ++j) cond[ps[j]] = st[j];
            vl[i]->cpt[cond].second.assign(spec[i].rows.begin() + r * k, spec[i].rows.begin() + (r + 1) * k);
            for(std::size_t j = ps.size(); j-- > 0;)
            {
                if(++st[j] < spec[spec[i].parents[j]].arity) break;
                st[j] = 0;
            }
        }
    }
    return g;
}

// R, S, W <- R, H <- R, S (all binary)
std::vector<node_spec> pearl_spec()
{
    return {{2, {}, {0.2, 0.8}},
            {2, {}, {0.1, 0.9}},
            {2, {0}, {1.0, 0.0, 0.2, 0.8}},
            {2, {0, 1}, {1.0, 0.0, 1.0, 0.0, 0.9, 0.1, 0.0, 1.0}}};
}

int failures = 0;
void expect(bool ok, char const* what)
{
    if(!ok) { ++failures; std::printf("FAIL %s\n", what); }
}

// over the assignments with H = h (h < 0: all sixteen): the largest joint probability, its assignment, the max-marginals [v][s]
double enumerate(std::vector<node_spec> const& spec, int h, int best_x[4], double mm[4][2])
{
    double best = -1.0;
    for(int v = 0; v < 4; ++v) mm[v][0] = mm[v][1] = 0;
    for(int code = 0; code < 16; ++code)
    {
        int const x[4] = {code >> 3 & 1, code >> 2 & 1, code >> 1 & 1, code & 1};
        if(h >= 0 && x[3] != h) continue;
        double p = 1.0;
        for(std::size_t v = 0; v < spec.size(); ++v)
        {
            std::size_t row = 0;
            for(int u : spec[v].parents) row = row * spec[u].arity + x[u];
            p *= spec[v].rows[row * spec[v].arity + x[v]];
        }
        if(p > best) { best = p; std::memcpy(best_x, x, sizeof x); }
        for(int v = 0; v < 4; ++v) mm[v][x[v]] = std::fmax(mm[v][x[v]], p);
    }
    return best;
}

}  // namespace

int main()
{
    auto const spec = pearl_spec();
    bn::graph_t const pearl = build(spec);
    auto const v = pearl.vertex_list();
    std::unordered_map<bn::vertex_type, bn::matrix_type> pre;
    bn::matrix_type h0(1, 2);
    h0[0][0] = 1.0; h0[0][1] = 0.0;
    pre[v[3]] = h0;

    bn::inference::junction_tree jt(pearl);
    auto const before = jt(pre);

    int want_x[4];
    double want_mm[4][2];
    double const best = enumerate(spec, 0, want_x, want_mm);
    auto const got = jt.mpe(pre);
    auto const mm = jt.max_marginals();
    expect(got.first.size() == 4, "mpe() does not name every vertex");
    expect(std::fabs(got.second - std::log(best)) <= 1e-12 * std::fabs(std::log(best)), "log probability != log of the best joint");
    std::printf("{\"log_p\":%.17g,\"states\":[", got.second);
    for(std::size_t i = 0; i < v.size(); ++i)
    {
        expect(got.first.at(v[i]) == want_x[i], "a state differs from the enumeration's argmax");
        std::printf("%s%d", i ? "," : "", got.first.at(v[i]));
    }
    std::printf("],\"max_marginals\":[");
    for(std::size_t i = 0; i < v.size(); ++i)
        for(std::size_t j = 0; j < 2; ++j)
        {
            double const a = mm.at(v[i])[j];
            expect(std::fabs(a - want_mm[i][j] / (want_mm[i][0] + want_mm[i][1])) <= 1e-12, "a max-marginal differs from the enumeration");
            std::printf("%s%.17g", (i || j) ? "," : "", a);
        }
    std::printf("],");

    // the marginals of operator() are what they were before the mpe() call
    {
        auto const after = jt(pre);
        for(std::size_t i = 0; i < v.size(); ++i)
            for(std::size_t j = 0; j < 2; ++j)
            {
                double const a = before.at(v[i])[0][j], b = after.at(v[i])[0][j];
                expect(std::memcmp(&a, &b, sizeof a) == 0, "operator() differs after an mpe() call");
            }
    }

    // no evidence
    {
        int x0[4];
        double mm0[4][2];
        double const best0 = enumerate(spec, -1, x0, mm0);
        auto const free = jt.mpe();
        expect(std::fabs(free.second - std::log(best0)) <= 1e-12 * std::fabs(std::log(best0)), "mpe() without evidence: log probability");
        for(std::size_t i = 0; i < v.size(); ++i) expect(free.first.at(v[i]) == x0[i], "mpe() without evidence: a state");
    }

    // a non-zero code of the library becomes an exception
    {
        bool threw = false;
        try {
            std::unordered_map<bn::vertex_type, bn::matrix_type> bad;
            bad[v[0]] = bn::matrix_type(1, 3);   // three entries for a binary node
            jt.mpe(bad);
        } catch(std::runtime_error const&) { threw = true; }
        expect(threw, "malformed evidence did not throw");
    }
    std::printf("\"failures\":%d}\n", failures);
    return failures;
}
