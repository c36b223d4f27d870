// test_junction_tree.cpp -- bn::inference::junction_tree (include/bayesian/inference/junction_tree.hpp) over the repository's stand-in
// data model (include/compat): built and run by tests/test_cpp_junction_tree.py, needs a GPU.  Prints one JSON object; exit status =
// failures.
//   Pearl's network (libs/bayesian/test/belief_propagation.cpp:9-62) with H = 0: the marginals equal the enumeration of the sixteen
//   joint assignments to 1e-12 and log_evidence() equals log P(H = 0); operator() equals run() bit for bit (and the test file compares
//   both with the Python result); reload() sees an edited CPT.
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

// P(x_v = s, H = 0) for the four binary nodes [v][s], and P(H = 0), by enumeration
double enumerate(std::vector<node_spec> const& spec, double out[4][2])
{
    double total = 0;
    for(int v = 0; v < 4; ++v) out[v][0] = out[v][1] = 0;
    for(int code = 0; code < 8; ++code)
    {
        int const x[4] = {code >> 2 & 1, code >> 1 & 1, code & 1, 0};
        double p = 1.0;
        for(std::size_t v = 0; v < spec.size(); ++v)
        {
            std::size_t row = 0;
            for(int u : spec[v].parents) row = row * spec[u].arity + x[u];
            p *= spec[v].rows[row * spec[v].arity + x[v]];
        }
        total += p;
        for(int v = 0; v < 4; ++v) out[v][x[v]] += p;
    }
    return total;
}

}  // namespace

int main()
{
    auto spec = pearl_spec();
    bn::graph_t const pearl = build(spec);
    auto const v = pearl.vertex_list();
    std::unordered_map<bn::vertex_type, bn::matrix_type> pre;
    bn::matrix_type h0(1, 2);
    h0[0][0] = 1.0; h0[0][1] = 0.0;
    pre[v[3]] = h0;

    double want[4][2];
    double const pe = enumerate(spec, want);

    bn::inference::junction_tree jt(pearl);
    auto const map = jt(pre);
    double const lg_map = jt.log_evidence();
    auto const view = jt.run(pre);
    expect(lg_map == jt.log_evidence(), "log_evidence() of operator() and run() differ");
    expect(std::fabs(jt.log_evidence() - std::log(pe)) <= 1e-12 * std::fabs(std::log(pe)), "log_evidence() != log P(H = 0)");
    std::printf("{\"log_evidence\":%.17g,\"beliefs\":[", jt.log_evidence());
    for(std::size_t i = 0; i < v.size(); ++i)
        for(std::size_t j = 0; j < 2; ++j)
        {
            double const a = map.at(v[i])[0][j], b = view.at(v[i])[j];
            expect(std::memcmp(&a, &b, sizeof a) == 0, "operator() and run() differ");
            expect(std::fabs(a - want[i][j] / pe) <= 1e-12, "a marginal differs from the enumeration");
            std::printf("%s%.17g", (i || j) ? "," : "", a);
        }
    std::printf("],");

    // no evidence: the by-pass overloads agree as well, and log P() = 0
    {
        auto const m0 = jt();
        auto const v0 = jt.run();
        expect(std::fabs(jt.log_evidence()) <= 1e-12, "log_evidence() without evidence is not 0");
        for(std::size_t i = 0; i < v.size(); ++i)
            for(std::size_t j = 0; j < 2; ++j)
            {
                double const a = m0.at(v[i])[0][j], b = v0.at(v[i])[j];
                expect(std::memcmp(&a, &b, sizeof a) == 0, "operator()() and run() differ");
            }
    }

    // reload(): an edited table is seen after it, not before (the functor flattened the tables in its constructor)
    {
        bn::condition_t cond;
        cond[v[0]] = 0;
        std::vector<double> const row = {0.0, 1.0};          // P(W | R = 0): was {1.0, 0.0}
        v[2]->cpt[cond].second.assign(row.begin(), row.end());
        spec[2].rows = {0.0, 1.0, 0.2, 0.8};
        auto const stale = jt(pre);
        for(std::size_t i = 0; i < v.size(); ++i)
            for(std::size_t j = 0; j < 2; ++j) expect(stale.at(v[i])[0][j] == map.at(v[i])[0][j], "an edited table was seen without reload()");
        jt.reload();
        auto const fresh = jt(pre);
        double edited[4][2];
        double const pe2 = enumerate(spec, edited);
        expect(std::fabs(edited[2][0] / pe2 - want[2][0] / pe) > 1e-3, "the edit does not change W's marginal: the test shows nothing");
        std::printf("\"reloaded_beliefs\":[");
        for(std::size_t i = 0; i < v.size(); ++i)
            for(std::size_t j = 0; j < 2; ++j)
            {
                expect(std::fabs(fresh.at(v[i])[0][j] - edited[i][j] / pe2) <= 1e-12, "reload() did not bring the edited table in");
                std::printf("%s%.17g", (i || j) ? "," : "", fresh.at(v[i])[0][j]);
            }
        std::printf("],");
        bn::inference::junction_tree rebuilt(pearl);
        auto const again = rebuilt(pre);
        for(std::size_t i = 0; i < v.size(); ++i)
            for(std::size_t j = 0; j < 2; ++j)
                expect(again.at(v[i])[0][j] == fresh.at(v[i])[0][j], "reload() differs from a functor built from the edited network");
    }

    // a non-zero code of the library becomes an exception
    {
        bool threw = false;
        try {
            std::unordered_map<bn::vertex_type, bn::matrix_type> bad;
            bad[v[0]] = bn::matrix_type(1, 3);   // three entries for a binary node
            jt(bad);
        } catch(std::runtime_error const&) { threw = true; }
        expect(threw, "malformed evidence did not throw");
    }
    std::printf("\"failures\":%d}\n", failures);
    return failures;
}
