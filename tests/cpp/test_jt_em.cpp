// test_jt_em.cpp -- bn::learning::junction_tree_em (include/bayesian/learning/junction_tree_em.hpp) over the repository's
// stand-in data model (include/compat): built and run by tests/test_cpp_jt_em.py, needs a GPU.  Prints one JSON object; exit status =
// failures.
//   Pearl's network (libs/bayesian/test/belief_propagation.cpp:9-62) with strictly positive starting tables and a table of eight rows
//   with unobserved cells: the functor writes the fitted tables into the vertices' cpt (every row sums to 1, the tables changed), returns
//   the iteration count, and what it prints is compared bit for bit with Engine.jt_em_fit by the test file.  A complete table with prior 0
//   gives the relative frequencies.  Malformed arguments become exceptions.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/learning/junction_tree_em.hpp>

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

// R, S, W <- R, H <- R, S (all binary): Pearl's structure, strictly positive tables
std::vector<node_spec> start_spec()
{
    return {{2, {}, {0.3, 0.7}},
            {2, {}, {0.4, 0.6}},
            {2, {0}, {0.9, 0.1, 0.2, 0.8}},
            {2, {0, 1}, {0.7, 0.3, 0.6, 0.4, 0.8, 0.2, 0.1, 0.9}}};
}

int failures = 0;
void expect(bool ok, char const* what)
{
    if(!ok) { ++failures; std::printf("FAIL %s\n", what); }
}

// the graph's tables, flat: nodes in vertex_list() order, rows in table order
std::vector<double> tables(bn::graph_t const& g) { return bn::mi355x::flatten(g).cpt; }

}  // namespace

int main()
{
    auto const spec = start_spec();
    bn::graph_t const graph = build(spec);
    std::uint8_t const M = bn::learning::junction_tree_em::missing;
    expect(M == 255, "missing != 255");
    std::vector<std::uint8_t> const patterns = {0, 1, M, 0,   1, M, 1, 1,   M, M, M, M,   1, 0, 0, M,
                                                0, 0, 1, 1,   M, 1, M, 0,   1, 1, 1, 0,   M, 0, M, 1};
    std::vector<std::uint64_t> const counts = {5, 3, 2, 7, 1, 4, 6, 2};
    std::vector<double> const before = tables(graph);

    bn::learning::junction_tree_em em(graph);
    bn::learning::jt_em_options opt;
    opt.max_iters = 5;
    opt.tol = 0.0;
    int const iters = em(graph, patterns, counts, opt);
    expect(iters == 5, "tol = 0 must run max_iters iterations");
    expect(em.delta_history().size() == 5, "one delta per iteration");
    std::vector<double> const fitted = tables(graph);
    expect(fitted.size() == before.size() && fitted != before, "the vertices' tables were not replaced");
    for(std::size_t q = 0; q + 1 < fitted.size(); q += 2)
        expect(std::fabs(fitted[q] + fitted[q + 1] - 1.0) <= 1e-15, "a fitted row does not sum to 1");
    std::printf("{\"iters\":%d,\"cpt\":[", iters);
    for(std::size_t q = 0; q < fitted.size(); ++q) std::printf("%s%.17g", q ? "," : "", fitted[q]);
    std::printf("],\"deltas\":[");
    for(std::size_t q = 0; q < em.delta_history().size(); ++q) std::printf("%s%.17g", q ? "," : "", em.delta_history()[q]);
    expect(em.loglik_history().size() == 5, "one log-likelihood per iteration");
    std::printf("],\"logliks\":[");
    for(std::size_t q = 0; q < em.loglik_history().size(); ++q) std::printf("%s%.17g", q ? "," : "", em.loglik_history()[q]);
    std::printf("],\"skipped\":%lld,", em.last_skipped());

    // a second call starts from the tables the graph holds now: it continues the iteration
    {
        opt.max_iters = 1;
        int const one = em(graph, patterns, counts, opt);
        expect(one == 1, "max_iters = 1");
        std::vector<double> const sixth = tables(graph);
        std::printf("\"sixth\":[");
        for(std::size_t q = 0; q < sixth.size(); ++q) std::printf("%s%.17g", q ? "," : "", sixth[q]);
        std::printf("],");
    }

    // a complete table, prior 0: the relative frequencies after one iteration (sampler::make_cpt's result)
    {
        bn::graph_t const g2 = build(spec);
        std::vector<std::uint8_t> const full = {0, 0, 0, 0,   0, 1, 0, 1,   1, 0, 1, 0,   1, 1, 1, 1,   1, 1, 0, 1};
        std::vector<std::uint64_t> const c2 = {2, 1, 3, 1, 1};
        bn::learning::junction_tree_em em2(g2);
        opt.max_iters = 1;
        em2(g2, full, c2, opt);
        std::vector<double> const t = tables(g2);
        double const n = 8.0;
        expect(t[0] == 3.0 / n && t[1] == 5.0 / n, "P(R) is not the relative frequency");
        expect(t[2] == 5.0 / n && t[3] == 3.0 / n, "P(S) is not the relative frequency");
        expect(t[4] == 1.0 && t[5] == 0.0 && t[6] == 1.0 / 5.0 && t[7] == 4.0 / 5.0, "P(W | R) is not the relative frequency");
    }

    // malformed arguments become exceptions
    {
        bool threw = false;
        try { std::vector<std::uint8_t> bad = patterns; bad[1] = 2; em(graph, bad, counts, opt); } catch(std::runtime_error const&) { threw = true; }
        expect(threw, "a state above the arity did not throw");
        threw = false;
        try { std::vector<std::uint64_t> short_counts(3, 1); em(graph, patterns, short_counts, opt); } catch(std::runtime_error const&) { threw = true; }
        expect(threw, "a count vector of the wrong length did not throw");
        threw = false;
        try { opt.max_iters = 0; em(graph, patterns, counts, opt); } catch(std::runtime_error const&) { threw = true; }
        expect(threw, "max_iters = 0 did not throw");
    }
    std::printf("\"failures\":%d}\n", failures);
    return failures;
}
