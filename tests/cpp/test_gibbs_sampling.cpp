// test_gibbs_sampling.cpp -- bn::inference::gibbs_sampling (include/bayesian/inference/gibbs_sampling.hpp) over the repository's
// stand-in data model (include/compat): built and run by tests/test_cpp_gibbs_sampling.py, needs a GPU.  Prints one JSON object;
// exit status = failures.
//   Pearl's network (libs/bayesian/test/belief_propagation.cpp:9-62) with H = 0, seed 12345, 256 chains x 20 sweeps, 5 of them
//   burn-in: operator() equals run() bit for bit (and the test file compares both with the Python result); a second call runs
//   fresh chains; reload() sees an edited CPT; a non-zero code of the library becomes an exception.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/inference/gibbs_sampling.hpp>

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

std::uint64_t const kSeed = 12345, kChains = 256, kSweeps = 20, kBurnIn = 5;

}  // namespace

int main()
{
    auto spec = pearl_spec();
    bn::graph_t const pearl = build(spec);
    auto const v = pearl.vertex_list();
    bn::inference::gibbs_sampling::evidence_list ev;
    ev[v[3]] = 0;

    bn::inference::gibbs_sampling gs(pearl);
    gs.seed(kSeed);
    auto const map = gs(ev, kChains, kSweeps, kBurnIn);
    expect(gs.last_kept() == kChains * (kSweeps - kBurnIn), "last_kept is not chains x kept sweeps");
    auto const second = gs(ev, kChains, kSweeps, kBurnIn);     // chains 256 .. 511: fresh ones
    gs.seed(kSeed);
    auto const view = gs.run(ev, kChains, kSweeps, kBurnIn);   // chains 0 .. 255 again
    std::vector<double> first;
    bool fresh_differs = false;
    std::printf("{\"marginals\":[");
    for(std::size_t i = 0; i < v.size(); ++i)
    {
        double sum = 0.0;
        for(std::size_t j = 0; j < 2; ++j)
        {
            double const a = map.at(v[i])[0][j], b = view.at(v[i])[j], c = second.at(v[i])[0][j];
            expect(std::memcmp(&a, &b, sizeof a) == 0, "operator() and run() differ");
            fresh_differs = fresh_differs || std::memcmp(&a, &c, sizeof a) != 0;
            std::printf("%s%.17g", (i || j) ? "," : "", a);
            first.push_back(a);
            sum += a;
        }
        expect(std::fabs(sum - 1.0) < 1e-12, "a node's marginals do not sum to one");
    }
    std::printf("],");
    expect(fresh_differs, "a second call did not run fresh chains");
    expect(first[6] == 1.0 && first[7] == 0.0, "the evidence node is not at its clamp");
    // P(R = 0 | H = 0) = 0.2 / (0.2 + 0.8 x 0.09) = 0.735: 3 840 kept states of 256 chains sit well within 0.1 of it
    expect(std::fabs(first[0] - 0.2 / 0.272) < 0.1, "P(R | H = 0) is far from the enumeration's");

    // reload(): an edited table is seen after it, not before (the functor flattened the tables in its constructor)
    {
        bn::condition_t cond;
        std::vector<double> const row = {0.9, 0.1};          // P(R): was {0.2, 0.8}
        v[0]->cpt[cond].second.assign(row.begin(), row.end());
        gs.seed(kSeed);
        auto const stale = gs.run(ev, kChains, kSweeps, kBurnIn);
        for(std::size_t i = 0; i < v.size(); ++i)
            for(std::size_t j = 0; j < 2; ++j) expect(stale.at(v[i])[j] == first[2 * i + j], "an edited table was seen without reload()");
        gs.reload();
        gs.seed(kSeed);
        auto const fresh = gs.run(ev, kChains, kSweeps, kBurnIn);
        std::vector<double> reloaded;
        for(std::size_t i = 0; i < v.size(); ++i)
            for(std::size_t j = 0; j < 2; ++j) reloaded.push_back(fresh.at(v[i])[j]);
        expect(reloaded != first, "reload() did not bring the edited table in");
        bn::inference::gibbs_sampling rebuilt(pearl);
        rebuilt.seed(kSeed);
        auto const again = rebuilt.run(ev, kChains, kSweeps, kBurnIn);
        for(std::size_t i = 0; i < v.size(); ++i)
            for(std::size_t j = 0; j < 2; ++j)
                expect(again.at(v[i])[j] == reloaded[2 * i + j], "reload() differs from a functor built from the edited network");
        std::printf("\"reloaded_marginals\":[");
        for(std::size_t i = 0; i < reloaded.size(); ++i) std::printf("%s%.17g", i ? "," : "", reloaded[i]);
        std::printf("],");
    }

    // a non-zero code of the library becomes an exception
    {
        bool threw = false;
        try {
            bn::inference::gibbs_sampling::evidence_list bad;
            bad[v[0]] = 2;   // a third state of a binary node
            gs(bad);
        } catch(std::runtime_error const&) { threw = true; }
        expect(threw, "an unknown evidence state did not throw");
        threw = false;
        try { gs(ev, kChains, kSweeps, kBurnIn, 0); } catch(std::runtime_error const&) { threw = true; }
        expect(threw, "thin = 0 did not throw");
    }
    std::printf("\"stuck\":%llu,\"failures\":%d}\n", static_cast<unsigned long long>(gs.last_stuck()), failures);
    return failures;
}
