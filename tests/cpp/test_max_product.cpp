// test_max_product.cpp -- bn::inference::max_product (include/bayesian/inference/max_product.hpp) over the repository's stand-in data
// model (include/compat): built and run by tests/test_cpp_max_product.py, needs a GPU.  Prints one JSON object; exit status = failures.
//   Pearl's network (libs/bayesian/test/belief_propagation.cpp:9-62) with H = 0: mpe() equals the assignment an enumeration of the
//   sixteen joint assignments finds; operator() equals run() bit for bit (and the test file compares both with the Python result);
//   reload() sees an edited CPT.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/inference/max_product.hpp>

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

// the joint probability of a complete assignment, from the spec
double joint(std::vector<node_spec> const& spec, std::vector<int> const& x)
{
    double p = 1.0;
    for(std::size_t v = 0; v < spec.size(); ++v)
    {
        std::size_t row = 0;
        for(int u : spec[v].parents) row = row * spec[u].arity + x[u];
        p *= spec[v].rows[row * spec[v].arity + x[v]];
    }
    return p;
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

    // enumeration: the best of the eight assignments with H = 0
    std::vector<int> best_x;
    double best = -1.0, second = -1.0;
    for(int code = 0; code < 8; ++code)
    {
        std::vector<int> x = {code >> 2 & 1, code >> 1 & 1, code & 1, 0};
        double const p = joint(spec, x);
        if(p > best) { second = best; best = p; best_x = x; }
        else if(p > second) second = p;
    }
    expect(second < best * (1.0 - 1e-9), "the best assignment of Pearl's network with H = 0 is not unique");

    bn::inference::max_product mp(pearl);
    mp.set_max_sweeps(50);
    auto const assignment = mp.mpe(pre);
    expect(mp.converged(), "max_product did not converge on Pearl's network");
    for(std::size_t i = 0; i < v.size(); ++i) expect(assignment.at(v[i]) == best_x[i], "mpe() differs from the enumeration");
    expect(std::fabs(mp.last_log_probability() - std::log(best)) <= 1e-12 * std::fabs(std::log(best)), "last_log_probability != log of the best joint");

    auto const map = mp(pre);
    auto const view = mp.run(pre);
    std::printf("{\"states\":[");
    for(std::size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? "," : "", assignment.at(v[i]));
    std::printf("],\"sweeps\":%d,\"log_probability\":%.17g,\"max_marginals\":[", mp.last_sweeps(), mp.last_log_probability());
    for(std::size_t i = 0; i < v.size(); ++i)
        for(std::size_t j = 0; j < 2; ++j)
        {
            double const a = map.at(v[i])[0][j], b = view.at(v[i])[j];
            expect(std::memcmp(&a, &b, sizeof a) == 0, "operator() and run() differ");
            std::printf("%s%.17g", (i || j) ? "," : "", a);
        }
    std::printf("],");

    // no evidence: the by-pass overloads agree as well
    {
        auto const m0 = mp(0.001);
        auto const v0 = mp.run(0.001);
        for(std::size_t i = 0; i < v.size(); ++i)
            for(std::size_t j = 0; j < 2; ++j)
            {
                double const a = m0.at(v[i])[0][j], b = v0.at(v[i])[j];
                expect(std::memcmp(&a, &b, sizeof a) == 0, "operator()(epsilon) and run(epsilon) differ");
            }
    }

    // reload(): an edited table is seen after it, not before (the functor flattened the tables in its constructor)
    {
        bn::condition_t cond;
        cond[v[0]] = 0;
        std::vector<double> const row = {0.0, 1.0};          // P(W | R = 0): was {1.0, 0.0}
        v[2]->cpt[cond].second.assign(row.begin(), row.end());
        spec[2].rows = {0.0, 1.0, 0.2, 0.8};
        auto const stale = mp.mpe(pre);
        for(std::size_t i = 0; i < v.size(); ++i) expect(stale.at(v[i]) == best_x[i], "an edited table was seen without reload()");
        mp.reload();
        auto const fresh = mp.mpe(pre);
        std::vector<int> nb;
        double b2 = -1.0;
        for(int code = 0; code < 8; ++code)
        {
            std::vector<int> x = {code >> 2 & 1, code >> 1 & 1, code & 1, 0};
            double const p = joint(spec, x);
            if(p > b2) { b2 = p; nb = x; }
        }
        expect(nb != best_x, "the edit does not change the most probable assignment: the test shows nothing");
        for(std::size_t i = 0; i < v.size(); ++i) expect(fresh.at(v[i]) == nb[i], "reload() did not bring the edited table in");
        bn::inference::max_product rebuilt(pearl);
        rebuilt.set_max_sweeps(50);
        auto const again = rebuilt.mpe(pre);
        for(std::size_t i = 0; i < v.size(); ++i) expect(again.at(v[i]) == fresh.at(v[i]), "reload() differs from a functor built from the edited network");
        std::printf("\"reloaded_states\":[");
        for(std::size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? "," : "", fresh.at(v[i]));
        std::printf("],");
    }

    // a non-zero code of the library becomes an exception
    {
        bool threw = false;
        try {
            std::unordered_map<bn::vertex_type, bn::matrix_type> bad;
            bad[v[0]] = bn::matrix_type(1, 3);   // three entries for a binary node
            mp(bad);
        } catch(std::runtime_error const&) { threw = true; }
        expect(threw, "malformed evidence did not throw");
    }
    std::printf("\"failures\":%d}\n", failures);
    return failures;
}
