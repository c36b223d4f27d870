// tests/cpp/test_bd.cpp -- the Bayesian-Dirichlet scores of the C++ drop-in (include/bayesian/evaluation/bdeu.hpp) under
// bn::learning::greedy, k2_algorithm and simulated_annealing, over this repository's stand-in data model (-Iinclude -Iinclude/compat),
// C++14.
//   test_bd NET.dsc SAMPLES SEED T0 T1 RATE
// NET.dsc gives the nodes and arities (its edges are dropped); SAMPLES is the sampler's file format.  Runs, each from the empty
// graph and with the same seed, so with the same shuffles and the same stream:
//   greedy<bdeu> (the learner on the device) and greedy<bdeu_literal> (a trivial subclass: the reference's literal loop, one
//   evaluation of the whole graph per candidate), k2_algorithm<k2_score> and its literal twin with a precondition,
//   simulated_annealing<bdeu> with one chain and its literal twin, and with 16 chains.
// The literal twins evaluate through the same device function as the learner, so edges AND scores must agree bit for bit.
// Prints one JSON object: per run the edges [parent, child] as positions in vertex_list(), the score, and (greedy, k2) the visits.
#include <cstdio>
#include <cstdlib>
#include <ratio>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include <bayesian/evaluation/bdeu.hpp>
#include <bayesian/graph.hpp>
#include <bayesian/learning/greedy.hpp>
#include <bayesian/learning/k2_algorithm.hpp>
#include <bayesian/learning/simulated_annealing.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/serializer/dsc.hpp>

namespace {

struct bdeu_literal : bn::evaluation::bdeu {
    bdeu_literal(bn::sampler const& s) : bn::evaluation::bdeu(s) {}
};
struct k2_literal : bn::evaluation::k2_score {
    k2_literal(bn::sampler const& s) : bn::evaluation::k2_score(s) {}
};

static_assert(bn::learning::detail::criterion_of<bn::evaluation::bdeu>::value == 2, "bdeu runs on the device");
static_assert(bn::learning::detail::criterion_of<bn::evaluation::basic_bdeu<std::ratio<5, 2>>>::value == 2, "any ess does");
static_assert(bn::learning::detail::criterion_of<bn::evaluation::k2_score>::value == 3, "k2_score runs on the device");
static_assert(bn::learning::detail::criterion_of<bdeu_literal>::value == -1 && bn::learning::detail::criterion_of<k2_literal>::value == -1,
              "a subclass takes the literal loop");

int position(bn::graph_t const& g, bn::vertex_type const& v)
{
    auto const& vl = g.vertex_list();
    for(std::size_t i = 0; i < vl.size(); ++i)
        if(vl[i] == v) return static_cast<int>(i);
    return -1;
}

void print_run(char const* name, bn::graph_t const& g, double score, std::vector<bn::learning::visit_t> const& visits, bool last)
{
    std::printf("\"%s\":{\"score\":%.17g,\"edges\":[", name, score);
    bool first = true;
    for(auto const& child : g.vertex_list())
        for(auto const& parent : g.in_vertexes(child))
        {
            std::printf("%s[%d,%d]", first ? "" : ",", position(g, parent), position(g, child));
            first = false;
        }
    std::printf("],\"visits\":[");
    for(std::size_t i = 0; i < visits.size(); ++i)
    {
        std::printf("%s[%d,[", i ? "," : "", position(g, visits[i].child));
        for(std::size_t j = 0; j < visits[i].candidates.size(); ++j) std::printf("%s%d", j ? "," : "", position(g, visits[i].candidates[j]));
        std::printf("]]");
    }
    std::printf("]}%s", last ? "" : ",");
}

template<class Eval>
double anneal(bn::sampler const& sampling, bn::graph_t& g, int chains, std::uint64_t seed, double t0, double t1, double rate,
              std::vector<std::pair<double, double>>* uphill = nullptr)
{
    bn::learning::simulated_annealing<Eval> sa(sampling);
    sa.set_chains(chains);
    sa.set_max_parents(2);
    sa.set_seed(seed);
    sa.set_rule(1);
    double const score = sa(g, t0, t1, rate);
    if(uphill) *uphill = sa.last_uphill();
    return score;
}

} // namespace

int main(int argc, char** argv)
{
    if(argc < 7) { std::fprintf(stderr, "usage: test_bd NET.dsc SAMPLES SEED T0 T1 RATE\n"); return 2; }
    try
    {
        bn::graph_t base = bn::serializer::dsc().from_file(argv[1]);
        base.erase_all_edge();
        auto const seed = static_cast<std::uint32_t>(std::strtoul(argv[3], nullptr, 10));
        double const t0 = std::atof(argv[4]), t1 = std::atof(argv[5]), rate = std::atof(argv[6]);
        bn::sampler sampling(argv[2]);
        if(!sampling.load_sample(base.vertex_list())) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        auto const nodes = base.vertex_list();
        std::vector<bn::learning::visit_t> const none;
        std::printf("{\"n\":%zu,", nodes.size());
        {
            bn::graph_t g = base, h = base;   // (copies share the vertices: each run fits its own CPTs at its end)
            bn::learning::greedy<bn::evaluation::bdeu> device(sampling, seed);
            double const s = device(g);
            print_run("greedy_bdeu", g, s, device.last_visits(), false);
            std::printf("\"greedy_bdeu_eval\":%.17g,", bn::evaluation::bdeu(sampling)(g));
            std::printf("\"greedy_bdeu_eval_ess\":%.17g,", bn::evaluation::basic_bdeu<std::ratio<5, 2>>(sampling)(g));
            std::printf("\"greedy_bdeu_eval_head\":%.17g,", bn::evaluation::bdeu(sampling)(g, {nodes[1], nodes[0]}));
            bn::learning::greedy<bdeu_literal> literal(sampling, seed);
            double const r = literal(h);
            print_run("greedy_bdeu_literal", h, r, literal.last_visits(), false);
        }
        {
            std::unordered_map<bn::vertex_type, std::vector<bn::vertex_type>> pre;
            pre[nodes[3]] = {nodes[0], nodes[1], nodes[2]};
            bn::graph_t g = base, h = base;
            bn::learning::k2_algorithm<bn::evaluation::k2_score> device(sampling, seed);
            double const s = device(g, pre);
            print_run("k2_k2", g, s, device.last_visits(), false);
            bn::learning::k2_algorithm<k2_literal> literal(sampling, seed);
            double const r = literal(h, pre);
            print_run("k2_k2_literal", h, r, literal.last_visits(), false);
        }
        {
            bn::graph_t g = base, h = base, many = base;
            double const s = anneal<bn::evaluation::bdeu>(sampling, g, 1, seed, t0, t1, rate);
            print_run("anneal_bdeu", g, s, none, false);
            std::vector<std::pair<double, double>> uphill;   // (u, p) of every uphill decision of the literal run
            double const r = anneal<bdeu_literal>(sampling, h, 1, seed, t0, t1, rate, &uphill);
            print_run("anneal_bdeu_literal", h, r, none, false);
            std::printf("\"uphill\":[");
            for(std::size_t i = 0; i < uphill.size(); ++i) std::printf("%s[%.17g,%.17g]", i ? "," : "", uphill[i].first, uphill[i].second);
            std::printf("],");
            double const m = anneal<bn::evaluation::bdeu>(sampling, many, 16, seed, t0, t1, rate);
            print_run("anneal_bdeu_16", many, m, none, true);
        }
        std::printf("}\n");
    }
    catch(std::exception const& ex)
    {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 1;
    }
    return 0;
}
