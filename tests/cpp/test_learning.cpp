// tests/cpp/test_learning.cpp -- bn::learning::greedy / k2_algorithm (include/bayesian/learning/) over this repository's stand-in
// data model (-Iinclude -Iinclude/compat), C++14.
//   test_learning NET.dsc SAMPLES SEED
// NET.dsc gives the nodes and arities (its edges are dropped); SAMPLES is the sampler's file format.  Runs, each from the empty
// graph and with the same seed, so with the same shuffles:
//   greedy<aic> (the learner on the device) and greedy<aic_literal> (a trivial subclass: the reference's literal loop),
//   k2_algorithm<mdl> and k2_algorithm<mdl_literal> with a precondition, greedy<mdl>::learn_with_hint and its literal twin.
// Prints one JSON object: per run the edges [parent, child] as positions in vertex_list(), the score, and the visits (child, the
// candidates offered) for tests/test_cpp_learning.py to replay through the Python learner.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include <bayesian/evaluation/aic.hpp>
#include <bayesian/evaluation/mdl.hpp>
#include <bayesian/graph.hpp>
#include <bayesian/learning/greedy.hpp>
#include <bayesian/learning/k2_algorithm.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/serializer/dsc.hpp>

namespace {

struct aic_literal : bn::evaluation::aic {
    aic_literal(bn::sampler const& s) : bn::evaluation::aic(s) {}
};
struct mdl_literal : bn::evaluation::mdl {
    mdl_literal(bn::sampler const& s) : bn::evaluation::mdl(s) {}
};

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

// the CPT of every node is over its parents in the graph and every row sums to 1: fitted CPTs of the final structure
bool cpts_normalised(bn::graph_t const& g)
{
    for(auto const& node : g.vertex_list())
    {
        auto const parents = g.in_vertexes(node);
        if(node->cpt.condition_node() != parents) return false;
        for(auto const& cond : node->cpt.pattern())
        {
            double s = 0.0;
            for(double x : node->cpt[cond].second) s += x;
            if(!(s > 1.0 - 1e-9 && s < 1.0 + 1e-9)) return false;
        }
    }
    return true;
}

} // namespace

int main(int argc, char** argv)
{
    if(argc < 4) { std::fprintf(stderr, "usage: test_learning NET.dsc SAMPLES SEED\n"); return 2; }
    try
    {
        bn::graph_t base = bn::serializer::dsc().from_file(argv[1]);
        base.erase_all_edge();
        auto const seed = static_cast<std::uint32_t>(std::strtoul(argv[3], nullptr, 10));
        bn::sampler sampling(argv[2]);
        if(!sampling.load_sample(base.vertex_list())) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        auto const nodes = base.vertex_list();
        std::printf("{\"n\":%zu,", nodes.size());
        {
            bn::graph_t g = base, h = base;   // (copies share the vertices: each run fits its own CPTs at its end)
            bn::learning::greedy<bn::evaluation::aic> device(sampling, seed);
            double const s = device(g);
            bool const ok = cpts_normalised(g);
            print_run("greedy_aic", g, s, device.last_visits(), false);
            std::printf("\"greedy_aic_cpts_ok\":%s,", ok ? "true" : "false");
            bn::learning::greedy<aic_literal> literal(sampling, seed);
            double const r = literal(h);
            print_run("greedy_aic_literal", h, r, literal.last_visits(), false);
        }
        {
            std::unordered_map<bn::vertex_type, std::vector<bn::vertex_type>> pre;
            pre[nodes[3]] = {nodes[0], nodes[1], nodes[2]};
            pre[nodes[nodes.size() - 1]] = std::vector<bn::vertex_type>(nodes.begin(), nodes.begin() + nodes.size() / 2);
            bn::graph_t g = base, h = base;
            bn::learning::k2_algorithm<bn::evaluation::mdl> device(sampling, seed);
            double const s = device(g, pre);
            print_run("k2_mdl", g, s, device.last_visits(), false);
            bn::learning::k2_algorithm<mdl_literal> literal(sampling, seed);
            double const r = literal(h, pre);
            print_run("k2_mdl_literal", h, r, literal.last_visits(), false);
        }
        {
            std::vector<bn::vertex_type> const parents(nodes.begin(), nodes.begin() + nodes.size() / 2), children(nodes.begin() + nodes.size() / 2, nodes.end());
            bn::graph_t g = base, h = base;
            bn::learning::greedy<bn::evaluation::mdl> device(sampling, seed);
            double const s = device.learn_with_hint(g, parents, children);
            print_run("hint_mdl", g, s, device.last_visits(), false);
            bn::learning::greedy<mdl_literal> literal(sampling, seed);
            double const r = literal.learn_with_hint(h, parents, children);
            print_run("hint_mdl_literal", h, r, literal.last_visits(), true);
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
