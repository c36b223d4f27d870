// tests/cpp/test_subsets.cpp -- bn::learning::brute_force / stepwise_structure (include/bayesian/learning/) over this repository's
// stand-in data model (-Iinclude -Iinclude/compat), C++14.
//   test_subsets NET.dsc SAMPLES SEED VERTEXES PARENTS CHILDREN CLUSTER_SIZE
// NET.dsc gives the nodes and arities (its edges are dropped); SAMPLES is the sampler's file format; VERTEXES / PARENTS / CHILDREN
// are comma-separated positions in vertex_list().  Runs, each from the empty graph:
//   brute_force<mdl>(graph, VERTEXES) (the learner on the device) and brute_force<mdl_literal> (a trivial subclass: the
//   reference's literal enumeration), brute_force<mdl>::learn_with_hint(graph, PARENTS, CHILDREN) and its literal twin, and
//   stepwise_structure<mdl, brute_force, greedy>(graph, CLUSTER_SIZE) with SEED.
// Prints one JSON object: per run the edges [parent, child] as positions in vertex_list() and the returned value; for the stepwise
// run also the clusters, the merged (parent, child) pairs and the greedy's visits per merge, for tests/test_cpp_subsets.py to
// replay through the Python learner.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include <bayesian/evaluation/aic.hpp>
#include <bayesian/evaluation/mdl.hpp>
#include <bayesian/graph.hpp>
#include <bayesian/learning/brute_force.hpp>
#include <bayesian/learning/greedy.hpp>
#include <bayesian/learning/stepwise_structure.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/serializer/dsc.hpp>

namespace {

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

std::vector<bn::vertex_type> pick(bn::graph_t const& g, std::string const& list)
{
    std::vector<bn::vertex_type> out;
    std::size_t at = 0;
    while(at < list.size())
    {
        std::size_t const end = list.find(',', at) == std::string::npos ? list.size() : list.find(',', at);
        out.push_back(g.vertex_list().at(static_cast<std::size_t>(std::stoul(list.substr(at, end - at)))));
        at = end + 1;
    }
    return out;
}

void print_positions(bn::graph_t const& g, std::vector<bn::vertex_type> const& vs)
{
    std::printf("[");
    for(std::size_t j = 0; j < vs.size(); ++j) std::printf("%s%d", j ? "," : "", position(g, vs[j]));
    std::printf("]");
}

void print_run(char const* name, bn::graph_t const& g, double value)
{
    std::printf("\"%s\":{\"value\":%.17g,\"edges\":[", name, value);
    bool first = true;
    for(auto const& child : g.vertex_list())
        for(auto const& parent : g.in_vertexes(child))
        {
            std::printf("%s[%d,%d]", first ? "" : ",", position(g, parent), position(g, child));
            first = false;
        }
    std::printf("]}");
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
    if(argc < 8) { std::fprintf(stderr, "usage: test_subsets NET.dsc SAMPLES SEED VERTEXES PARENTS CHILDREN CLUSTER_SIZE\n"); return 2; }
    try
    {
        bn::graph_t base = bn::serializer::dsc().from_file(argv[1]);
        base.erase_all_edge();
        auto const seed = static_cast<std::uint32_t>(std::strtoul(argv[3], nullptr, 10));
        bn::sampler sampling(argv[2]);
        if(!sampling.load_sample(base.vertex_list())) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        std::printf("{\"n\":%zu,", base.vertex_list().size());
        {
            bn::graph_t g = base, h = base;   // (copies share the vertices: each run fits its own CPTs at its end)
            auto const vs = pick(base, argv[4]);
            bn::learning::brute_force<bn::evaluation::mdl> device(sampling);
            double const s = device(g, vs);
            bool const ok = cpts_normalised(g);
            print_run("bf_mdl", g, s);
            std::printf(",\"bf_mdl_cpts_ok\":%s,", ok ? "true" : "false");
            bn::learning::brute_force<mdl_literal> literal(sampling);
            double const r = literal(h, vs);
            print_run("bf_mdl_literal", h, r);
            std::printf(",");
        }
        {
            bn::graph_t g = base, h = base;
            auto const parents = pick(base, argv[5]), children = pick(base, argv[6]);
            bn::learning::brute_force<bn::evaluation::mdl> device(sampling);
            double const s = device.learn_with_hint(g, parents, children);
            print_run("hint_mdl", g, s);
            std::printf(",");
            bn::learning::brute_force<mdl_literal> literal(sampling);
            double const r = literal.learn_with_hint(h, parents, children);
            print_run("hint_mdl_literal", h, r);
            std::printf(",");
        }
        {
            bn::graph_t g = base;
            bn::learning::stepwise_structure<bn::evaluation::mdl, bn::learning::brute_force, bn::learning::greedy> device(sampling, seed);
            double const s = device(g, static_cast<std::size_t>(std::strtoul(argv[7], nullptr, 10)));
            bool const ok = cpts_normalised(g);
            print_run("stepwise_mdl", g, s);
            std::printf(",\"stepwise_mdl_cpts_ok\":%s,\"clusters\":[", ok ? "true" : "false");
            for(std::size_t i = 0; i < device.last_clusters().size(); ++i)
            {
                std::printf("%s", i ? "," : "");
                print_positions(g, device.last_clusters()[i]);
            }
            std::printf("],\"pairs\":[");
            for(std::size_t i = 0; i < device.last_pairs().size(); ++i)
                std::printf("%s[%zu,%zu]", i ? "," : "", device.last_pairs()[i].first, device.last_pairs()[i].second);
            std::printf("],\"between_visits\":[");
            for(std::size_t i = 0; i < device.last_between_visits().size(); ++i)
            {
                std::printf("%s[", i ? "," : "");
                auto const& visits = device.last_between_visits()[i];
                for(std::size_t j = 0; j < visits.size(); ++j)
                {
                    std::printf("%s[%d,", j ? "," : "", position(g, visits[j].child));
                    print_positions(g, visits[j].candidates);
                    std::printf("]");
                }
                std::printf("]");
            }
            std::printf("]");
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
