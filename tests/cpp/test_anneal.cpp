// tests/cpp/test_anneal.cpp -- bn::learning::simulated_annealing (include/bayesian/learning/simulated_annealing.hpp) over this
// repository's stand-in data model (-Iinclude -Iinclude/compat), C++14.
//   test_anneal NET.dsc SAMPLES SEED INITIAL_TEMP FINAL_TEMP RATE
// NET.dsc gives the nodes and arities (its edges are dropped); SAMPLES is the sampler's file format.  Runs, each from the empty
// graph with the same seed and the Metropolis rule:
//   simulated_annealing<mdl> with one chain (the device path) and simulated_annealing<mdl_literal> (a trivial subclass: the
//   reference's literal loop on the host, chain 0 of the same stream), and simulated_annealing<mdl> with 64 chains.
// Prints one JSON object: per run the edges [parent, child] as positions in vertex_list() and the score; for the literal run the
// (u, p) of every uphill decision; for the 64-chain run the winning chain -- for tests/test_cpp_anneal.py.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include <bayesian/evaluation/mdl.hpp>
#include <bayesian/graph.hpp>
#include <bayesian/learning/simulated_annealing.hpp>
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

void print_run(char const* name, bn::graph_t const& g, double score)
{
    std::printf("\"%s\":{\"score\":%.17g,\"edges\":[", name, score);
    bool first = true;
    for(auto const& child : g.vertex_list())
        for(auto const& parent : g.in_vertexes(child))
        {
            std::printf("%s[%d,%d]", first ? "" : ",", position(g, parent), position(g, child));
            first = false;
        }
    std::printf("]},");
}

} // namespace

int main(int argc, char** argv)
{
    if(argc < 7) { std::fprintf(stderr, "usage: test_anneal NET.dsc SAMPLES SEED INITIAL_TEMP FINAL_TEMP RATE\n"); return 2; }
    try
    {
        bn::graph_t base = bn::serializer::dsc().from_file(argv[1]);
        base.erase_all_edge();
        auto const seed = static_cast<std::uint64_t>(std::strtoull(argv[3], nullptr, 10));
        double const t0 = std::atof(argv[4]), t1 = std::atof(argv[5]), rate = std::atof(argv[6]);
        bn::sampler sampling(argv[2]);
        if(!sampling.load_sample(base.vertex_list())) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        std::printf("{\"n\":%zu,", base.vertex_list().size());
        {
            bn::graph_t g = base, h = base;
            bn::learning::simulated_annealing<bn::evaluation::mdl> device(sampling, seed);
            device.set_chains(1);
            device.set_rule(1);
            double const s = device(g, t0, t1, rate);
            print_run("one_chain", g, s);
            bn::learning::simulated_annealing<mdl_literal> literal(sampling, seed);
            literal.set_rule(1);
            double const r = literal(h, t0, t1, rate);
            print_run("literal", h, r);
            std::printf("\"uphill\":[");
            for(std::size_t i = 0; i < literal.last_uphill().size(); ++i)
                std::printf("%s[%.17g,%.17g]", i ? "," : "", literal.last_uphill()[i].first, literal.last_uphill()[i].second);
            std::printf("],");
        }
        {
            bn::graph_t g = base;
            bn::learning::simulated_annealing<bn::evaluation::mdl> device(sampling, seed);   // 64 chains, at most 3 parents
            device.set_rule(1);
            double const s = device(g, t0, t1, rate);
            print_run("chains64", g, s);
            std::printf("\"winner\":%d,", device.last_winner());
            bool refused = false;
            try { device(g, t0, t1, 1.0); } catch(std::invalid_argument const&) { refused = true; }
            std::printf("\"rate_one_refused\":%s}\n", refused ? "true" : "false");
        }
    }
    catch(std::exception const& ex)
    {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 1;
    }
    return 0;
}
