// tests/cpp/test_optimal_structure.cpp -- bn::learning::optimal_structure (include/bayesian/learning/optimal_structure.hpp) over
// this repository's stand-in data model (-Iinclude -Iinclude/compat), C++14.
//   test_optimal_structure NET.dsc SAMPLES MAX_PARENTS
// NET.dsc gives the nodes and arities (its edges are dropped); SAMPLES is the sampler's file format.  Runs, each from the empty
// graph: optimal_structure<mdl>, <aic> and <bdeu>, then <mdl> with every node allowed its lower-numbered nodes only.
// Prints one JSON object: per run the edges [parent, child] as positions in vertex_list(), the score and the search's own value --
// for tests/test_cpp_optimal.py.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include <bayesian/evaluation/aic.hpp>
#include <bayesian/evaluation/bdeu.hpp>
#include <bayesian/evaluation/mdl.hpp>
#include <bayesian/graph.hpp>
#include <bayesian/learning/optimal_structure.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/serializer/dsc.hpp>

namespace {

struct mdl_other : bn::evaluation::mdl {
    mdl_other(bn::sampler const& s) : bn::evaluation::mdl(s) {}
};

int position(bn::graph_t const& g, bn::vertex_type const& v)
{
    auto const& vl = g.vertex_list();
    for(std::size_t i = 0; i < vl.size(); ++i)
        if(vl[i] == v) return static_cast<int>(i);
    return -1;
}

void print_run(char const* name, bn::graph_t const& g, double score, double value)
{
    std::printf("\"%s\":{\"score\":%.17g,\"value\":%.17g,\"edges\":[", name, score, value);
    bool first = true;
    for(auto const& child : g.vertex_list())
        for(auto const& parent : g.in_vertexes(child))
        {
            std::printf("%s[%d,%d]", first ? "" : ",", position(g, parent), position(g, child));
            first = false;
        }
    std::printf("]},");
}

template<class Eval>
void search(char const* name, bn::sampler const& sampling, bn::graph_t const& base, int max_parents, std::vector<std::uint64_t> allowed = {})
{
    bn::graph_t g = base;
    bn::learning::optimal_structure<Eval> opt(sampling);
    opt.set_max_parents(max_parents);
    opt.set_allowed(allowed);
    double const s = opt(g);
    print_run(name, g, s, opt.last_value());
}

} // namespace

int main(int argc, char** argv)
{
    if(argc < 4) { std::fprintf(stderr, "usage: test_optimal_structure NET.dsc SAMPLES MAX_PARENTS\n"); return 2; }
    try
    {
        bn::graph_t base = bn::serializer::dsc().from_file(argv[1]);
        base.erase_all_edge();
        int const max_parents = std::atoi(argv[3]);
        bn::sampler sampling(argv[2]);
        if(!sampling.load_sample(base.vertex_list())) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        std::size_t const n = base.vertex_list().size();
        std::printf("{\"n\":%zu,", n);
        search<bn::evaluation::mdl>("mdl", sampling, base, max_parents);
        search<bn::evaluation::aic>("aic", sampling, base, max_parents);
        search<bn::evaluation::bdeu>("bdeu", sampling, base, max_parents);
        std::vector<std::uint64_t> lower(n, 0);
        for(std::size_t v = 0; v < n; ++v) lower[v] = (std::uint64_t(1) << v) - 1;
        search<bn::evaluation::mdl>("mdl_lower", sampling, base, max_parents, lower);
        bool refused = false, no_twin = false, short_allowed = false;
        bn::graph_t g = base;
        bn::learning::optimal_structure<bn::evaluation::mdl> opt(sampling);
        opt.set_max_parents(0);
        try { opt(g); } catch(std::invalid_argument const&) { refused = true; }
        opt.set_max_parents(max_parents);
        opt.set_allowed(std::vector<std::uint64_t>(n + 1, 1));
        try { opt(g); } catch(std::invalid_argument const&) { short_allowed = true; }
        bn::learning::optimal_structure<mdl_other> other(sampling);
        try { other(g); } catch(std::invalid_argument const&) { no_twin = true; }
        std::printf("\"max_parents_0_refused\":%s,\"allowed_size_refused\":%s,\"other_eval_refused\":%s}\n", refused ? "true" : "false",
                    short_allowed ? "true" : "false", no_twin ? "true" : "false");
    }
    catch(std::exception const& ex)
    {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 1;
    }
    return 0;
}
