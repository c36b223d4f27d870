// tests/cpp/test_hill_climbing.cpp -- bn::learning::hill_climbing (include/bayesian/learning/hill_climbing.hpp) over this
// repository's stand-in data model (-Iinclude -Iinclude/compat), C++14.
//   test_hill_climbing NET.dsc SAMPLES SEED TABU_LEN MAX_WORSE PERTURB RUNS MAX_STEPS
// NET.dsc gives the nodes and arities (its edges are dropped); SAMPLES is the sampler's file format.  Runs, each from the empty
// graph: hill_climbing<mdl>, <aic> and <bdeu> as the classic greedy climb (one run, no tabu list), and hill_climbing<mdl> with the
// given tabu list, restarts and seed.
// Prints one JSON object: per run the edges [parent, child] as positions in vertex_list() and the score; for the last run the
// winning run -- for tests/test_cpp_climb.py.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include <bayesian/evaluation/aic.hpp>
#include <bayesian/evaluation/bdeu.hpp>
#include <bayesian/evaluation/mdl.hpp>
#include <bayesian/graph.hpp>
#include <bayesian/learning/hill_climbing.hpp>
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

template<class Eval>
void greedy_climb(char const* name, bn::sampler const& sampling, bn::graph_t const& base, std::uint32_t max_steps)
{
    bn::graph_t g = base;
    bn::learning::hill_climbing<Eval> climb(sampling, 0);
    climb.set_max_steps(max_steps);
    double const s = climb(g);
    print_run(name, g, s);
}

} // namespace

int main(int argc, char** argv)
{
    if(argc < 9) { std::fprintf(stderr, "usage: test_hill_climbing NET.dsc SAMPLES SEED TABU_LEN MAX_WORSE PERTURB RUNS MAX_STEPS\n"); return 2; }
    try
    {
        bn::graph_t base = bn::serializer::dsc().from_file(argv[1]);
        base.erase_all_edge();
        auto const seed = static_cast<std::uint64_t>(std::strtoull(argv[3], nullptr, 10));
        int const tabu_len = std::atoi(argv[4]), runs = std::atoi(argv[7]);
        auto const max_worse = static_cast<unsigned int>(std::atoi(argv[5]));
        auto const perturb = static_cast<std::uint32_t>(std::atoi(argv[6])), max_steps = static_cast<std::uint32_t>(std::atoi(argv[8]));
        bn::sampler sampling(argv[2]);
        if(!sampling.load_sample(base.vertex_list())) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        std::printf("{\"n\":%zu,", base.vertex_list().size());
        greedy_climb<bn::evaluation::mdl>("greedy_mdl", sampling, base, max_steps);
        greedy_climb<bn::evaluation::aic>("greedy_aic", sampling, base, max_steps);
        greedy_climb<bn::evaluation::bdeu>("greedy_bdeu", sampling, base, max_steps);
        {
            bn::graph_t g = base;
            bn::learning::hill_climbing<bn::evaluation::mdl> climb(sampling, seed);
            climb.set_runs(runs);
            climb.set_perturb(perturb);
            climb.set_max_steps(max_steps);
            double const s = climb(g, tabu_len, max_worse);
            print_run("tabu_mdl", g, s);
            std::printf("\"winner\":%d,", climb.last_winner());
            bool refused = false, no_twin = false;
            try { climb(g, 65, 0); } catch(std::invalid_argument const&) { refused = true; }
            bn::learning::hill_climbing<mdl_other> other(sampling, seed);
            try { other(g); } catch(std::invalid_argument const&) { no_twin = true; }
            std::printf("\"tabu_65_refused\":%s,\"other_eval_refused\":%s}\n", refused ? "true" : "false", no_twin ? "true" : "false");
        }
    }
    catch(std::exception const& ex)
    {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 1;
    }
    return 0;
}
