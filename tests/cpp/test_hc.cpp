// tests/cpp/test_hc.cpp -- bn::learning::stepwise_structure_hc (include/bayesian/learning/stepwise_structure_hc.hpp) over this
// repository's stand-in data model (-Iinclude -Iinclude/compat), C++14.
//   test_hc NET.dsc SAMPLES SEED ALPHA
// NET.dsc gives the nodes and arities; SAMPLES is the sampler's file format.  Runs, each on a graph that still holds the
// network's edges (the algorithm clears them) and with the same seed:
//   stepwise_structure_hc<aic, greedy>: the runs resident on the device, 64 of them, at most 3 parents;
//   stepwise_structure_hc<aic_literal, recording_greedy> (a trivial subclass of aic; greedy with a learn_with_hint that notes
//   its arguments first): the literal loop on the host, one run.
// Prints one JSON object: per run the edges [parent, child] as positions in vertex_list(), operator()'s return and the aic functor
// of the returned graph; for the host run the (parent nodes, child nodes) of every learn_with_hint call, in order; the winning run of the device path; the mutual_information_holder's similarity of nodes 0 and 1 beside
// the mutual_information functor's; whether a negative alpha is refused -- for tests/test_cpp_hc.py.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include <bayesian/evaluation/aic.hpp>
#include <bayesian/graph.hpp>
#include <bayesian/learning/greedy.hpp>
#include <bayesian/learning/stepwise_structure_hc.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/serializer/dsc.hpp>

namespace {

struct aic_literal : bn::evaluation::aic {
    aic_literal(bn::sampler const& s) : bn::evaluation::aic(s) {}
};

// what the host path handed to learn_with_hint, call by call
struct hint_call {
    std::vector<bn::vertex_type> parents, children;
};
std::vector<hint_call> hint_calls;

template<class Eval>
class recording_greedy : public bn::learning::greedy<Eval> {
public:
    recording_greedy(bn::sampler const& s) : bn::learning::greedy<Eval>(s) {}
    double learn_with_hint(bn::graph_t& graph, std::vector<bn::vertex_type> parent_nodes, std::vector<bn::vertex_type> child_nodes)
    {
        hint_calls.push_back(hint_call{parent_nodes, child_nodes});
        return bn::learning::greedy<Eval>::learn_with_hint(graph, std::move(parent_nodes), std::move(child_nodes));
    }
};

int position(bn::graph_t const& g, bn::vertex_type const& v)
{
    auto const& vl = g.vertex_list();
    for(std::size_t i = 0; i < vl.size(); ++i)
        if(vl[i] == v) return static_cast<int>(i);
    return -1;
}

void print_run(char const* name, bn::graph_t const& g, double score, double functor)
{
    std::printf("\"%s\":{\"score\":%.17g,\"aic\":%.17g,\"edges\":[", name, score, functor);
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
    if(argc < 5) { std::fprintf(stderr, "usage: test_hc NET.dsc SAMPLES SEED ALPHA\n"); return 2; }
    try
    {
        bn::graph_t base = bn::serializer::dsc().from_file(argv[1]);
        auto const seed = static_cast<std::uint64_t>(std::strtoull(argv[3], nullptr, 10));
        double const alpha = std::atof(argv[4]);
        bn::sampler sampling(argv[2]);
        if(!sampling.load_sample(base.vertex_list())) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        bn::evaluation::aic const aic(sampling);
        std::printf("{\"n\":%zu,", base.vertex_list().size());
        {
            bn::graph_t g = base;
            bn::learning::stepwise_structure_hc<bn::evaluation::aic, bn::learning::greedy> device(sampling, seed);
            double const s = device(g, alpha);
            print_run("device", g, s, aic(g));
            std::printf("\"winner\":%d,", device.last_winner());
            bool refused = false;
            try { device(g, -1.0); } catch(std::invalid_argument const&) { refused = true; }
            std::printf("\"negative_alpha_refused\":%s,", refused ? "true" : "false");
        }
        {
            bn::graph_t h = base;
            bn::learning::stepwise_structure_hc<aic_literal, recording_greedy> host(sampling, seed);
            double const r = host(h, alpha);
            sampling.make_cpt(h);   // (the literal loop leaves the CPTs of its last rejected candidate in the graph, as the reference does)
            print_run("host", h, r, aic(h));
            std::printf("\"hint_calls\":[");
            for(std::size_t i = 0; i < hint_calls.size(); ++i)
            {
                std::printf("%s[[", i ? "," : "");
                for(std::size_t x = 0; x < hint_calls[i].parents.size(); ++x) std::printf("%s%d", x ? "," : "", position(h, hint_calls[i].parents[x]));
                std::printf("],[");
                for(std::size_t x = 0; x < hint_calls[i].children.size(); ++x) std::printf("%s%d", x ? "," : "", position(h, hint_calls[i].children[x]));
                std::printf("]]");
            }
            std::printf("],");
        }
        bn::learning::mutual_information_holder holder(sampling);
        holder.prepare(base.vertex_list());
        auto const& vl = base.vertex_list();
        std::printf("\"holder_mi\":%.17g,\"functor_mi\":%.17g,\"holder_h\":%.17g,\"functor_h\":%.17g}\n", holder.calculate_similarity(vl[0], vl[1]),
                    bn::evaluation::mutual_information()(sampling, vl[0], vl[1]), holder.calculate_entropy(vl[0]),
                    bn::evaluation::entropy()(sampling, vl[0]));
    }
    catch(std::exception const& ex)
    {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 1;
    }
    return 0;
}
