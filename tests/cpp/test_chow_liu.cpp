// tests/cpp/test_chow_liu.cpp -- bn::learning::chow_liu and bn::learning::tree_augmented (include/bayesian/learning/chow_liu.hpp) over
// this repository's stand-in data model (-Iinclude -Iinclude/compat), C++14.
//   test_chow_liu NET.dsc SAMPLES
// NET.dsc gives the nodes and arities (its edges are dropped); SAMPLES is the sampler's file format.
// Prints one JSON object: per learner the edges [parent, child] left in the graph as positions in vertex_list(), the tree parents and
// the weights as the 16 hex digits of their bits -- for tests/test_cpp_tree.py.  tree_augmented's class is the first vertex.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include <bayesian/graph.hpp>
#include <bayesian/learning/chow_liu.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/serializer/dsc.hpp>

namespace {

int position(bn::graph_t const& g, bn::vertex_type const& v)
{
    auto const& vl = g.vertex_list();
    for(std::size_t i = 0; i < vl.size(); ++i)
        if(vl[i] == v) return static_cast<int>(i);
    return -1;
}

template<class Learner>
void print_result(char const* name, bn::graph_t const& g, Learner const& learner, std::size_t const edges)
{
    std::printf("\"%s\":{\"n_edges\":%zu,\"edges\":[", name, edges);
    bool first = true;
    for(auto const& child : g.vertex_list())
        for(auto const& parent : g.in_vertexes(child))
        {
            std::printf("%s[%d,%d]", first ? "" : ",", position(g, parent), position(g, child));
            first = false;
        }
    std::printf("],\"parent\":[");
    for(std::size_t i = 0; i < learner.parent().size(); ++i) std::printf("%s%d", i ? "," : "", int(learner.parent()[i]));
    std::printf("],\"weights\":[");
    for(std::size_t i = 0; i < learner.weights().size(); ++i)
    {
        std::uint64_t bits = 0;
        double const w = learner.weights()[i];
        std::memcpy(&bits, &w, 8);
        std::printf("%s\"%016llx\"", i ? "," : "", static_cast<unsigned long long>(bits));
    }
    std::printf("]}");
}

} // namespace

int main(int argc, char** argv)
{
    if(argc < 3) { std::fprintf(stderr, "usage: test_chow_liu NET.dsc SAMPLES\n"); return 2; }
    try
    {
        bn::graph_t g = bn::serializer::dsc().from_file(argv[1]);
        g.erase_all_edge();
        bn::sampler sampling(argv[2]);
        if(!sampling.load_sample(g.vertex_list())) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        std::printf("{\"n\":%zu,", g.vertex_list().size());
        bn::learning::chow_liu cl(sampling);
        std::size_t edges = cl(g);
        print_result("chow_liu", g, cl, edges);
        std::printf(",");
        edges = cl(g, g.vertex_list()[5]);
        print_result("chow_liu_root5", g, cl, edges);
        std::printf(",");
        bn::learning::tree_augmented tan(sampling);
        edges = tan(g, g.vertex_list()[0]);
        print_result("tree_augmented", g, tan, edges);
        bn::sampler empty;
        bool refused = false;
        try { bn::learning::chow_liu none(empty); none(g); } catch(std::invalid_argument const&) { refused = true; }
        std::printf(",\"empty_refused\":%s}\n", refused ? "true" : "false");
    }
    catch(std::exception const& ex)
    {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 1;
    }
    return 0;
}
