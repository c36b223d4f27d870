// tests/cpp/test_pc_algorithm.cpp -- bn::learning::pc (include/bayesian/learning/pc_algorithm.hpp) over this repository's stand-in
// data model (-Iinclude -Iinclude/compat), C++14.
//   test_pc_algorithm NET.dsc SAMPLES ALPHA MAX_COND
// NET.dsc gives the nodes and arities (its edges are dropped); SAMPLES is the sampler's file format.
// Prints one JSON object: the CPDAG marks, the edges [parent, child] of the DAG left in the graph as positions in vertex_list(), and
// the separating sets by "a,b" -- for tests/test_cpp_pc.py.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include <bayesian/graph.hpp>
#include <bayesian/learning/pc_algorithm.hpp>
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

} // namespace

int main(int argc, char** argv)
{
    if(argc < 5) { std::fprintf(stderr, "usage: test_pc_algorithm NET.dsc SAMPLES ALPHA MAX_COND\n"); return 2; }
    try
    {
        bn::graph_t g = bn::serializer::dsc().from_file(argv[1]);
        g.erase_all_edge();
        bn::sampler sampling(argv[2]);
        if(!sampling.load_sample(g.vertex_list())) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        bn::learning::pc pc(sampling);
        std::size_t const edges = pc(g, std::atof(argv[3]), std::atoi(argv[4]));
        std::size_t const n = g.vertex_list().size();
        std::printf("{\"n\":%zu,\"n_edges\":%zu,\"cpdag\":[", n, edges);
        for(std::size_t i = 0; i < n * n; ++i) std::printf("%s%d", i ? "," : "", int(pc.cpdag()[i]));
        std::printf("],\"edges\":[");
        bool first = true;
        for(auto const& child : g.vertex_list())
            for(auto const& parent : g.in_vertexes(child))
            {
                std::printf("%s[%d,%d]", first ? "" : ",", position(g, parent), position(g, child));
                first = false;
            }
        std::printf("],\"sepsets\":{");
        first = true;
        for(std::size_t a = 0; a < n; ++a)
            for(std::size_t b = a + 1; b < n; ++b)
            {
                if(!pc.has_sepset(a, b)) continue;
                std::printf("%s\"%zu,%zu\":[", first ? "" : ",", a, b);
                auto const s = pc.sepset(a, b);
                for(std::size_t j = 0; j < s.size(); ++j) std::printf("%s%d", j ? "," : "", int(s[j]));
                std::printf("]");
                first = false;
            }
        bool refused = false;
        try { pc(g, 1.0, 2); } catch(std::invalid_argument const&) { refused = true; }
        std::printf("},\"alpha_refused\":%s}\n", refused ? "true" : "false");
    }
    catch(std::exception const& ex)
    {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 1;
    }
    return 0;
}
