// tests/cpp/test_scores.cpp -- bn::evaluation::aic / mdl (include/bayesian/evaluation/aic.hpp, mdl.hpp over
// basic_info_criteria.hpp) over this repository's stand-in data model (-Iinclude -Iinclude/compat), C++14.
//   test_scores --dsc NET.dsc SAMPLES   |   test_scores --pearl SAMPLES
// SAMPLES: the sampler's file format, one row per distinct pattern, "count s_0 s_1 ..." in vertex_list() order.
// Prints one JSON object: aic / mdl over the whole graph and over a vertex subset (the odd positions, last first),
// the per-node and per-pattern log-likelihoods with the patterns' order, the parameter count (aic minus likelihood
// is not exact, so it is recomputed here from the graph), and what an empty sampler does.  tests/test_cpp_scores.py
// compares every number with the Python side and with the restatement of the reference.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <bayesian/evaluation/aic.hpp>
#include <bayesian/evaluation/mdl.hpp>
#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/serializer/dsc.hpp>

namespace {

struct node_spec {
    int arity;
    std::vector<int> parents;
    std::vector<double> rows;
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

// the four-node network of the reference's BP tests (two roots, a child of the first, a child of both)
std::vector<node_spec> pearl_spec()
{
    return {{2, {}, {0.2, 0.8}},
            {2, {}, {0.1, 0.9}},
            {2, {0}, {1.0, 0.0, 0.2, 0.8}},
            {2, {0, 1}, {1.0, 0.0, 1.0, 0.0, 0.9, 0.1, 0.0, 1.0}}};
}

void print_array(char const* name, std::vector<double> const& v)
{
    std::printf("\"%s\":[", name);
    for(std::size_t i = 0; i < v.size(); ++i)
    {
        if(std::isinf(v[i])) std::printf("%s\"%sinf\"", i ? "," : "", v[i] < 0 ? "-" : "");
        else std::printf("%s%.17g", i ? "," : "", v[i]);
    }
    std::printf("],");
}

} // namespace

int main(int argc, char** argv)
{
    if(argc < 3) { std::fprintf(stderr, "usage: test_scores --dsc NET.dsc SAMPLES | --pearl SAMPLES\n"); return 2; }
    bool const from_dsc = std::strcmp(argv[1], "--dsc") == 0;
    if(from_dsc && argc < 4) return 2;
    bn::graph_t const graph = from_dsc ? bn::serializer::dsc().from_file(argv[2]) : build(pearl_spec());
    auto const nodes = graph.vertex_list();
    try
    {
        bn::sampler sampling(from_dsc ? argv[3] : argv[2]);
        if(!sampling.load_sample(nodes)) { std::fprintf(stderr, "cannot read the sample file\n"); return 2; }
        std::vector<bn::vertex_type> subset;
        for(std::size_t i = nodes.size(); i-- > 0;)
            if(i % 2 == 1) subset.push_back(nodes[i]);

        bn::evaluation::aic const aic(sampling);
        bn::evaluation::mdl const mdl(sampling);
        std::printf("{\"n\":%zu,\"sampling_size\":%zu,", nodes.size(), sampling.sampling_size());
        std::printf("\"aic\":%.17g,\"mdl\":%.17g,", aic(graph), mdl(graph));
        std::printf("\"aic_again\":%.17g,", aic(graph));   // (the table is kept, a new engine is built: the same bits)
        std::printf("\"aic_subset\":%.17g,\"mdl_subset\":%.17g,", aic(graph, subset), mdl(graph, subset));
        print_array("ll_node", mdl.log_likelihood(graph));
        print_array("ll_rows", mdl.log_likelihood_rows(graph));
        std::printf("\"row_patterns\":[");
        auto const& rows = mdl.row_patterns();
        for(std::size_t r = 0; r < rows.size(); ++r)
        {
            std::printf("%s[", r ? "," : "");
            for(std::size_t i = 0; i < nodes.size(); ++i) std::printf("%s%d", i ? "," : "", rows[r].at(nodes[i]));
            std::printf("]");
        }
        std::printf("],");

        bn::sampler const empty;
        bn::evaluation::aic const aic_empty(empty);
        bn::evaluation::mdl const mdl_empty(empty);
        bool threw = false;
        try { (void)mdl_empty(graph); }
        catch(std::runtime_error const& ex) { threw = std::string(ex.what()) == "Sampling is not finished yet."; }
        std::printf("\"empty_aic\":%.17g,\"empty_mdl_throws\":%s}\n", aic_empty(graph), threw ? "true" : "false");
    }
    catch(std::exception const& ex)
    {
        std::fprintf(stderr, "exception: %s\n", ex.what());
        return 1;
    }
    return 0;
}
