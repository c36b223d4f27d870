// oracle/ref_learn_driver.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// Runs the UNMODIFIED reference headers for CPT fitting, AIC / MDL and the structure searches (included from $(REF) where
// they lie; nothing is copied into this repository) and prints what they did as JSON.  Built by oracle/Makefile into
// oracle/_ref/ref_learn_driver (git-ignored); tests/golden/make_golden.py --learning turns its output into
// tests/golden/learn_*.npz.
//
// The three Boost names those headers need come from oracle/shim/boost/ (this project's text).  The standard headers are
// included BEFORE `#define private public`: libstdc++'s own headers do not survive that define.  `private` is made public
// for one purpose only: to reseed the searches' engine_ (the reference seeds it from std::random_device).
//
// No loop of the reference is restated here.  The searches are given an Eval that wraps the reference's aic / mdl and
// records every graph it is asked about with the value it returned; stepwise_structure is given thin subclasses of
// brute_force / greedy that record the cluster, or the parent and child lists, they are called with.
//
// Input (whitespace separated, the sample path on a line of its own):
//   BNLEARN1  n  k[0..n)  { m p[0..m) } x n      arities and the start graph (parents per node)
//   <path of a sample file: rows "count s0 s1 ... s(n-1)">   read by the reference's sampler::load_sample(node_list)
//   one command:
//     make_cpt
//     score   aic|mdl  nv v[0..nv)                      nv = -1: operator()(graph); else operator()(graph, vertex_list)
//     greedy  aic|mdl seed  all | vertexes nv v.. | hint np p.. nc c..
//     k2      aic|mdl seed  npre { target m x[0..m) } x npre
//     brute   aic|mdl       all | vertexes nv v.. | hint np p.. nc c..
//     stepwise aic|mdl seed between_seed initial_cluster_size
// Node v is position v of graph_t::vertex_list().  Doubles are printed with %.17g.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <unordered_map>
#include <vector>

#define private public
#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/evaluation/aic.hpp>
#include <bayesian/evaluation/mdl.hpp>
#include <bayesian/learning/greedy.hpp>
#include <bayesian/learning/k2_algorithm.hpp>
#include <bayesian/learning/brute_force.hpp>
#include <bayesian/learning/stepwise_structure.hpp>
#undef private
#include "../include/bayesian/inference/mi355x_flatten.hpp"          // this repo: graph_t -> flat arrays

namespace {

using nodes_t = std::vector<bn::vertex_type>;

[[noreturn]] void die(char const* msg) { std::fprintf(stderr, "ref_learn_driver: %s\n", msg); std::exit(2); }

// ---- what the wrappers record -------------------------------------------------------------------------
struct evaluation { std::vector<int> edges; bool has_vertexes; std::vector<int> vertexes; double value; };
struct call_record { std::vector<int> first, second; std::size_t eval_begin; };   // a cluster, or (parents, children)

std::unordered_map<bn::vertex_t const*, int> g_position;
std::vector<evaluation> g_evals;
std::vector<call_record> g_inner_calls, g_between_calls;
unsigned g_between_seed = 0;

int position(bn::vertex_type const& v) { return g_position.at(v.get()); }

std::vector<int> positions(nodes_t const& vs)
{
    std::vector<int> out;
    for(auto const& v : vs) out.push_back(position(v));
    return out;
}

std::vector<int> edges_of(bn::graph_t const& graph)   // parent, child, ... : children in node order, parents ascending
{
    std::vector<int> out;
    for(auto const& node : graph.vertex_list())
        for(auto const& parent : graph.in_vertexes(node)) { out.push_back(position(parent)); out.push_back(position(node)); }
    return out;
}

// Eval: the reference's criterion, every call recorded
template<class Criterion>
struct logged {
    logged(bn::sampler const& sampling) : criterion_(sampling) {}
    double operator()(bn::graph_t const& graph) const
    {
        double const value = criterion_(graph);
        g_evals.push_back(evaluation{edges_of(graph), false, {}, value});
        return value;
    }
    double operator()(bn::graph_t const& graph, nodes_t const& vertex_list) const
    {
        double const value = criterion_(graph, vertex_list);
        g_evals.push_back(evaluation{edges_of(graph), true, positions(vertex_list), value});
        return value;
    }
    Criterion criterion_;
};

// InnerLearning / BetweenLearning of stepwise_structure: the reference's searches, their calls recorded
template<class Eval>
struct inner_brute_force : bn::learning::brute_force<Eval> {
    inner_brute_force(bn::sampler const& sampling) : bn::learning::brute_force<Eval>(sampling) {}
    double operator()(bn::graph_t& graph, nodes_t const& cluster)
    {
        g_inner_calls.push_back(call_record{positions(cluster), {}, g_evals.size()});
        return bn::learning::brute_force<Eval>::operator()(graph, cluster);
    }
};

template<class Eval>
struct between_greedy : bn::learning::greedy<Eval> {
    between_greedy(bn::sampler const& sampling) : bn::learning::greedy<Eval>(sampling) { this->engine_ = std::mt19937(g_between_seed); }
    double learn_with_hint(bn::graph_t& graph, nodes_t parent_nodes, nodes_t child_nodes)
    {
        g_between_calls.push_back(call_record{positions(parent_nodes), positions(child_nodes), g_evals.size()});
        return bn::learning::greedy<Eval>::learn_with_hint(graph, parent_nodes, child_nodes);
    }
};

// ---- output ----------------------------------------------------------------------------------------------
void print_ints(std::vector<int> const& v)
{
    std::printf("[");
    for(std::size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? "," : "", v[i]);
    std::printf("]");
}

void print_doubles(std::vector<double> const& v)
{
    std::printf("[");
    for(std::size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? "," : "", v[i]);
    std::printf("]");
}

void print_calls(char const* name, std::vector<call_record> const& calls)
{
    std::printf(",\"%s\":[", name);
    for(std::size_t i = 0; i < calls.size(); ++i) {
        std::printf("%s{\"first\":", i ? "," : ""); print_ints(calls[i].first);
        std::printf(",\"second\":"); print_ints(calls[i].second);
        std::printf(",\"eval_begin\":%zu}", calls[i].eval_begin);
    }
    std::printf("]");
}

void print_search(char const* command, bn::graph_t const& graph, double value, double seconds)
{
    std::printf("{\"command\":\"%s\",\"value\":%.17g,\"run_s\":%.6f,\"final_edges\":", command, value, seconds);
    print_ints(edges_of(graph));
    std::printf(",\"evals\":[");
    for(std::size_t i = 0; i < g_evals.size(); ++i) {
        std::printf("%s{\"edges\":", i ? "," : ""); print_ints(g_evals[i].edges);
        if(g_evals[i].has_vertexes) { std::printf(",\"vertexes\":"); print_ints(g_evals[i].vertexes); }
        std::printf(",\"value\":%.17g}", g_evals[i].value);
    }
    std::printf("]");
    print_calls("inner_calls", g_inner_calls);
    print_calls("between_calls", g_between_calls);
    std::printf("}\n");
}

nodes_t read_nodes(std::istream& in, nodes_t const& all)
{
    int count; in >> count;
    if(!in || count < 0) die("bad node list");
    nodes_t out;
    for(int i = 0; i < count; ++i) {
        int v; in >> v;
        if(!in || v < 0 || v >= static_cast<int>(all.size())) die("node out of range");
        out.push_back(all[v]);
    }
    return out;
}

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

template<class Criterion>
int run(std::string const& command, std::istream& in, bn::graph_t& graph, bn::sampler const& sampling)
{
    using eval_t = logged<Criterion>;
    auto const all = graph.vertex_list();
    auto const t0 = std::chrono::steady_clock::now();
    if(command == "score") {
        int nv; in >> nv;
        if(!in) die("truncated score command");
        sampling.make_cpt(graph);
        eval_t const eval(sampling);
        double value;
        if(nv < 0) value = eval(graph);
        else {
            nodes_t vs;
            for(int i = 0; i < nv; ++i) { int v; in >> v; if(!in || v < 0 || v >= static_cast<int>(all.size())) die("node out of range"); vs.push_back(all[v]); }
            value = eval(graph, vs);
        }
        print_search("score", graph, value, seconds_since(t0));
        return 0;
    }
    if(command == "greedy") {
        unsigned seed; std::string form; in >> seed >> form;
        bn::learning::greedy<eval_t> search(sampling);
        search.engine_ = std::mt19937(seed);
        double value;
        if(form == "all") value = search(graph);
        else if(form == "vertexes") value = search(graph, read_nodes(in, all));
        else if(form == "hint") { auto const ps = read_nodes(in, all); auto const cs = read_nodes(in, all); value = search.learn_with_hint(graph, ps, cs); }
        else die("greedy: all | vertexes | hint");
        print_search("greedy", graph, value, seconds_since(t0));
        return 0;
    }
    if(command == "k2") {
        unsigned seed; int npre; in >> seed >> npre;
        if(!in || npre < 0) die("truncated k2 command");
        std::unordered_map<bn::vertex_type, nodes_t> precondition;
        for(int i = 0; i < npre; ++i) {
            int target; in >> target;
            if(!in || target < 0 || target >= static_cast<int>(all.size())) die("node out of range");
            precondition[all[target]] = read_nodes(in, all);
        }
        bn::learning::k2_algorithm<eval_t> search(sampling);
        search.engine_ = std::mt19937(seed);
        double const value = search(graph, precondition);
        print_search("k2", graph, value, seconds_since(t0));
        return 0;
    }
    if(command == "brute") {
        std::string form; in >> form;
        bn::learning::brute_force<eval_t> search(sampling);
        double value;
        if(form == "all") value = search(graph);
        else if(form == "vertexes") value = search(graph, read_nodes(in, all));
        else if(form == "hint") { auto const ps = read_nodes(in, all); auto const cs = read_nodes(in, all); value = search.learn_with_hint(graph, ps, cs); }
        else die("brute: all | vertexes | hint");
        print_search("brute", graph, value, seconds_since(t0));
        return 0;
    }
    if(command == "stepwise") {
        unsigned seed; std::size_t size; in >> seed >> g_between_seed >> size;
        if(!in || size == 0) die("truncated stepwise command");
        bn::learning::stepwise_structure<eval_t, inner_brute_force, between_greedy> search(sampling);
        search.engine_ = std::mt19937(seed);
        double const value = search(graph, size);
        print_search("stepwise", graph, value, seconds_since(t0));
        return 0;
    }
    die("unknown command");
}

} // namespace

int main(int argc, char** argv)
{
    if(argc < 2) die("usage: ref_learn_driver request.txt");
    std::ifstream in(argv[1]);
    if(!in) die("cannot open input");
    std::string magic; int n;
    in >> magic >> n;
    if(magic != "BNLEARN1" || !in || n <= 0) die("bad header");
    bn::graph_t graph;
    for(int v = 0; v < n; ++v) {
        int k; in >> k;
        if(!in || k <= 0) die("bad arity");
        auto vx = graph.add_vertex();
        vx->id = v;
        vx->selectable_num = static_cast<std::size_t>(k);
        g_position[vx.get()] = v;
    }
    auto const all = graph.vertex_list();
    for(int v = 0; v < n; ++v) {
        int m; in >> m;
        if(!in || m < 0) die("bad parent count");
        for(int j = 0; j < m; ++j) {
            int p; in >> p;
            if(!in || p < 0 || p >= n) die("parent out of range");
            if(!graph.add_edge(all[p], all[v])) die("add_edge refused (cycle or duplicate)");
        }
    }
    std::string path;
    std::getline(in >> std::ws, path);
    if(!in || path.empty()) die("sample path missing");
    bn::sampler sampling(path);
    if(!sampling.load_sample(all)) die("load_sample failed");      // the reference's own reader
    if(sampling.sampling_size() == 0) die("empty sample");

    std::string command;
    in >> command;
    if(!in) die("command missing");
    if(command == "make_cpt") {
        auto const t0 = std::chrono::steady_clock::now();
        if(!sampling.make_cpt(graph)) die("make_cpt failed");
        double const s = seconds_since(t0);
        auto const flat = bn::mi355x::flatten(graph);
        std::printf("{\"command\":\"make_cpt\",\"run_s\":%.6f,\"sampling_size\":%zu,\"edges\":", s, sampling.sampling_size());
        print_ints(edges_of(graph));
        std::printf(",\"cpt\":"); print_doubles(flat.cpt);
        std::printf("}\n");
        return 0;
    }
    std::string criterion;
    in >> criterion;
    if(criterion == "aic") return run<bn::evaluation::aic>(command, in, graph, sampling);
    if(criterion == "mdl") return run<bn::evaluation::mdl>(command, in, graph, sampling);
    die("criterion: aic | mdl");
}
