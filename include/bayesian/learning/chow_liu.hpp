// bayesian/learning/chow_liu.hpp -- NOT IN THE REFERENCE: bn::learning::chow_liu and bn::learning::tree_augmented, the tree learners
// (bnlearn's chow.liu and tree.bayes, pgmpy's TreeSearch "chow-liu" / "tan"), running on the MI355X through bn_learn_tree
// (include/bn_mi355x.h states the contract).  C++14, no Boost.
//
// Shaped like this repository's pc_algorithm.hpp: chow_liu(sampler const&), operator()(graph, root = first vertex) replaces the graph's
// edges by the maximum spanning tree of the all-pairs mutual information over graph.vertex_list(), oriented away from root, fits the CPTs
// with one sampling_.make_cpt(graph) and returns the number of edges.  tree_augmented's operator()(graph, class_node, root = first
// feature) builds the tree over every vertex but class_node under the mutual information given the class, and adds class_node -> feature
// for every feature.  weights() and parent() give the rest of the last call's result.
//
// Ties between equal weights are broken by the positions in vertex_list() (the lower pair first), so the tree is unique.
//
// There is no host twin: an empty sampler throws std::invalid_argument.
#ifndef BNI_LEARNING_CHOW_LIU_HPP
#define BNI_LEARNING_CHOW_LIU_HPP

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/evaluation/transinformation.hpp>

namespace bn {
namespace learning {

namespace detail {

// the common part: positions are those of graph.vertex_list(); cond < 0: Chow-Liu
class tree_learner {
public:
    explicit tree_learner(bn::sampler const& sampling)
        : sampling_(sampling)
    {
    }

    // per feature (vertex_list() order, the class left out): the position of its tree parent, -1 at the root
    std::vector<std::int32_t> const& parent() const { return parent_; }
    // ... and the weight of that edge (0.0 at the root): the mutual information (given the class) of the two vertices
    std::vector<double> const& weights() const { return weight_; }

protected:
    std::size_t learn(graph_t& graph, char const* who, std::int32_t const cond, std::int32_t const root)
    {
        if(sampling_.sampling_size() == 0) throw std::invalid_argument(std::string(who) + ": the sampler holds no samples");
        auto const nodes = graph.vertex_list();
        auto const n = static_cast<std::int32_t>(nodes.size());
        std::vector<std::int32_t> vars;
        for(std::int32_t v = 0; v < n; ++v)
            if(v != cond) vars.push_back(v);
        if(vars.empty()) throw std::invalid_argument(std::string(who) + ": no feature vertex");
        evaluation::information_table table(sampling_, nodes);
        parent_.assign(vars.size(), -1);
        weight_.assign(vars.size(), 0.0);
        mi355x::engine_handle::check(bn_learn_tree(table.handle(), cond, static_cast<std::int32_t>(vars.size()), vars.data(), root,
                                                   parent_.data(), weight_.data(), nullptr));
        graph.erase_all_edge();
        std::size_t edges = 0;
        for(std::size_t i = 0; i < vars.size(); ++i)
        {
            auto const& child = nodes[static_cast<std::size_t>(vars[i])];
            if(parent_[i] >= 0)
            {
                if(!graph.add_edge(nodes[static_cast<std::size_t>(parent_[i])], child))
                    throw std::logic_error(std::string(who) + ": the graph refused an edge of the tree");
                ++edges;
            }
            if(cond >= 0)
            {
                if(!graph.add_edge(nodes[static_cast<std::size_t>(cond)], child))
                    throw std::logic_error(std::string(who) + ": the graph refused an edge from the class");
                ++edges;
            }
        }
        sampling_.make_cpt(graph);
        return edges;
    }

    static std::int32_t position(graph_t const& graph, vertex_type const& v, char const* who)
    {
        auto const& nodes = graph.vertex_list();
        for(std::size_t i = 0; i < nodes.size(); ++i)
            if(nodes[i] == v) return static_cast<std::int32_t>(i);
        throw std::invalid_argument(std::string(who) + ": the vertex is not in the graph");
    }

    sampler const& sampling_;
    std::vector<std::int32_t> parent_;
    std::vector<double> weight_;
};

} // namespace detail

class chow_liu : public detail::tree_learner {
public:
    explicit chow_liu(bn::sampler const& sampling)
        : tree_learner(sampling)
    {
    }

    std::size_t operator()(graph_t& graph) { return learn(graph, "chow_liu", -1, -1); }
    std::size_t operator()(graph_t& graph, vertex_type const& root) { return learn(graph, "chow_liu", -1, position(graph, root, "chow_liu")); }
};

class tree_augmented : public detail::tree_learner {
public:
    explicit tree_augmented(bn::sampler const& sampling)
        : tree_learner(sampling)
    {
    }

    std::size_t operator()(graph_t& graph, vertex_type const& class_node)
    {
        return learn(graph, "tree_augmented", position(graph, class_node, "tree_augmented"), -1);
    }
    std::size_t operator()(graph_t& graph, vertex_type const& class_node, vertex_type const& root)
    {
        return learn(graph, "tree_augmented", position(graph, class_node, "tree_augmented"), position(graph, root, "tree_augmented"));
    }
};

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_CHOW_LIU_HPP
