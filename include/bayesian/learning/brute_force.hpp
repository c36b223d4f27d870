// bayesian/learning/brute_force.hpp -- drop-in for the reference's bn::learning::brute_force<Eval> (bayesian/learning/brute_force.hpp),
// the search running on the MI355X through bn_learn_brute_force / bn_learn_brute_force_hint (include/bn_mi355x.h) when Eval is
// bn::evaluation::aic or mdl.  C++14, no Boost.
//
// Same class, same members: brute_force(sampler const&), operator()(graph), operator()(graph, vertexes),
// learn_with_hint(graph, parent_nodes, child_nodes).
//
// How it runs.  AIC and MDL are decomposable, so for Eval = aic / mdl (exactly those types) an enumerated graph is scored from the
// family terms of the vertexes whose parents it changes.  Those terms -- every subset of the other vertexes (operator()) or of the
// parent nodes (learn_with_hint) as additional parents -- come from ONE pass over the device-resident table per vertex (the subset
// lattice, bn_learn_score_subsets); the enumeration itself walks the reference's graphs in the reference's order on the host,
// over those numbers, instead of one make_cpt and one evaluation of the whole graph per enumerated graph.  The best graph's edges
// are applied to the caller's graph with add_edge; one sampling_.make_cpt(graph) at the end.
// Any other Eval (a subclass of aic included) runs the reference's literal enumeration: make_cpt + eval_ per graph.
//
// Differences from the reference (aic / mdl path):
//   - the score is the learner's: the family terms take the device's fp64 logarithm (bn_mi355x.h states the function), so the
//     returned value agrees with eval_ to a few ulp per term, not bit for bit; two graphs whose scores are equal in exact
//     arithmetic (the two orientations of an edge) may therefore be ranked the other way round;
//   - the graph ends with CPTs fitted to the FINAL structure (the reference leaves the CPTs of the last enumerated graph);
//   - operator() takes at most 8 vertexes, and a family is limited to 16 parents, 2^20 table entries and 2^25 cells over all
//     subsets of its candidates: beyond them the call throws instead of running for days;
//   - learn_with_hint: when no child node reaches a parent node the search is made per child (no add_edge can be refused for a
//     cycle, and the edges into different children are independent terms); otherwise at most 20 possible edges are taken;
//   - an empty sampler takes the literal enumeration (and behaves as there).
// Not in the reference (labelled so below): learn_on / hint_on, the searches on an open learner session.
#ifndef BNI_LEARNING_BRUTE_FORCE_HPP
#define BNI_LEARNING_BRUTE_FORCE_HPP

#include <cstddef>
#include <utility>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/learning/greedy.hpp>

namespace bn {
namespace learning {

template<class Eval>
class brute_force {
public:
    brute_force(bn::sampler const& sampling)
        : sampling_(sampling), eval_(sampling_)
    {
    }

    double operator()(graph_t& graph)
    {
        return (*this)(graph, graph.vertex_list());
    }

    // the best graph over `vertexes`; returns eval_(graph, vertexes) of it
    double operator()(graph_t& graph, std::vector<vertex_type> const& vertexes)
    {
        if(on_device())
        {
            detail::learner_session session(sampling_, graph, detail::criterion_of<Eval>::value, detail::criterion_of<Eval>::spec());
            double const best = session.brute_force(graph, vertexes);
            sampling_.make_cpt(graph);
            return best;
        }
        sampling_.make_cpt(graph);
        graph_t best_graph = graph;
        double best = eval_(graph, vertexes);
        walk_levels(0, graph, vertexes, best_graph, best);
        graph = std::move(best_graph);
        return best;
    }

    // only edges from a node of parent_nodes to a node of child_nodes; returns eval_(graph) of the best graph
    double learn_with_hint(graph_t& graph, std::vector<vertex_type> parent_nodes, std::vector<vertex_type> child_nodes)
    {
        if(on_device())
        {
            detail::learner_session session(sampling_, graph, detail::criterion_of<Eval>::value, detail::criterion_of<Eval>::spec());
            double const best = session.brute_force_hint(graph, parent_nodes, child_nodes);
            sampling_.make_cpt(graph);
            return best;
        }
        std::vector<std::pair<vertex_type, vertex_type>> edges;   // parent-major
        for(auto const& parent : parent_nodes)
            for(auto const& child : child_nodes) edges.emplace_back(parent, child);
        sampling_.make_cpt(graph);
        graph_t best_graph = graph;
        double best = eval_(graph);
        walk_edges(0, edges, graph, best_graph, best);
        graph = std::move(best_graph);
        return best;
    }

    // NOT IN THE REFERENCE: the two searches on a learner session that is already open (stepwise_structure.hpp); the CPTs are
    // left to the caller.  learn_on returns the evaluated quantity of operator(), hint_on the session's score.
    double learn_on(detail::learner_session& session, graph_t& graph, std::vector<vertex_type> const& vertexes)
    {
        return session.brute_force(graph, vertexes);
    }

    double hint_on(detail::learner_session& session, graph_t& graph, std::vector<vertex_type> const& parent_nodes,
                   std::vector<vertex_type> const& child_nodes)
    {
        return session.brute_force_hint(graph, parent_nodes, child_nodes);
    }

private:
    bool on_device() const
    {
        return detail::criterion_of<Eval>::value >= 0 && sampling_.sampling_size() != 0;
    }

    void judge(graph_t& graph, double now, graph_t& best_graph, double& best)
    {
        if(now < best)
        {
            best = now;
            best_graph = graph;
        }
    }

    // every subset of edges[at ..]: without the edge first, then with it where add_edge takes it
    void walk_edges(std::size_t at, std::vector<std::pair<vertex_type, vertex_type>> const& edges, graph_t& graph, graph_t& best_graph,
                    double& best)
    {
        if(at == edges.size())
        {
            sampling_.make_cpt(graph);
            judge(graph, eval_(graph), best_graph, best);
            return;
        }
        walk_edges(at + 1, edges, graph, best_graph, best);
        if(auto const edge = graph.add_edge(edges[at].first, edges[at].second))
        {
            walk_edges(at + 1, edges, graph, best_graph, best);
            graph.erase_edge(edge);
        }
    }

    // level `level` pairs vertexes[level] with every later vertex: no edge, one way, the other way, each followed by the next level
    void walk_levels(std::size_t level, graph_t& graph, std::vector<vertex_type> const& vertexes, graph_t& best_graph, double& best)
    {
        if(level == vertexes.size() - 1)
        {
            sampling_.make_cpt(graph);
            judge(graph, eval_(graph, vertexes), best_graph, best);
            return;
        }
        for(std::size_t other = level + 1; other < vertexes.size(); ++other)
        {
            walk_levels(level + 1, graph, vertexes, best_graph, best);
            for(int way = 0; way < 2; ++way)
            {
                auto const& from = vertexes[way == 0 ? level : other];
                auto const& to = vertexes[way == 0 ? other : level];
                if(auto const edge = graph.add_edge(from, to))
                {
                    walk_levels(level + 1, graph, vertexes, best_graph, best);
                    graph.erase_edge(edge);
                }
            }
        }
    }

    sampler const& sampling_;
    Eval const eval_;
};

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_BRUTE_FORCE_HPP
