// bayesian/learning/optimal_structure.hpp -- NOT IN THE REFERENCE: bn::learning::optimal_structure<Eval>, the exact search for the
// DAG of globally smallest score by dynamic programming over node subsets (Silander & Myllymaki 2006; the search of pgmpy's
// ExhaustiveSearch), running on the MI355X through bn_learn_optimal (include/bn_mi355x.h states the contract) when Eval is
// bn::evaluation::aic, mdl, basic_bdeu<> or k2_score.  C++14, no Boost.
//
// Shaped like this repository's hill_climbing.hpp: optimal_structure(sampler const&), operator()(graph) returns the score of the
// learned graph and leaves the graph in `graph`; the edges `graph` comes with do not steer the search.
//
// How it runs.  The family term of EVERY parent set of at most max_parents() nodes per child is computed once (bn_terms_create);
// over that table the device finds, for every child and every candidate set, the best parent set inside it (a min-zeta transform
// over n * 2^(n - 1) cells), then the best sink of every node subset level by level, and walks the sinks back from the full set.
// The result is a graph no DAG within the in-degree bound scores better than; it replaces the caller's edges; one
// sampling_.make_cpt(graph) at the end.  At most 24 nodes (2.4 GB of device memory at 24); more throw from the library's check.
// set_allowed(masks): one mask per node in vertex_list() order, bit u of masks[v] set: u may be a parent of v (empty: no limit).
// last_value(): the cost as the search added it up, R[V]; the returned score is the learner's own arithmetic on the same graph and
// may differ from it in the last bits.
//
// There is no host twin: an Eval other than those four, or an empty sampler, throws std::invalid_argument.
#ifndef BNI_LEARNING_OPTIMAL_STRUCTURE_HPP
#define BNI_LEARNING_OPTIMAL_STRUCTURE_HPP

#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/learning/greedy.hpp>

namespace bn {
namespace learning {

template<class Eval>
class optimal_structure {
public:
    optimal_structure(bn::sampler const& sampling)
        : sampling_(sampling)
    {
    }

    // the in-degree bound (1 .. 16) and the parents every node may have
    void set_max_parents(int max_parents) { max_parents_ = max_parents; }
    void set_allowed(std::vector<std::uint64_t> allowed) { allowed_ = std::move(allowed); }
    int max_parents() const { return max_parents_; }
    double last_value() const { return last_value_; }

    double operator()(graph_t& graph)
    {
        if(detail::criterion_of<Eval>::value < 0) throw std::invalid_argument("optimal_structure: Eval must be aic, mdl, basic_bdeu<> or k2_score");
        if(sampling_.sampling_size() == 0) throw std::invalid_argument("optimal_structure: the sampler holds no samples");
        if(max_parents_ < 1 || max_parents_ > 16) throw std::invalid_argument("optimal_structure: max_parents must be in 1..16");
        if(!allowed_.empty() && allowed_.size() != graph.vertex_list().size())
            throw std::invalid_argument("optimal_structure: allowed must hold one mask per node");
        detail::learner_session session(sampling_, graph, detail::criterion_of<Eval>::value, detail::criterion_of<Eval>::spec());
        last_value_ = session.optimal(graph, max_parents_, allowed_);
        sampling_.make_cpt(graph);
        return session.score();
    }

private:
    sampler const& sampling_;
    int max_parents_ = 3;
    std::vector<std::uint64_t> allowed_;
    double last_value_ = 0.0;
};

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_OPTIMAL_STRUCTURE_HPP
