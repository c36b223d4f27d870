// bayesian/inference/junction_tree.hpp -- EXACT marginals by junction-tree (clique-tree) propagation on the MI355X.  Not in the
// reference; the surface is that of this repository's belief_propagation functor:
//
//     bn::inference::junction_tree jt(graph);
//     auto marginals = jt(precondition);        // per node normalise(P(x_v, e)), a 1 x k matrix
//     double logp    = jt.log_evidence();       // log P(e) of the last call
//     auto best      = jt.mpe(precondition);    // exact MPE: (vertex -> state, log max_x P(x, e)), decoded by backtracking
//
// belief_propagation is exact on polytrees and an approximation on networks with loops; this functor is exact on every network
// whose clique tree the library's planner takes (bn_mi355x.h, bn_jt_run: no clique table above 2^20 entries, the state of one
// query within the scratch budget) and throws std::runtime_error with the planner's reason on the others.  Evidence is a
// LIKELIHOOD, hard or soft, and an evidence node's marginal is its posterior -- not the reference BP's e^2 / sum(e^2).  Evidence
// of probability 0 gives NaN marginals and log_evidence() = -infinity.
// Header-only C++14; link with -lbn_mi355x.
#ifndef BNI_INFERENCE_JUNCTION_TREE_HPP
#define BNI_INFERENCE_JUNCTION_TREE_HPP

#include <unordered_map>
#include <utility>
#include <vector>

#include "mi355x_flatten.hpp"
#include "mi355x_marginals.hpp"

namespace bn {
namespace inference {

class junction_tree {
public:
    typedef std::unordered_map<vertex_type, matrix_type> return_type;
    typedef mi355x::marginals_view view_type;

    explicit junction_tree(graph_t const& graph)
        : graph_(graph), model_(mi355x::flatten(graph)), engine_(model_)
    {
    }
    // (copies own a second device engine built from the same flat model, like belief_propagation's)
    junction_tree(junction_tree const& other)
        : graph_(other.graph_), model_(other.model_), engine_(model_)
    {
    }
    junction_tree& operator=(junction_tree const& other)
    {
        if(this != &other)
        {
            graph_ = other.graph_;
            model_ = other.model_;
            engine_ = mi355x::engine_handle(model_);
            marginals_.clear();
            max_marginals_.clear();
            states_.clear();
        }
        return *this;
    }
    junction_tree(junction_tree&&) = default;
    junction_tree& operator=(junction_tree&&) = default;
    virtual ~junction_tree() = default;

    // the marginals, as the map belief_propagation::operator() returns
    inline return_type operator()()
    {
        std::unordered_map<vertex_type, matrix_type> const precondition;
        return operator()(precondition);
    }
    return_type operator()(std::unordered_map<vertex_type, matrix_type> const& precondition)
    {
        return run(precondition).to_map();
    }

    // the same run, the marginals read in place: a non-owning view of this functor's result buffer, valid until its next call
    inline view_type run()
    {
        std::unordered_map<vertex_type, matrix_type> const precondition;
        return run(precondition);
    }
    view_type run(std::unordered_map<vertex_type, matrix_type> const& precondition)
    {
        pack(precondition);
        marginals_.resize(static_cast<std::size_t>(model_.node_off.back()));
        double log_evidence = 0;
        mi355x::engine_handle::check(bn_jt_run(
            engine_.get(), static_cast<std::int32_t>(node_.size()), node_.data(), off_.data(), val_.data(), marginals_.data(), &log_evidence));
        log_evidence_ = log_evidence;
        return view_type(model_, marginals_.data());
    }

    // exact MPE (bn_jt_mpe_run: max-propagation with backtracking): the most probable joint assignment, vertex -> state with the
    // evidence nodes included, and log max_x P(x, e).  Exact also where assignments tie -- the decoded assignment attains the
    // maximum, which max_product's per-node decoding cannot promise.  Evidence of probability 0: -infinity, and states without
    // meaning.  max_marginals() reads the call's normalised max-marginals in place.
    typedef std::pair<std::unordered_map<vertex_type, int>, double> mpe_type;
    mpe_type mpe(std::unordered_map<vertex_type, matrix_type> const& precondition)
    {
        pack(precondition);
        max_marginals_.resize(static_cast<std::size_t>(model_.node_off.back()));
        states_.resize(model_.k.size());
        double log_p = 0;
        mi355x::engine_handle::check(bn_jt_mpe_run(
            engine_.get(), static_cast<std::int32_t>(node_.size()), node_.data(), off_.data(), val_.data(), max_marginals_.data(), states_.data(),
            &log_p));
        mpe_type out;
        out.first.reserve(states_.size());
        for(std::size_t v = 0; v < states_.size(); ++v) out.first.emplace(model_.nodes[v], static_cast<int>(states_[v]));
        out.second = log_p;
        return out;
    }
    inline mpe_type mpe()
    {
        std::unordered_map<vertex_type, matrix_type> const precondition;
        return mpe(precondition);
    }
    // a non-owning view of the last mpe()'s max-marginals, valid until the next mpe()
    view_type max_marginals() const { return view_type(model_, max_marginals_.data()); }

    // tables edited after the functor was built (see belief_propagation::reload): the structure must be unchanged
    void reload() { mi355x::reload_cpts(graph_, model_, engine_); }
    void reload(graph_t const& graph) { mi355x::reload_cpts(graph, model_, engine_); graph_ = graph; }

    double log_evidence() const { return log_evidence_; }   // log P(e) of the last run

private:
    // the evidence of a call as the library takes it
    void pack(std::unordered_map<vertex_type, matrix_type> const& precondition)
    {
        node_.clear();
        val_.clear();
        off_.assign(1, 0);
        for(auto const& p : precondition)
        {
            std::int32_t const position = model_.lookup.find(p.first.get());
            if(position < 0) throw std::runtime_error("junction_tree: evidence on an unknown vertex");
            if(p.second.height() != 1) throw std::runtime_error("junction_tree: evidence must be a 1 x k matrix");
            node_.push_back(position);
            val_.insert(val_.end(), p.second[0].begin(), p.second[0].end());
            off_.push_back(static_cast<std::int32_t>(val_.size()));
        }
    }

    graph_t graph_;
    mi355x::flat_model model_;
    mi355x::engine_handle engine_;
    std::vector<std::int32_t> node_, off_, states_;
    std::vector<double> val_, marginals_, max_marginals_;
    double log_evidence_ = 0;
};

} // namespace inference
} // namespace bn

#endif // #ifndef BNI_INFERENCE_JUNCTION_TREE_HPP
