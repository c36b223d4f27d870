// bayesian/inference/max_product.hpp -- most probable explanation (MPE / MAP, Pearl's belief revision) by MAX-PRODUCT belief
// propagation on the MI355X.  Not in the reference; the surface is that of this repository's belief_propagation functor:
//
//     bn::inference::max_product mp(graph);
//     auto max_marginals = mp(precondition, epsilon);   // per node the normalised max-marginal, a 1 x k matrix
//     auto assignment    = mp.mpe(precondition);        // vertex -> state of the most probable joint assignment
//     double logp        = mp.last_log_probability();   // log P(assignment), evidence nodes included
//
// The loop is the reference's (belief_propagation.hpp:33-158) with one line changed: pi(v) and the lambda-messages take the
// LARGEST term over the parent assignments where sum-product adds them (bn_mi355x.h, bn_mpe_run: the fold's NaN rule, the
// state's tie rule -- lowest index of the largest element).  Exact on polytrees; on a loopy network an approximation that may
// not converge: a run is cut after 10 000 sweeps (max_sweeps()), and converged() tells.
// Header-only C++14; link with -lbn_mi355x.
#ifndef BNI_INFERENCE_MAX_PRODUCT_HPP
#define BNI_INFERENCE_MAX_PRODUCT_HPP

#include <cmath>
#include <unordered_map>
#include <vector>

#include "mi355x_flatten.hpp"
#include "mi355x_marginals.hpp"

namespace bn {
namespace inference {

class max_product {
public:
    typedef std::unordered_map<vertex_type, matrix_type> return_type;
    typedef mi355x::marginals_view view_type;

    explicit max_product(graph_t const& graph)
        : graph_(graph), model_(mi355x::flatten(graph)), engine_(model_)
    {
    }
    // (copies own a second device engine built from the same flat model, like belief_propagation's)
    max_product(max_product const& other)
        : graph_(other.graph_), model_(other.model_), engine_(model_), max_sweeps_(other.max_sweeps_)
    {
    }
    max_product& operator=(max_product const& other)
    {
        if(this != &other)
        {
            graph_ = other.graph_;
            model_ = other.model_;
            engine_ = mi355x::engine_handle(model_);
            max_sweeps_ = other.max_sweeps_;
            states_.clear();
            marginals_.clear();
        }
        return *this;
    }
    max_product(max_product&&) = default;
    max_product& operator=(max_product&&) = default;
    virtual ~max_product() = default;

    // the max-marginals, as the map belief_propagation::operator() returns
    inline return_type operator()(double const epsilon = 0.001)
    {
        std::unordered_map<vertex_type, matrix_type> const precondition;
        return operator()(precondition, epsilon);
    }
    return_type operator()(std::unordered_map<vertex_type, matrix_type> const& precondition, double const epsilon = 0.001)
    {
        return run(precondition, epsilon).to_map();
    }

    // the same run, the max-marginals read in place: a non-owning view of this functor's result buffer, valid until its next call
    inline view_type run(double const epsilon = 0.001)
    {
        std::unordered_map<vertex_type, matrix_type> const precondition;
        return run(precondition, epsilon);
    }
    view_type run(std::unordered_map<vertex_type, matrix_type> const& precondition, double const epsilon = 0.001)
    {
        node_.clear();
        val_.clear();
        off_.assign(1, 0);
        for(auto const& p : precondition)
        {
            std::int32_t const position = model_.lookup.find(p.first.get());
            if(position < 0) throw std::runtime_error("max_product: evidence on an unknown vertex");
            if(p.second.height() != 1) throw std::runtime_error("max_product: evidence must be a 1 x k matrix");
            node_.push_back(position);
            val_.insert(val_.end(), p.second[0].begin(), p.second[0].end());
            off_.push_back(static_cast<std::int32_t>(val_.size()));
        }
        marginals_.resize(static_cast<std::size_t>(model_.node_off.back()));
        states_.resize(model_.k.size());
        std::int32_t sweeps = 0, converged = 0;
        double residual = 0;
        mi355x::engine_handle::check(bn_mpe_run(
            engine_.get(), static_cast<std::int32_t>(node_.size()), node_.data(), off_.data(), val_.data(), epsilon, max_sweeps_,
            marginals_.data(), states_.data(), &sweeps, &residual, &converged));
        last_sweeps_ = sweeps;
        last_residual_ = residual;
        converged_ = converged != 0;
        // log P(assignment) = sum over the nodes, in node order, of log cpt_v[row(states)][states_v] (fp64, on the host)
        double logp = 0.0;
        for(std::size_t v = 0; v < model_.k.size(); ++v)
        {
            std::int64_t row = 0;
            for(std::int32_t e = model_.in_ptr[v]; e < model_.in_ptr[v + 1]; ++e)
                row = row * model_.k[model_.in_idx[e]] + states_[model_.in_idx[e]];
            logp += std::log(model_.cpt[static_cast<std::size_t>(model_.cpt_off[v] + row * model_.k[v] + states_[v])]);
        }
        last_log_probability_ = logp;
        return view_type(model_, marginals_.data());
    }

    // the most probable joint assignment: vertex -> state, evidence nodes included
    std::unordered_map<vertex_type, int> mpe(std::unordered_map<vertex_type, matrix_type> const& precondition, double const epsilon = 0.001)
    {
        run(precondition, epsilon);
        std::unordered_map<vertex_type, int> out;
        out.reserve(states_.size());
        for(std::size_t v = 0; v < states_.size(); ++v) out.emplace(model_.nodes[v], static_cast<int>(states_[v]));
        return out;
    }
    inline std::unordered_map<vertex_type, int> mpe(double const epsilon = 0.001)
    {
        std::unordered_map<vertex_type, matrix_type> const precondition;
        return mpe(precondition, epsilon);
    }

    // tables edited after the functor was built (see belief_propagation::reload): the structure must be unchanged
    void reload() { mi355x::reload_cpts(graph_, model_, engine_); }
    void reload(graph_t const& graph) { mi355x::reload_cpts(graph, model_, engine_); graph_ = graph; }

    double last_log_probability() const { return last_log_probability_; }   // of the last run's decoded assignment
    bool converged() const { return converged_; }                           // false: the last run was cut by the cap
    int last_sweeps() const { return last_sweeps_; }
    double last_residual() const { return last_residual_; }
    int max_sweeps() const { return max_sweeps_ == 0 ? 10000 : max_sweeps_; }
    void set_max_sweeps(int cap) { max_sweeps_ = cap < 0 ? 0 : cap; }       // 0: the library's cap of 10 000 sweeps

private:
    graph_t graph_;
    mi355x::flat_model model_;
    mi355x::engine_handle engine_;
    std::vector<std::int32_t> node_, off_, states_;
    std::vector<double> val_, marginals_;
    std::int32_t max_sweeps_ = 0;
    int last_sweeps_ = 0;
    double last_residual_ = 0;
    double last_log_probability_ = 0;
    bool converged_ = false;
};

} // namespace inference
} // namespace bn

#endif // #ifndef BNI_INFERENCE_MAX_PRODUCT_HPP
