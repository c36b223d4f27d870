// bayesian/learning/expectation_maximization.hpp -- CPTs fitted from a table with UNOBSERVED cells by expectation-maximisation on the
// MI355X.  Not in the reference, whose sampler::make_cpt counts complete rows only; the surface follows this repository's functors:
//
//     bn::learning::expectation_maximization em(graph);
//     int iterations = em(graph, patterns, counts);      // the fitted tables are written into every vertex's cpt, as make_cpt does
//
// patterns holds one row of graph.vertex_list().size() states per pattern, row after row, in vertex_list() order; a cell of
// expectation_maximization::missing (255) is "not observed".  counts has one occurrence count per row.  The E-step runs one
// sum-product query per row on the GPU (the observed cells as hard evidence) and adds the family posteriors, weighted by the counts;
// the M-step normalises (include/bn_mi355x.h, bn_em_fit: the rules, the order of every sum, the stopping rule).  The iteration starts
// from the tables the graph holds at the call.  Networks that do not fit one workgroup: std::runtime_error with the planner's reason.
// Header-only C++14; link with -lbn_mi355x.
#ifndef BNI_LEARNING_EXPECTATION_MAXIMIZATION_HPP
#define BNI_LEARNING_EXPECTATION_MAXIMIZATION_HPP

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../inference/mi355x_flatten.hpp"

namespace bn {
namespace learning {

struct em_options {
    int max_iters = 100;       // 1 .. 10 000
    double tol = 1e-6;         // stop after the iteration whose largest change of a table entry is below it (strict)
    double bp_eps = 1e-3;      // belief propagation: epsilon of each row's run
    int bp_max_sweeps = 0;     // ... and its sweep cap (0: 10 000)
    double prior = 0.0;        // added to every expected count before the M-step (>= 0)
};

class expectation_maximization {
public:
    static constexpr std::uint8_t missing = BN_EM_MISSING;
    typedef em_options options_type;

    explicit expectation_maximization(graph_t const& graph)
        : model_(mi355x::flatten(graph)), engine_(model_)
    {
    }
    virtual ~expectation_maximization() = default;

    // Fits the tables of `graph` (the structure this functor was built from) and writes them into the vertices' cpt.
    // Returns the number of iterations run.
    int operator()(graph_t const& graph, std::vector<std::uint8_t> const& patterns, std::vector<std::uint64_t> const& counts,
                   options_type const& options = options_type())
    {
        mi355x::flat_model const now = mi355x::flatten(graph);
        if(now.nodes != model_.nodes || now.k != model_.k || now.in_ptr != model_.in_ptr || now.in_idx != model_.in_idx)
            throw std::runtime_error("expectation_maximization: the graph's structure changed since the functor was built (build a new one)");
        std::size_t const n = model_.k.size();
        if(n == 0 || patterns.size() != counts.size() * n)
            throw std::runtime_error("expectation_maximization: patterns must hold one row of vertex_list().size() states per count");
        bn_em_options opt;
        opt.max_iters = options.max_iters;
        opt.tol = options.tol;
        opt.bp_eps = options.bp_eps;
        opt.bp_max_sweeps = options.bp_max_sweeps;
        opt.prior = options.prior;
        std::vector<double> fitted(now.cpt.size());
        delta_history_.assign(static_cast<std::size_t>(options.max_iters > 0 ? options.max_iters : 0), 0.0);
        std::int32_t iters = 0;
        mi355x::engine_handle::check(bn_em_fit(
            engine_.get(), static_cast<std::int64_t>(counts.size()), patterns.data(), reinterpret_cast<std::uint64_t const*>(counts.data()), &opt,
            now.cpt.data(), fitted.data(), &iters, delta_history_.data(), static_cast<std::int32_t>(delta_history_.size())));
        delta_history_.resize(static_cast<std::size_t>(iters));
        mi355x::store_cpts(graph, model_, fitted);
        last_capped_ = bn_get_info(engine_.get(), "em_capped");
        last_skipped_ = bn_get_info(engine_.get(), "em_skipped");
        return static_cast<int>(iters);
    }

    std::vector<double> const& delta_history() const { return delta_history_; }   // the largest change of an entry, per iteration
    long long last_capped() const { return last_capped_; }      // row runs cut by the sweep cap in the last call
    long long last_skipped() const { return last_skipped_; }    // row families whose evidence had probability 0 under the tables

private:
    mi355x::flat_model model_;
    mi355x::engine_handle engine_;
    std::vector<double> delta_history_;
    long long last_capped_ = 0, last_skipped_ = 0;
};

} // namespace learning
} // namespace bn

#endif // #ifndef BNI_LEARNING_EXPECTATION_MAXIMIZATION_HPP
