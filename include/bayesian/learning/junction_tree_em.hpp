// bayesian/learning/junction_tree_em.hpp -- CPTs fitted from a table with UNOBSERVED cells by expectation-maximisation with an EXACT
// E-step on the MI355X: the family posteriors come from junction-tree propagation, not from loopy belief propagation, so they are
// P(x_v, pa(v) | e) on networks with loops too (expectation_maximization.hpp is exact on polytrees only).  Not in the reference; the
// surface is expectation_maximization's:
//
//     bn::learning::junction_tree_em em(graph);
//     int iterations = em(graph, patterns, counts);      // the fitted tables are written into every vertex's cpt, as make_cpt does
//
// patterns holds one row of graph.vertex_list().size() states per pattern, row after row, in vertex_list() order; a cell of
// junction_tree_em::missing (255) is "not observed".  counts has one occurrence count per row.  The E-step runs one junction-tree
// propagation per row on the GPU and adds the family posteriors, weighted by the counts; the M-step normalises
// (include/bn_mi355x.h, bn_jt_em_fit: the rules, the order of every sum, the stopping rule).  The iteration starts from the tables
// the graph holds at the call.  loglik_history() holds the observed-data log-likelihood of the table under the tables each
// iteration started from.  Networks whose clique tree is beyond the plan's limits: std::runtime_error with the planner's reason.
// Header-only C++14; link with -lbn_mi355x.
#ifndef BNI_LEARNING_JUNCTION_TREE_EM_HPP
#define BNI_LEARNING_JUNCTION_TREE_EM_HPP

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../inference/mi355x_flatten.hpp"

namespace bn {
namespace learning {

struct jt_em_options {
    int max_iters = 100;       // 1 .. 10 000
    double tol = 1e-6;         // stop after the iteration whose largest change of a table entry is below it (strict)
    double prior = 0.0;        // added to every expected count before the M-step (>= 0)
};

class junction_tree_em {
public:
    static constexpr std::uint8_t missing = BN_EM_MISSING;
    typedef jt_em_options options_type;

    explicit junction_tree_em(graph_t const& graph)
        : model_(mi355x::flatten(graph)), engine_(model_)
    {
    }
    virtual ~junction_tree_em() = default;

    // Fits the tables of `graph` (the structure this functor was built from) and writes them into the vertices' cpt.
    // Returns the number of iterations run.
    int operator()(graph_t const& graph, std::vector<std::uint8_t> const& patterns, std::vector<std::uint64_t> const& counts,
                   options_type const& options = options_type())
    {
        mi355x::flat_model const now = mi355x::flatten(graph);
        if(now.nodes != model_.nodes || now.k != model_.k || now.in_ptr != model_.in_ptr || now.in_idx != model_.in_idx)
            throw std::runtime_error("junction_tree_em: the graph's structure changed since the functor was built (build a new one)");
        std::size_t const n = model_.k.size();
        if(n == 0 || patterns.size() != counts.size() * n)
            throw std::runtime_error("junction_tree_em: patterns must hold one row of vertex_list().size() states per count");
        bn_jt_em_options opt;
        opt.max_iters = options.max_iters;
        opt.tol = options.tol;
        opt.prior = options.prior;
        std::vector<double> fitted(now.cpt.size());
        std::size_t const cap = static_cast<std::size_t>(options.max_iters > 0 ? options.max_iters : 0);
        delta_history_.assign(cap, 0.0);
        loglik_history_.assign(cap, 0.0);
        std::int32_t iters = 0;
        mi355x::engine_handle::check(bn_jt_em_fit(
            engine_.get(), static_cast<std::int64_t>(counts.size()), patterns.data(), reinterpret_cast<std::uint64_t const*>(counts.data()), &opt,
            now.cpt.data(), fitted.data(), &iters, delta_history_.data(), loglik_history_.data(), static_cast<std::int32_t>(cap)));
        delta_history_.resize(static_cast<std::size_t>(iters));
        loglik_history_.resize(static_cast<std::size_t>(iters));
        mi355x::store_cpts(graph, model_, fitted);
        last_skipped_ = bn_get_info(engine_.get(), "jt_em_skipped");
        return static_cast<int>(iters);
    }

    std::vector<double> const& delta_history() const { return delta_history_; }     // the largest change of an entry, per iteration
    std::vector<double> const& loglik_history() const { return loglik_history_; }   // log-likelihood under the tables an iteration started from
    long long last_skipped() const { return last_skipped_; }    // row families whose evidence had probability 0 under the tables

private:
    mi355x::flat_model model_;
    mi355x::engine_handle engine_;
    std::vector<double> delta_history_, loglik_history_;
    long long last_skipped_ = 0;
};

} // namespace learning
} // namespace bn

#endif // #ifndef BNI_LEARNING_JUNCTION_TREE_EM_HPP
