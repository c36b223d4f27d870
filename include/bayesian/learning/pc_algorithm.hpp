// bayesian/learning/pc_algorithm.hpp -- NOT IN THE REFERENCE: bn::learning::pc, constraint-based structure learning (the search of
// bnlearn's pc.stable, pgmpy's PC and pcalg) under the G^2 conditional-independence test, running on the MI355X through bn_learn_pc
// (include/bn_mi355x.h states the contract).  C++14, no Boost.
//
// Shaped like this repository's hill_climbing.hpp: pc(sampler const&), operator()(graph, alpha = 0.05, max_cond = 3) replaces the
// graph's edges by a DAG of the learned equivalence class (bn_pdag_to_dag: the lowest eligible node first), fits the CPTs with one
// sampling_.make_cpt(graph) and returns the number of edges; cpdag() and sepset(a, b) give the rest of the last call's result.
//
// How it runs.  The skeleton starts complete over graph.vertex_list().  At level l = 0 .. max_cond every test "x independent of y
// given S", |S| = l, S among x's neighbours at the start of the level, is decided on the device in one batch per level (a test is
// independent iff its p-value > alpha); an edge with an independent test is removed and the S of its lowest-rank independent test is
// its separating set.  Then v-structures and Meek's rules R1-R3 orient the skeleton into the CPDAG.
//
// There is no host twin: an empty sampler throws std::invalid_argument, and so does a CPDAG without a consistent extension.
#ifndef BNI_LEARNING_PC_ALGORITHM_HPP
#define BNI_LEARNING_PC_ALGORITHM_HPP

#include <cstdint>
#include <stdexcept>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/evaluation/transinformation.hpp>

namespace bn {
namespace learning {

class pc {
public:
    pc(bn::sampler const& sampling)
        : sampling_(sampling)
    {
    }

    // the rule for the degrees of freedom (0 nominal, bnlearn "mi"; 1 adjusted, "mi-adf") and the per-level cap on tests (0: 2^22)
    void set_df_rule(int df_rule) { df_rule_ = df_rule; }
    void set_max_tests(std::int64_t max_tests) { max_tests_ = max_tests; }
    int df_rule() const { return df_rule_; }

    std::size_t operator()(graph_t& graph, double const alpha = 0.05, int const max_cond = 3)
    {
        if(sampling_.sampling_size() == 0) throw std::invalid_argument("pc: the sampler holds no samples");
        if(!(alpha > 0.0 && alpha < 1.0)) throw std::invalid_argument("pc: alpha must be inside (0, 1)");
        if(max_cond < 0 || max_cond > 8) throw std::invalid_argument("pc: max_cond must be in 0..8");
        nodes_ = graph.vertex_list();
        auto const n = nodes_.size();
        evaluation::information_table table(sampling_, nodes_);
        bn_pc_params const params{alpha, max_cond, df_rule_, max_tests_};
        std::vector<std::uint8_t> skeleton(n * n + 1, 0);
        std::vector<std::int32_t> sep_idx(n * n * static_cast<std::size_t>(max_cond) + 1, 0);
        std::vector<bn_pc_level> levels(static_cast<std::size_t>(max_cond) + 1);
        std::int32_t n_levels = 0;
        cpdag_.assign(n * n + 1, 0);
        sep_len_.assign(n * n + 1, -1);
        mi355x::engine_handle::check(bn_learn_pc(table.handle(), &params, nullptr, skeleton.data(), cpdag_.data(), sep_len_.data(),
                                                 sep_idx.data(), levels.data(), &n_levels, &tests_skipped_));
        cpdag_.resize(n * n);
        stride_ = static_cast<std::size_t>(max_cond);
        sep_idx_.swap(sep_idx);
        std::vector<std::int32_t> in_ptr(n + 1, 0), in_idx(n * n + 1, 0);
        if(bn_pdag_to_dag(static_cast<std::int32_t>(n), cpdag_.data(), in_ptr.data(), in_idx.data()) < 0)
            throw std::invalid_argument(std::string("pc: ") + bn_last_error());
        graph.erase_all_edge();
        for(std::size_t v = 0; v < n; ++v)
            for(std::int32_t e = in_ptr[v]; e < in_ptr[v + 1]; ++e)
                if(!graph.add_edge(nodes_[static_cast<std::size_t>(in_idx[static_cast<std::size_t>(e)])], nodes_[v]))
                    throw std::logic_error("pc: the graph refused an edge of the DAG extension");
        sampling_.make_cpt(graph);
        return static_cast<std::size_t>(in_ptr[n]);
    }

    // the last call's CPDAG over vertex_list() positions, [n][n] marks: both [a][b] and [b][a] set: a - b; only [a][b]: a -> b
    std::vector<std::uint8_t> const& cpdag() const { return cpdag_; }
    // the separating set of the positions a, b (increasing positions); has_sepset: false for a pair that stayed adjacent
    bool has_sepset(std::size_t a, std::size_t b) const { return sep_len_[a * nodes_.size() + b] >= 0; }
    std::vector<std::int32_t> sepset(std::size_t a, std::size_t b) const
    {
        auto const at = a * nodes_.size() + b;
        if(sep_len_[at] < 0) return {};
        auto const first = sep_idx_.begin() + static_cast<std::ptrdiff_t>(at * stride_);
        return std::vector<std::int32_t>(first, first + sep_len_[at]);
    }
    std::int64_t tests_skipped() const { return tests_skipped_; }

private:
    sampler const& sampling_;
    int df_rule_ = 0;
    std::int64_t max_tests_ = 0;
    std::vector<vertex_type> nodes_;
    std::vector<std::uint8_t> cpdag_;
    std::vector<std::int32_t> sep_len_, sep_idx_;
    std::size_t stride_ = 0;
    std::int64_t tests_skipped_ = 0;
};

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_PC_ALGORITHM_HPP
