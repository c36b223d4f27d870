// bayesian/evaluation/basic_info_criteria.hpp -- drop-in for the reference's bn::evaluation::basic_info_criteria
// (bayesian/evaluation/basic_info_criteria.hpp:13-125), the base of aic and mdl, with calc_likelihood computed on the
// MI355X through bn_score_nodes (include/bn_mi355x.h).  C++14.
//
// Same class, same members: basic_info_criteria(sampler const&), both operator() overloads, calc_likelihood(graph[,
// vertex_list]) = -log P(D | graph) over the listed nodes (natural logarithm, :51-91), calc_parameters(graph) = sum over
// ALL nodes of (selectable_num - 1) x product of the parents' selectable_num (:100-117), sampling_size().
//
// How it runs.  The sampler's table is marshalled over graph.vertex_list() at the FIRST call and kept on the device
// (an information_table): a sampler reloaded afterwards needs a new functor.  Every call flattens the graph it is given
// and builds an engine from it (the graph carries no mark that would tell a cached engine its CPTs are still current);
// that costs one flatten() and one bn_create per call -- about a millisecond on an ALARM-sized network, more than the
// scoring kernels themselves.  Callers that score one network many times use the C ABI with an engine of their own.
// The per-node sums come back in node order and are then subtracted in the order of `vertex_list`, like the
// reference's loop over the nodes; inside a node the order of the additions is bn_score_nodes', not the unspecified
// order of the reference's unordered_map.  An empty sampler gives likelihood 0.0 without touching the GPU.
// An error of the C ABI throws std::runtime_error.
//
// Differences from the reference: an entry of probability 0 that no sample shows adds nothing (the same there: it
// never enters the statistics); a graph whose vertices or arities differ from the ones the table was marshalled
// with is an error, not a lookup failure.
// Not in the reference (labelled so below): log_likelihood, log_likelihood_rows, row_patterns.
#ifndef BNI_EVALUATION_BASIC_INFO_CRITERIA_HPP
#define BNI_EVALUATION_BASIC_INFO_CRITERIA_HPP

#include <cstdint>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/evaluation/basic_evaluation.hpp>
#include <bayesian/evaluation/transinformation.hpp>
#include <bayesian/inference/mi355x_flatten.hpp>

namespace bn {
namespace evaluation {

class basic_info_criteria : basic_evaluation {
public:
    basic_info_criteria(sampler const& sampling) : sampling_(sampling) {}

    // API
    virtual double operator() (graph_t const& graph) const
    {
        return (*this)(graph, graph.vertex_list());
    }
    virtual double operator() (graph_t const& graph, std::vector<bn::vertex_type> const& vertex_list) const = 0;

    // NOT IN THE REFERENCE: per node of graph.vertex_list(), sum over the CPT entries the samples show of
    // count x log(entry) (bn_score_nodes); empty for an empty sampler
    std::vector<double> log_likelihood(graph_t const& graph) const
    {
        if(sampling_size() == 0) return {};
        mi355x::flat_model const fm = mi355x::flatten(graph);
        mi355x::engine_handle const engine(fm);
        std::vector<double> ll(fm.k.size(), 0.0);
        mi355x::engine_handle::check(bn_score_nodes(engine.get(), table(graph), ll.data(), nullptr));
        return ll;
    }

    // NOT IN THE REFERENCE: per distinct pattern of the table, in the order of row_patterns(), the sum over every node
    // of log P(state | parents' states) (bn_score_rows); -inf for a pattern the graph gives probability 0
    std::vector<double> log_likelihood_rows(graph_t const& graph) const
    {
        if(sampling_size() == 0) return {};
        mi355x::flat_model const fm = mi355x::flatten(graph);
        mi355x::engine_handle const engine(fm);
        bn_info_table* const t = table(graph);
        std::vector<double> ll(rows_.size(), 0.0);
        mi355x::engine_handle::check(bn_score_rows(engine.get(), t, 0, nullptr, ll.data()));
        return ll;
    }

    // NOT IN THE REFERENCE: the distinct patterns in the order log_likelihood_rows reports them (set by the first call)
    std::vector<condition_t> const& row_patterns() const { return rows_; }

protected:
    // - log P_theta^N(D)
    double calc_likelihood(graph_t const& graph) const
    {
        return calc_likelihood(graph, graph.vertex_list());
    }
    double calc_likelihood(graph_t const& graph, std::vector<bn::vertex_type> const& vertex_list) const
    {
        double likelihood = 0.0;
        if(sampling_size() == 0) return likelihood;
        auto const nodes = graph.vertex_list();
        auto const ll = log_likelihood(graph);
        for(auto const& node : vertex_list)
        {
            auto const it = std::find(nodes.begin(), nodes.end(), node);
            if(it == nodes.end()) throw std::out_of_range("bn::evaluation::basic_info_criteria: vertex not in the graph");
            likelihood -= ll[static_cast<std::size_t>(it - nodes.begin())];
        }
        return likelihood;
    }

    // + d: over the whole graph, whatever vertex_list the score is asked for (aic.hpp:23-24, mdl.hpp:24-25)
    double calc_parameters(graph_t const& graph) const
    {
        std::int64_t parameters = 0;
        for(auto const& node : graph.vertex_list())
        {
            auto const parents = graph.in_vertexes(node);
            std::int64_t rows = static_cast<std::int64_t>(node->selectable_num) - 1;
            for(auto const& parent : parents) rows *= static_cast<std::int64_t>(parent->selectable_num);
            parameters += rows;
        }
        return static_cast<double>(parameters);
    }

    std::size_t sampling_size() const { return sampling_.sampling_size(); }

private:
    // the sampler's table over graph.vertex_list(), marshalled once
    bn_info_table* table(graph_t const& graph) const
    {
        if(!table_)
        {
            auto const nodes = graph.vertex_list();
            std::vector<condition_t> rows;
            table_.reset(new information_table(sampling_, nodes, BN_DEVICE_CURRENT, &rows));
            rows_.swap(rows);
        }
        return table_->handle();
    }

    sampler const& sampling_;
    mutable std::unique_ptr<information_table> table_;
    mutable std::vector<condition_t> rows_;
};

} // namespace evaluation
} // namespace bn

#endif // BNI_EVALUATION_BASIC_INFO_CRITERIA_HPP
