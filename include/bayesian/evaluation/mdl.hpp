// bayesian/evaluation/mdl.hpp -- drop-in for the reference's bn::evaluation::mdl (bayesian/evaluation/mdl.hpp):
// MDL = -log P(D | graph) + parameters x log2(N) / 2, N the number of samples; natural logarithm in the likelihood
// and log2 in the correction, as there (:21-36).  The likelihood runs on the MI355X (basic_info_criteria.hpp); the
// parameters are those of the whole graph also for a vertex_list; an empty sampler throws
// std::runtime_error("Sampling is not finished yet.").
#ifndef BNI_EVALUATION_MDL_HPP
#define BNI_EVALUATION_MDL_HPP

#include <cmath>
#include <stdexcept>

#include <bayesian/graph.hpp>
#include <bayesian/evaluation/basic_info_criteria.hpp>

namespace bn {
namespace evaluation {

struct mdl : basic_info_criteria {
    mdl(sampler const& sampling) : basic_info_criteria(sampling) {}

    double operator() (graph_t const& graph) const override
    {
        return (*this)(graph, graph.vertex_list());
    }

    double operator() (graph_t const& graph, std::vector<bn::vertex_type> const& vertex_list) const override
    {
        auto const likelihood = calc_likelihood(graph, vertex_list);
        auto const parameters = calc_parameters(graph);
        if(auto const sampling_size = this->sampling_size())
        {
            auto const correction = std::log2(static_cast<double>(sampling_size)) / 2;
            return likelihood + parameters * correction;
        }
        throw std::runtime_error("Sampling is not finished yet.");
    }
};

} // namespace evaluation
} // namespace bn

#endif // BNI_EVALUATION_MDL_HPP
