// bayesian/evaluation/basic_evaluation.hpp -- drop-in for the reference's bn::evaluation::basic_evaluation
// (bayesian/evaluation/basic_evaluation.hpp): the interface of a functor that scores a graph.  C++14.
#ifndef BNI_EVALUATION_BASIC_EVALUATION_HPP
#define BNI_EVALUATION_BASIC_EVALUATION_HPP

#include <bayesian/graph.hpp>

namespace bn {
namespace evaluation {

struct basic_evaluation {
    virtual ~basic_evaluation() = default;
    // API
    virtual double operator() (graph_t const& graph) const = 0;
};

} // namespace evaluation
} // namespace bn

#endif // BNI_EVALUATION_BASIC_EVALUATION_HPP
