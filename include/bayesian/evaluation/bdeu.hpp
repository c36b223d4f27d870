// bayesian/evaluation/bdeu.hpp -- NOT IN THE REFERENCE: the Bayesian-Dirichlet scores as evaluation functors of the reference's
// shape (a sampler at construction, operator()(graph) and operator()(graph, vertex_list)), computed on the MI355X through
// bn_learn_create_spec / bn_learn_terms (include/bn_mi355x.h, "Bayesian-Dirichlet scores").  C++14.
//
//   basic_bdeu<std::ratio<N, D>>   BDeu with the equivalent sample size N / D;  bdeu = basic_bdeu<std::ratio<1>>
//   k2_score                       the K2 (Cooper-Herskovits) score: every Dirichlet hyperparameter 1
//
// The value is MINUS the log marginal likelihood of the samples under the graph's structure (its CPTs are not read): smaller is
// better, like aic and mdl, so the learning classes use them unchanged.  likelihood = 0.0; likelihood -= bd[v] over vertex_list in
// the given order; for the whole graph that is the learner's score, bit for bit.  The table is marshalled over graph.vertex_list()
// at every call.  An empty sampler gives 0.0 without touching the GPU.  An error of the C ABI throws std::runtime_error.
#ifndef BNI_EVALUATION_BDEU_HPP
#define BNI_EVALUATION_BDEU_HPP

#include <algorithm>
#include <cstdint>
#include <ratio>
#include <stdexcept>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/evaluation/basic_evaluation.hpp>
#include <bayesian/evaluation/transinformation.hpp>

namespace bn {
namespace evaluation {

class basic_bd_score : basic_evaluation {
public:
    basic_bd_score(sampler const& sampling, bn_score_spec const& spec) : sampling_(sampling), spec_(spec) {}
    virtual ~basic_bd_score() = default;

    virtual double operator() (graph_t const& graph) const
    {
        return (*this)(graph, graph.vertex_list());
    }

    virtual double operator() (graph_t const& graph, std::vector<bn::vertex_type> const& vertex_list) const
    {
        if(sampling_.sampling_size() == 0) return 0.0;
        auto const nodes = graph.vertex_list();
        information_table const table(sampling_, nodes);
        auto const index_of = [&nodes](vertex_type const& v)
        {
            auto const it = std::find(nodes.begin(), nodes.end(), v);
            if(it == nodes.end()) throw std::out_of_range("bn::evaluation: vertex not in the graph");
            return static_cast<std::int32_t>(it - nodes.begin());
        };
        std::vector<std::int32_t> in_ptr(1, 0), in_idx;
        for(auto const& node : nodes)
        {
            for(auto const& parent : graph.in_vertexes(node)) in_idx.push_back(index_of(parent));
            in_ptr.push_back(static_cast<std::int32_t>(in_idx.size()));
        }
        bn_learner* learner = nullptr;
        mi355x::engine_handle::check(bn_learn_create_spec(table.handle(), in_ptr.data(), in_idx.data(), spec_.kind, &spec_, 16, &learner));
        std::vector<double> bd(nodes.size() + 1, 0.0);
        int const rc = bn_learn_terms(learner, bd.data(), nullptr);
        bn_learn_destroy(learner);
        mi355x::engine_handle::check(rc);
        double likelihood = 0.0;
        for(auto const& v : vertex_list) likelihood -= bd[static_cast<std::size_t>(index_of(v))];
        return likelihood;
    }

    // what bn_learn_create_spec takes for this score
    bn_score_spec const& spec() const { return spec_; }

private:
    sampler const& sampling_;
    bn_score_spec spec_;
};

template<class Ess = std::ratio<1>>
struct basic_bdeu : basic_bd_score {
    static_assert(Ess::num > 0 && Ess::den > 0, "the equivalent sample size is positive");
    static constexpr double ess() { return static_cast<double>(Ess::num) / static_cast<double>(Ess::den); }
    basic_bdeu(sampler const& sampling) : basic_bd_score(sampling, bn_score_spec{2, 0, ess()}) {}
};

using bdeu = basic_bdeu<std::ratio<1>>;

struct k2_score : basic_bd_score {
    k2_score(sampler const& sampling) : basic_bd_score(sampling, bn_score_spec{3, 0, 0.0}) {}
};

} // namespace evaluation
} // namespace bn

#endif // BNI_EVALUATION_BDEU_HPP
