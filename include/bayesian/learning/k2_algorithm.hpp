// bayesian/learning/k2_algorithm.hpp -- drop-in for the reference's bn::learning::k2_algorithm<Eval>
// (bayesian/learning/k2_algorithm.hpp), the search running on the MI355X through bn_learn_* (include/bn_mi355x.h) when Eval is
// bn::evaluation::aic or mdl.  C++14, no Boost.
//
// Same class, same members: k2_algorithm(sampler const&), operator()(graph, precondition).  The targets are shuffled; a target's
// candidates are every node of vertex_list() in that order but the target itself and the nodes precondition lists for it; an
// accepted parent gets the target into ITS list (:57), so the reverse edge is not offered later.
// How it runs, and the differences from the reference: as greedy.hpp states them (one device pass per accepted edge and child;
// the learner's score; CPTs of the final structure; the limits of 16 parents and 2^20 entries per family; the literal loop for
// any other Eval and for an empty sampler).
// Not in the reference (labelled so below): the constructor taking a seed, last_visits().
#ifndef BNI_LEARNING_K2_ALGORITHM_HPP
#define BNI_LEARNING_K2_ALGORITHM_HPP

#include <algorithm>
#include <cstdint>
#include <memory>
#include <random>
#include <unordered_map>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/learning/greedy.hpp>

namespace bn {
namespace learning {

template<class Eval>
class k2_algorithm {
public:
    k2_algorithm(bn::sampler const& sampling)
        : sampling_(sampling), eval_(sampling_), engine_(detail::make_engine())
    {
    }

    // NOT IN THE REFERENCE: a reproducible run
    k2_algorithm(bn::sampler const& sampling, std::uint32_t seed)
        : sampling_(sampling), eval_(sampling_), engine_(seed)
    {
    }

    double operator()(graph_t& graph, std::unordered_map<vertex_type, std::vector<vertex_type>> preconditon)
    {
        bool const on_device = detail::criterion_of<Eval>::value >= 0 && sampling_.sampling_size() != 0;
        std::unique_ptr<detail::learner_session> session;
        double eval_best = 0.0;
        if(on_device) session.reset(new detail::learner_session(sampling_, graph, detail::criterion_of<Eval>::value, detail::criterion_of<Eval>::spec()));
        else
        {
            sampling_.make_cpt(graph);
            eval_best = eval_(graph);
        }

        auto vertexes = graph.vertex_list();
        std::shuffle(vertexes.begin(), vertexes.end(), engine_);
        visits_.clear();

        for(auto const& target : vertexes)
        {
            std::vector<vertex_type> candidature;
            auto const ignore_nodes = preconditon.find(target);
            for(auto const& node : graph.vertex_list())
            {
                if(node == target) continue;
                if(ignore_nodes != preconditon.end() &&
                   std::find(ignore_nodes->second.begin(), ignore_nodes->second.end(), node) != ignore_nodes->second.end()) continue;
                candidature.push_back(node);
            }
            visits_.push_back(visit_t{target, candidature});

            if(on_device)
            {
                auto const before = graph.in_vertexes(target);
                session->try_parents(graph, target, candidature);
                for(auto const& parent : graph.in_vertexes(target))
                    if(std::find(before.begin(), before.end(), parent) == before.end()) preconditon[parent].push_back(target);
                continue;
            }
            for(auto const& parent : candidature)
            {
                if(auto edge = graph.add_edge(parent, target))
                {
                    sampling_.make_cpt(graph);
                    auto const eval_now = eval_(graph);
                    if(eval_now < eval_best)
                    {
                        eval_best = eval_now;
                        preconditon[parent].push_back(target);
                    }
                    else graph.erase_edge(edge);
                }
            }
        }

        if(!on_device) return eval_best;
        sampling_.make_cpt(graph);
        return session->score();
    }

    // NOT IN THE REFERENCE: the targets of the last run and the candidates each was offered, in order
    std::vector<visit_t> const& last_visits() const { return visits_; }

private:
    sampler const& sampling_;
    Eval const eval_;
    std::mt19937 engine_;
    std::vector<visit_t> visits_;
};

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_K2_ALGORITHM_HPP
