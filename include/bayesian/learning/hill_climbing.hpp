// bayesian/learning/hill_climbing.hpp -- NOT IN THE REFERENCE: bn::learning::hill_climbing<Eval>, tabu hill climbing over add,
// delete and reverse moves (the search of bnlearn's hc / tabu and pgmpy's HillClimbSearch), running on the MI355X through
// bn_learn_climb (include/bn_mi355x.h states the contract) when Eval is bn::evaluation::aic, mdl, basic_bdeu<> or k2_score.
// C++14, no Boost.
//
// Shaped like this repository's simulated_annealing.hpp: hill_climbing(sampler const&), hill_climbing(sampler const&, seed),
// operator()(graph, tabu_len = 0, max_worse = 0) returns the score of the learned graph and leaves the graph in `graph`.
//
// How it runs.  The family term of EVERY parent set of at most max_parents() nodes per child is computed once (bn_terms_create),
// and runs() independent climbs run resident on the device over that table: run 0 from the caller's graph, run j >= 1 from that
// graph after perturb() random proposals of the library's stream (seed, j).  A step applies the legal, non-tabu move with the
// smallest delta (ties: the lowest move id); a move on a node pair is tabu for tabu_len applied steps; a run ends when nothing
// improves and max_worse steps in a row brought no new best, and returns the best graph it saw.  The best graph of the run with
// the strictly smallest score (the lowest run among equals) replaces the caller's edges; one sampling_.make_cpt(graph) at the end.
// tabu_len = 0, max_worse = 0 is the classic greedy climb.
//
// There is no host twin: an Eval other than those four, or an empty sampler, throws std::invalid_argument.
#ifndef BNI_LEARNING_HILL_CLIMBING_HPP
#define BNI_LEARNING_HILL_CLIMBING_HPP

#include <cstdint>
#include <random>
#include <stdexcept>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/learning/greedy.hpp>

namespace bn {
namespace learning {

template<class Eval>
class hill_climbing {
public:
    hill_climbing(bn::sampler const& sampling)
        : sampling_(sampling), seed_(std::random_device()())
    {
    }

    // a reproducible run
    hill_climbing(bn::sampler const& sampling, std::uint64_t seed)
        : sampling_(sampling), seed_(seed)
    {
    }

    // the number of runs (1 .. 65536), the in-degree bound (1 .. 16), the seed, the random proposals a restart makes first
    // (at most 2^16) and the cap on applied steps (0: 2^16; at most 2^20)
    void set_runs(int runs) { runs_ = runs; }
    void set_max_parents(int max_parents) { max_parents_ = max_parents; }
    void set_seed(std::uint64_t seed) { seed_ = seed; }
    void set_perturb(std::uint32_t perturb) { perturb_ = perturb; }
    void set_max_steps(std::uint32_t max_steps) { max_steps_ = max_steps; }
    int runs() const { return runs_; }
    int max_parents() const { return max_parents_; }
    std::uint32_t perturb() const { return perturb_; }
    // the winning run of the last call
    int last_winner() const { return last_winner_; }

    double operator()(graph_t& graph, int const tabu_len = 0, unsigned int const max_worse = 0)
    {
        if(detail::criterion_of<Eval>::value < 0) throw std::invalid_argument("hill_climbing: Eval must be aic, mdl, basic_bdeu<> or k2_score");
        if(sampling_.sampling_size() == 0) throw std::invalid_argument("hill_climbing: the sampler holds no samples");
        if(max_parents_ < 1 || max_parents_ > 16) throw std::invalid_argument("hill_climbing: max_parents must be in 1..16");
        if(tabu_len < 0 || tabu_len > 64) throw std::invalid_argument("hill_climbing: tabu_len must be in 0..64");
        detail::learner_session session(sampling_, graph, detail::criterion_of<Eval>::value, detail::criterion_of<Eval>::spec());
        bn_climb_params const params{max_parents_, tabu_len, max_worse, max_steps_, perturb_, -1, 0, 0};
        last_winner_ = session.climb(graph, params, runs_, seed_);
        sampling_.make_cpt(graph);
        return session.score();
    }

private:
    sampler const& sampling_;
    std::uint64_t seed_;
    int runs_ = 1, max_parents_ = 3;
    std::uint32_t perturb_ = 0, max_steps_ = 0;
    int last_winner_ = -1;
};

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_HILL_CLIMBING_HPP
