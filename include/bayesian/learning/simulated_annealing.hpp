// bayesian/learning/simulated_annealing.hpp -- drop-in for the reference's bn::learning::simulated_annealing<Eval>
// (bayesian/learning/simulated_annealing.hpp), the search running on the MI355X through bn_learn_anneal (include/bn_mi355x.h)
// when Eval is bn::evaluation::aic or mdl.  C++14, no Boost.
//
// Same class, same members: simulated_annealing(sampler const&), operator()(graph, initial_temp, final_temp, decreasing_rate,
// boltzmann = 1.0, same_state_max = 100) with the reference's defaults (:21-27).
//
// How it runs.  For Eval = aic / mdl (exactly those types) the family term of EVERY parent set of at most max_parents() nodes per
// child is computed once (bn_terms_create), and chains() independent chains of the reference's loop run resident on the device
// over that table, each from the caller's graph; the graph of the chain with the strictly smallest final evaluation (the lowest
// index among equals) replaces the caller's edges; one sampling_.make_cpt(graph) at the end.  Any other Eval (a subclass of aic
// included) runs the reference's literal loop on the host -- make_cpt + eval_ per proposal -- as ONE chain, chain 0 of the same
// random stream, with the same in-degree bound: the twin the tests compare the device path with.
//
// Differences from the reference:
//   - the random numbers are the library's stream, not std::mt19937 + std::uniform_int (which libstdc++ does not provide: the
//     reference's header does not compile against it): chain j draws from xoshiro128++ seeded by Philox4x32-10 on (seed, j);
//     integer in [0, m): (uint64(r) * m) >> 32; real: (r + 0.5) * 2^-32 (bn_mi355x.h states the order of the draws);
//   - 64 chains by default, the best final graph returned (the reference runs one); set_chains(1) runs one;
//   - the in-degree is bounded (default 3, at most 16): add_edge is refused at the bound, a refused reversal still moves the edge
//     to the end of edge_list(); a family over 2^20 table entries is not eligible (device path);
//   - the loop also ends after max_proposals() iterations (default 2^20), so it ends for every input; decreasing_rate outside
//     (0, 1), a non-positive or non-finite temperature or boltzmann throw std::invalid_argument (the reference loops forever on
//     a rate >= 1);
//   - set_rule(1) replaces the reference's acceptance rule u < exp(-now / (boltzmann * T)) (:97: `now`, not `diff`, which almost
//     never climbs at realistic score magnitudes) by Metropolis' exp(-diff / (boltzmann * T)); 0, the reference's, is the default;
//   - aic / mdl path: the score is the learner's (the device's fp64 logarithm), and the graph ends with CPTs fitted to the FINAL
//     structure; an empty sampler takes the literal loop.
// Not in the reference (labelled so below): the constructor taking a seed, the setters, last_winner(), last_uphill().
#ifndef BNI_LEARNING_SIMULATED_ANNEALING_HPP
#define BNI_LEARNING_SIMULATED_ANNEALING_HPP

#include <cmath>
#include <cstdint>
#include <random>
#include <stdexcept>
#include <utility>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/learning/greedy.hpp>

namespace bn {
namespace learning {

namespace detail {

// the library's stream on the host (oracle/lw_oracle.c, stream_seed): chain j of a seed
class anneal_stream {
public:
    anneal_stream(std::uint64_t seed, std::uint64_t j)
    {
        std::uint32_t c0 = static_cast<std::uint32_t>(j), c1 = static_cast<std::uint32_t>(j >> 32), c2 = 0, c3 = 0;
        std::uint32_t k0 = static_cast<std::uint32_t>(seed), k1 = static_cast<std::uint32_t>(seed >> 32);
        for(int r = 0; r < 10; ++r)   // Philox4x32-10
        {
            std::uint64_t const p0 = std::uint64_t(0xD2511F53u) * c0, p1 = std::uint64_t(0xCD9E8D57u) * c2;
            std::uint32_t const n0 = static_cast<std::uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<std::uint32_t>(p0 >> 32) ^ c3 ^ k1;
            c0 = n0; c1 = static_cast<std::uint32_t>(p1); c2 = n2; c3 = static_cast<std::uint32_t>(p0);
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        x_[0] = c0; x_[1] = c1; x_[2] = c2; x_[3] = c3;
        if((c0 | c1 | c2 | c3) == 0) x_[0] = 1;
    }

    std::uint32_t next()   // xoshiro128++
    {
        std::uint32_t const result = rotl(x_[0] + x_[3], 7) + x_[0], t = x_[1] << 9;
        x_[2] ^= x_[0]; x_[3] ^= x_[1]; x_[1] ^= x_[2]; x_[0] ^= x_[3];
        x_[2] ^= t;
        x_[3] = rotl(x_[3], 11);
        return result;
    }
    std::size_t below(std::size_t m) { return static_cast<std::size_t>((std::uint64_t(next()) * m) >> 32); }
    double uniform() { return (static_cast<double>(next()) + 0.5) * (1.0 / 4294967296.0); }

private:
    static std::uint32_t rotl(std::uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
    std::uint32_t x_[4];
};

} // namespace detail

template<class Eval>
class simulated_annealing {
public:
    simulated_annealing(bn::sampler const& sampling)
        : sampling_(sampling), eval_(sampling_), seed_(std::random_device()())
    {
    }

    // NOT IN THE REFERENCE: a reproducible run
    simulated_annealing(bn::sampler const& sampling, std::uint64_t seed)
        : sampling_(sampling), eval_(sampling_), seed_(seed)
    {
    }

    // NOT IN THE REFERENCE: the number of chains (1 .. 65536), the in-degree bound (1 .. 16), the seed, the acceptance rule
    // (0: the reference's, 1: Metropolis) and the cap on loop iterations (at most 2^24)
    void set_chains(int chains) { chains_ = chains; }
    void set_max_parents(int max_parents) { max_parents_ = max_parents; }
    void set_seed(std::uint64_t seed) { seed_ = seed; }
    void set_rule(int rule) { rule_ = rule; }
    void set_max_proposals(std::uint32_t max_proposals) { max_proposals_ = max_proposals; }
    int chains() const { return chains_; }
    int max_parents() const { return max_parents_; }
    // NOT IN THE REFERENCE: the winning chain of the last device run; (u, p) of every uphill decision of the last literal run
    int last_winner() const { return last_winner_; }
    std::vector<std::pair<double, double>> const& last_uphill() const { return uphill_; }

    double operator()(
        graph_t& graph,
        double const initial_temp, double const final_temp,
        double const decreasing_rate,
        double const boltzmann = 1.0,
        unsigned int const same_state_max = 100
        )
    {
        if(!(std::isfinite(initial_temp) && initial_temp > 0 && std::isfinite(final_temp) && final_temp > 0))
            throw std::invalid_argument("simulated_annealing: the temperatures must be finite and positive");
        if(!(decreasing_rate > 0 && decreasing_rate < 1)) throw std::invalid_argument("simulated_annealing: decreasing_rate must be in (0, 1)");
        if(!(std::isfinite(boltzmann) && boltzmann > 0)) throw std::invalid_argument("simulated_annealing: boltzmann must be finite and positive");
        if(max_parents_ < 1 || max_parents_ > 16) throw std::invalid_argument("simulated_annealing: max_parents must be in 1..16");
        if(rule_ != 0 && rule_ != 1) throw std::invalid_argument("simulated_annealing: rule 0 or 1");
        if(detail::criterion_of<Eval>::value >= 0 && sampling_.sampling_size() != 0)
        {
            detail::learner_session session(sampling_, graph, detail::criterion_of<Eval>::value, detail::criterion_of<Eval>::spec());
            bn_anneal_params params{initial_temp, final_temp, decreasing_rate, boltzmann, same_state_max, max_proposals_, rule_, -1, 0, 0};
            last_winner_ = session.anneal(graph, max_parents_, params, chains_, seed_);
            sampling_.make_cpt(graph);
            return session.score();
        }
        return literal(graph, initial_temp, final_temp, decreasing_rate, boltzmann, same_state_max);
    }

private:
    // graph.add_edge with the in-degree bound
    edge_type add_edge_bounded(graph_t& graph, vertex_type const& from, vertex_type const& to) const
    {
        if(graph.in_vertexes(to).size() >= static_cast<std::size_t>(max_parents_)) return nullptr;
        return graph.add_edge(from, to);
    }

    // graph.change_edge_direction (graph.hpp:339-358) over add_edge_bounded
    edge_type change_edge_direction_bounded(graph_t& graph, edge_type const& e) const
    {
        auto const to = graph.target(e);
        auto const from = graph.source(e);
        if(!graph.erase_edge(e)) return nullptr;
        if(auto const new_edge = add_edge_bounded(graph, to, from)) return new_edge;
        graph.add_edge(from, to);
        return nullptr;
    }

    // the reference's loop (simulated_annealing.hpp:29-117), one chain: chain 0 of the stream
    double literal(graph_t& graph, double const initial_temp, double const final_temp, double const decreasing_rate, double const boltzmann,
                   unsigned int const same_state_max)
    {
        detail::anneal_stream engine(seed_, 0);
        uphill_.clear();
        sampling_.make_cpt(graph);
        graph_t best_graph = graph;
        double best_eval = eval_(graph);

        auto const vertexes = graph.vertex_list();
        auto const vertex_num = vertexes.size();

        unsigned int no_changed_num = 0;
        std::uint32_t proposals = 0;
        double temperature = initial_temp;
        while(temperature > final_temp && no_changed_num < same_state_max && proposals < (max_proposals_ ? max_proposals_ : (1u << 20)))
        {
            ++proposals;
            bool is_operated = false;
            auto const method = engine.below(3);
            if(method == 0)
            {
                auto const from = vertexes[engine.below(vertex_num)];
                auto const to   = vertexes[engine.below(vertex_num)];
                if(add_edge_bounded(graph, from, to)) is_operated = true;
            }
            else if(method == 1)
            {
                auto const edges = graph.edge_list();
                if(edges.size() < 1) continue;
                auto const target_edge = edges[engine.below(edges.size())];
                if(graph.erase_edge(target_edge)) is_operated = true;
            }
            else if(method == 2)
            {
                auto const edges = graph.edge_list();
                if(edges.size() < 1) continue;
                auto const target_edge = edges[engine.below(edges.size())];
                if(change_edge_direction_bounded(graph, target_edge)) is_operated = true;
            }

            if(!is_operated) continue;

            sampling_.make_cpt(graph);
            double const now_eval = eval_(graph);
            double const diff_eval = now_eval - best_eval;

            bool is_acceptance;
            if(diff_eval <= 0) is_acceptance = true;
            else
            {
                double const u = engine.uniform();
                double const scale = boltzmann * temperature;
                double const p = std::exp(-(rule_ == 0 ? now_eval : diff_eval) / scale);
                uphill_.emplace_back(u, p);
                is_acceptance = u < p;
            }

            if(is_acceptance)
            {
                best_graph = graph;
                best_eval = now_eval;
                no_changed_num = 0;
            }
            else
            {
                graph = best_graph;
                ++no_changed_num;
            }

            temperature *= decreasing_rate;
        }

        return best_eval;
    }

    sampler const& sampling_;
    Eval const eval_;
    std::uint64_t seed_;
    int chains_ = 64, max_parents_ = 3, rule_ = 0;
    std::uint32_t max_proposals_ = 1u << 20;
    int last_winner_ = -1;
    std::vector<std::pair<double, double>> uphill_;
};

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_SIMULATED_ANNEALING_HPP
