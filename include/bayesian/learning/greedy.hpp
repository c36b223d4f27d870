// bayesian/learning/greedy.hpp -- drop-in for the reference's bn::learning::greedy<Eval> (bayesian/learning/greedy.hpp), the
// search running on the MI355X through bn_learn_* (include/bn_mi355x.h) when Eval is bn::evaluation::aic, mdl, basic_bdeu<> or k2_score
// (evaluation/bdeu.hpp; under the last two the score is the likelihood alone and eval_(graph) has its bits).  C++14, no Boost.
//
// Same class, same members: greedy(sampler const&), operator()(graph), operator()(graph, vertexes),
// learn_with_hint(graph, parent_nodes, child_nodes); the shuffles are the reference's (std::shuffle with a std::mt19937).
//
// How it runs.  AIC and MDL are decomposable, so for Eval = aic / mdl (exactly those types) the candidates of a child are scored
// as families of that child in one pass over the device-resident table per ACCEPTED edge (bn_learn_try_parents), instead of one
// make_cpt and one evaluation of the whole graph per candidate.  The table is an information_table over graph.vertex_list(),
// marshalled at each call; accepted edges are applied to the caller's graph with add_edge; one sampling_.make_cpt(graph) at the end.
// Any other Eval (a subclass of aic included) runs the reference's literal loop: make_cpt + eval_ per candidate.
//
// Differences from the reference (aic / mdl path):
//   - the score is the learner's: the family terms take the device's fp64 logarithm (bn_mi355x.h states the function), so the
//     returned value agrees with eval_(graph) to a few ulp per term, not bit for bit;
//   - the graph ends with CPTs fitted to the FINAL structure (the reference leaves the CPTs of the last rejected candidate);
//   - a family is limited to 16 parents and 2^20 table entries: a candidate beyond them is not added;
//   - an empty sampler takes the literal loop (and behaves as there).
// Not in the reference (labelled so below): the constructor taking a seed, last_visits().
#ifndef BNI_LEARNING_GREEDY_HPP
#define BNI_LEARNING_GREEDY_HPP

#include <algorithm>
#include <cstdint>
#include <memory>
#include <random>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/evaluation/aic.hpp>
#include <bayesian/evaluation/bdeu.hpp>
#include <bayesian/evaluation/mdl.hpp>
#include <bayesian/evaluation/transinformation.hpp>

namespace bn {
namespace learning {

// NOT IN THE REFERENCE: a child and the candidates it was offered, in order (what a run visited; tests replay it)
struct visit_t {
    vertex_type child;
    std::vector<vertex_type> candidates;
};

namespace detail {

// 0 AIC, 1 MDL, 2 BDeu, 3 K2, -1: any other evaluation (the literal loop); spec(): the family term bn_learn_create_spec takes
struct loglik_spec {
    static bn_score_spec spec() { return bn_score_spec{0, 0, 0.0}; }
};
template<class Eval> struct criterion_of : std::integral_constant<int, -1>, loglik_spec {};
template<> struct criterion_of<evaluation::aic> : std::integral_constant<int, 0>, loglik_spec {};
template<> struct criterion_of<evaluation::mdl> : std::integral_constant<int, 1>, loglik_spec {};
template<class Ess> struct criterion_of<evaluation::basic_bdeu<Ess>> : std::integral_constant<int, 2> {
    static bn_score_spec spec() { return bn_score_spec{2, 0, evaluation::basic_bdeu<Ess>::ess()}; }
};
template<> struct criterion_of<evaluation::k2_score> : std::integral_constant<int, 3> {
    static bn_score_spec spec() { return bn_score_spec{3, 0, 0.0}; }
};

// (reference bayesian/utility.hpp: make_engine)
inline std::mt19937 make_engine()
{
    std::random_device rd;
    return std::mt19937(rd());
}

// a bn_learner over the graph's vertex_list(), starting from the graph's edges
class learner_session {
public:
    learner_session(sampler const& sampling, graph_t const& graph, int criterion, bn_score_spec const& spec = bn_score_spec{0, 0, 0.0},
                    int max_parents = 16)
        : nodes_(graph.vertex_list()), table_(sampling, nodes_), spec_(spec)
    {
        std::vector<std::int32_t> in_ptr(1, 0), in_idx;
        for(auto const& node : nodes_)
        {
            for(auto const& parent : graph.in_vertexes(node)) in_idx.push_back(index_of(parent));
            in_ptr.push_back(static_cast<std::int32_t>(in_idx.size()));
        }
        mi355x::engine_handle::check(bn_learn_create_spec(table_.handle(), in_ptr.data(), in_idx.data(), criterion, &spec_, max_parents, &learner_));
    }
    ~learner_session() { bn_learn_destroy(learner_); }
    learner_session(learner_session const&) = delete;
    learner_session& operator=(learner_session const&) = delete;

    // the reference's inner loop for one child; accepted edges are added to `graph`
    void try_parents(graph_t& graph, vertex_type const& child, std::vector<vertex_type> const& candidates)
    {
        std::vector<std::int32_t> cand;
        for(auto const& c : candidates) cand.push_back(index_of(c));
        std::vector<std::uint8_t> accepted(cand.size() + 1, 0);
        mi355x::engine_handle::check(bn_learn_try_parents(learner_, index_of(child), static_cast<std::int32_t>(cand.size()), cand.data(),
                                                          accepted.data()));
        for(std::size_t i = 0; i < cand.size(); ++i)
            if(accepted[i] && !graph.add_edge(candidates[i], child))
                throw std::logic_error("bn::learning: the graph refused an edge the learner accepted");
    }

    // brute_force::operator()(graph, vertexes) on the learner; the best graph's new edges are added to `graph`.  Returns the
    // reference's evaluated quantity (the likelihood over `vertexes`, the penalty of the whole graph).
    double brute_force(graph_t& graph, std::vector<vertex_type> const& vertexes)
    {
        auto const vs = indexes_of(vertexes);
        double eval = 0.0;
        mi355x::engine_handle::check(bn_learn_brute_force(learner_, static_cast<std::int32_t>(vs.size()), vs.data(), &eval));
        apply_structure(graph);
        return eval;
    }

    // brute_force::learn_with_hint on the learner; returns the score
    double brute_force_hint(graph_t& graph, std::vector<vertex_type> const& parent_nodes, std::vector<vertex_type> const& child_nodes)
    {
        auto const ps = indexes_of(parent_nodes), cs = indexes_of(child_nodes);
        mi355x::engine_handle::check(bn_learn_brute_force_hint(learner_, static_cast<std::int32_t>(ps.size()), ps.data(),
                                                               static_cast<std::int32_t>(cs.size()), cs.data()));
        apply_structure(graph);
        return score();
    }

    double score() const
    {
        double s = 0.0;
        mi355x::engine_handle::check(bn_learn_score(learner_, &s));
        return s;
    }

    // simulated_annealing.hpp: the chains run on the learner over a term table of this session's table; the winner's graph
    // REPLACES the edges of `graph` (annealing also erases and reverses edges).  Returns the winning chain.
    std::int32_t anneal(graph_t& graph, std::int32_t max_parents, bn_anneal_params const& params, std::int32_t chains, std::uint64_t seed)
    {
        bn_term_table* terms = nullptr;
        mi355x::engine_handle::check(bn_terms_create_spec(table_.handle(), &spec_, max_parents, &terms));
        std::int32_t winner = 0;
        int const rc = bn_learn_anneal(learner_, terms, &params, chains, seed, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &winner);
        bn_terms_destroy(terms);
        mi355x::engine_handle::check(rc);
        graph.erase_all_edge();
        apply_structure(graph);
        return winner;
    }

    // stepwise_structure_hc.hpp: the runs start from the empty graph over a term table of this session's table and the table's
    // all-pairs mutual information; the winner's graph REPLACES the edges of `graph`.  Returns the winning run.
    std::int32_t hc(graph_t& graph, std::int32_t max_parents, double alpha, std::int32_t runs, std::uint64_t seed)
    {
        bn_term_table* terms = nullptr;
        mi355x::engine_handle::check(bn_terms_create_spec(table_.handle(), &spec_, max_parents, &terms));
        bn_hc_params const params{alpha, max_parents, -1, 0, 0};
        std::int32_t winner = 0;
        int const rc = bn_learn_hc(learner_, terms, &params, runs, seed, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &winner);
        bn_terms_destroy(terms);
        mi355x::engine_handle::check(rc);
        graph.erase_all_edge();
        apply_structure(graph);
        return winner;
    }

    // hill_climbing.hpp: the runs climb on the learner over a term table of this session's table, run 0 from the learner's
    // graph; the winner's best graph REPLACES the edges of `graph`.  Returns the winning run.
    std::int32_t climb(graph_t& graph, bn_climb_params const& params, std::int32_t runs, std::uint64_t seed)
    {
        bn_term_table* terms = nullptr;
        mi355x::engine_handle::check(bn_terms_create_spec(table_.handle(), &spec_, params.max_parents, &terms));
        std::int32_t winner = 0;
        int const rc = bn_learn_climb(learner_, terms, &params, runs, seed, nullptr, nullptr, nullptr, nullptr, &winner);
        bn_terms_destroy(terms);
        mi355x::engine_handle::check(rc);
        graph.erase_all_edge();
        apply_structure(graph);
        return winner;
    }

    // optimal_structure.hpp: the exact search on the learner over a term table of this session's table; the optimal graph REPLACES
    // the edges of `graph` (the learner's own graph is not read).  allowed: empty, or one mask per node in vertex_list() order.
    // Returns R[V], the cost of the graph as the search added it up.
    double optimal(graph_t& graph, std::int32_t max_parents, std::vector<std::uint64_t> const& allowed)
    {
        bn_term_table* terms = nullptr;
        mi355x::engine_handle::check(bn_terms_create_spec(table_.handle(), &spec_, max_parents, &terms));
        bn_optimal_params const params{max_parents, 0, allowed.empty() ? nullptr : allowed.data(), 0};
        double value = 0.0;
        int const rc = bn_learn_optimal(learner_, terms, &params, &value, nullptr, nullptr);
        bn_terms_destroy(terms);
        mi355x::engine_handle::check(rc);
        graph.erase_all_edge();
        apply_structure(graph);
        return value;
    }

private:
    std::vector<std::int32_t> indexes_of(std::vector<vertex_type> const& vs) const
    {
        std::vector<std::int32_t> out;
        for(auto const& v : vs) out.push_back(index_of(v));
        return out;
    }

    // every edge of the learner's graph that `graph` lacks is added (the searches only add edges; a subset of a DAG's edges
    // closes no cycle, so the order does not matter)
    void apply_structure(graph_t& graph)
    {
        std::int64_t edges = 0;
        mi355x::engine_handle::check(bn_learn_get(learner_, "edges", &edges));
        std::vector<std::int32_t> in_ptr(nodes_.size() + 1, 0), in_idx(static_cast<std::size_t>(edges) + 1, 0);
        mi355x::engine_handle::check(bn_learn_structure(learner_, in_ptr.data(), in_idx.data()));
        for(std::size_t v = 0; v < nodes_.size(); ++v)
        {
            auto const have = graph.in_vertexes(nodes_[v]);
            for(std::int32_t e = in_ptr[v]; e < in_ptr[v + 1]; ++e)
            {
                auto const& parent = nodes_[static_cast<std::size_t>(in_idx[static_cast<std::size_t>(e)])];
                if(std::find(have.begin(), have.end(), parent) != have.end()) continue;
                if(!graph.add_edge(parent, nodes_[v]))
                    throw std::logic_error("bn::learning: the graph refused an edge the learner added");
            }
        }
    }

    std::int32_t index_of(vertex_type const& v) const
    {
        auto const it = std::find(nodes_.begin(), nodes_.end(), v);
        if(it == nodes_.end()) throw std::out_of_range("bn::learning: vertex not in the graph");
        return static_cast<std::int32_t>(it - nodes_.begin());
    }

    std::vector<vertex_type> nodes_;
    evaluation::information_table table_;
    bn_score_spec spec_;
    bn_learner* learner_ = nullptr;
};

} // namespace detail

template<class Eval>
class greedy {
public:
    greedy(bn::sampler const& sampling)
        : sampling_(sampling), eval_(sampling_), engine_(detail::make_engine())
    {
    }

    // NOT IN THE REFERENCE: a reproducible run
    greedy(bn::sampler const& sampling, std::uint32_t seed)
        : sampling_(sampling), eval_(sampling_), engine_(seed)
    {
    }

    double operator()(graph_t& graph)
    {
        return (*this)(graph, graph.vertex_list());
    }

    double operator()(graph_t& graph, std::vector<vertex_type> vertexes)
    {
        draw_visits(std::move(vertexes));
        return run(graph);
    }

    // only edges from a node of parent_nodes to a node of child_nodes
    double learn_with_hint(graph_t& graph, std::vector<vertex_type> parent_nodes, std::vector<vertex_type> child_nodes)
    {
        draw_hint_visits(std::move(parent_nodes), std::move(child_nodes));
        return run(graph);
    }

    // NOT IN THE REFERENCE: the same two searches on a learner session that is already open (stepwise_structure.hpp runs every
    // step of a run on one); the CPTs are left to the caller.  Each returns the session's score.
    double learn_on(detail::learner_session& session, graph_t& graph, std::vector<vertex_type> vertexes)
    {
        draw_visits(std::move(vertexes));
        for(auto const& visit : visits_) session.try_parents(graph, visit.child, visit.candidates);
        return session.score();
    }

    double hint_on(detail::learner_session& session, graph_t& graph, std::vector<vertex_type> parent_nodes, std::vector<vertex_type> child_nodes)
    {
        draw_hint_visits(std::move(parent_nodes), std::move(child_nodes));
        for(auto const& visit : visits_) session.try_parents(graph, visit.child, visit.candidates);
        return session.score();
    }

    // NOT IN THE REFERENCE: the children of the last run and the candidates each was offered, in order
    std::vector<visit_t> const& last_visits() const { return visits_; }

private:
    void draw_visits(std::vector<vertex_type> vertexes)
    {
        std::shuffle(vertexes.begin(), vertexes.end(), engine_);
        visits_.clear();
        for(auto it = vertexes.begin(); it != vertexes.end();)
        {
            auto const child_iter = it;
            std::shuffle(++it, vertexes.end(), engine_);
            visits_.push_back(visit_t{*child_iter, std::vector<vertex_type>(it, vertexes.end())});
        }
    }

    void draw_hint_visits(std::vector<vertex_type> parent_nodes, std::vector<vertex_type> child_nodes)
    {
        std::shuffle(std::begin(child_nodes), std::end(child_nodes), engine_);
        visits_.clear();
        for(auto const& child : child_nodes)
        {
            std::shuffle(std::begin(parent_nodes), std::end(parent_nodes), engine_);
            visits_.push_back(visit_t{child, parent_nodes});
        }
    }

    // The shuffles draw from the engine only, never from the scores, so drawing them all first leaves every order as the
    // reference's interleaved loop has it.
    double run(graph_t& graph)
    {
        if(detail::criterion_of<Eval>::value >= 0 && sampling_.sampling_size() != 0)
        {
            detail::learner_session session(sampling_, graph, detail::criterion_of<Eval>::value, detail::criterion_of<Eval>::spec());
            for(auto const& visit : visits_) session.try_parents(graph, visit.child, visit.candidates);
            sampling_.make_cpt(graph);
            return session.score();
        }
        // the reference's loop (greedy.hpp:31-61, :73-100)
        sampling_.make_cpt(graph);
        double eval_now = eval_(graph);
        for(auto const& visit : visits_)
        {
            for(auto const& parent : visit.candidates)
            {
                if(auto edge = graph.add_edge(parent, visit.child))
                {
                    sampling_.make_cpt(graph);
                    auto const eval_next = eval_(graph);
                    if(eval_next < eval_now) eval_now = eval_next;
                    else graph.erase_edge(edge);
                }
            }
        }
        return eval_now;
    }

    sampler const& sampling_;
    Eval const eval_;
    std::mt19937 engine_;
    std::vector<visit_t> visits_;
};

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_GREEDY_HPP
