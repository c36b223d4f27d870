// bayesian/learning/stepwise_structure_hc.hpp -- drop-in for the reference's bn::learning::stepwise_structure_hc<Eval,
// BetweenLearning> and mutual_information_holder (bayesian/learning/stepwise_structure_hc.hpp), the search running on the MI355X
// through bn_learn_hc (include/bn_mi355x.h) when Eval is bn::evaluation::aic or mdl and BetweenLearning is greedy.  C++14, no Boost.
//
// Same classes, same members: stepwise_structure_hc(sampler const&), double operator()(graph_t&, double alpha);
// mutual_information_holder(sampler const&) with calculate_entropy, calculate_joint_entropy, calculate_similarity and the three
// delete_* members.
//
// How it runs.  Eval exactly aic / mdl and BetweenLearning = greedy: the family term of every parent set of at most max_parents()
// nodes per child is computed once (bn_terms_create), and runs() independent runs of the reference's loop run resident on the
// device over that table and the all-pairs mutual information; the graph of the run with the strictly smallest final score (the
// lowest among equals) replaces the caller's edges; one sampling_.make_cpt(graph) at the end.  Anything else runs the reference's
// literal loop on the host through learning_machine_.learn_with_hint as ONE run: the coin and the pruning draws are run 0's.
//
// Differences from the reference:
//   - the reference's header does not compile (it includes transinformation.hpp, which does not); this is its first working form;
//   - the reference orders clusters, and the two halves of a similarity, by shared_ptr address (:199, :257), which depends on the
//     allocator.  Here a cluster has an id: node i of vertex_list() starts in cluster i, the cluster made by merge number s is
//     n + s, and "smaller address" reads "smaller id";
//   - the coin and the pruning draws are the library's stream, not std::mt19937: run j draws from xoshiro128++ seeded by
//     Philox4x32-10 on (seed, j); integer in [0, m): (uint64(r) * m) >> 32; real: (r + 0.5) * 2^-32.  On the device path the
//     shuffles of learn_with_hint come from the same stream (bn_mi355x.h states the order); on the host path they are
//     BetweenLearning's own;
//   - 64 runs by default on the device path, the best final graph returned (the reference runs one); set_runs(1) runs one;
//   - device path: the in-degree is bounded (default 3), at most 64 nodes, a family over 2^20 table entries is not eligible; the
//     score is the learner's (the device's fp64 logarithm) and the graph ends with CPTs fitted to the FINAL structure;
//   - with nothing to merge (one node) the device path returns the score of the empty graph; the host path returns DBL_MAX as
//     the reference does;
//   - mutual_information_holder is backed by ONE all-pairs call over the variables it was prepared with (prepare(), or on first
//     use the variables of the sampler's first pattern) instead of per-pair entropies; the delete_* members forget nothing that
//     would have to be recomputed and are kept for source compatibility.
// Not in the reference (labelled so below): the constructor taking a seed, set_runs, set_max_parents, set_seed, last_winner(),
// mutual_information_holder::prepare.
#ifndef BNI_LEARNING_STEPWISE_STRUCTURE_HC_HPP
#define BNI_LEARNING_STEPWISE_STRUCTURE_HC_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>
#include <tuple>
#include <type_traits>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/evaluation/transinformation.hpp>
#include <bayesian/learning/greedy.hpp>
#include <bayesian/learning/simulated_annealing.hpp>

namespace bn {
namespace learning {

class mutual_information_holder {
public:
    mutual_information_holder(bn::sampler const& sampling)
        : sampling_(sampling)
    {
    }

    // NOT IN THE REFERENCE: the variables the one all-pairs call covers
    void prepare(std::vector<vertex_type> const& variables)
    {
        table_.reset(new evaluation::information_table(sampling_, variables));
        matrix_ = table_->pair_entropies();
    }

    double calculate_entropy(vertex_type const& node)
    {
        return matrix_.h[index_of(node)];
    }

    // lhs, rhs: in any order
    double calculate_joint_entropy(vertex_type const& lhs, vertex_type const& rhs)
    {
        auto const l = index_of(lhs), r = index_of(rhs);
        return matrix_.hxy[l * matrix_.m + r];
    }

    double calculate_similarity(vertex_type const& lhs, vertex_type const& rhs)
    {
        auto const l = index_of(lhs), r = index_of(rhs);
        return matrix_.mi[l * matrix_.m + r];
    }

    void delete_entropy(vertex_type const&) {}
    void delete_joint_entropy(vertex_type const&, vertex_type const&) {}
    void delete_similarity(vertex_type const&, vertex_type const&) {}

private:
    std::size_t index_of(vertex_type const& v)
    {
        if(!table_)
        {
            std::vector<vertex_type> variables;
            auto const table = sampling_.table();
            if(!table.empty())
                for(auto const& entry : table.begin()->first) variables.push_back(entry.first);
            prepare(variables);
        }
        auto const& vars = table_->variables();
        auto const it = std::find(vars.begin(), vars.end(), v);
        if(it == vars.end()) throw std::out_of_range("bn::learning::mutual_information_holder: variable not prepared");
        return static_cast<std::size_t>(it - vars.begin());
    }

    sampler const& sampling_;
    std::unique_ptr<evaluation::information_table> table_;
    evaluation::information_table::matrix matrix_;
};

template<class Eval, template<class> class BetweenLearning>
class stepwise_structure_hc {
public:
    using cluster_type = std::shared_ptr<std::vector<vertex_type>>;
    using similarity_type = std::tuple<cluster_type, cluster_type, double>;
    using Similarity = bn::evaluation::mutual_information;

    stepwise_structure_hc(bn::sampler const& sampling)
        : sampling_(sampling), eval_(sampling_), learning_machine_(sampling_), seed_(std::random_device()()), info_holder_(sampling_)
    {
    }

    // NOT IN THE REFERENCE: a reproducible run
    stepwise_structure_hc(bn::sampler const& sampling, std::uint64_t seed)
        : sampling_(sampling), eval_(sampling_), learning_machine_(sampling_), seed_(seed), info_holder_(sampling_)
    {
    }

    // NOT IN THE REFERENCE: the number of runs (1 .. 65536) and the in-degree bound (1 .. 16) of the device path, the seed, and the
    // winning run of the last device run
    void set_runs(int runs) { runs_ = runs; }
    void set_max_parents(int max_parents) { max_parents_ = max_parents; }
    void set_seed(std::uint64_t seed) { seed_ = seed; }
    int runs() const { return runs_; }
    int max_parents() const { return max_parents_; }
    int last_winner() const { return last_winner_; }

    // graph: whatever edges it holds are cleared; alpha: the pruning coefficient
    double operator()(graph_t& graph, double const alpha)
    {
        if(!(std::isfinite(alpha) && alpha >= 0)) throw std::invalid_argument("stepwise_structure_hc: alpha must be finite and >= 0");
        graph.erase_all_edge();
        if(resident && sampling_.sampling_size() != 0)
        {
            detail::learner_session session(sampling_, graph, detail::criterion_of<Eval>::value, detail::criterion_of<Eval>::spec());
            last_winner_ = session.hc(graph, max_parents_, alpha, runs_, seed_);
            sampling_.make_cpt(graph);
            return session.score();
        }
        info_holder_.prepare(graph.vertex_list());
        initial_clustering(graph.vertex_list());
        initial_similarities();
        return learning_between_clusters(graph, alpha);
    }

private:
    static constexpr bool resident =
        detail::criterion_of<Eval>::value >= 0 && std::is_same<BetweenLearning<Eval>, greedy<Eval>>::value;

    // a cluster's id stands for its address
    std::size_t id_of(cluster_type const& c) const
    {
        for(auto const& entry : ids_)
            if(entry.first == c) return entry.second;
        throw std::logic_error("stepwise_structure_hc: unknown cluster");
    }
    bool before(cluster_type const& lhs, cluster_type const& rhs) const { return id_of(lhs) < id_of(rhs); }

    void initial_clustering(std::vector<vertex_type> const& nodes)
    {
        clusters_.clear();
        ids_.clear();
        clusters_.reserve(nodes.size());
        for(auto const& node : nodes)
        {
            auto cluster = std::make_shared<cluster_type::element_type>();
            cluster->push_back(node);
            ids_.emplace_back(cluster, ids_.size());
            clusters_.push_back(std::move(cluster));
        }
    }

    void initial_similarities()
    {
        similarities_.clear();
        average_similar_ = 0.0;
        auto const max_edge_num = clusters_.size() * (clusters_.size() - 1) / 2;
        for(std::size_t i = 0; i < clusters_.size(); ++i)
            for(std::size_t j = i + 1; j < clusters_.size(); ++j)
            {
                auto similarity = make_similarity_tuple(clusters_[i], clusters_[j]);
                average_similar_ += std::get<2>(similarity) / static_cast<double>(max_edge_num);
                similarities_.push_back(std::move(similarity));
            }
    }

    bool is_related(similarity_type const& similarity, cluster_type const& cluster) const
    {
        return std::get<0>(similarity) == cluster || std::get<1>(similarity) == cluster;
    }

    bool is_connected(similarity_type const& similarity, cluster_type const& lhs, cluster_type const& rhs) const
    {
        return std::get<0>(similarity) == (before(lhs, rhs) ? lhs : rhs) && std::get<1>(similarity) == (before(lhs, rhs) ? rhs : lhs);
    }

    cluster_type combine_clusters(cluster_type const& lhs, cluster_type const& rhs)
    {
        auto new_cluster = std::make_shared<cluster_type::element_type>();
        new_cluster->reserve(lhs->size() + rhs->size());
        new_cluster->insert(new_cluster->end(), lhs->cbegin(), lhs->cend());
        new_cluster->insert(new_cluster->end(), rhs->cbegin(), rhs->cend());
        clusters_.erase(std::find(clusters_.begin(), clusters_.end(), lhs));
        clusters_.erase(std::find(clusters_.begin(), clusters_.end(), rhs));
        ids_.emplace_back(new_cluster, ids_.size());
        return new_cluster;
    }

    similarity_type most_similarity(detail::anneal_stream& engine)
    {
        auto const most_similar = std::max_element(
            similarities_.begin(), similarities_.end(),
            [](similarity_type const& lhs, similarity_type const& rhs){ return std::get<2>(lhs) < std::get<2>(rhs); }
            );
        auto result = *most_similar;
        similarities_.erase(most_similar);
        if(engine.below(2)) std::swap(std::get<0>(result), std::get<1>(result));
        return result;
    }

    similarity_type make_similarity_tuple(cluster_type const& lhs, cluster_type const& rhs)
    {
        auto const combination_num = lhs->size() * rhs->size();
        double value = 0;
        for(auto const& lhs_nodes : *lhs)
            for(auto const& rhs_nodes : *rhs)
                value += info_holder_.calculate_similarity(lhs_nodes, rhs_nodes) / static_cast<double>(combination_num);
        return before(lhs, rhs) ? std::make_tuple(lhs, rhs, value) : std::make_tuple(rhs, lhs, value);
    }

    double learning_between_clusters(graph_t& graph, double const alpha)
    {
        detail::anneal_stream engine(seed_, 0);
        double score = std::numeric_limits<double>::max();
        while(clusters_.size() != 1 && !similarities_.empty())
        {
            similarity_type const combine_target = most_similarity(engine);
            auto const parent = std::get<0>(combine_target);
            auto const child  = std::get<1>(combine_target);
            score = learning_machine_.learn_with_hint(graph, *parent, *child);
            clusters_.push_back(combine_clusters(parent, child));
            auto const inserted_cluster = clusters_.back();
            stochastic_pruning(alpha, inserted_cluster, combine_target, engine);
        }
        return score;
    }

    void stochastic_pruning(double const alpha, cluster_type const& new_cluster, similarity_type const& old_connection,
                            detail::anneal_stream& engine)
    {
        auto const clusters = clusters_;
        for(auto const& cluster : clusters)
        {
            if(cluster == new_cluster) continue;
            std::vector<similarity_type> connection;
            for(auto it = similarities_.begin(); it != similarities_.end(); )
            {
                if(is_connected(*it, cluster, std::get<0>(old_connection)) || is_connected(*it, cluster, std::get<1>(old_connection)))
                {
                    connection.push_back(*it);
                    it = similarities_.erase(it);
                }
                else ++it;
            }
            auto new_similarity = make_similarity_tuple(new_cluster, cluster);
            double probability;
            if(connection.size() == 2) probability = std::pow(alpha, std::get<2>(new_similarity) / average_similar_);
            else if(connection.size() == 1) probability = std::pow(alpha, std::get<2>(old_connection) / std::get<2>(connection[0]));
            else if(connection.size() == 0) continue;
            else throw std::runtime_error("too connection");
            if(engine.uniform() < probability) continue;
            similarities_.push_back(std::move(new_similarity));
        }
        for(auto it = similarities_.begin(); it != similarities_.end(); )
        {
            if(is_related(*it, std::get<0>(old_connection)) || is_related(*it, std::get<1>(old_connection))) it = similarities_.erase(it);
            else ++it;
        }
    }

    sampler const& sampling_;
    Eval const eval_;
    BetweenLearning<Eval> learning_machine_;
    std::uint64_t seed_;
    mutual_information_holder info_holder_;
    int runs_ = 64, max_parents_ = 3;
    int last_winner_ = -1;

    std::vector<cluster_type> clusters_;
    std::vector<std::pair<cluster_type, std::size_t>> ids_;
    std::vector<similarity_type> similarities_;
    double average_similar_ = 0.0;
};

template<class Eval, template<class> class BetweenLearning>
constexpr bool stepwise_structure_hc<Eval, BetweenLearning>::resident;

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_STEPWISE_STRUCTURE_HC_HPP
