// bayesian/learning/stepwise_structure.hpp -- drop-in for the reference's bn::learning::stepwise_structure<Eval, InnerLearning,
// BetweenLearning> (bayesian/learning/stepwise_structure.hpp).  C++14, no Boost.
//
// Same class, same template parameters, same members: stepwise_structure(sampler const&), operator()(graph, initial_cluster_size).
// The run is the reference's: every edge erased; the shuffled vertexes dealt round-robin into
// ceil(n / initial_cluster_size) clusters (std::shuffle with a std::mt19937); InnerLearning<Eval> learns each cluster
// (operator()(graph, cluster)); then, until one cluster is left, a child cluster and a different parent cluster are drawn
// (std::uniform_int_distribution, the child first), BetweenLearning<Eval>::learn_with_hint(graph, parent, child) learns the edges
// between them, and the two are replaced by parent + child at the end of the list.  Returns the last learn_with_hint's value.
//
// How it runs.  For Eval = bn::evaluation::aic / mdl (exactly those types), when both learners have the hooks learn_on / hint_on
// (this repository's greedy.hpp and brute_force.hpp), the whole run uses ONE learner session: the sample table is marshalled and
// uploaded once, every step runs on the MI355X through bn_learn_* (include/bn_mi355x.h), and sampling_.make_cpt(graph) is called
// once at the end.  Otherwise the reference's calls are made one by one, each learner choosing its own path.
//
// Differences from the reference (one-session path): those of greedy.hpp / brute_force.hpp (the learner's score, CPTs fitted to the
// final structure, the limits of a family); the value returned after at least one merge is the session's whole-graph score.
// As in the reference, a run that starts with ONE cluster merges nothing and returns std::numeric_limits<double>::max().
// Not in the reference (labelled so below): the constructor taking a seed, last_clusters(), last_pairs(), last_between_visits().
#ifndef BNI_LEARNING_STEPWISE_STRUCTURE_HPP
#define BNI_LEARNING_STEPWISE_STRUCTURE_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <memory>
#include <random>
#include <type_traits>
#include <utility>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bayesian/learning/greedy.hpp>

namespace bn {
namespace learning {

namespace detail {

template<class...> struct voided { using type = void; };

// the learner can run on an open session: learn_on(session, graph, vertexes) and hint_on(session, graph, parents, children)
template<class Learner, class = void> struct has_session_hooks : std::false_type {};
template<class Learner>
struct has_session_hooks<Learner, typename voided<
    decltype(std::declval<Learner&>().learn_on(std::declval<learner_session&>(), std::declval<graph_t&>(), std::declval<std::vector<vertex_type>>())),
    decltype(std::declval<Learner&>().hint_on(std::declval<learner_session&>(), std::declval<graph_t&>(), std::declval<std::vector<vertex_type>>(),
                                              std::declval<std::vector<vertex_type>>()))>::type> : std::true_type {};

// the greedy's visits of a between-cluster step, where the learner records them (replaying a run needs its shuffles)
template<class Learner>
auto visits_of(Learner const& learner, int) -> decltype(learner.last_visits()) { return learner.last_visits(); }
template<class Learner>
std::vector<visit_t> visits_of(Learner const&, long) { return {}; }

} // namespace detail

template<class Eval, template<class> class InnerLearning, template<class> class BetweenLearning>
class stepwise_structure {
public:
    using cluster_type = std::vector<vertex_type>;

    stepwise_structure(bn::sampler const& sampling)
        : sampling_(sampling), eval_(sampling), engine_(detail::make_engine())
    {
    }

    // NOT IN THE REFERENCE: a reproducible run (the learners draw from generators seeded from this one)
    stepwise_structure(bn::sampler const& sampling, std::uint32_t seed)
        : sampling_(sampling), eval_(sampling), engine_(seed), seeded_(true)
    {
    }

    double operator()(graph_t& graph, std::size_t const& initial_cluster_size)
    {
        graph.erase_all_edge();
        auto clusters = deal(graph.vertex_list(), initial_cluster_size);
        clusters_ = clusters;
        pairs_.clear();
        between_visits_.clear();
        auto const inner_owner = make<InnerLearning<Eval>>();
        auto const between_owner = make<BetweenLearning<Eval>>();
        auto& inner = *inner_owner;
        auto& between = *between_owner;
        constexpr bool hooks = detail::has_session_hooks<InnerLearning<Eval>>::value && detail::has_session_hooks<BetweenLearning<Eval>>::value;
        if(hooks && detail::criterion_of<Eval>::value >= 0 && sampling_.sampling_size() != 0)
            return on_session(graph, clusters, inner, between, std::integral_constant<bool, hooks>());
        for(auto const& cluster : clusters) inner(graph, cluster);
        double score = std::numeric_limits<double>::max();
        while(clusters.size() != 1)
        {
            auto const pair = draw_pair(clusters.size());
            score = between.learn_with_hint(graph, clusters[pair.first], clusters[pair.second]);
            between_visits_.push_back(detail::visits_of(between, 0));
            merge(clusters, pair);
        }
        return score;
    }

    // NOT IN THE REFERENCE: what the last run did -- the initial clusters, the (parent index, child index) pairs merged, in order,
    // and per merge the visits of the between-cluster learner where it records them (greedy)
    std::vector<cluster_type> const& last_clusters() const { return clusters_; }
    std::vector<std::pair<std::size_t, std::size_t>> const& last_pairs() const { return pairs_; }
    std::vector<std::vector<visit_t>> const& last_between_visits() const { return between_visits_; }

private:
    // (the learners hold an evaluation and are neither copied nor moved)
    template<class Learner>
    auto make_seeded(int) -> decltype(new Learner(std::declval<bn::sampler const&>(), std::uint32_t()))
    {
        return new Learner(sampling_, static_cast<std::uint32_t>(engine_()));
    }
    template<class Learner>
    Learner* make_seeded(long) { return new Learner(sampling_); }
    template<class Learner>
    std::unique_ptr<Learner> make() { return std::unique_ptr<Learner>(seeded_ ? make_seeded<Learner>(0) : new Learner(sampling_)); }

    std::vector<cluster_type> deal(std::vector<vertex_type> nodes, std::size_t size)
    {
        std::size_t const count = nodes.size() / size + (nodes.size() % size ? 1 : 0);
        std::vector<cluster_type> clusters(count);
        std::shuffle(nodes.begin(), nodes.end(), engine_);
        for(std::size_t i = 0; i < nodes.size(); ++i) clusters[i % count].push_back(nodes[i]);
        return clusters;
    }

    // (parent index, child index): the child is drawn first, the parent until it differs
    std::pair<std::size_t, std::size_t> draw_pair(std::size_t count)
    {
        std::uniform_int_distribution<std::size_t> dist(0, count - 1);
        std::size_t const child = dist(engine_);
        std::size_t parent = dist(engine_);
        while(parent == child) parent = dist(engine_);
        pairs_.emplace_back(parent, child);
        return {parent, child};
    }

    static void merge(std::vector<cluster_type>& clusters, std::pair<std::size_t, std::size_t> const& pair)
    {
        cluster_type merged = clusters[pair.first];
        merged.insert(merged.end(), clusters[pair.second].begin(), clusters[pair.second].end());
        clusters.erase(clusters.begin() + static_cast<std::ptrdiff_t>(std::max(pair.first, pair.second)));
        clusters.erase(clusters.begin() + static_cast<std::ptrdiff_t>(std::min(pair.first, pair.second)));
        clusters.push_back(std::move(merged));
    }

    template<class Inner, class Between>
    double on_session(graph_t& graph, std::vector<cluster_type>& clusters, Inner& inner, Between& between, std::true_type)
    {
        detail::learner_session session(sampling_, graph, detail::criterion_of<Eval>::value, detail::criterion_of<Eval>::spec());
        for(auto const& cluster : clusters) inner.learn_on(session, graph, cluster);
        double score = std::numeric_limits<double>::max();
        while(clusters.size() != 1)
        {
            auto const pair = draw_pair(clusters.size());
            between.hint_on(session, graph, clusters[pair.first], clusters[pair.second]);
            score = session.score();
            between_visits_.push_back(detail::visits_of(between, 0));
            merge(clusters, pair);
        }
        sampling_.make_cpt(graph);
        return score;
    }
    template<class Inner, class Between>
    double on_session(graph_t&, std::vector<cluster_type>&, Inner&, Between&, std::false_type) { return 0.0; }   // (never called)

    sampler sampling_;
    Eval eval_;
    std::mt19937 engine_;
    bool seeded_ = false;
    std::vector<cluster_type> clusters_;
    std::vector<std::pair<std::size_t, std::size_t>> pairs_;
    std::vector<std::vector<visit_t>> between_visits_;
};

} // namespace learning
} // namespace bn

#endif // BNI_LEARNING_STEPWISE_STRUCTURE_HPP
