// bayesian/inference/gibbs_sampling.hpp -- Gibbs sampling on the MI355X.  The reference has no such functor; this one has the shape
// of its likelihood_weighting (reference likelihood_weighting.hpp:13-59), with the chain and sweep counts as arguments:
//
//     bn::inference::gibbs_sampling gs(graph);
//     auto marginals = gs(evidence, chains, sweeps, burn_in, thin);   // 4096 chains, 200 sweeps, 100 of them burn-in, thin 1
//
// The chains run in the HIP kernel behind bn_gibbs_run (include/bn_mi355x.h states what one update does and where its random
// number comes from).  Hard evidence is clamped; the chains move inside it, so the marginals converge where the evidence is
// unlikely and likelihood weighting's weights vanish.  The seed is drawn from std::random_device once, as likelihood_weighting
// draws its own; chains are numbered consecutively -- successive calls run fresh chains.
#ifndef BNI_INFERENCE_GIBBS_SAMPLING_HPP
#define BNI_INFERENCE_GIBBS_SAMPLING_HPP

#include <cstdint>
#include <random>
#include <stdexcept>
#include <unordered_map>
#include <vector>

#include "mi355x_flatten.hpp"
#include "mi355x_marginals.hpp"

namespace bn {
namespace inference {

class gibbs_sampling {
public:
    typedef std::unordered_map<vertex_type, int> evidence_list;
    typedef std::unordered_map<vertex_type, matrix_type> return_type;

    explicit gibbs_sampling(graph_t const& graph)
        : graph_(graph), model_(mi355x::flatten(graph)), engine_(model_)
    {
        std::random_device rand_dev;
        seed_ = (static_cast<std::uint64_t>(rand_dev()) << 32) ^ rand_dev();
    }

    virtual ~gibbs_sampling() = default;

    // The functor flattened the tables once, in its constructor: reload() brings the device images up to date after an edit
    // (same structure required) -- through the functor's own copy of the graph, whose vertices are the caller's.
    void reload() { mi355x::reload_cpts(graph_, model_, engine_); }
    void reload(graph_t const& graph) { mi355x::reload_cpts(graph, model_, engine_); graph_ = graph; }

    // deterministic runs (tests)
    void seed(std::uint64_t s) { seed_ = s; next_chain_ = 0; }
    // of the last call: updates that kept their state because every state had weight 0; kept sweeps x chains
    std::uint64_t last_stuck() const { return last_stuck_; }
    std::uint64_t last_kept() const { return last_kept_; }

    return_type operator()(evidence_list const& evidence, std::uint64_t const chains = 4096, std::uint64_t const sweeps = 200,
                           std::uint64_t const burn_in = 100, std::uint64_t const thin = 1)
    {
        return run(evidence, chains, sweeps, burn_in, thin).to_map();
    }

    // The same call with the marginals read in place (mi355x_marginals.hpp); valid until the next call on this functor.
    typedef mi355x::marginals_view view_type;
    view_type run(evidence_list const& evidence, std::uint64_t const chains = 4096, std::uint64_t const sweeps = 200,
                  std::uint64_t const burn_in = 100, std::uint64_t const thin = 1)
    {
        std::vector<std::int32_t> ev_node, ev_state;
        for(auto const& e : evidence)
        {
            auto const it = model_.index.find(e.first);
            if(it == model_.index.end()) throw std::runtime_error("gibbs_sampling: evidence on an unknown vertex");
            ev_node.push_back(it->second);
            ev_state.push_back(e.second);
        }
        std::size_t const hn = static_cast<std::size_t>(model_.node_off.back());
        counts_.assign(hn, 0);
        marginals_.resize(hn);
        mi355x::engine_handle::check(bn_gibbs_run(
            engine_.get(), static_cast<std::int32_t>(ev_node.size()), ev_node.data(), ev_state.data(), next_chain_, chains,
            0, sweeps, burn_in, thin, seed_, nullptr, counts_.data(), nullptr, &last_stuck_, &last_kept_));
        next_chain_ += chains;
        if(last_kept_ == 0) throw std::runtime_error("gibbs_sampling: no sweep was kept (burn_in is not below sweeps, or no chains)");
        for(std::size_t i = 0; i < hn; ++i)
            marginals_[i] = static_cast<double>(counts_[i]) / static_cast<double>(last_kept_);
        return view_type(model_, marginals_.data());
    }

private:
    graph_t graph_;   // as likelihood_weighting keeps one
    mi355x::flat_model model_;
    mi355x::engine_handle engine_;
    std::vector<std::uint64_t> counts_;
    std::vector<double> marginals_;   // what run()'s view reads
    std::uint64_t seed_ = 0;
    std::uint64_t next_chain_ = 0;
    std::uint64_t last_stuck_ = 0, last_kept_ = 0;
};

} // namespace inference
} // namespace bn

#endif // #ifndef BNI_INFERENCE_GIBBS_SAMPLING_HPP
