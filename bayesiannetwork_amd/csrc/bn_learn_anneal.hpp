// bn_learn_anneal.hpp -- simulated annealing over a precomputed table of family terms (reference bayesian/learning/
// simulated_annealing.hpp).  Host-side view of the kernel in bn_learn_anneal.hip; the C ABI (bn_learn_anneal of include/bn_mi355x.h)
// is in bn_learn_search.cpp.  The term table and its rank tables are bn_learn_terms.hpp's; a chain is a run of the frame.
#pragma once

#include "bn_learn_search.hpp"

namespace bnmi {

constexpr int kAnnealWaves = 4;              // chains per workgroup
constexpr int kAnnealMaxEdges = 1024;        // n * q <= 64 * 16
constexpr uint32_t kAnnealMaxProposals = 1u << 24;

constexpr uint32_t kAnnealEndTemp = 1, kAnnealEndSame = 2, kAnnealEndCap = 4;

struct AnnealRecord {     // per chain
    double eval;          // the final evaluation
    uint32_t proposals, operated, accepted, flags;
    uint32_t n_edges, pad_;
};

struct AnnealTrace {      // per operated proposal of the traced chain
    uint64_t now_bits;    // the bits of the proposal's evaluation
    uint8_t method, from, to, accepted;   // from -> to: the edge drawn (method 2 turns it into to -> from)
    uint32_t pad_;
};

struct AnnealArgs : SearchArgs, StartGraph {
    const uint16_t* edges0;     // [n_edges0] from | to << 8, child-major, parents increasing per child
    int32_t n_edges0;
    int32_t rule;
    double initial_temp, final_temp, rate, boltzmann;
    uint32_t same_state_max, max_proposals;
    AnnealRecord* rec;          // [runs]
    uint16_t* edges;            // null, or [runs][edge_stride] the final ordered edge lists
    int32_t edge_stride;
    AnnealTrace* trace;         // null, or [trace_cap]
};

// returns a hipError_t value (0: success)
int learn_launch_anneal(const AnnealArgs& a, void* stream);

}  // namespace bnmi
