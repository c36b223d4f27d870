// bn_learn_climb.hpp -- tabu hill climbing over a precomputed table of family terms: steepest descent over add, delete and reverse
// moves with a tabu list and perturbed restarts.  Host-side view of the kernel in bn_learn_climb.hip; the C ABI (bn_learn_climb of
// include/bn_mi355x.h) is in bn_learn_search.cpp.  The term table and its rank tables are bn_learn_terms.hpp's.
#pragma once

#include "bn_learn_search.hpp"

namespace bnmi {

constexpr int kClimbWaves = 4;               // runs per workgroup: they share the rank tables in LDS and nothing else
constexpr int kClimbMaxTabu = 64;            // the ring has a lane per entry
constexpr uint32_t kClimbMaxSteps = 1u << 20;
constexpr uint32_t kClimbMaxPerturb = 1u << 16;

constexpr uint32_t kClimbEndNoMove = 1, kClimbEndOptimum = 2, kClimbEndCap = 4;

struct ClimbRecord {      // per run
    double best_eval;     // the learner's score of the best graph the run saw
    uint32_t steps, improving, perturbed, best_step, flags, tabu_legal;
};

struct ClimbTrace {       // per applied step of the traced run
    uint64_t d_bits;      // the bits of the move's delta
    uint64_t current_bits;   // the bits of the learner's score of the graph after the move
    uint8_t kind, from, to, pad8_;   // kind 0 adds from -> to, 1 deletes it, 2 turns it into to -> from
    uint32_t pad32_;
    uint64_t pad_;
};

struct ClimbArgs : SearchArgs, StartGraph {   // (masks, ll: of the best graph a run saw)
    int32_t tabu_len;
    uint32_t max_worse, max_steps, perturb;
    ClimbRecord* rec;           // [runs]
    ClimbTrace* trace;          // null, or [trace_cap]
};

// returns a hipError_t value (0: success)
int learn_launch_climb(const ClimbArgs& a, void* stream);

}  // namespace bnmi
