// bn_learn_anneal.hpp -- simulated annealing over a precomputed table of family terms (reference bayesian/learning/
// simulated_annealing.hpp).  Host-side view of the kernel in bn_learn_anneal.hip; the C ABI (bn_terms_*, bn_learn_anneal of
// include/bn_mi355x.h) is in bn_learn.cpp.
//
// The term table: per child c, ll(c, S) of every parent set S of at most q nodes other than c, at
//     rank(c, S) = offset[j] + sum over i = 1..j of C(s'_i, i),     S = {s_1 < ... < s_j},  s' = s - (s > c),
//     offset[j] = sum over t < j of C(n - 1, t);   T(n, q) = offset[q + 1] entries per child,  child c's row at c * T.
// A family over the per-family limit holds a quiet NaN: "not eligible".
#pragma once

#include <cstdint>

namespace bnmi {

constexpr int kAnnealMaxNodes = 64;          // a node has a lane
constexpr int kAnnealWaves = 4;              // chains per workgroup
constexpr int kAnnealMaxEdges = 1024;        // n * q <= 64 * 16
constexpr int64_t kAnnealMaxEntries = int64_t(1) << 22;   // n * T(n, q): 32 MiB of terms
constexpr int kAnnealMaxChains = 1 << 16;
constexpr uint32_t kAnnealMaxProposals = 1u << 24;
// the rank tables as the kernel reads them: offset[j], j <= 16, then C(a, i) at [kAnnealTabBinom + i * 64 + a], i <= 16, a < 64
// (an entry no rank of the table's (n, q) can ask for holds 0)
constexpr int kAnnealTabBinom = 17;
constexpr int kAnnealTabWords = kAnnealTabBinom + 17 * 64;

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

struct AnnealArgs {
    const double* terms;        // [n][T]
    const uint32_t* tab;        // [kAnnealTabWords]
    int64_t T;
    const int32_t* k;           // [n] arities
    const uint64_t* pmask0;     // [n] the starting graph: parent masks, row products, family terms
    const int64_t* rows0;
    const double* ll0;
    const uint16_t* edges0;     // [n_edges0] from | to << 8, child-major, parents increasing per child
    int32_t n_edges0;
    int32_t n, q, max_parents;  // q: the table's bound (the rank tables); max_parents <= q: what a chain refuses at
    int32_t criterion, rule;
    int64_t params0;
    double penalty, initial_temp, final_temp, rate, boltzmann;
    uint32_t same_state_max, max_proposals;
    uint32_t seed_lo, seed_hi;
    int32_t chains;
    int32_t trace_chain;        // -1: none
    uint32_t trace_cap;
    AnnealRecord* rec;          // [chains]
    uint64_t* masks;            // [chains][n] final parent masks
    double* ll;                 // [chains][n] final family terms
    uint16_t* edges;            // null, or [chains][edge_stride] the final ordered edge lists
    int32_t edge_stride;
    AnnealTrace* trace;         // null, or [trace_cap]
};

// returns a hipError_t value (0: success)
int learn_launch_anneal(const AnnealArgs& a, void* stream);

}  // namespace bnmi
