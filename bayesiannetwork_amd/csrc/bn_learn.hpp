// bn_learn.hpp -- scoring many candidate families of a child in one pass over a pattern table (the primitive under the reference's
// bayesian/learning/greedy.hpp and k2_algorithm.hpp: AIC / MDL are decomposable, so a candidate edge u -> c changes one family term).
// Host-side view of the kernels in bn_learn_kernels.hip and bn_learn_lattice.hip; the C ABI (bn_learn_* of include/bn_mi355x.h) is in bn_learn.cpp.
#pragma once

#include <cstdint>

namespace bnmi {

constexpr int kLearnBlock = 256;            // threads per workgroup of both kernels
constexpr int kLearnLanePatterns = 8;       // counting kernel: patterns per lane (one 8-byte load of a node's row, the row kernel's scheme)
constexpr int kLearnTile = kLearnBlock * kLearnLanePatterns;   // patterns per workgroup and iteration
// LDS budget of a counting workgroup: 4096 uint64 cells = 32 KiB, so five workgroups (20 waves) share a CU's 160 KiB -- the
// occupancy the 8-byte row loads want to hide their latency; it is also fit_count_kernel's boundary (kFitLdsEntries).
constexpr int kLearnLdsCells = 4096;
constexpr int kLearnMaxLdsCand = 32;        // candidates per chunk counted in LDS (their tables share the 4096 cells)
constexpr int kLearnMaxGlobalCand = 8;      // candidates per chunk counted in device memory
constexpr int kLearnMaxParents = 16;        // per family (the library's input domain)
constexpr int64_t kLearnMaxEntries = int64_t(1) << 20;        // per family table (32-bit cell index)
constexpr int64_t kLearnMaxScratchCells = int64_t(1) << 25;   // count scratch per pass: 256 MiB; a larger batch runs in several passes
constexpr int kLearnLanes = 256;            // family sums: bn_score_nodes' partial sums, folded by halves

// One chunk = the base parents of a group with a run of its candidates: what one column of counting workgroups counts.
// Cells of a candidate family are candidate-LAST: ((row over the base parents) * k_u + s_u) * k_c + s_c.
struct LearnChunk {
    int64_t count_at;     // first cell of the chunk's counter block in N
    int32_t child, kc;
    int32_t base_at, n_base;    // the group's base parents: par_id / par_k [base_at, base_at + n_base)
    int32_t cand_at, n_cand;    // the chunk's candidates: cand_id / cand_k / cand_cell [cand_at, cand_at + n_cand)
    int32_t base_cell;    // where the base family's cells start inside the block; -1: another chunk of the group counts it
    int32_t cells;        // cells of the block
    int32_t in_lds;       // the block is counted in LDS (cells <= kLearnLdsCells)
    int32_t pad_;
};

// One family as the scoring kernel reads it.  Entry r of the fitted layout (parents in increasing id, first most significant,
// state least): s = r % kc, row = r / kc, lo = row % low, t = row / low, su = t % ku, hi = t / ku; counted cell
// ((hi * low + lo) * ku + su) * kc + s.  The base family has ku = low = 1 (the identity).
struct LearnFamily {
    int64_t count_at;     // first counted cell in N
    int64_t out_at;       // first entry in the fitted-layout copy of the counts
    int32_t entries;      // rows * kc
    int32_t kc, ku, low;
};

struct LearnArgs {
    const uint8_t* T;                    // [n][Ppad] states
    const unsigned long long* w;         // [P] pattern weights
    int64_t P, Ppad;
    const LearnChunk* chunks;
    const int32_t* par_id;               // base parents of every group, and their arities
    const int32_t* par_k;
    const int32_t* cand_id;              // candidates of every chunk, their arities, and where their cells start in the chunk's block
    const int32_t* cand_k;
    const int32_t* cand_cell;
    unsigned long long* N;               // count scratch of the pass, zeroed by the host
    const LearnFamily* fams;
    double* ll;                          // [families]
    unsigned long long* counts_out;      // fitted-layout counts, or null
};

// each returns a hipError_t value (0: success).  chunk0 / fam0: first chunk / family of the pass; N is the pass's own scratch.
int learn_launch_count(const LearnArgs& a, int32_t chunk0, int32_t n_chunks, int splits, void* stream);
int learn_launch_score(const LearnArgs& a, int32_t fam0, int32_t n_fams, void* stream);
// the Bayesian-Dirichlet form (bn_learn_bd.hip): kind 2 BDeu with equivalent sample size ess, kind 3 K2 (ess not read)
int learn_launch_score_bd(const LearnArgs& a, int32_t fam0, int32_t n_fams, int32_t kind, double ess, void* stream);

// ---- the subset lattice (bn_learn_lattice.hip): the counts of base + every subset of the candidates, from the counts of the TOP
// family base + all candidates.  The top family's variables are held in increasing id (position 0 most significant); family `mask`
// (bit j: candidate j is a parent) keeps the positions whose variable is a base parent or a candidate with its bit set.  Every
// family is written in the fitted layout, so the scoring kernel reads it with ku = low = 1.

// The one-launch form (top family <= kLearnLdsCells cells): everything a workgroup needs to sum a family out of the top table.
struct LatticeLds {
    unsigned long long* N;        // the count scratch; the top family is at fams[n_fams - 1].count_at
    const LearnFamily* fams;      // [n_fams = 2^m] in mask order; count_at: where the family's counts go
    int32_t n_fams, nv, top_cells, pad_;
    int32_t k[kLearnMaxParents];      // arity of the variable at position p
    int32_t bit[kLearnMaxParents];    // candidate index of position p, or -1: a base parent
};

// The per-level form: family `out` = the family `in` with the variable of arity kx summed out, `inner` cells below it.
//   out[h * inner + l] = sum over s < kx of in[(h * kx + s) * inner + l],  h * inner + l < cells
struct LatticeStep {
    int64_t in_at, out_at;
    int32_t cells, inner, kx, pad_;
};

int learn_launch_lattice_lds(const LatticeLds& a, int blocks, void* stream);
int learn_launch_lattice_level(unsigned long long* N, const LatticeStep* steps, int32_t step0, int32_t n_steps, int32_t max_cells, void* stream);

}  // namespace bnmi
