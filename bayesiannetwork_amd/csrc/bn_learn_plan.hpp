// bn_learn_plan.hpp -- what a batch of family scores does before it touches the device, as pure functions of the arities: the
// argument checks, the families, the LDS / device-memory chunks, the passes over the count scratch and the launch order of the
// families (plan_groups); the family table and the per-level steps of the subset lattice (plan_subsets).  No HIP: bn_learn_plan.cpp
// is also compiled alone by tests/cpp/test_learn_plan.cpp.  bn_learn_batch.cpp uploads a plan, runs its passes and scatters by `order`.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bn_learn.hpp"

namespace bn_eng __attribute__((visibility("hidden"))) {
int fail(int code, const std::string& msg);   // bn_last_error (bn_engine.cpp; the stand-alone test has its own)
}  // namespace bn_eng

#pragma GCC visibility push(hidden)   // (internal to the library: nothing here is part of its surface)
namespace bnmi {

// one group: the base family of `child` and one family per candidate (base + that candidate)
struct GroupIn {
    int32_t child;
    const int32_t* base;
    int32_t n_base;
    const int32_t* cand;
    int32_t n_cand;
};

// a run of whole chunks whose counter blocks share the scratch, and the run of families (launch order) counted there
struct LearnPass {
    int32_t chunk0, n_chunks;
    int32_t fam0, n_fams;
    int64_t cells;
};

struct GroupPlan {
    std::vector<LearnChunk> chunks;
    std::vector<LearnFamily> fams;      // in launch order: by pass, within a pass in input order
    std::vector<int32_t> order;         // fams[i] is family order[i] of the input (group-major, base first)
    std::vector<LearnPass> passes;
    std::vector<int32_t> par_id, par_k, cand_id, cand_k, cand_cell;   // LearnArgs' arrays
    std::vector<int32_t> cand_fam;      // input family of every chunk candidate (beside cand_id)
    std::vector<int32_t> base_fam;      // per chunk: the input family of the base it counts, or -1
    int64_t out_cells = 0;              // fitted-layout counts of every family, back to back in input order
    int64_t scratch_cells = 0;          // the largest pass
};

// k [n]: the arities.  max_scratch_cells: cells of the count scratch (the library passes kLearnMaxScratchCells); a chunk larger
// than that is a pass of its own.  BN_OK, or what bn_eng::fail returned; no families: an empty plan.
int plan_groups(const int32_t* k, int32_t n, const std::vector<GroupIn>& groups, int64_t max_scratch_cells, GroupPlan& out);

struct SubsetPlan {
    std::vector<int32_t> id, k, bit;    // the top family's variables in increasing id; bit: the candidate's index, -1 for a base parent
    int32_t kc = 1, nv = 0, n_fams = 1;
    int64_t top_cells = 0, all_cells = 0;
    bool lds = false;                   // the top family fits kLearnLdsCells: the one-launch lattice
    std::vector<LearnFamily> fams;      // [2^m] in mask order, back to back
    std::vector<LatticeStep> steps;     // the per-level form (not lds): level l = masks with l candidates absent
    std::vector<int32_t> level_at, level_max;   // steps [level_at[l], level_at[l + 1]); the largest family of the level
    std::vector<LearnChunk> chunks;     // the one chunk that counts the top family
};

int plan_subsets(const int32_t* k, int32_t n, int32_t child, int32_t n_base, const int32_t* base, int32_t m, const int32_t* cand,
                 int64_t max_scratch_cells, SubsetPlan& out);

}  // namespace bnmi
#pragma GCC visibility pop
