// bn_score.hpp -- log-likelihood of a pattern table under the engine's network (reference
// bayesian/evaluation/basic_info_criteria.hpp:44-78, calc_likelihood).  Host-side view of the kernels in
// bn_score_kernels.hip; the C ABI (bn_score_* of include/bn_mi355x.h) is in bn_score.cpp.
#pragma once

#include <cstdint>

namespace bnmi {

constexpr int kScoreSegShift = 8;          // row sums: nodes are added in segments of 256 consecutive ids
constexpr int kScoreLanePatterns = 8;      // row kernel: patterns per lane (4, 8 or 16: one load of that many bytes of a node's row)
constexpr int kScoreBlock = 256;           // threads per workgroup of both kernels
constexpr int kScoreTile = kScoreBlock * kScoreLanePatterns;   // patterns per workgroup of the row kernel
constexpr int kScoreNodeLanes = 256;       // node sums: partial sums (entry r goes to partial r % 256), then a binary tree
constexpr int64_t kScoreLoopTiles = 2048;  // from this many pattern tiles a workgroup walks the segments itself
constexpr int64_t kScoreMaxPartBytes = int64_t(1) << 30;   // ... or when the segment sums would need more scratch than this

// the row kernel's launch shape: true = one workgroup per pattern tile walks every segment (no scratch); false = a
// grid of tiles x segments and a second kernel that adds the segment sums.  The additions are the same.
inline bool score_rows_loop(int32_t n_segs, int64_t Ppad) {
    return n_segs <= 1 || (Ppad + kScoreTile - 1) / kScoreTile >= kScoreLoopTiles || int64_t(n_segs) * Ppad * 8 > kScoreMaxPartBytes;
}

// the model as the kernels read it (device pointers; wave-uniform, read through the scalar cache)
struct ScoreModel {
    int32_t n;
    const int32_t* k;         // [n]
    const int32_t* in_ptr;    // [n + 1]
    const int32_t* in_idx;    // [edges]
    const int64_t* cpt_off;   // [n + 1]
    const double* L;          // [entries] log of the flat CPT
};

struct ScoreRowsArgs {
    ScoreModel m;
    const uint8_t* T;         // [n][Ppad] states, zero beyond P
    int64_t P, Ppad;
    const uint32_t* sel;      // [ceil(n / 32)] bit v & 31 of word v >> 5: node v is selected
    const int32_t* segs;      // [n_segs] the segments holding a selected node, increasing
    int32_t n_segs;
    double* part;             // [n_segs][Ppad] segment sums (unused when one workgroup walks every segment)
    double* out;              // [Ppad]
};

// each returns a hipError_t value (0: success)
// wide: some node's table has 2^32 entries or more (64-bit mixed-radix index)
int score_launch_rows(const ScoreRowsArgs& a, bool wide, void* stream);
// ll_node[v] = sum over the node's entries with N != 0 of double(N[q]) * L[q], order of bn_mi355x.h
int score_launch_nodes(const ScoreModel& m, const unsigned long long* N, double* ll_node, void* stream);

}  // namespace bnmi
