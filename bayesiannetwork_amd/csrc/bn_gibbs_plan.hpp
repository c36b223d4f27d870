// bn_gibbs_plan.hpp -- the plan of Gibbs sampling with coloured parallel chains (bn_gibbs.hip, bn_engine_gibbs.cpp; the contract of
// the arithmetic: bn_gibbs.hpp).  Pure host code: no HIP, no engine -- tests/cpp/test_gibbs_plan.cpp compiles bn_gibbs_plan.cpp alone.
//
// From the flat model (arities, parent lists, CPT offsets): the moral graph (a node's parents, its children and the other parents of
// its children); its greedy colouring -- nodes in ascending index, each takes the smallest colour no moral neighbour holds; the
// slots, one per node, in (colour, node) order: colour c owns slots [colour_ptr[c], colour_ptr[c + 1]).  Nodes of one colour share
// no family, so a sweep that updates a colour's nodes at once equals the sequential scan in slot order.  The colouring does not
// depend on the evidence: a clamped node keeps its slot and the kernel passes it by.
// A slot names everything one update reads, so the kernel searches nothing:
//   the node's own row      = sum of state[term.node] * term.stride over the slot's terms (its parents; first parent most significant)
//   per child c, ascending  = its table, its arity, the stride of the node inside c's row index, and c's OTHER parents as terms:
//                             row_c(x) = sum of the other parents' state * stride  +  x * child.stride
// Launch shape: a chain is a group of `lanes_per_chain` lanes of a wave -- the power of two from 8 to 64 that covers the largest
// colour class, so that a small network does not leave most of a wave idle -- and a workgroup of kGibbsThreads threads runs
// kGibbsThreads / lanes_per_chain chains (fewer, with wider groups, where their states would outgrow kGibbsLdsBudget).
// Limits of this first form (`ok` / `why`): n <= kGibbsMaxNodes and sum of arities <= kGibbsMaxCells -- a chain's states and the
// workgroup's histogram live in LDS.
#ifndef BN_GIBBS_PLAN_HPP
#define BN_GIBBS_PLAN_HPP
#include <cstdint>
#include <string>
#include <vector>

namespace bnmi {

constexpr int32_t kGibbsMaxNodes = 4096;        // state bytes of one chain in LDS
constexpr int32_t kGibbsMaxCells = 8192;        // sum of the arities: cells of the workgroup's histogram in LDS
constexpr int32_t kGibbsThreads = 256;          // a workgroup: four waves
constexpr int32_t kGibbsMinLanes = 8;           // lanes of a chain: 8, 16, 32 or 64 (a whole wave)
constexpr int32_t kGibbsLdsBudget = 48 * 1024;  // histogram + states of a workgroup
constexpr int32_t kGibbsMaxSweepsPerLaunch = 1 << 20;   // (x 32 chains stays far below the 2^32 of a histogram cell in LDS)
// the default of option "gibbs_sweeps_per_launch": as many sweeps as read about kGibbsLaunchReads table entries per chain, at most
// kGibbsDefaultSweeps -- a wave spends well under a microsecond per round of 64 reads, so a launch stays in the tens of milliseconds
constexpr int64_t kGibbsLaunchReads = int64_t(1) << 22;
constexpr int32_t kGibbsDefaultSweeps = 256;

struct GibbsTerm { int64_t stride; int32_t node, pad_; };
struct GibbsChild {
    int64_t cpt_off;                // the child's table in the flat CPT array
    int64_t stride;                 // of the slot's node inside the child's row index
    int32_t node, k;                // the child, its arity
    int32_t term_lo, term_n;        // terms[term_lo .. term_lo + term_n): the child's other parents
};
struct GibbsSlot {
    int64_t cpt_off;                // the node's table in the flat CPT array
    int32_t node, k;
    int32_t hist_off;               // first cell of the node in the histogram (node_off[node])
    int32_t term_lo, term_n;        // terms[term_lo .. term_lo + term_n): the node's parents
    int32_t child_lo, child_n;      // children[child_lo .. child_lo + child_n): ascending child index
    int32_t pad_;
};

struct GibbsPlan {
    bool ok = false;
    std::string why;
    int32_t n = 0, cells = 0, n_colours = 0, max_class = 0;
    int64_t reads_per_sweep = 0;    // table entries one chain reads per sweep with nothing clamped: sum of k[v] * (1 + children of v)
    std::vector<int32_t> colour;        // [n]
    std::vector<int32_t> colour_ptr;    // [n_colours + 1]
    std::vector<GibbsSlot> slots;       // [n] in (colour, node) order
    std::vector<GibbsChild> children;
    std::vector<GibbsTerm> terms;
    // launch shape
    int32_t threads = kGibbsThreads;
    int32_t lanes_per_chain = 64, chains_per_block = 4;   // chains_per_block = threads / lanes_per_chain
    int32_t state_stride = 0;           // bytes of one chain's states in LDS (n rounded up to 16)
    int32_t lds_bytes = 0;              // histogram (4 bytes a cell, rounded up to 16) + chains_per_block x state_stride
    int32_t default_sweeps = 1;         // per launch
};

void build_gibbs_plan(int32_t n, const int32_t* k, const int32_t* in_ptr, const int32_t* in_idx, const int64_t* cpt_off, GibbsPlan& out);

// One launch's share of a run: sweeps [begin, begin + count).
struct GibbsLaunch { uint64_t begin, count; };
// [sweep_begin, sweep_begin + n_sweeps) in launches of at most `cap` sweeps (cap < 1: 1), in order, each sweep exactly once:
// the launch that follows `done` < n_sweeps sweeps of the run (what the engine's loop asks), and the whole list
inline GibbsLaunch gibbs_launch_at(uint64_t sweep_begin, uint64_t n_sweeps, int64_t cap, uint64_t done) {
    const uint64_t per = cap < 1 ? 1 : uint64_t(cap), left = n_sweeps - done;
    return GibbsLaunch{sweep_begin + done, left < per ? left : per};
}
std::vector<GibbsLaunch> gibbs_launches(uint64_t sweep_begin, uint64_t n_sweeps, int64_t cap);
// sweeps g of [sweep_begin, sweep_begin + n_sweeps) with g >= burn_in and (g - burn_in) % thin == 0 (thin >= 1)
uint64_t gibbs_kept_sweeps(uint64_t sweep_begin, uint64_t n_sweeps, uint64_t burn_in, uint64_t thin);
inline int64_t gibbs_blocks(uint64_t n_chains, int32_t chains_per_block) {
    return int64_t((n_chains + uint64_t(chains_per_block) - 1) / uint64_t(chains_per_block));
}

}  // namespace bnmi

#endif  // BN_GIBBS_PLAN_HPP
