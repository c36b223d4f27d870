// bn_engine_policy.hpp -- which kernel runs a query: the shape of a resident launch and the choice between the one-launch paths, as
// pure functions of a few facts about the plans, the device's CU count and the options; the same for a batch of evidence sets, with
// the chunks its sets are launched in.  No HIP, no engine, no plan headers, no environment: tests/cpp/test_engine_policy.cpp and
// tests/cpp/test_batch_plan.cpp compile this with bn_engine_policy.cpp alone and check both sides of every threshold on a CPU.
// bn_engine_create.cpp fills the facts (path_facts_of) and mirrors the constants below with static_asserts.
#ifndef BN_ENGINE_POLICY_HPP
#define BN_ENGINE_POLICY_HPP
#include <cstdint>
#include <vector>

namespace bn_policy __attribute__((visibility("hidden"))) {   // (not part of the library's exported surface)

// (bn_device.hpp has the originals: kResidentWaves, kResidentMaxBlocks, kFlowMaxTiles, kMaxRanks, kResidentMaxSets; bn_dag.hpp: kDagMaxSets)
constexpr int kResidentWaves = 8;
constexpr int kResidentMaxBlocks = 256;
constexpr int kFlowMaxTiles = kResidentWaves * kResidentMaxBlocks;
constexpr int kMaxRanks = 16;
constexpr int kResidentMaxSets = 4;
constexpr int kDagMaxSets = 16;

// What the choice reads of an engine's plans (bn_plan.hpp Plan, bn_small.hpp SmallPlan / MidPlan, bn_dag.hpp DagPlan).
struct PathFacts {
    int32_t nranks = 1;
    bool latency_rules_applied = false;   // Plan: the layout trades wavefront count for the latency of one query
    int64_t n_tiles = 0;
    bool all_uniform = true;        // every tile is the uniform variant (and Plan::variants says so)
    int32_t tile_cmax = 0;          // maxima over the tiles of TileDesc::cmax and TileDesc::m
    int32_t tile_m = 0;
    bool any_in_ref = false;        // some tile has in_ref_base >= 0
    int32_t tile_kv = 0;            // the tiles' common kv, 0 if mixed (or no tile)
    bool any_cmax_gt2 = false;      // some tile has cmax > 2
    int64_t rec_total_doubles = 0;
    bool nbr_empty = true;          // Plan::nbr
    int32_t kmax = 0;               // largest arity of a node
    struct Small { bool ok = false; int32_t n = 0, re = 0, rb = 0, rc = 0, mmax = 0; } small;
    struct Mid { bool ok = false; int32_t parts = 0, mmax = 0; int64_t est_total = 0; } mid;   // mmax: over all parts
    struct Dag { bool ok = false, uniform4 = false, has_groups = false; double fill = 0.0; bool stream = false; int32_t blocks = 0; } dag;
};

// The launch shape of the resident kernel (bn_resident.hip) and what the network is eligible for on it.
struct ResidentShape {
    int waves = kResidentWaves;     // tiles per block of the resident kernel (8, or 4 on networks small enough)
    int blocks = 0;                 // tile blocks of a launch ("resident_blocks")
    bool resident_ok = false;       // every tile register-resident and co-resident: the whole run in one launch (bn_resident.hip)
    bool shard_shapes_ok = false;   // this shard's tiles are what the resident kernel runs (uniform arity, <= 2 parents, <= 8 children)
    int lean = 0;                   // ... and every node has this arity (2, 3 or 4) and <= 2 children; else 0
    bool flow_ok = false;           // dataflow form: more than one tile block, every tile has <= 64 neighbour tiles
};
// forced_waves: BN_RESIDENT_WAVES (0: not set); 8 is always honoured, 4 and 2 only where the blocks fit
ResidentShape plan_resident(const PathFacts& f, int n_cus, int forced_waves);

// the options "multisweep", "small", "mid", "dag" (0 never, 1 where measured faster, 2 wherever eligible)
struct PathModes { int multisweep = 1, small = 1, mid = 1, dag = 1; };
// what only the device side of an engine knows: the path's tables are uploaded and its kernel prepared (shard_flow: the peers are mapped)
struct PathOks { bool small = false, mid = false, dag = false, shard_flow = false; };

bool mid_fits(const PathFacts& f, int n_cus);   // the several-workgroup plan's parts within 0.9 x CUs (n_cus 0: unknown, fits)
int32_t dag_cap(int n_cus);                     // block cap of the DAG plan: 0.9 x CUs, a multiple of 8

bool resident_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m);
bool small_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m);
bool mid_applies(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m);
bool dag_applies(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m);
bool dag_first_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m);
bool dag_later_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m);

// ---- the first-sweep image of the resident path (option "memo0"; bn_device.hpp Memo0Args): sweep 0 of a run reads no message, so
// what it leaves is stored once per CPT image, patched per evidence set, and a run starts at sweep 1 ----
// Whether a run of the resident kernel starts from the image.
struct Memo0Run {
    bool enabled = false;       // option "memo0"
    bool image_valid = false;   // the image exists and holds the evidence in force
    bool flow = false;          // the launch is the dataflow form (shards included)
    int32_t max_sweeps = 0;     // 0: unbounded
    double eps = 0.0;
    double const_residual = 0.0;   // largest sweep-0 contribution among the nodes without evidence (memo0_const_residual)
};
// sweep 0 must be known not to end the run without looking at the evidence nodes: max_sweeps is 0 or >= 2, and eps is at most the
// constant part of its residual (the stop test is residual < eps), which must be finite and positive
bool memo0_applies(const Memo0Run& r);
// Membership of the new evidence set: stamp[v] == epoch.  Stamps the `ne` nodes of the set (a fresh epoch; the array is cleared when
// it has another size than n or the epoch would wrap).
void memo0_stamp(const int32_t* ev_node, int32_t ne, int32_t n, std::vector<uint32_t>& stamp, uint32_t& epoch);
// the nodes whose slots of the image go back to "no evidence": in the set applied before and not in the stamped one; order of `applied`
void memo0_restore_list(const std::vector<int32_t>& applied, const std::vector<uint32_t>& stamp, uint32_t epoch, std::vector<int32_t>& out);
// the constant part of sweep 0's residual: `order` lists the nodes by descending contribution cv[]; the first one outside the stamped
// set decides (usually the very first).  0.0 when every node carries evidence.
double memo0_const_residual(const std::vector<int32_t>& order, const std::vector<double>& cv, const std::vector<uint32_t>& stamp, uint32_t epoch);

// ---- the second-sweep image (option "memo1"; bn_device.hpp Memo1Args): what sweep 1 leaves at node v depends on the CPTs and on the
// evidence of v's closed neighbourhood N[v] alone, so it is stored once per CPT image, recomputed on N[E + R] per evidence set, and a
// run starts at sweep 2 ----
struct Memo1Run {
    Memo0Run level0;            // everything memo0_applies asks
    bool enabled = false;       // option "memo1"
    bool image_valid = false;   // the second-sweep image exists and holds the evidence in force
    double seed = 0.0;          // largest pristine sweep-1 contribution among the nodes outside N[E] (memo1_seed)
};
// memo0_applies, and sweep 1 must be known not to end the run without looking at the ring: max_sweeps is 0 or >= 3, and eps is at
// most the seed (the true sweep-1 residual is at least the seed), which must be finite and positive
bool memo1_applies(const Memo1Run& r);
// Node-level adjacency: adj[adj_off[v] .. adj_off[v + 1]) = v's parents, then its children.  From the parents' CSR of the model.
// Returns the largest degree.
int32_t memo1_adjacency(int32_t n, const std::vector<int32_t>& in_ptr, const std::vector<int32_t>& in_idx, std::vector<int32_t>& adj_off,
                        std::vector<int32_t>& adj);
// The seed: `order` lists the nodes by descending pristine contribution cv1[]; the first one with no stamped node in its closed
// neighbourhood decides (O(degree) per candidate, usually the very first).  0.0 when every node is inside the ring.
double memo1_seed(const std::vector<int32_t>& order, const std::vector<double>& cv1, const std::vector<int32_t>& adj_off,
                  const std::vector<int32_t>& adj, const std::vector<uint32_t>& stamp, uint32_t epoch);
// Whether a set patches the second-sweep image: (|E| + |R|) x (1 + max degree) threads' worth of work within the limit
bool memo1_patch_fits(int64_t ne, int64_t n_restore, int32_t max_degree, int64_t limit);
// What one evidence set does to the second-sweep image.  `applied` is the set that image holds (its OWN list: a set that does not
// patch leaves the list alone, and the next set that does restores what is still non-pristine).  patch == true: `list` = E then
// R (R = applied minus the stamped set), `applied` becomes E, the image holds the set in force.  Nothing to apply and nothing to
// restore: no launch, the image is the pristine one and holds the (empty) set.  Over the limit, or `wanted` off (a one-shot call that
// does not pay for the launch): no launch, `applied` and the image stay as they are, the image does not hold the set in force.
struct Memo1Plan {
    bool patch = false;   // launch the step kernel over `list`
    bool holds = false;   // after this set (and the launch, if any) the image holds the set in force
};
Memo1Plan memo1_plan_set(const int32_t* ev_node, int32_t ne, const std::vector<uint32_t>& stamp, uint32_t epoch, bool wanted, int32_t max_degree,
                         int64_t limit, std::vector<int32_t>& applied, std::vector<int32_t>& list);

// ---- a batch of evidence sets (bn_bp_run_batch_device): the same questions for the batch forms of the paths ----
// what only the device side knows of a batch: the per-set state of the one-workgroup path is allocated (Batch::d_s_state), a staging
// block holds the sets' evidence (Batch::ev_base)
struct BatchDevice { bool small_state = false, staged = false; };
bool batch_small_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m, const BatchDevice& d);
bool batch_dag_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m, const BatchDevice& d);
bool batch_mid_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m, const BatchDevice& d);
bool batch_resident_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m, const BatchDevice& d);

// the batch belongs on a second engine with the dense layout (bn_engine_batch.cpp, dense_engine_for_batch)
bool batch_wants_dense(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m, int32_t n_sets);
// ... unless that layout gives some node's sums another order.  One entry per node of a layout: the node's class (negative: not in
// this plan, skipped), the class's tile variant and lanes per node, the entries of its table.
struct NodeLayout { int32_t cls = -1, variant = 0, G = 0; int64_t entries = 0; };
bool dense_keeps_bits(const NodeLayout* own, int32_t n_own, const NodeLayout* dense, int32_t n_dense);

// how many sets share a launch
std::vector<int32_t> resident_batch_chunks(int32_t n_sets);              // balanced chunks of at most kResidentMaxSets, the larger first
int32_t mid_sets_per_launch(int n_cus, int32_t parts, int32_t n_sets);   // a workgroup per CU within 0.9 x CUs, at least one set
int32_t dag_sets_per_launch(int forced);                                 // forced: BN_DAG_SETS (0: not set) -> 1..kDagMaxSets

// ---- max-product (bn_mpe_run): which form of bn_maxprod.hip runs a network.  0 none, 1 one workgroup, 2 several workgroups.
// forced: option "mpe_form" (0: the rule, 1 / 2: that form or none)
int mpe_form(const PathFacts& f, int n_cus, int forced);

// ---- expectation-maximisation (bn_em_*, bn_em.hpp): how the pattern rows of an E-step are cut into launches, and where the sums of
// the 256-blocks of the E sum close.  A launch runs `chunk` rows, one workgroup each, and leaves chunk x entries family posteriors in a
// scratch array of at most scratch_cells doubles (option "em_scratch_cells"); chunk boundaries need not fall on block boundaries -- the
// accumulating kernel carries the block in hand across them -- so the result does not depend on the cut.
constexpr int32_t kEmBlock = 256;                 // (bn_em.hpp has the original)
constexpr int64_t kEmScratchCells = 1ll << 22;    // 32 MiB of doubles: 4 096 rows of an ALARM-sized network in one launch
constexpr int32_t kEmMaxChunk = 1 << 16;          // workgroups of one launch
struct EmPlan {
    int32_t chunk = 0;        // rows per launch (the last launch may have fewer)
    int64_t n_chunks = 0;
    int64_t n_blocks = 0;     // block sums added into E
    int64_t scratch = 0;      // doubles of the scratch array: chunk x entries
};
struct EmChunk {
    int64_t first = 0;        // global index of the chunk's first row
    int32_t count = 0;
    int32_t closes = 0;       // block sums that close inside the chunk (a block closes at its 256th row, the last one at the table's last row)
    bool opens_inside = false;   // the chunk's first row is not the first of a block: it continues the sum the chunk before left
};
// n_patterns >= 1, entries >= 1; scratch_cells < entries still gives one row per launch
EmPlan em_plan(int64_t n_patterns, int32_t entries, int64_t scratch_cells);
EmChunk em_chunk(const EmPlan& p, int64_t n_patterns, int64_t c);
// The M-step's view of the flat CPT array (bn_em.hpp EmMstepArgs): for every entry q, the CPT row it is normalised in -- the row's
// first entry and the node's arity.  From the plan's cpt_off [n + 1] and k [n] alone; cpt_off[n] < 2^31.
struct EmRow {
    int32_t first, k;
};
std::vector<EmRow> em_rows(int32_t n, const int64_t* cpt_off, const int32_t* k);

// ---- exact expectation-maximisation (bn_jt_em_*, bn_jt.hpp): the rows of one launch of the junction-tree E-step.  As em_plan under
// option "jt_em_scratch_cells" (the launch's family posteriors); in form 2 (jt_form: the per-row state in device scratch) also no
// more rows than state slices fit option "jt_scratch_cells", at least one.  em_chunk cuts the table as for em_plan: launch edges
// need not fall on block edges.
constexpr int64_t kJtEmScratchCells = kEmScratchCells;
EmPlan jt_em_plan(int64_t n_patterns, int32_t entries, int64_t b_scratch_cells, int form, int64_t state_cells, int64_t state_scratch_cells);

}  // namespace bn_policy

#endif  // BN_ENGINE_POLICY_HPP
