// bn_engine_policy.cpp -- the shape of a resident launch and the choice between the one-launch paths, for one query and for a batch
// (bn_engine_policy.hpp).  Host arithmetic only; the thresholds below were measured on MI355X (the comments carry the figures).
#include "bn_engine_policy.hpp"

#include <algorithm>

namespace bn_policy {

namespace {
// blocks a launch of `w` waves per block needs (single engines round up to a multiple of 8 for the XCD-contiguous
// mapping; shards keep the CUs for each other)
int64_t resident_blocks(const PathFacts& f, int w) {
    int64_t b = (f.n_tiles + w - 1) / w;
    if (b > 1 && f.nranks == 1) b = (b + 7) & ~int64_t(7);
    return b;
}
// ... + the barrier's service block must fit 0.9 x CUs: decided on the ROUNDED count (a 239 x 240 grid
// has 898 tiles = 225 blocks of four, 232 after rounding: too many -- it keeps 8 waves per block)
bool resident_fits(const PathFacts& f, int n_cus, int w) {
    const int64_t b = resident_blocks(f, w);
    return b + 1 <= int64_t(n_cus) * 9 / 10 && b <= kResidentMaxBlocks;
}
}  // namespace

// resident path (bn_resident.hip): one-lane tiles (<= 2 parents, <= 8 children per node), one wave per tile, every block co-resident (one 512-thread block of <= 256 VGPRs per CU)
ResidentShape plan_resident(const PathFacts& f, int n_cus, int forced_waves) {
    ResidentShape r;
    const int64_t nt = f.n_tiles;
    // One 8-wave block per CU is two waves per SIMD sharing its issue slots.  A network whose tiles fit the chip at
    // FOUR waves per block (the CPT slots in LDS keep it at one block per CU) gives every wave a SIMD of its own.
    // BN_RESIDENT_WAVES=8 / 4 forces either (A/B).
    r.waves = kResidentWaves;
    if (nt > kResidentWaves && resident_fits(f, n_cus, kResidentWaves / 2)) r.waves = kResidentWaves / 2;
    const int v = forced_waves;
    if (v == kResidentWaves || (v == kResidentWaves / 2 && resident_fits(f, n_cus, v)) || (v == 2 && nt > 2 && resident_fits(f, n_cus, v))) r.waves = v;
    r.blocks = int(resident_blocks(f, r.waves));
    const bool shapes = f.all_uniform && resident_fits(f, n_cus, r.waves) &&
                        f.rec_total_doubles * 8 < (int64_t(1) << 31) &&  // 32-bit byte offsets into a record buffer
                        f.tile_cmax <= 8 && f.tile_m <= 2;
    r.resident_ok = shapes && f.nranks == 1 && nt > 0 && !f.any_in_ref;
    r.shard_shapes_ok = shapes && f.nranks > 1 && f.nranks <= kMaxRanks;
    r.lean = (r.resident_ok || r.shard_shapes_ok) && nt > 0 && !f.any_cmax_gt2 ? f.tile_kv : 0;
    r.flow_ok = r.resident_ok && r.blocks > 1 && !f.nbr_empty && nt <= kFlowMaxTiles;
    return r;
}

bool memo0_applies(const Memo0Run& r) {
    if (!r.enabled || !r.image_valid || r.flow) return false;
    if (r.max_sweeps == 1) return false;   // the run ends behind sweep 0: it has to be executed
    // (written so that a NaN on either side says no)
    return r.const_residual > 0.0 && r.const_residual <= 1.7976931348623157e308 && r.eps <= r.const_residual;
}

void memo0_stamp(const int32_t* ev_node, int32_t ne, int32_t n, std::vector<uint32_t>& stamp, uint32_t& epoch) {
    if (stamp.size() != size_t(n > 0 ? n : 0) || epoch == 0xffffffffu) { stamp.assign(size_t(n > 0 ? n : 0), 0u); epoch = 0; }
    ++epoch;
    for (int32_t j = 0; j < ne; ++j)
        if (ev_node[j] >= 0 && ev_node[j] < n) stamp[size_t(ev_node[j])] = epoch;
}

void memo0_restore_list(const std::vector<int32_t>& applied, const std::vector<uint32_t>& stamp, uint32_t epoch, std::vector<int32_t>& out) {
    out.clear();
    for (int32_t v : applied)
        if (v >= 0 && size_t(v) < stamp.size() && stamp[size_t(v)] != epoch) out.push_back(v);
}

double memo0_const_residual(const std::vector<int32_t>& order, const std::vector<double>& cv, const std::vector<uint32_t>& stamp, uint32_t epoch) {
    for (int32_t v : order)
        if (size_t(v) >= stamp.size() || stamp[size_t(v)] != epoch) return cv[size_t(v)];
    return 0.0;
}

bool memo1_applies(const Memo1Run& r) {
    if (!memo0_applies(r.level0) || !r.enabled || !r.image_valid) return false;
    if (r.level0.max_sweeps != 0 && r.level0.max_sweeps < 3) return false;   // the run ends behind sweep 0 or 1: they have to be executed
    // (written so that a NaN on either side says no)
    return r.seed > 0.0 && r.seed <= 1.7976931348623157e308 && r.level0.eps <= r.seed;
}

int32_t memo1_adjacency(int32_t n, const std::vector<int32_t>& in_ptr, const std::vector<int32_t>& in_idx, std::vector<int32_t>& adj_off,
                        std::vector<int32_t>& adj) {
    const size_t nn = size_t(n > 0 ? n : 0);
    adj_off.assign(nn + 1, 0);
    adj.clear();
    if (in_ptr.size() < nn + 1) return 0;
    std::vector<int32_t> deg(nn, 0);
    for (size_t v = 0; v < nn; ++v) {
        deg[v] += in_ptr[v + 1] - in_ptr[v];
        for (int32_t q = in_ptr[v]; q < in_ptr[v + 1]; ++q)
            if (in_idx[size_t(q)] >= 0 && size_t(in_idx[size_t(q)]) < nn) ++deg[size_t(in_idx[size_t(q)])];
    }
    int32_t dmax = 0;
    for (size_t v = 0; v < nn; ++v) {
        adj_off[v + 1] = adj_off[v] + deg[v];
        dmax = deg[v] > dmax ? deg[v] : dmax;
    }
    adj.assign(size_t(adj_off[nn]), -1);
    std::vector<int32_t> at(nn);
    for (size_t v = 0; v < nn; ++v) {   // parents first ...
        at[v] = adj_off[v];
        for (int32_t q = in_ptr[v]; q < in_ptr[v + 1]; ++q) adj[size_t(at[v]++)] = in_idx[size_t(q)];
    }
    for (size_t v = 0; v < nn; ++v)     // ... then children, ascending
        for (int32_t q = in_ptr[v]; q < in_ptr[v + 1]; ++q) {
            const int32_t u = in_idx[size_t(q)];
            if (u >= 0 && size_t(u) < nn) adj[size_t(at[size_t(u)]++)] = int32_t(v);
        }
    return dmax;
}

double memo1_seed(const std::vector<int32_t>& order, const std::vector<double>& cv1, const std::vector<int32_t>& adj_off,
                  const std::vector<int32_t>& adj, const std::vector<uint32_t>& stamp, uint32_t epoch) {
    auto stamped = [&](int32_t v) { return v >= 0 && size_t(v) < stamp.size() && stamp[size_t(v)] == epoch; };
    for (int32_t v : order) {
        if (v < 0 || size_t(v) + 1 >= adj_off.size()) continue;
        bool ring = stamped(v);
        for (int32_t q = adj_off[size_t(v)]; !ring && q < adj_off[size_t(v) + 1]; ++q) ring = stamped(adj[size_t(q)]);
        if (!ring) return cv1[size_t(v)];
    }
    return 0.0;
}

bool memo1_patch_fits(int64_t ne, int64_t n_restore, int32_t max_degree, int64_t limit) {
    return (ne + n_restore) * (1 + int64_t(max_degree)) <= limit;
}

Memo1Plan memo1_plan_set(const int32_t* ev_node, int32_t ne, const std::vector<uint32_t>& stamp, uint32_t epoch, bool wanted, int32_t max_degree,
                         int64_t limit, std::vector<int32_t>& applied, std::vector<int32_t>& list) {
    Memo1Plan r;
    list.clear();
    if (!wanted && (ne > 0 || !applied.empty())) return r;   // (something to apply or to restore, and no launch: nothing to work out)
    std::vector<int32_t> restore;
    memo0_restore_list(applied, stamp, epoch, restore);
    if (ne <= 0 && restore.empty()) {
        applied.clear();
        r.holds = true;
        return r;
    }
    if (!wanted || !memo1_patch_fits(ne, int64_t(restore.size()), max_degree, limit)) return r;
    if (ne > 0) list.assign(ev_node, ev_node + ne);
    list.insert(list.end(), restore.begin(), restore.end());
    if (ne > 0) applied.assign(ev_node, ev_node + ne);
    else applied.clear();
    r.patch = true;
    r.holds = true;
    return r;
}

bool mid_fits(const PathFacts& f, int n_cus) {
    // the workgroups of a run wait for each other: one per CU, with room to spare
    return !(n_cus > 0 && int64_t(f.mid.parts) > int64_t(n_cus) * 9 / 10);
}

int32_t dag_cap(int n_cus) { return int32_t((int64_t(n_cus) * 9 / 10) & ~int64_t(7)); }

// resident tiles pay on one block (no grid barrier at all) and on large networks (the CPT traffic saved outweighs the barrier); with 8
// waves per block the crossover was measured at ~600 tiles (160x160 grid, 402 tiles: 8.2 vs 8.9 us per sweep; 200x200, 627: 9.5 vs
// 9.2); at 4 waves per block (networks up to ~900 tiles: every wave has a SIMD of its own) it is faster than the launches from the
// smallest multi-block network on (32x32 grid 7.2 vs 7.4-7.8, 128x128 7.7 vs 8.0, 200x200 8.7 vs 9.5).  Shards: the in-kernel exchange
// wherever every rank's tiles qualify and the peers are mapped ("multisweep" 0 = per-sweep launches + one RCCL all-gather per sweep).
bool resident_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m) {
    constexpr int64_t kResidentMinTiles = 600;
    if (f.nranks > 1) return ok.shard_flow && m.multisweep != 0;
    const bool pays = r.blocks == 1 || r.waves < kResidentWaves || f.n_tiles >= kResidentMinTiles;
    return r.resident_ok && (m.multisweep == 2 || (m.multisweep == 1 && pays));
}

// The one-workgroup path is taken wherever the network fits, except where the resident-tile kernel runs the network in ONE block and
// was measured faster (scripts/experiments/small_vs_resident.py, us per sweep small / resident): chains and trees (one parent per
// node) beyond ~128 nodes or one round of entry items (200-node chain, k = 4: 5.2 / 2.8; 100 nodes: 2.9 / 2.6), and networks that
// need two rounds of accumulator or product items (16 x 16 grid, k = 2: 4.3 / 3.5).  With two parents per node the tile kernel's
// 64-entry contraction costs more than the items (8 x 8 grid, k = 4: 4.2 / 5.1; 40-node DAG: 2.6 / 6.4).
bool small_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m) {
    if (!ok.small || m.multisweep == 0 || m.small == 0) return false;
    if (m.small == 2) return true;
    return !(r.resident_ok && r.blocks == 1) ||
           (f.small.rb == 1 && f.small.rc == 1 && (f.small.mmax >= 2 || (f.small.re == 1 && f.small.n <= 128)));
}

// the mid-size kernel is the path of choice for this engine (measured: grids, chains and trees run faster on the resident tiles)
bool mid_applies(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m) {
    if (!ok.mid || m.multisweep == 0 || m.mid == 0) return false;
    if (m.mid == 2 || !r.resident_ok) return true;
    // Networks the resident tiles cover as well (scripts/experiments/mid_path.py, us per sweep resident / this path): with two
    // parents per node and four states the tile's 64-entry contraction costs more than the items (16 x 16 grid 5.9 / 4.3,
    // 32 x 32 7.0 / 6.4, 200-node DAG 6.7 / 4.3); chains, trees and smaller tables stay on the tiles (400-node chain 3.2 / 4.3,
    // 12 x 12 grid of k = 3: 3.7 / 4.3).
    // ... up to the size of the 40 x 40 grid (6.6 against 6.6-6.9); larger ones stay on the tiles (64 x 64: 6.4)
    // (mmax over all parts: the first one may hold a grid's first row only)
    return f.mid.mmax >= 2 && f.kmax >= 4 && f.mid.est_total <= 580000;
}

// k = 4 networks with up to 5 parents per node whose size puts them beyond the item kernels (BASELINE configs[1]): the
// register-resident DAG path (bn_dag.hip) where no other one-launch path takes the network; "dag" 2 = wherever eligible
bool dag_applies(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m) {
    if (!ok.dag || m.multisweep == 0 || m.dag == 0) return false;
    if (m.dag == 2) return true;
    // Networks the one-workgroup path (state in LDS) takes as well, us per query (profiles/r05_paths.json), that path / this one: one
    // round of entry items (ALARM-sized) 48.6 / 68.7, Pearl's four nodes 19.3 / 24.5 -- but 8 x 8 grid, k = 4 (four rounds) 86.0 / 64.4,
    // 60 nodes of mixed arity with <= 3 parents (three rounds) 72.3 / 64.6.  Chains and trees the resident tiles run in ONE block
    // stay there (200-node chain: 71.9 resident, 81.6 this path, 113.6 one workgroup).
    if (ok.small && f.small.re <= 2) return false;   // (two rounds: not measured; the one-workgroup path also keeps the reference's order for >= 3 parents)
    // ... and where the two paths' BITS differ -- some node has >= 3 parents: lane groups re-associate, the one-workgroup path keeps the
    // reference's order -- the small network stays on the one-workgroup path whatever its rounds: a batch of such a network runs one
    // workgroup per set (bn_engine_batch.cpp), and a set's answer must not depend on whether it was asked alone or in a batch
    // (scripts/soak_gpu.py found a 30-node network where the two differed by 2e-16; round 6).  Price: 60 nodes of mixed arity, <= 3
    // parents: 72 instead of 65 us per query.
    if (ok.small && f.dag.has_groups) return false;
    if (ok.small && f.small.mmax <= 1 && r.resident_ok && r.blocks == 1) return false;
    // Arities below 4 (padded form), us per sweep, this path / the default before (scripts/time_dag_mixed.py): mixed arities 2-4 with
    // <= 3 parents 300 / 3 000 / 10 000 nodes 4.6 / 5.4, 5.7 / 7.1, 6.5 / 9.2 (item kernels); <= 4 parents, 10 000 nodes (723 k entries:
    // beyond the item kernels) 6.5 / 32.5; binary, <= 4 parents, 10 000 nodes 6.2 / 7.7; k = 3 grid 64 x 64 5.0 / 6.1 -- but k = 2 grid
    // 128 x 128 6.4 / 5.5 (resident tiles): an eighth of every padded table is real there.
    if (!f.dag.uniform4 && !f.dag.has_groups && f.dag.fill < 0.25) return false;
    // Measured, us per query (evidence staged, profiles/r04_paths.json), this path / the best of the others:
    //   lane-group tiles (some node has 3-5 parents): 200 nodes 76 / 122, 1 000 nodes 87 / 165, 3 000 nodes 101 / 182, 10 000 nodes
    //   (BASELINE configs[1]) 117 / 215; nodes of <= 2 parents: 16 x 16 grid 86 / 95, 40 x 40 117 / 135, 64 x 64 113 / 139, 128 x 128
    //   133 / 146, 3 000-node DAG 106 / 119, 200-node chain 74 / 74 -- but 200 x 200 grid 283 / 151, 316 x 316 634 / 234: there the
    //   network no longer fits the chip at one tile per wave (stream form) and the resident tiles keep it.
    // stream form re-reads the padded image every sweep: not where less than a quarter of it is real (a padded binary network
    // with 5-parent nodes is 64x its model), whatever the parent counts -- only <= 10 k-node networks were measured in that form
    if (f.dag.stream && f.dag.fill < 0.25) return false;
    if (f.dag.has_groups) return true;
    return !f.dag.stream;
}

// the register-resident DAG path AHEAD of the one-workgroup path: forced ("dag" 2), or a small network of three or more rounds of
// entry items (dag_applies has the measurements)
bool dag_first_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m) {
    return (m.dag == 2 || (ok.small && m.small != 2)) && dag_applies(f, r, ok, m);
}
bool dag_later_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m) {
    return !dag_first_wanted(f, r, ok, m) && dag_applies(f, r, ok, m);
}

// ---- a batch of evidence sets ----
// Which way a batch goes (measured, scripts/time_batch.py, us per set-sweep at the best batch size of either path): a small network runs one
// workgroup per set; otherwise the register-resident DAG path and the several-workgroup item kernel where their single-query policy
// chooses them; the resident tiles from ~900 tiles up -- per-sweep launches with one set per blockIdx.y share the launch latency among
// the sets, which is what smaller networks pay for (128x128 grid: 1.8 vs 7.7 resident, 200x200: 5.0 vs 8.0); on larger ones the CPT
// traffic the resident kernel saves weighs more (250x250: 9.1 vs 8.2, 316x316: 14.6 vs 8.6).  "multisweep" 2 forces the resident
// kernel wherever eligible, 0 the launches; "dag" 2 puts the DAG path in front of the one-workgroup path, as for single queries.
bool batch_small_wanted(const PathFacts&, const ResidentShape&, const PathOks& ok, const PathModes& m, const BatchDevice& d) {
    return ok.small && m.small != 0 && m.multisweep != 0 && d.small_state && !(m.dag == 2 && ok.dag);
}
bool batch_dag_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m, const BatchDevice& d) {
    return !batch_small_wanted(f, r, ok, m, d) && dag_applies(f, r, ok, m) && d.staged && f.nranks == 1;
}
bool batch_mid_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m, const BatchDevice& d) {
    return !batch_small_wanted(f, r, ok, m, d) && mid_applies(f, r, ok, m) && d.staged;
}
bool batch_resident_wanted(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m, const BatchDevice& d) {
    constexpr int64_t kResidentBatchMinTiles = 900;
    if (batch_small_wanted(f, r, ok, m, d)) return false;
    return r.resident_ok && (m.multisweep == 2 || (m.multisweep == 1 && f.n_tiles >= kResidentBatchMinTiles));
}

// Batches want throughput; a layout built for the latency of one query (wide lane groups, any-arity tiles for nodes with many
// children: bn_plan.cpp) has up to 4x the wavefronts.  Such an engine answers batches of two or more sets through a second engine
// built from the same model with the dense layout -- except on the paths where the layout plays no part: one workgroup per set
// (bn_small.hip), a few per set (bn_mid.hip), the register-resident DAG path (bn_dag.hip).
bool batch_wants_dense(const PathFacts& f, const ResidentShape& r, const PathOks& ok, const PathModes& m, int32_t n_sets) {
    if (!f.latency_rules_applied || f.nranks > 1 || n_sets < 2) return false;
    if (ok.small && m.small != 0 && m.multisweep != 0) return false;
    return !mid_applies(f, r, ok, m) && !dag_applies(f, r, ok, m);
}

// "each set gets exactly the result its single query gives it" (bn_mi355x.h): the two layouts may put a node on DIFFERENT tile
// variants (the latency layout gives nodes with many children the any-arity tiles), and for tables beyond 128 entries -- >= 3
// parents, or two parents of arity >= 6 -- the variants sum in different orders (each within 1e-12 of the reference, but not the
// same bits; scripts/soak_gpu.py, round 6: a 200-node network of arities {4, 6} differed by 1e-16 between a batch and its single
// queries).  Where that happens to some node the batch runs on the engine's own layout.
bool dense_keeps_bits(const NodeLayout* own, int32_t n_own, const NodeLayout* dense, int32_t n_dense) {
    if (n_own != n_dense) return false;
    for (int32_t v = 0; v < n_own; ++v) {
        if (own[v].cls < 0 || dense[v].cls < 0) continue;
        if ((own[v].variant != dense[v].variant || own[v].G != dense[v].G) && own[v].entries > 128) return false;
    }
    return true;
}

std::vector<int32_t> resident_batch_chunks(int32_t n_sets) {
    const int32_t n_chunks = (n_sets + kResidentMaxSets - 1) / kResidentMaxSets;
    std::vector<int32_t> counts;
    for (int32_t c = 0, first = 0; c < n_chunks; ++c) {
        counts.push_back((n_sets - first + (n_chunks - c) - 1) / (n_chunks - c));
        first += counts.back();
    }
    return counts;
}

// as many sets per launch as fit the chip with a workgroup per CU (the grid barrier needs every workgroup of a set resident)
int32_t mid_sets_per_launch(int n_cus, int32_t parts, int32_t n_sets) { return std::max(1, std::min(n_sets, (n_cus * 9 / 10) / parts)); }

// Config 2, us per set-sweep at B = 16: 8.7 / 6.9 / 6.2 / 5.9 with 1 / 2 / 4 / 8 sets per launch in round 4; round 5 (a turn's arrival
// behind the next turn's loads, one evidence launch per chunk, one host wait): 4.65 with 8, 4.49 with 16 -- the pace inside the kernel
// is a wave's set-turn, but a launch's ramp, its evidence launch and the tail where few sets are left come once instead of twice
// (scripts/time_dag_batch.py)
int32_t dag_sets_per_launch(int forced) { return forced == 0 ? kDagMaxSets : std::max(1, std::min(kDagMaxSets, forced)); }

// Max-product (bn_mpe_run, bn_maxprod.hip): the one-workgroup form wherever the one-workgroup plan exists, else the several-workgroup
// form where its plan exists and its workgroups fit 0.9 x CUs (one launch per sweep needs no co-residency, but the same bound keeps a
// sweep one wave of workgroups), else none.  forced: option "mpe_form" -- 1 / 2 give that form where the network is eligible for it,
// else none.
int mpe_form(const PathFacts& f, int n_cus, int forced) {
    const bool one = f.small.ok, several = f.mid.ok && mid_fits(f, n_cus);
    if (forced == 1) return one ? 1 : 0;
    if (forced == 2) return several ? 2 : 0;
    return one ? 1 : (several ? 2 : 0);
}

// Expectation-maximisation: as many rows per launch as the scratch array holds (at least one, at most kEmMaxChunk and the table).
EmPlan em_plan(int64_t n_patterns, int32_t entries, int64_t scratch_cells) {
    EmPlan p;
    const int64_t fit = scratch_cells / std::max<int64_t>(entries, 1);
    p.chunk = int32_t(std::max<int64_t>(1, std::min<int64_t>({fit, int64_t(kEmMaxChunk), n_patterns})));
    p.n_chunks = (n_patterns + p.chunk - 1) / p.chunk;
    p.n_blocks = (n_patterns + kEmBlock - 1) / kEmBlock;
    p.scratch = int64_t(p.chunk) * entries;
    return p;
}

EmChunk em_chunk(const EmPlan& p, int64_t n_patterns, int64_t c) {
    EmChunk k;
    k.first = c * p.chunk;
    k.count = int32_t(std::min<int64_t>(p.chunk, n_patterns - k.first));
    const int64_t end = k.first + k.count;   // one past the chunk's last row
    k.closes = int32_t(end / kEmBlock - k.first / kEmBlock) + (end == n_patterns && end % kEmBlock != 0 ? 1 : 0);
    k.opens_inside = k.first % kEmBlock != 0;
    return k;
}

std::vector<EmRow> em_rows(int32_t n, const int64_t* cpt_off, const int32_t* k) {
    std::vector<EmRow> rows(static_cast<size_t>(cpt_off[n]));
    for (int32_t v = 0; v < n; ++v)
        for (int64_t q = cpt_off[v]; q < cpt_off[v + 1]; ++q) rows[size_t(q)] = {int32_t(cpt_off[v] + (q - cpt_off[v]) / k[v] * k[v]), k[v]};
    return rows;
}

// Exact expectation-maximisation: em_plan's rows, and in form 2 at most the state slices the junction tree's scratch budget holds.
EmPlan jt_em_plan(int64_t n_patterns, int32_t entries, int64_t b_scratch_cells, int form, int64_t state_cells, int64_t state_scratch_cells) {
    EmPlan p = em_plan(n_patterns, entries, b_scratch_cells);
    if (form == 2) {
        const int64_t slices = std::max<int64_t>(1, state_scratch_cells / std::max<int64_t>(state_cells, 1));
        if (slices < p.chunk) {
            p.chunk = int32_t(slices);
            p.n_chunks = (n_patterns + p.chunk - 1) / p.chunk;
            p.scratch = int64_t(p.chunk) * entries;
        }
    }
    return p;
}

}  // namespace bn_policy
