// bn_jt.hpp -- exact inference by junction-tree propagation: the kernels' interface (bn_jt.hip) and the rules of the arithmetic.
// The plan and its item tables: bn_jt_plan.hpp.  The entry points: bn_engine_jt.cpp.
//
// Hugin-style two-pass propagation in fp64, one workgroup per evidence set, __syncthreads() between phases, no communication
// between workgroups.  Every sum and product has a stated order that depends on the plan only -- not on the form, the workgroup
// size or a set's position in a batch -- so the device equals the host restatement (tests/jtree_refs.py) bit for bit.
//   Two-level sum of terms t_0, t_1, ...: runs of kJtRun (64) consecutive terms, each run added left to right from +0.0, then the
//     run sums added left to right from +0.0.  (One lane adds one sum today; the order lets a later kernel spread a long sum.)
//   Base potentials (once per engine and after bn_reload_cpt): psi0_c[e] = 1.0 x the entries of the CPTs assigned to c, in
//     ascending node id.
//   Per query: psi_c[e] = psi0_c[e] x the evidence vectors of the nodes whose home is c, in ascending node id.  Evidence is a
//     LIKELIHOOD, hard or soft: the answer is normalise(P(x_v, e)) for every node, evidence nodes included.
//   Collect, deepest level first: raw separator entry = two-level sum of the clique's matching entries in ascending entry index;
//     s = the separator's entries added left to right from +0.0 (kept: the scale of the clique); the message is raw / s where s > 0,
//     else raw; the parent's entries multiply their children's messages in, in ascending child-clique id.  A root's "separator" has
//     one entry, the two-level sum of all its entries: the root's scale.
//   Distribute, top level first: new = two-level sum of the parent's matching entries; ratio = new / message, and exactly 0 where
//     the message is 0; the child's entries are multiplied by their ratio.
//   Read-out: u[x] = two-level sum of the home clique's entries with x_v = x, ascending entry index; belief = u[x] / (u[0] + u[1] +
//     ... left to right from +0.0), no zero guard: P(e) = 0 gives NaN.
//   Scales: [n_cliques] in clique id order; P(e) is their product (the host adds their std::log in that order).
//
// Exact MPE (bn_jt_mpe_run, jt_mpe_kernel): the same walk over the same tables with every sum replaced by a maximum, and a
// top-down backtrack.  Restated by tests/jtmpe_refs.py; states, max-marginals and scales are equal bit for bit.
//   Max fold of terms (bn_maxprod.hpp): acc = +0.0, then acc = x if acc < x else acc.  A NaN never replaces acc: the result is the
//     largest term above +0.0, else +0.0, WHATEVER THE ORDER -- this pass has no stated order of its folds, so a long fold may be
//     spread over lanes and reduced without changing a bit.
//   Potentials: as above.
//   Collect, deepest level first: raw separator entry = max fold of the clique's matching entries; s = max fold of the separator's
//     entries (kept: the scale of the clique); the message is raw / s where s > 0, else raw; the parent's entries multiply their
//     children's messages in, in ascending child-clique id.  A root's "separator" is the max fold of all its entries.
//   Distribute, top level first: ratio = (max fold of the parent's matching entries) / message, exactly 0 where the message is 0;
//     the child's entries are multiplied by their ratio.
//   Scales: their product is max_x P(x, e); log_p = the sum of their std::log in clique order, -inf when a factor is 0.  (The
//     divisors are constants of the set, so they factor out of every maximum as they factor out of every sum.)
//   Max-marginals: u[x] = max fold of the home clique's entries with x_v = x; output u[x] / (u[0] + u[1] + ... left to right from
//     +0.0), no zero guard -- bn_mpe_run's normalisation.
//   Decode by backtracking, pick[c] an entry index of clique c: a root picks the lowest entry index of its largest entry
//     (best = t[0]; t[i] > best takes i).  A child's separator entry is j = up_map[up_off + pick[parent]]; the child picks, among
//     its entries that match j -- the terms c_base[sep_off + j] + c_res[cres_off + t], ascending -- the lowest entry index of the
//     largest.  The child's entries are read AS THEY STAND AFTER COLLECT, before the clique's own distribute multiply: ties are not
//     disturbed by the rounding of the ratio, and the pick of a level rides the phase that computes the level's ratios (it needs
//     pick[parent] of the phase before only), so decoding adds no barrier.  states[v] = (pick[home[v]] / stride_v) % k_v.
//     With P(e) = 0 the states are what the rule gives: meaningless, but pinned by the restatement.
//
// Exact EM (bn_jt_em_expected_counts, bn_jt_em_fit, jt_em_kernel): bn_em.hpp's table, sums, M-step and loop with the E-step taken
// from this propagation instead of loopy belief propagation -- exact wherever the tree fits, not on polytrees only.  Restated by
// tests/jtem_refs.py; E, theta after every iteration, the deltas and the skipped count are equal bit for bit.
//   The table: patterns [P][n] uint8, counts [P] uint64, 255 for a cell that is not observed (bn_em.hpp).
//   Per iteration the base potentials are computed from the current theta (jt_base_kernel), into an array the EM state owns.
//   Per row: psi_c[e] = psi0_c[e] x, for every OBSERVED node whose home is c in ascending node id, 1.0 where the node's digit in e
//     equals the cell and 0.0 elsewhere -- the bits of bn_jt_run with a one-hot vector.  Collect and distribute as above.
//   Family read-out: node v's CPT lies in clique c = cpt_clique[v], which holds pa(v) and v.  For a flat CPT entry q of v (first
//     parent most significant, own state last): u[q] = two-level sum of the entries of clique c whose digits match q, in ascending
//     entry index; s_v = two-level sum of u[q] over v's entries in flat order; b[q] = u[q] / s_v where s_v > 0.  Where `s_v > 0` is
//     false (zero or NaN: the row has probability 0 under theta in v's tree) the family contributes nothing (b = 0.0) and is counted.
//     A fully observed family has one non-zero u, so b is exactly 1.0: on a complete table with theta > 0, E is the integer counts.
//   Row log-likelihood: ll_p = the sum of log(scale_c) over the cliques, -inf when a factor is 0; computed on the device (its log
//     is not libm's) and added in no stated order: the one quantity that is not pinned bit for bit.
//     L = sum_p (count_p > 0 ? double(count_p) x ll_p : 0.0), reported per iteration; it does not steer the loop.
//   E[q] = sum_p double(count_p) x b_p[q] in bn_em.hpp's block-of-256 order (em_accumulate_kernel); the M-step, delta and the stop
//     rule are bn_em.hpp's, bit for bit.
#ifndef BN_JT_HPP
#define BN_JT_HPP
#include <cstddef>
#include <cstdint>

#include "bn_jt_plan.hpp"

namespace bnmi {

// The plan's dimensions and item tables on the device (bn_jt_plan.hpp) and the base potentials of one set of CPTs: what every walk
// over the tree reads.  Filled by bn_eng::jt_tables_of.
struct JtTables {
    int32_t n, N, nc, nlev;
    int32_t pot_cells, sep_cells, state_cells;
    const JtClique* cliques;
    const JtLevel* levels;
    const JtNode* nodes;
    const int32_t* ent_clique;
    const int32_t* dn_map;
    const int32_t* sep_clique;
    const int32_t* c_base;
    const int32_t* p_base;
    const int32_t* c_res;
    const int32_t* p_res;
    const int32_t* up_map;
    const int32_t* home_nodes;
    const int32_t* elem_node;
    const double* psi0;             // [pot_cells]
};

struct JtArgs {
    JtTables t;
    int32_t set_base;               // the launch's first set: workgroup b runs set set_base + b in state slot b
    // evidence: the caller's arrays in a staging block (bn_batch_stage.hpp), set q's header at ev_meta + 8 q
    const int32_t* ev_node;
    const int32_t* ev_off;
    const double* ev_val;
    const int32_t* ev_meta;
    int32_t* ev_slot;               // [slots][n] scratch: where a node's evidence vector starts, -1: none
    double* scratch;                // form 2: [slots][state_cells]
    double* beliefs;                // [sets][N]  (a max run: the max-marginals)
    double* scales;                 // [sets][nc]
    int32_t* states;                // [sets][n]  a max run's decoded assignment; a sum run does not touch it
};

enum JtKind : int { kJtNone = 0, kJtSum = 1, kJtMax = 2 };   // bn_get_info "jt_last_kind"

struct JtBaseArgs {
    int32_t pot_cells;
    const JtClique* cliques;
    const int32_t* ent_clique;
    const int32_t* asg_ptr;
    const JtAsg* asg;
    const JtFam* fam;
    const double* cpt;              // the flat CPT array
    double* psi0;
};

int launch_jt_base(const JtBaseArgs& a, void* stream);

// ---- exact EM: one workgroup per pattern row of the launch (blockIdx.x), the state in LDS (form 1) or in slice blockIdx.x of scratch
constexpr int kJtEmMissing = 255;   // BN_EM_MISSING
struct JtEmArgs {
    JtTables t;                     // psi0: of the current theta
    int32_t S;                      // CPT entries
    const JtFamily* families;       // [n]
    const int32_t* f_node;          // [S]
    const int32_t* f_base;          // [S]
    const int32_t* f_res;
    const uint8_t* patterns;        // the launch's rows, [rows][n]
    double* scratch;                // form 2: [rows][state_cells]
    double* b;                      // [rows][S] family posteriors, flat CPT order
    double* loglik;                 // [rows] of the launch
    int32_t* skipped;               // [rows] families with s_v not > 0
};
int launch_jt_em(const JtEmArgs& a, int form, int n_rows, void* stream);

struct JtEmTotalArgs {
    int64_t n_patterns;
    const unsigned long long* counts;
    const double* loglik;           // [n_patterns]
    const int32_t* skipped;         // [n_patterns]
    double* L;                      // written
    unsigned long long* skipped_total;   // added to
};
int launch_jt_em_total(const JtEmTotalArgs& a, void* stream);

// form 1: state in LDS; form 2: in a.scratch.  One workgroup per set.  kind: kJtSum (jt_kernel) or kJtMax (jt_mpe_kernel).
int launch_jt(const JtArgs& a, int form, int kind, int n_sets, void* stream);

}  // namespace bnmi

#endif  // BN_JT_HPP
