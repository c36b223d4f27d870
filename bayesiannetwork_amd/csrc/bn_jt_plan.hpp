// bn_jt_plan.hpp -- the plan of exact inference by junction-tree (clique-tree) propagation (bn_jt.hip, bn_engine_jt.cpp; the rules
// of the arithmetic: bn_jt.hpp).  Pure host code: no HIP, no engine -- tests/cpp/test_jt_plan.cpp compiles bn_jt_plan.cpp alone.
//
// From the flat model (arities, parent lists): the moral graph; a min-fill elimination order -- the node whose elimination adds the
// fewest edges, ties to the smaller table of {node} + neighbours, then to the lower node id; the MAXIMAL elimination cliques; the
// clique forest (a clique hangs below the clique that holds what is left of it once its own node is eliminated), every tree rooted
// at its centre so that it is as shallow as it can be; the separators.  Cliques are numbered level by level, root level first, the
// children of one clique next to each other: a level is a range of clique ids, of potential entries and of separator entries.
// Variables inside a clique or separator are in ascending node id, first most significant.
//   CPT of node v   -> the clique that absorbed the elimination clique of v's earliest-eliminated family member (it holds the family);
//   home of node v  -> the clique with the smallest table among those that hold v (ties: lowest clique id): it receives v's evidence
//                      vector and is where v's marginal is read.
// Exact expectation-maximisation (bn_jt.hpp, "Exact EM") reads every family's posterior from the clique of its CPT: the family tables
// below (families, f_node, f_base, f_res; tests/cpp/test_jt_em_plan.cpp walks them).
// Limits (facts of the plan, `ok` / `why`): an elimination clique of more than kJtMaxClique entries stops the planner where it
// meets it; a per-set state above the scratch budget makes the network ineligible too (jt_apply_budget: re-checked when the option
// changes, nothing is rebuilt).
#ifndef BN_JT_PLAN_HPP
#define BN_JT_PLAN_HPP
#include <cstdint>
#include <string>
#include <vector>

namespace bnmi {

constexpr int64_t kJtMaxClique = int64_t(1) << 20;      // entries of one clique table (the per-family limit of the EM path)
constexpr int64_t kJtScratchCells = int64_t(1) << 22;   // default of option "jt_scratch_cells": doubles of device scratch
constexpr int64_t kJtMaxScratchCells = int64_t(1) << 30;
constexpr int32_t kJtRun = 64;                          // terms per run of a two-level sum (bn_jt.hpp)
constexpr int64_t kJtLdsCells = 8192;                   // form 1: the per-set state fits 64 KiB of LDS (two sets per CU)

struct JtClique {
    int32_t pot_off, size;          // its potential: state[pot_off .. pot_off + size)
    int32_t sep_off, sep_size;      // its separator towards the parent: state[pot_cells + sep_off ..); a root's has ONE entry, the total
    int32_t parent, level;          // -1 / 0: a root
    int32_t child_lo, child_hi;     // its children are the cliques [child_lo, child_hi)
    int32_t cres_off, cres_cnt;     // c_res[cres_off ..): offsets, inside this clique, of the terms of one separator entry's sum
    int32_t pres_off, pres_cnt;     // p_res[pres_off ..): the same inside the parent (distribute)
    int32_t up_off;                 // up_map[up_off + e]: the separator entry that entry e of the PARENT reads
    int32_t home_lo, home_hi;       // home_nodes[home_lo .. home_hi): the nodes whose home this clique is, ascending
    int32_t pad_;
};
struct JtLevel { int32_t c_lo, c_hi, pot_lo, pot_hi, sep_lo, sep_hi, pad0_, pad1_; };
struct JtNode { int32_t home, stride, k, bel_off; };   // digit of the node in entry e of its home clique: (e / stride) % k
struct JtFam { int32_t stride, k, cstride; };           // a family member: its digit in the clique entry, times cstride into the CPT
struct JtAsg { int64_t cpt_off; int32_t node, fam_lo, fam_hi, pad_; };
// a node's family inside the clique of its CPT (exact EM's read-out, bn_jt.hpp): flat CPT entries [cpt_lo, cpt_lo + cpt_cnt), the
// clique's potential at pot_off, f_res[res_off .. res_off + res_cnt): the offsets of one entry's terms from its first, ascending
struct JtFamily { int32_t pot_off, cpt_lo, cpt_cnt, res_off, res_cnt, pad_; };

struct JtPlan {
    bool built = false;             // the structure is complete (`why` may still name the scratch budget)
    bool ok = false;
    std::string why;
    int32_t n = 0, N = 0, nc = 0, nlev = 0, max_clique_vars = 0;
    int64_t pot_cells = 0, sep_cells = 0, state_cells = 0, max_clique = 0;
    // structure: what bn_jt_plan_dump hands out
    std::vector<int32_t> order;                 // [n] the elimination order
    std::vector<int32_t> parent, level;         // [nc]
    std::vector<int32_t> var_ptr, vars;         // [nc + 1], the cliques' variables
    std::vector<int32_t> sep_ptr, sep_vars;     // [nc + 1], the separators' (none for a root)
    std::vector<int32_t> cpt_clique, home;      // [n]
    // item tables: what the kernels read
    std::vector<JtClique> cliques;
    std::vector<JtLevel> levels;
    std::vector<JtNode> nodes;
    std::vector<int32_t> ent_clique, dn_map;    // [pot_cells]: clique of an entry; the entry of its own separator it belongs to
    std::vector<int32_t> sep_clique, c_base, p_base;   // [sep_cells]: clique of a separator entry; first term's offset in the clique / the parent
    std::vector<int32_t> c_res, p_res, up_map, home_nodes, elem_node;
    std::vector<int32_t> asg_ptr;               // [nc + 1] the CPTs of a clique, ascending node id
    std::vector<JtAsg> asg;
    std::vector<JtFam> fam;
    // family tables, in the style of c_base / c_res: present where the flat CPT array has fewer than 2^31 entries (else empty)
    std::vector<JtFamily> families;             // [n]
    std::vector<int32_t> f_node, f_base;        // [CPT entries]: the entry's node; the offset, inside the clique, of its sum's first term
    std::vector<int32_t> f_res;
};

// state of one evidence set, in doubles: potentials | separators | unnormalised marginals [N] | scales [nc]
void build_jt_plan(int32_t n, const int32_t* k, const int32_t* in_ptr, const int32_t* in_idx, const int64_t* cpt_off, int64_t scratch_cells,
                   JtPlan& out);
// ok / why of a built plan under another scratch budget
void jt_apply_budget(JtPlan& p, int64_t scratch_cells);
// 1: state in LDS, 2: state in device scratch, 0: the plan cannot take the form asked for (option 0: the rule -- 1 where it fits)
int jt_form(const JtPlan& p, int option);

}  // namespace bnmi

#endif  // BN_JT_PLAN_HPP
