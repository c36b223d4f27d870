// bn_em.hpp -- expectation-maximisation: CPTs fitted from a table with unobserved cells, the E-step being the sum-product loop of
// bn_bp_run on the one-workgroup path (bn_small.hip), one workgroup per pattern row.  Everything is fp64.
//
// The table.   patterns [n_patterns][n_nodes] uint8, counts [n_patterns] uint64: bn_fit_cpt's layout.  A cell of kEmMissing (255)
//   is "not observed" (arities are <= 255, so 255 is never a state); any other cell must be < k[v].  A row may be fully observed,
//   fully missing, or have count 0.
// The E-step, per pattern p, under the current tables theta:
//   1. every observed node, in increasing id, gets a one-hot evidence vector (1.0 at its state): pi(v) and lambda(v) (:68-73);
//   2. the loop of belief_propagation.hpp:33-158 with (bp_eps, bp_max_sweeps) -- bp_max_sweeps == 0 means kMpeDefaultCap sweeps, NOT
//      unbounded (bn_maxprod.hpp: no loop without an end on the device).  A run cut by the cap is used as it stands and counted.  Sweep
//      count, final pi-messages, final pi(v) and lambda(v) have the bits of bn_bp_run on the one-workgroup path for that evidence;
//   3. from the state the run stopped in, for every node v with parents u_1 < ... < u_m, every assignment a (first parent most
//      significant) and own state i:
//        t'[a,i] = (...((cpt[a,i] x pimsg(u_1 -> v)[a_1]) x pimsg(u_2 -> v)[a_2]) ... x pimsg(u_m -> v)[a_m])
//                  -- the term, and the bits, that pi(v)[i]'s sum adds (:174-200)
//        r[i]    = sum_a t'[a,i], front to back in table order from +0.0 (pi(v)[i] before its normalisation)
//        s       = sum_i (r[i] x lambda(v)[i]), left to right from +0.0
//        b[a,i]  = (t'[a,i] x lambda(v)[i]) / s            = P(x_v = i, pa(v) = a | e) on a polytree
//      An evidence node goes through the same formula: its lambda(v) IS its one-hot vector.  Where `s > 0` is false (zero or NaN: the
//      evidence has probability 0 under theta) that family of that pattern contributes nothing and is counted ("em_skipped");
//   4. E[q] = sum_p double(counts[p]) x b_p[q] in a FIXED order: patterns in blocks of kEmBlock (256) consecutive indices; inside a
//      block added in increasing p from +0.0; the block sums added in increasing block order from +0.0.
//      E DEPENDS ON THE ORDER OF THE ROWS (permuting the table may change last bits); it does not depend on how the rows are cut
//      into launches (chunks) or on the launch shape.
//   A fully observed family has exactly one non-zero t', so b is exactly 1.0 there: on a complete table with strictly positive theta
//   E is the exact integer counts as doubles.
// The M-step.  E'[q] = E[q] + prior (prior >= 0, finite); per CPT row tot = sum_i E'[a,i] left to right from +0.0;
//   theta_new[a,i] = E'[a,i] / tot; a row where `tot > 0` is false becomes uniform, 1.0 / double(k[v]).  With prior = 0 on a complete
//   table these are bn_fit_cpt's bits (bn_fit_kernels.hip: double(count) / double(total), sums of integers below 2^53 being exact).
// The loop.    delta = max_q |theta_new[q] - theta[q]| (md = +0.0; md = (md < d) ? d : md -- a NaN never replaces md); stop after the
//   iteration where delta < tol (strict <: tol = 0 never stops early) or after max_iters iterations (1 .. kEmMaxIters).
//
// The kernels read the SmallPlan tables the engine uploaded (entry, accumulator and product items, bn_small.hpp) as they are; the CPT
// values -- the entry items' ent_cpt image and the roots' initial pi(v) -- are copies the EM state owns and rewrites every M-step.
// Nothing the bn_bp_* / bn_mpe_* calls use is touched.
#pragma once

#include <cstdint>

#include "bn_engine_policy.hpp"
#include "bn_maxprod.hpp"
#include "bn_small.hpp"

namespace bnmi {

constexpr int kEmMissing = 255;      // BN_EM_MISSING
constexpr int kEmBlock = 256;        // patterns per block of the E sum
constexpr int kEmMaxIters = 10000;

// ---- E-step: one workgroup per pattern of the chunk (blockIdx.x), the whole run in LDS
struct EmSmallArgs {
    double eps;
    int32_t max_sweeps;           // > 0 always (the cap)
    int32_t n, N, M, S, T, TT, CL, re, rb, rc;
    const SmallEntry* ent;        // the engine's item tables
    const double* ent_cpt;        // the EM state's own image of theta, [re][threads]
    const uint32_t* term;
    const uint16_t* clist;
    const SmallSlot* bslot;
    const SmallSlot* cslot;
    const double* npi_init;       // the EM state's own: the CPT row of a root, else 1.0
    const int32_t* node_off;      // [n + 1]
    const int32_t* ent_flat;      // [re][threads] entry slot -> flat CPT entry | (first entry of its family) << 16; -1: no entry
    const uint8_t* patterns;      // the chunk's rows, [chunk][n]
    double* b;                    // [chunk][S] family posteriors, flat CPT order
    int32_t* sweeps;              // [chunk]
    unsigned long long* counters; // [0] runs cut by the cap, [1] families with s not > 0 (added to)
};
int prepare_em_small();   // once per device, before the first launch
int launch_em_small(const EmSmallArgs& a, int waves, size_t lds_bytes, int32_t chunk, void* stream);

// ---- the chunk's count x b into the block partials and E (one thread per CPT entry)
struct EmAccArgs {
    int32_t S, chunk;
    int64_t first, n_patterns;    // global index of the chunk's first pattern, patterns of the table
    const double* b;              // [chunk][S]
    const unsigned long long* counts;   // [n_patterns]
    double* partial;              // [S] the sum of the block in hand
    double* E;                    // [S]
};
int launch_em_accumulate(const EmAccArgs& a, void* stream);

// ---- M-step (one thread per CPT entry), of this E-step and of the junction tree's (bn_jt.hpp, "Exact EM")
struct EmMstepArgs {
    int32_t S;
    double prior;
    const double* E;              // [S]
    const bn_policy::EmRow* row;  // [S] the entry's CPT row: first entry, arity (bn_policy::em_rows)
    const int32_t* slot_of;       // [S] flat entry -> its slot in ent_cpt; null: no images to rewrite (the three below are not read)
    const int32_t* init_of;       // [S] flat entry -> element of npi_init (a root's), -1: none
    double* theta;                // [S] in: the current tables, out: the new ones
    double* ent_cpt;
    double* npi_init;
    unsigned long long* delta_bits;   // max |theta_new - theta|, bit pattern of a non-negative double (zeroed by the host)
};
int launch_em_mstep(const EmMstepArgs& a, void* stream);

}  // namespace bnmi
