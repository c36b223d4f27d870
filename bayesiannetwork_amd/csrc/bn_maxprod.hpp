// bn_maxprod.hpp -- max-product belief propagation (Pearl's belief revision): the most probable explanation.
//
// The algorithm is the reference's loop (belief_propagation.hpp:33-158) with ONE line changed: where pi(v) (:174-200) and the
// lambda-message to a parent (:240-266) add their terms over the parent assignments, they take the LARGEST term.  Everything
// else is as in sum-product: the terms' products (cpt x pi-messages, parents ascending; (lambda(v)[i] x cpt) x the other
// parents' pi-messages, ascending), lambda(v) and the pi-messages as products over the children, the normalisation (:298-311,
// left-to-right sum), evidence as both pi(v) and lambda(v) (:68-73), the residual over the messages only (:105-131), the
// strict `<` of the stop decision (:147), belief = normalize(pi % lambda) (:151-158): here the node's max-marginal.
//
// The fold.    acc = +0.0;  for every term x of the run:  acc = (acc < x) ? x : acc;
//   A NaN term never replaces acc (acc < NaN is false), and acc itself is never NaN: the result is the largest term above +0.0,
//   else +0.0, whatever the ORDER of the terms.  So the fold needs no order -- the kernels keep eight (or four) partial maxima and
//   combine them with the same rule, one v_max_f64 per term (bn_maxprod.hip mpe_max) -- and the zero padding of the staged runs (bn_small_plan.cpp) is harmless.
// The state.   After the belief the node's state is decoded from the normalised max-marginal vector b[0 .. k):
//   idx = 0, best = b[0];  for i = 1 .. k-1:  if (b[i] > best) { best = b[i]; idx = i; }
//   -- the LOWEST index that holds the largest element (strict >); a vector of NaNs (an all-zero evidence vector: 0 / 0)
//   gives state 0.
// The cap.     max_sweeps == 0 means kMpeDefaultCap sweeps, NOT unbounded: max-product on a loopy network may oscillate for
//   ever, and a loop without an end on the device is a hang.  A run that stops on the cap reports done == 2.
//
// Two forms, both over the item tables an engine has built and uploaded for the sum-product paths (bn_small.hpp: SmallPlan,
// MidPlan, MidTables), read as they are:
//   one workgroup       (SmallPlan ok)  the whole run in one launch, state in LDS; a batch: one workgroup per evidence set;
//   several workgroups  (MidPlan ok)    one workgroup per MidPart, state in device memory (double buffered), ONE LAUNCH PER
//                                       SWEEP: the launch boundary is the only synchronisation between workgroups -- no grid
//                                       barrier, no wait, no polling inside a kernel.  Every workgroup of launch s + 1 first
//                                       reduces the residual words the workgroups of launch s left and takes the stop decision
//                                       itself; launches queued behind the stopping sweep return at once.
#pragma once

#include <cstdint>

#include "bn_small.hpp"

namespace bnmi {

constexpr int kMpeDefaultCap = 10000;   // sweeps of a run with max_sweeps == 0
constexpr int kMpeDefaultGroup = 16;    // several-workgroup form: sweep launches between two reads of the control record
constexpr int kMpeMaxGroup = 64;

// What a run reports (page-locked host memory the kernels write themselves; one per evidence set)
struct MpeCtl {
    int32_t done;       // 0 running, 1 converged (maximum_difference < eps), 2 stopped on the cap
    int32_t n_sweeps;   // iterations executed
    uint32_t run_id;    // the run the other fields describe
    uint32_t pad_;
    double last_res;    // maximum_difference of the last executed sweep
    unsigned long long t_first, t_last;   // 100 MHz clock: start of the first sweep, end of the last
};

// ---- one workgroup: every evidence set of the call in one launch (blockIdx.x = set)
struct MpeSmallArgs {
    double eps;
    int32_t max_sweeps, sweep_begin, budget;   // max_sweeps > 0 always (the cap)
    uint32_t run_id;
    MpeCtl* host_ctl;             // [n_sets]
    int32_t n, N, M, T, TT, CL, re, rb, rc;
    const SmallEntry* ent;
    const double* ent_cpt;
    const uint32_t* term;
    const uint16_t* clist;
    const SmallSlot* bslot;
    const SmallSlot* cslot;
    const double* npi_init;
    const int32_t* node_off;      // [n + 1]
    const int32_t* elem_node;     // [N] the node of a node-vector element
    // evidence: the caller's arrays in a staging block (bn_batch_stage.hpp), set q's header at ev_meta + 8 q
    const int32_t* ev_node;
    const int32_t* ev_off;
    const double* ev_val;
    const int32_t* ev_meta;
    // per set, at these strides
    double* max_marginals;        // [N]
    int32_t* states;              // [n]
    double* res_hist;             // [res_cap]
    double* state;                // [2 M + 2 N] pi-messages, lambda-messages (CSR edge order), pi(v), lambda(v) the launch stopped in
    int32_t res_cap;
};
int prepare_mpe_small();   // once per device, before the first launch
int launch_mpe_small(const MpeSmallArgs& a, int waves, size_t lds_bytes, int n_sets, void* stream);

// ---- several workgroups: one evidence set, one launch per sweep
struct MpeMidSync {               // device memory
    int32_t stop_sweeps;          // -1: the run goes on; else the number of sweeps it stopped after
    int32_t pad_;
    unsigned long long t_first;
    unsigned long long words[2][kMidMaxParts];   // [parity of the sweep][workgroup]: its maximum_difference, bit pattern
};
struct MpeMidArgs {
    double eps;
    int32_t max_sweeps;           // > 0 (the cap)
    uint32_t run_id;
    MpeCtl* host_ctl;             // this set's
    int32_t n, N, M, nparts;
    const MidPart* parts;
    const SmallEntry* ent;
    const double* ent_cpt;
    const uint32_t* term;
    const uint16_t* clist;
    const SmallSlot* bslot;
    const SmallSlot* cslot;
    const double* npi_init;
    const int32_t* node_off;
    const int32_t* elem_node;
    int32_t ev_ne;                // this set's evidence
    const int32_t* ev_node;
    const int32_t* ev_off;
    const double* ev_val;
    double* pi;                   // [2][M]
    double* lam;                  // [2][M]
    double* npi;                  // [2][N]
    double* nlam;                 // [2][N]
    uint8_t* frz;                 // [N]
    MpeMidSync* sync;
    double* max_marginals;        // this set's [N]
    int32_t* states;              // [n]
    double* res_hist;             // [res_cap]
    int32_t res_cap;
};
int prepare_mpe_mid();
int launch_mpe_mid_init(const MpeMidArgs& a, void* stream);                 // initial state, evidence marks, stop word
int launch_mpe_mid_evidence(const MpeMidArgs& a, void* stream);             // the evidence vectors into pi(v) and lambda(v)
// sweep number `s` (0, 1, ...): decides on sweep s - 1 first.  finish: no sweep -- the decision, then (if the run has stopped)
// max-marginals and states from the state it stopped in
int launch_mpe_mid_sweep(const MpeMidArgs& a, int32_t s, bool finish, int waves, int rounds, size_t lds_bytes, void* stream);

}  // namespace bnmi
