/*
 * bn_mi355x.h -- C ABI of the MI355X-native inference engine (libbn_mi355x.so).
 *
 * The reference (godai0519/BayesianNetwork) has no FFI layer: its boundary is the C++ class
 * surface of bayesian/inference.  These entry points are what a binding underneath that
 * surface needs, and each one names the reference interface it replaces.  The header-only
 * C++14 drop-in classes that sit on top are in include/bayesian/inference/ (same names and
 * signatures as the reference's); INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - Plain C types only; no exceptions cross the boundary.  Every int-returning function
 *     returns BN_OK (0) or a negative bn_status; bn_last_error() gives the message of the
 *     calling thread's last failure.
 *   - The caller keeps ownership of every array it passes; the engine copies what it needs.
 *   - An engine handle is NOT thread-safe (the reference's functors are not either:
 *     belief_propagation.hpp:320-333 holds mutable scratch state).
 *   - Node identity is the position in graph_t::vertex_list() (graph.hpp:214); parents are
 *     ascending (graph.hpp:389-402); the CPT of a node is row-major with the first parent most
 *     significant and the node's own state fastest (belief_propagation.hpp:269-295).
 */
#ifndef BN_MI355X_H
#define BN_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum bn_status {
    BN_OK = 0,
    BN_ERR_ARG = -1,        /* malformed model / evidence / argument            */
    BN_ERR_HIP = -2,        /* a HIP runtime call failed                         */
    BN_ERR_NO_DEVICE = -3,  /* no gfx950 device visible                          */
    BN_ERR_ALLOC = -4,      /* host allocation failed                            */
    BN_ERR_COMM = -5,       /* RCCL call failed / communicator not initialised   */
    BN_ERR_STATE = -6       /* call not valid in the engine's current state      */
} bn_status;

#define BN_MAX_PARENTS 16
#define BN_MAX_BATCH_SETS 256 /* evidence sets per bn_bp_run_batch call */
#define BN_DEVICE_HOST_ONLY (-2) /* build the layout plan only; no HIP call is made */
#define BN_DEVICE_CURRENT (-1)

/*
 * Flat model = graph_t + every vertex_t::cpt, flattened once.
 * Replaces: graph_t const& taken by belief_propagation::belief_propagation
 * (belief_propagation.hpp:16) and likelihood_weighting::likelihood_weighting
 * (likelihood_weighting.hpp:20), plus cpt_t lookups (graph.hpp:117).
 */
typedef struct bn_model_desc {
    int32_t n_nodes;
    const int32_t *k;       /* [n]    vertex_t::selectable_num                         */
    const int32_t *in_ptr;  /* [n+1]  CSR over parents                                 */
    const int32_t *in_idx;  /* [E]    parents, strictly ascending per node             */
    const int64_t *cpt_off; /* [n+1]  prefix sums of k[v] * prod k[parents]            */
    const double *cpt;      /* flat CPTs, reference row order                          */
    int32_t device;         /* HIP ordinal, BN_DEVICE_CURRENT or BN_DEVICE_HOST_ONLY   */
    int32_t lanes_per_node; /* 0 = automatic: small networks get a layout that shortens the   */
                            /*     latency of ONE query (more, lighter wavefronts: any-arity */
                            /*     tiles for nodes with many children, the wide lane-group   */
                            /*     split of 3 / 4 below);                                    */
                            /* 1 = one lane per node everywhere (no lane groups, no          */
                            /*     wavefront-per-node variant: A/B tests);                   */
                            /* 2 = dense: fewest wavefronts, for throughput (what the engine */
                            /*     builds internally for bn_bp_run_batch on such networks);  */
                            /* 3, 4 = 0, 2 plus the wide lane-group split (k = 4 with 3 or 4 */
                            /*     parents: 16 table entries per lane instead of 64) on small*/
                            /*     networks: ~10 % less latency per query, 4x the wavefronts;*/
                            /*     marginals agree with 0 / 2 to rounding, not bit for bit   */
} bn_model_desc;

typedef struct bn_engine bn_engine;

/* Validate the model, build the device layout, upload it.  Replaces the functor constructors. */
int bn_create(const bn_model_desc *desc, bn_engine **out);
void bn_destroy(bn_engine *eng);
/*
 * New CPT values on the SAME structure.  The reference reads node->cpt on every call (belief_propagation.hpp:61,186,252;
 * likelihood_weighting.hpp:148-158), so a table edited or re-fitted (sampler::make_cpt) after a functor was built is seen by
 * its next call; an engine holds device images made at bn_create and sees new values only through this call.
 * cpt [n_entries] is the whole flat array in bn_model_desc.cpt's layout; n_entries must equal the model's cpt_off[n].
 * Costs one pass over the tables on the host and one host-to-device copy per image; every later bn_bp_run* / bn_lw_run /
 * bn_rs_run uses the new values.  Staged evidence stays in force.
 */
int bn_reload_cpt(bn_engine *eng, const double *cpt, int64_t n_entries);

/*
 * Multi-GPU: one process per GPU, each creating shard `rank` of `nranks` from the SAME global
 * model.  owner[v] in [0,nranks) is the edge-cut partition (NULL = contiguous ranges balanced by
 * CPT bytes: row stripes on a row-major grid).  The pi-message of an edge is computed by the
 * parent's owner, the lambda-message by the child's owner; cut edges are exchanged by ONE
 * in-place RCCL all-gather per sweep, which also carries the residual so that every rank stops on
 * the same sweep.  Bootstrap: rank 0 calls bn_comm_unique_id, ships the 128 bytes to the other
 * ranks by any means (bench.py: torch.distributed broadcast), every rank calls bn_comm_init.
 * Beliefs of a sharded engine are node-major over ALL nodes with zeros for nodes of other ranks
 * (summing the ranks' arrays gives the global result).
 */
int bn_create_sharded(const bn_model_desc *desc, int32_t rank, int32_t nranks, const int32_t *owner,
                      bn_engine **out);
/*
 * Halo exchange INSIDE the resident kernel (no collective per sweep): every rank exports a blob -- handles of its
 * record buffers and sync block, and which of its tiles hold the nodes on cut edges -- the caller ships the blobs by
 * any means (bench.py / tests: torch.distributed all_gather_object, a pipe), and every rank imports all of them
 * (blobs[r] = rank r's, its own included).  After that a run of the sharded engine is ONE launch per rank: a tile
 * stores the message halves it produces for a cut edge into the peer's exchange region as well as its own
 * (peer-mapped memory: hipIpc handles between processes, plain pointers inside one; system-scope write-through
 * stores over xGMI), tiles wait for their neighbour tiles' generation granules wherever those live, and each rank's
 * service block hands its residual to every rank, so all ranks stop on the same sweep (belief_propagation.hpp:
 * 105-147).  Networks whose tiles the resident kernel does not cover (any rank) stay on bn_comm_init + per-sweep
 * launches; bn_get_info("shard_flow") tells.  Every rank must then run the same sequence of bn_bp_run* calls.
 */
int64_t bn_peer_blob_size(bn_engine *eng);
int bn_peer_export(bn_engine *eng, void *blob, int64_t cap);
int bn_peer_import(bn_engine *eng, const void *const *blobs, const int64_t *sizes, int32_t n);
int bn_comm_unique_id(void *id_out128);
int bn_comm_init(bn_engine *eng, const void *id128);
const char *bn_last_error(void);
const char *bn_version(void);

/*
 * Loopy belief propagation to convergence.
 * Replaces: belief_propagation::operator()(precondition, epsilon) (belief_propagation.hpp:31-159).
 *   ev_node[ne], ev_off[ne+1], ev_val[ev_off[ne]] : evidence vectors (1 x k[v] each, used as both
 *       pi and lambda, :68-73); ne may be 0 (the by-pass overload, :24-28).
 *   eps        : strict '<' on the maximum absolute message change (:147)
 *   max_sweeps : 0 = unbounded like the reference
 *   beliefs_out: [sum k] node-major, normalize(pi % lambda) (:151-158); host memory
 *   sweeps_out / residual_out : iterations executed and the last maximum_difference (optional)
 */
int bn_bp_run(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_off,
              const double *ev_val, double eps, int32_t max_sweeps, double *beliefs_out,
              int32_t *sweeps_out, double *residual_out);

/*
 * The same in two steps, for callers that keep inputs and outputs resident in HBM (bench.py times
 * this path): bn_bp_set_evidence validates, uploads and applies an evidence set once (it stays in
 * force until the next call); bn_bp_run_device runs belief propagation on it -- any number of
 * times, each run starts directly with its first sweep -- and leaves the beliefs in device
 * memory (bn_bp_beliefs_device, node-major [sum k]); only the sweep count and the last
 * maximum_difference come back.  bn_bp_run == set_evidence + run_device + copy_beliefs.
 */
int bn_bp_set_evidence(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_off,
                       const double *ev_val);
int bn_bp_run_device(bn_engine *eng, double eps, int32_t max_sweeps, int32_t *sweeps_out,
                     double *residual_out);
const double *bn_bp_beliefs_device(bn_engine *eng);
/* bn_bp_run with the marginals left in a page-locked host buffer owned by the engine (*beliefs_view, [sum k],
 * valid until the next run on this engine): evidence upload, run and the copy of the beliefs are queued back
 * to back and waited for ONCE, and a caller that unpacks the flat array anyway (the C++ functor building its
 * map of 1 x k matrices, belief_propagation.hpp:151-158) reads it in place. */
int bn_bp_run_view(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_off,
                   const double *ev_val, double eps, int32_t max_sweeps, const double **beliefs_view,
                   int32_t *sweeps_out, double *residual_out);
int bn_bp_copy_beliefs(bn_engine *eng, double *beliefs_out);

/*
 * Several evidence sets on ONE network in one call -- an extension beside the drop-in: the reference's
 * operator() (belief_propagation.hpp:31) takes one query at a time, and each set here gets exactly the
 * result that call would give it (same sweep count, same bits).  Networks the resident kernel covers
 * (bn_set_option "multisweep") run up to 4 sets per launch, walked round-robin: one resident CPT image
 * serves every set and each set's grid barrier completes while the others compute (more sets: consecutive
 * launches).  Every other network runs ALL sets in each per-sweep launch (one evidence set per blockIdx.y):
 * B queries share the launch, its latency and the CPT lines in the caches; a set that has converged drops
 * out of the following launches.  n_sets in 1..BN_MAX_BATCH_SETS.
 *   ne[n_sets]           : evidence nodes per set
 *   ev_node, ev_val      : the sets' arrays concatenated
 *   ev_off               : per set a block of ne[q] + 1 offsets STARTING AT 0, blocks concatenated
 *   beliefs_out          : [n_sets][sum k]; sweeps_out / residual_out : [n_sets]
 * bn_bp_set_evidence_batch + bn_bp_run_batch_device + bn_bp_copy_beliefs_batch == bn_bp_run_batch, with the
 * inputs and outputs left resident in HBM in between (bench.py times the middle call).
 */
int bn_bp_run_batch(bn_engine *eng, int32_t n_sets, const int32_t *ne, const int32_t *ev_node, const int32_t *ev_off,
                    const double *ev_val, double eps, int32_t max_sweeps, double *beliefs_out, int32_t *sweeps_out,
                    double *residual_out);
int bn_bp_set_evidence_batch(bn_engine *eng, int32_t n_sets, const int32_t *ne, const int32_t *ev_node,
                             const int32_t *ev_off, const double *ev_val);
int bn_bp_run_batch_device(bn_engine *eng, double eps, int32_t max_sweeps, int32_t *sweeps_out, double *residual_out);
int bn_bp_copy_beliefs_batch(bn_engine *eng, double *beliefs_out);
int bn_bp_residual_history_batch(bn_engine *eng, int32_t set, double *out, int32_t cap);

/* Diagnostics of the last bn_bp_run*: per-sweep maximum_difference (returns the count written),
 * and the final pi / lambda messages in CSR edge order (each sum_e k[parent(e)] doubles). */
int bn_bp_residual_history(bn_engine *eng, double *out, int32_t cap);
int bn_bp_messages(bn_engine *eng, double *pi_msg_out, double *lambda_msg_out);

/*
 * Most probable explanation (MPE / MAP, Pearl's belief revision): MAX-PRODUCT belief propagation -- an extension beside the
 * drop-in, the reference has no such functor.  The loop is belief_propagation.hpp:33-158 with one line changed: pi(v) (:174-200)
 * and the lambda-message to a parent (:240-266) take the LARGEST term over the parent assignments where sum-product adds them;
 * products, normalisation, evidence, residual, the strict `<` of the stop decision and belief = normalize(pi % lambda) are
 * unchanged.  Exact on polytrees once the messages have crossed the graph; on loopy networks an approximation that may oscillate.
 *   The fold:   acc = +0.0; for every term x: acc = (acc < x) ? x : acc -- a NaN term never replaces acc, the order of the
 *               terms does not matter.
 *   The state:  of the node's normalised max-marginal vector b: idx = 0, best = b[0]; for i = 1..k-1: if (b[i] > best) take i
 *               -- the LOWEST index holding the largest element; a vector of NaNs (all-zero evidence: 0 / 0) gives state 0.
 *   max_sweeps: 0 means a cap of 10 000 sweeps, NOT unbounded as in bn_bp_run: a loopy max-product run need not converge, and
 *               a loop without an end on the device is a hang.  converged_out: 1 = maximum_difference < eps, 0 = cut by the cap.
 * Evidence arguments and their checks are those of bn_bp_run / bn_bp_run_batch (layout of the batch arrays: see there).
 *   max_marginals_out : [sum k] (batch: [n_sets][sum k]) node-major, each node's vector normalised
 *   states_out        : [n]     (batch: [n_sets][n])     the decoded state of every node, evidence nodes included
 *   sweeps_out / residual_out / converged_out : one value (batch: [n_sets]); may be NULL
 * Two forms (bn_get_info "mpe_form": the one the next run takes, 0 none; "mpe_last_form"): 1 = networks that fit ONE workgroup
 * (the "small" plan: the whole run in one launch, state in LDS; a batch runs one workgroup per set), 2 = networks of the "mid"
 * plan (several workgroups, state in device memory, one launch per sweep, stop decision on the device; a batch runs set after
 * set).  Networks with neither plan -- a node with more than 8 parents, more than 224 workgroups' worth -- sharded engines and
 * BN_DEVICE_HOST_ONLY engines: BN_ERR_STATE, bn_last_error names the limit.  bn_set_option "mpe_form" 0 (default: form 1 where
 * eligible, else 2) / 1 / 2: forcing a form the network is not eligible for gives BN_ERR_STATE at the run (2 on a network that
 * fits one workgroup: the engine keeps no "mid" plan for those, max-product builds one of its own at the first use;
 * bn_get_info "mpe_parts": the workgroups of form 2); "mpe_group" 1..64: form 2 enqueues that many sweeps between two reads of
 * its control record (default 16, chosen by measurement: DESIGN 4.16).
 * A bn_mpe_* call leaves everything the bn_bp_* calls use as it was -- evidence in force, batch staging, bn_bp_messages,
 * bn_bp_last_path -- and the other way round; bn_reload_cpt reaches the tables of both.
 * bn_mpe_residual_history: per-sweep maximum_difference of set `set` of the last bn_mpe_run* (returns the count written);
 * bn_mpe_messages: final pi / lambda messages of the last bn_mpe_run (not of a batch), laid out as by bn_bp_messages.
 */
int bn_mpe_run(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_off, const double *ev_val, double eps,
               int32_t max_sweeps, double *max_marginals_out, int32_t *states_out, int32_t *sweeps_out, double *residual_out,
               int32_t *converged_out);
int bn_mpe_run_batch(bn_engine *eng, int32_t n_sets, const int32_t *ne, const int32_t *ev_node, const int32_t *ev_off,
                     const double *ev_val, double eps, int32_t max_sweeps, double *max_marginals_out, int32_t *states_out,
                     int32_t *sweeps_out, double *residual_out, int32_t *converged_out);
int bn_mpe_residual_history(bn_engine *eng, int32_t set, double *out, int32_t cap);
int bn_mpe_messages(bn_engine *eng, double *pi_msg_out, double *lambda_msg_out);

/*
 * Expectation-maximisation: CPTs fitted from a table with UNOBSERVED cells -- an extension beside the drop-in (sampler::make_cpt and
 * bn_fit_cpt count complete rows only).  The E-step is belief propagation: every pattern row is one sum-product query with the
 * observed cells as hard evidence, one workgroup per row on the one-workgroup path, and from the state each run stops in the family
 * posteriors P(x_v, pa(v) | e) are taken and added, weighted by the row's count; the M-step normalises.  All in fp64.
 *   patterns [n_patterns][n_nodes] uint8 and counts [n_patterns] uint64 are bn_fit_cpt's layout; a cell of BN_EM_MISSING (255) is
 *   "not observed".  A row may be fully observed, fully missing or have count 0.  BN_ERR_ARG (checked on the host, before any device
 *   work): a cell >= k[v] that is not 255 (the text names the pattern and the node), n_patterns < 1, a null pointer, a zero total.
 * E-step, per pattern, under the current tables: one-hot evidence on the observed nodes; the loop of bn_bp_run with (bp_eps,
 *   bp_max_sweeps) -- bp_max_sweeps == 0 means a cap of 10 000 sweeps, NOT unbounded (as bn_mpe_run); a run cut by the cap is used as
 *   it stands and counted -- with the bits of bn_bp_run on the one-workgroup path; then for every node v, parent assignment a (first
 *   parent most significant) and own state i
 *       t'[a,i] = cpt[a,i] x the parents' final pi-messages at a, ascending parents   (the term pi(v)[i]'s sum adds)
 *       r[i] = sum_a t'[a,i] in table order;  s = sum_i r[i] x lambda(v)[i];  b[a,i] = (t'[a,i] x lambda(v)[i]) / s
 *   (all sums front to back from +0.0).  Where `s > 0` is false -- the evidence has probability 0 under the tables -- the family
 *   contributes nothing and is counted.  E[q] = sum_p double(counts[p]) x b_p[q], added in blocks of 256 consecutive patterns:
 *   inside a block in increasing p from +0.0, the block sums in increasing order from +0.0.  E therefore depends on the ORDER of the
 *   rows, not on how the call cuts them into launches.  On a complete table with strictly positive tables E is the exact counts.
 * M-step: E'[q] = E[q] + prior; per CPT row tot = sum_i E'[a,i] left to right; theta_new = E' / tot, or 1.0 / k[v] for the whole row
 *   where `tot > 0` is false.  With prior = 0 on a complete table: bn_fit_cpt's bits.
 * Loop: delta = max_q |theta_new[q] - theta[q]|; stop after the iteration where delta < tol (strict: tol = 0 never stops early) or
 *   after max_iters (1..10 000) iterations.  Starts from cpt_init (flat, bn_model_desc.cpt's layout) or, if NULL, from the engine's
 *   current tables.  The engine's own tables are never written: apply cpt_out with bn_reload_cpt if wanted.
 *   bn_em_fit: cpt_out [n_entries]; iters_out, delta_hist_out [hist_cap] (the first hist_cap deltas) may be NULL.  BN_ERR_ARG:
 *   max_iters out of range, prior negative or not finite, tol or bp_eps NaN, bp_max_sweeps < 0.
 *   bn_em_expected_counts: ONE E-step under the engine's current tables: ecounts_out [n_entries], sweeps_out [n_patterns] or NULL.
 * Eligible: networks with a one-workgroup plan (bn_get_info "em_eligible"; the "small" option does not matter).  Without one, and on
 * sharded engines: BN_ERR_STATE, bn_last_error gives the planner's reason.  BN_DEVICE_HOST_ONLY engines: BN_ERR_NO_DEVICE, after the
 * argument checks.  A bn_em_* call leaves everything the bn_bp_* / bn_mpe_* calls use as it was.
 * bn_get_info: "em_last_iters"; "em_capped" / "em_skipped": pattern-runs cut by the cap / pattern-families with s not > 0 in the last
 * call, summed over its iterations; "em_estep_ns" / "em_mstep_ns": device time of the last call's E-step / M-step kernels.
 * bn_set_option "em_scratch_cells": doubles of the scratch array that holds one launch's posteriors (0: the default, 2^22); it
 * bounds the rows per launch and changes no result.
 */
#define BN_EM_MISSING 255
typedef struct bn_em_options {
    int32_t max_iters;
    double tol;
    double bp_eps;
    int32_t bp_max_sweeps;
    double prior;
} bn_em_options;
int bn_em_expected_counts(bn_engine *eng, int64_t n_patterns, const uint8_t *patterns, const uint64_t *counts, double bp_eps,
                          int32_t bp_max_sweeps, double *ecounts_out, int32_t *sweeps_out);
int bn_em_fit(bn_engine *eng, int64_t n_patterns, const uint8_t *patterns, const uint64_t *counts, const bn_em_options *opt,
              const double *cpt_init, double *cpt_out, int32_t *iters_out, double *delta_hist_out, int32_t hist_cap);

/*
 * Exact inference: junction-tree (clique-tree) propagation -- an extension beside the drop-in.  bn_bp_run is exact on polytrees
 * and an approximation on networks with loops; this path is exact on every network whose clique tree fits: Hugin-style two-pass
 * propagation in fp64, one workgroup per evidence set, the whole query in one launch.
 * Evidence arguments and their checks are those of bn_bp_run / bn_bp_run_batch (layout of the batch arrays: see there), but
 * evidence is a LIKELIHOOD here, hard or soft: the answer is normalise(P(x_v, e)) for EVERY node, evidence nodes included -- not
 * the reference BP's treatment, where an evidence node's belief is e^2 / sum(e^2) and soft evidence enters pi and lambda both.
 * For one-hot evidence on a polytree the two agree.
 *   beliefs_out      : [sum k] (batch: [n_sets][sum k]) node-major; P(e) = 0 gives NaN (0 / 0: no zero guard)
 *   log_evidence_out : one value (batch: [n_sets]), may be NULL: log P(e) = the std::log of the scales added in array order;
 *                      -inf when a factor is 0
 *   bn_jt_scales     : the scale array of set `set` of the last run, [jt_cliques] in clique id order (returns the count written):
 *                      per clique the sum its message to the parent was divided by, per root the total; their product is P(e).
 *                      set = -1: every set's, [n_sets][jt_cliques] (cap must hold them all)
 * The plan (built at the first call that asks for it; pure host work, also on BN_DEVICE_HOST_ONLY engines): moral graph, min-fill
 * elimination (ties: smaller table of node + neighbours, then lower node id), the MAXIMAL cliques, a clique forest with every tree
 * rooted at its centre, cliques numbered level by level.  Variables of a clique or separator: ascending node id, first most
 * significant.  Each CPT goes to one clique that holds its family; each node has one home clique, which receives its evidence
 * vector and is where its marginal is read.
 *   bn_jt_plan_dims: dims_out[12] = eligible, cliques, levels, potential entries, separator entries (a root counts one), state
 *     cells (potentials + separators + sum k + cliques), largest clique table, its variable count, sum of the cliques' variable
 *     counts, sum of the separators', terms per run of a two-level sum (64), the form of the next run.
 *   bn_jt_plan_dump (any pointer may be NULL): order [n] the elimination order; parent, level [cliques] (-1 / 0: a root);
 *     var_ptr [cliques + 1] into vars; sep_ptr [cliques + 1] into sep_vars (a root has none); cpt_clique, home [n].
 * The arithmetic (every order depends on the plan only; tests/jtree_refs.py restates it bit for bit):
 *   two-level sum: runs of 64 consecutive terms, each added left to right from +0.0, then the run sums left to right from +0.0;
 *   base potential of a clique = 1.0 x its CPTs' entries, ascending node id (computed on the device once, and after bn_reload_cpt);
 *   per query: x the evidence vectors of the clique's home nodes, ascending node id;
 *   collect, deepest level first: raw separator entry = two-level sum of the clique's matching entries, ascending entry index;
 *     s = the separator's entries added left to right from +0.0 (the clique's scale); message = raw / s where s > 0, else raw; the
 *     parent's entries multiply their children's messages in, ascending child id; a root's scale = two-level sum of all its entries;
 *   distribute, top level first: new = two-level sum of the parent's matching entries; ratio = new / message, exactly 0 where the
 *     message is 0; the child's entries are multiplied by it;
 *   read-out: u[x] = two-level sum of the home clique's entries with x_v = x; belief = u[x] / (u[0] + u[1] + ... left to right).
 * Limits are facts of the plan, not failures of bn_create: an elimination clique of more than 2^20 entries, or a per-set state
 * above option "jt_scratch_cells" (doubles; 0 = the default, 2^22), make the network ineligible: BN_ERR_STATE at the run, with the
 * planner's reason (it names the clique, its variable count and its size).  Sharded engines: BN_ERR_STATE.  BN_DEVICE_HOST_ONLY
 * engines: BN_ERR_NO_DEVICE, after the argument checks (BN_ERR_ARG) and the plan's.
 * Two forms from one plan, the same bits: 1 = the set's state in LDS (states of at most 8192 doubles), 2 = in a slice of device
 * scratch; a batch in form 2 launches as many sets as the scratch holds and queues the launches behind each other.  Option
 * "jt_form" 0 (default: 1 where it fits) / 1 / 2; forcing form 1 on a plan that does not fit gives BN_ERR_STATE at the run.
 * bn_get_info: "jt_eligible" (builds the plan), "jt_form" (of the next run, 0 none), "jt_last_form", "jt_last_launches",
 * "jt_cliques", "jt_max_clique", "jt_state_cells", "jt_levels"; with option "timing" 1, "jt_last_kernel_ns": HIP events around the
 * last run's launches.
 * A bn_jt_* call leaves everything the bn_bp_* / bn_mpe_* / bn_em_* calls use as it was; bn_reload_cpt reaches its potentials.
 */
#define BN_JT_MAX_BATCH_SETS 65536
int bn_jt_run(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_off, const double *ev_val, double *beliefs_out,
              double *log_evidence_out);
int bn_jt_run_batch(bn_engine *eng, int32_t n_sets, const int32_t *ne, const int32_t *ev_node, const int32_t *ev_off,
                    const double *ev_val, double *beliefs_out, double *log_evidence_out);
int bn_jt_scales(bn_engine *eng, int32_t set, double *out, int32_t cap);

/*
 * Exact MPE: max-propagation with backtracking on the junction tree -- the pair of bn_jt_run as bn_mpe_run is the pair of
 * bn_bp_run.  bn_mpe_run (max-product loopy BP) is exact on polytrees only and decodes node by node: where two joint assignments
 * tie, the per-node argmaxes may combine into an assignment that is no maximiser (node 0 uniform, node 1 = "not node 0": both
 * max-marginals are [0.5, 0.5], per-node decoding gives (0, 0), which has probability 0).  This call is exact on every network
 * the junction tree takes, and decodes by backtracking: its assignment always attains the maximum it reports.
 * Arguments, evidence (a LIKELIHOOD, hard or soft), their checks, the plan, the two forms, the options, the batch rules and the
 * errors are those of bn_jt_run / bn_jt_run_batch: BN_ERR_ARG first; BN_ERR_STATE with the planner's reason on ineligible or
 * sharded engines or a forced form that does not fit; BN_ERR_NO_DEVICE on BN_DEVICE_HOST_ONLY engines after both.
 *   max_marginals_out : [sum k] (batch: [n_sets][sum k]) node-major, each node's vector normalised; P(e) = 0 gives NaN
 *   states_out        : [n] (batch: [n_sets][n]): the most probable joint assignment x*, evidence nodes included.  With
 *                       P(e) = 0 the states are what the rule below gives: defined, and meaningless
 *   log_p_out         : one value (batch: [n_sets]), may be NULL: log max_x P(x, e) = the std::log of the scales added in
 *                       clique order; -inf when a factor is 0
 * The arithmetic, fp64 without contraction (tests/jtmpe_refs.py restates it: states, max-marginals and scales bit for bit):
 *   max fold of terms: acc = +0.0, then acc = x if acc < x else acc -- a NaN never replaces acc, so the result is the largest term
 *     above +0.0, else +0.0, whatever the order: this pass states no order of its folds;
 *   potentials: as bn_jt_run;
 *   collect, deepest level first: raw separator entry = max fold of the clique's matching entries; s = max fold of the
 *     separator's entries (the clique's scale); message = raw / s where s > 0, else raw; the parent's entries multiply their
 *     children's messages in, ascending child id; a root's scale = max fold of all its entries;
 *   distribute, top level first: ratio = (max fold of the parent's matching entries) / message, exactly 0 where the message is
 *     0; the child's entries are multiplied by it;
 *   max-marginals: u[x] = max fold of the home clique's entries with x_v = x; output u[x] / (u[0] + u[1] + ... left to right
 *     from +0.0), no zero guard (bn_mpe_run's normalisation);
 *   decode: a root picks the lowest entry index of its largest entry (best = t[0]; t[i] > best takes i); a child picks, among
 *     its entries that agree with its parent's pick on the separator, the lowest entry index of the largest one -- the child's
 *     entries AS THEY STAND AFTER COLLECT, before its own distribute multiply, so that ties are not disturbed by the rounding of
 *     a ratio; state of node v = its digit in the pick of its home clique.
 * A limit: after distribute a clique's table carries the scales of the cliques on its path to the root, each a maximum below 1;
 * on a tree more than about a thousand levels deep they underflow and the max-marginals of deep nodes are 0 / 0 = NaN.  The
 * states and log_p are not affected: the picks read the tables as collect left them.
 * bn_jt_scales reports the scales of the last bn_jt_* run of either kind (a max run: their product is max_x P(x, e)).
 * bn_get_info "jt_last_kind": 0 none, 1 a sum run (bn_jt_run*), 2 a max run (bn_jt_mpe_run*); "jt_last_form", "jt_last_launches"
 * and "jt_last_kernel_ns" are updated as for a sum run.
 */
int bn_jt_mpe_run(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_off, const double *ev_val,
                  double *max_marginals_out, int32_t *states_out, double *log_p_out);
int bn_jt_mpe_run_batch(bn_engine *eng, int32_t n_sets, const int32_t *ne, const int32_t *ev_node, const int32_t *ev_off,
                        const double *ev_val, double *max_marginals_out, int32_t *states_out, double *log_p_out);

/*
 * Exact EM: bn_em_fit with its E-step taken from the junction tree -- the pair of bn_em_fit as bn_jt_run is the pair of bn_bp_run.
 * bn_em_fit's family posteriors come from loopy belief propagation and are P(x_v, pa(v) | e) on polytrees only; here they are
 * exact on every network the junction tree takes.  One workgroup per pattern row, the row's state in LDS (form 1) or device
 * scratch (form 2), as bn_jt_run_batch.  All in fp64; every sum but the row log-likelihood has a stated order that depends on
 * the plan only (tests/jtem_refs.py restates it: E, the tables after every iteration, the deltas and the skipped count are
 * equal bit for bit).
 *   The table is bn_em_fit's: patterns [n_patterns][n_nodes] uint8, counts [n_patterns] uint64, BN_EM_MISSING for a cell that is
 *   not observed; rows may be fully observed, fully missing or have count 0.  Its checks, their texts and their order are
 *   bn_em_fit's (without bp_eps and bp_max_sweeps).
 * E-step per row, under the current tables theta: the base potentials are computed from theta once per iteration, into an array of
 *   the call's own; an observed node multiplies the entries of its home clique by 1.0 where its digit equals the cell and by 0.0
 *   elsewhere (ascending node id) -- the bits of bn_jt_run with a one-hot vector; collect and distribute as bn_jt_run.
 * Family read-out: node v's CPT lies in the clique cpt_clique[v] (bn_jt_plan_dump), which holds v and its parents.  For a flat CPT
 *   entry q of v (first parent most significant, own state last): u[q] = two-level sum (runs of 64) of that clique's entries whose
 *   digits match q, in ascending entry index; s_v = two-level sum of u[q] over v's entries in flat order; b[q] = u[q] / s_v where
 *   s_v > 0.  Where `s_v > 0` is false the family contributes nothing and is counted.  A fully observed family has one non-zero u,
 *   so b is exactly 1.0: on a complete table with strictly positive tables E is the exact counts and the M-step has bn_fit_cpt's
 *   bits.
 * Row log-likelihood: ll_p = sum over the cliques of log(scale), -inf when a factor is 0; computed on the device (its log is not
 *   libm's), added in no stated order -- the one quantity that is not pinned bit for bit.
 *   L = sum_p (counts[p] > 0 ? double(counts[p]) x ll_p : 0.0): the observed-data log-likelihood of the table.
 * E[q] = sum_p double(counts[p]) x b_p[q] in bn_em_fit's order (blocks of 256 consecutive patterns); the M-step, delta and the stop
 *   rule (strict delta < tol, max_iters in 1..10 000) are bn_em_fit's, bit for bit.  L is reported and does not steer the loop.
 *   bn_jt_em_expected_counts: ONE E-step under the engine's current tables: ecounts_out [n_entries]; row_loglik_out [n_patterns]
 *     (ll_p) or NULL.
 *   bn_jt_em_fit: starts from cpt_init or, if NULL, the engine's current tables; cpt_out [n_entries]; iters_out, delta_hist_out
 *     [hist_cap] and loglik_hist_out [hist_cap] may be NULL: entry i of the latter is L under the tables iteration i STARTED from.
 *     The engine's own tables are never written: apply cpt_out with bn_reload_cpt if wanted.
 * Eligible: what the junction tree takes (bn_get_info "jt_eligible"), whatever the one-workgroup plan of bn_em_fit says; options
 * "jt_form" and "jt_scratch_cells" hold as for bn_jt_run_batch.  Errors follow bn_jt_run: BN_ERR_ARG first; BN_ERR_STATE with the
 * planner's reason on ineligible or sharded engines or a forced form that does not fit; BN_ERR_NO_DEVICE on BN_DEVICE_HOST_ONLY
 * engines after both.
 * bn_get_info: "jt_em_last_iters"; "jt_em_skipped": row-families with s_v not > 0 in the last call, summed over its iterations;
 * "jt_em_estep_ns" / "jt_em_mstep_ns": device time of the last call's E-steps (potentials included) / M-steps; "jt_em_last_form";
 * "jt_em_last_launches": launches of jt_em_kernel per E-step.  bn_set_option "jt_em_scratch_cells": doubles of the scratch array
 * that holds one launch's posteriors (0: the default, 2^22); it bounds the rows per launch -- as "jt_scratch_cells" does in form
 * 2 -- and changes no result.
 * A bn_jt_em_* call leaves everything the other call families use as it was: the engine's potentials, the scales bn_jt_scales
 * reports, "jt_last_kind" and the other "jt_last_*" values among it.
 */
typedef struct bn_jt_em_options {
    int32_t max_iters;
    double tol;
    double prior;
} bn_jt_em_options;
int bn_jt_em_expected_counts(bn_engine *eng, int64_t n_patterns, const uint8_t *patterns, const uint64_t *counts, double *ecounts_out,
                             double *row_loglik_out);
int bn_jt_em_fit(bn_engine *eng, int64_t n_patterns, const uint8_t *patterns, const uint64_t *counts, const bn_jt_em_options *opt,
                 const double *cpt_init, double *cpt_out, int32_t *iters_out, double *delta_hist_out, double *loglik_hist_out,
                 int32_t hist_cap);

int bn_jt_plan_dims(bn_engine *eng, int64_t *dims_out);
int bn_jt_plan_dump(bn_engine *eng, int32_t *order, int32_t *parent, int32_t *level, int32_t *var_ptr, int32_t *vars, int32_t *sep_ptr,
                    int32_t *sep_vars, int32_t *cpt_clique, int32_t *home);

/* Options: "timing" 1/0 -- HIP events on the engine's stream around every batch of sweep launches
 * (bn_bp_stats.sweep_kernel_ms).  Default 0 (BN_TIMING=1 in the environment turns it on): an event
 * record between two launches opens a bubble of several microseconds in the queue, so a timed run is
 * slower than an untimed one; bn_bp_stats.sweep_devclock_ms -- the device's 100 MHz clock read by the
 * kernels themselves at the first sweep's start and the last sweep's end -- costs nothing and is always on.
 * "overlap" 1/0 -- sharded runs: launch the interior tiles of a sweep while the previous sweep's
 *   all-gather is in flight on a second stream (default 1; BN_OVERLAP=0), or kernel and collective
 *   back to back on one stream.
 * "multisweep" 0/1/2 -- the one-launch path (BN_MULTISWEEP in the environment sets the default, 1):
 *   networks of one-lane tiles (uniform arity 2..4, <= 2 parents, <= 8 children per node) that fit the chip
 *   can run the whole run in ONE launch with CPTs, references and node vectors resident in registers / LDS
 *   and a grid barrier per sweep.  0 = always one launch per sweep; 1 = that path where it was measured
 *   faster (one-block networks, networks of >= 600 tiles); 2 = wherever eligible (tests, experiments).
 *   Results are bit-identical on either path.
 * "small" 0/1/2 -- SMALL networks (the state fits one CU's LDS: up to a few thousand CPT entries, <= 8 parents per
 *   node -- ALARM-sized): the whole run in ONE workgroup with messages, node vectors and staged terms in LDS, one
 *   work item per CPT entry / per message element instead of one wavefront per handful of nodes; sums and
 *   products in the reference's order for any table size, i.e. bit-identical to the CPU restatement.  0 = never,
 *   1 = where eligible and not measured slower than the resident tiles (default: everything eligible except long chains /
 *   trees and two-round networks the resident kernel runs in one block; "multisweep" 0 also turns it off), 2 = wherever
 *   eligible.  bn_bp_run_batch on such a network runs one workgroup per evidence set, all sets in one launch.
 *   bn_get_info "small_eligible".
 * "mid" 0/1/2 -- MID-SIZE networks (beyond one workgroup's LDS, up to 224 workgroups' worth: a few hundred to ten thousand nodes
 *   of mixed arity with <= 8 parents): the same items as "small", spread over several workgroups by node ranges, state in
 *   device memory, a grid barrier per iteration, one launch per run; bit-identical to the CPU restatement as well.  0 = never,
 *   1 = where eligible and not measured slower than the resident tiles (default: everything the resident tiles do not cover,
 *   and k = 4 networks with two parents per node), 2 = wherever eligible.  bn_bp_last_path = 4.
 *   Batches run as many sets per launch as fit the chip.  bn_get_info "mid_eligible", "mid_parts", "mid_aborts".
 * "flow" 1/0 -- resident path, one evidence set, more than one tile block (BN_RESIDENT_FLOW sets the default, 0):
 *   1 = dataflow form: a tile waits for the tiles it exchanges messages with instead of for a grid barrier, and
 *   the stop decision lags one iteration behind; 0 = grid barrier per sweep.  Same bits either way.
 * "direct" 1/0 -- resident path, grid-barrier form, one evidence set (BN_RESIDENT_DIRECT sets the default, 1): 1 = every tile block
 *   reads all blocks' arrival words itself and takes the stop decision (one hand-off per barrier); 0 = a service block collects
 *   them and publishes the decision (two).  Same bits.
 * "memo0" 1/0 -- resident path, grid-barrier form, one evidence set (BN_MEMO0 sets the default, 1): sweep 0 of a run reads no message,
 *   so what it leaves behind -- every node's first messages and vectors -- depends on the CPTs and, node by node, on the node's own
 *   evidence alone.  1 = the engine keeps that state in device memory (one more record and node buffer; built by the first run that
 *   can use it, rebuilt after bn_reload_cpt), the launch that applies an evidence set recomputes the slots of the set's nodes and of the
 *   nodes it drops, and a run starts at sweep 1; 0 = every run executes sweep 0.  Same sweep counts, residual histories and bits either
 *   way; runs with max_sweeps 1 or eps above sweep 0's residual execute sweep 0 regardless.  bn_get_info "memo0_active" (the image
 *   exists and is in use), "memo0_bytes"; bn_bp_stats.memo_sweeps tells what the last run did.
 * "memo1" 1/0 -- the same one sweep further (BN_MEMO1 sets the default, 1): what sweep 1 leaves at a node depends on the CPTs and on the
 *   evidence of the node's closed neighbourhood (itself, its parents, its children) alone.  1 = the engine also keeps the state behind
 *   sweep 1 (one more record and node buffer, a node-level adjacency), a launch behind the one that applies an evidence set recomputes
 *   the closed neighbourhoods of the set's nodes and of the nodes it drops, and a run starts at sweep 2; 0 = runs start at sweep 1.
 *   Same sweep counts, residual histories and bits either way.  Runs with max_sweeps 1 or 2, or eps above what sweep 1's residual
 *   is known to reach, start earlier; a set whose patch would cost more than a sweep (BN_MEMO1_LIMIT, in threads) does not patch, and
 *   runs start at sweep 1 until a smaller set arrives.  bn_get_info "memo1_active"; bn_bp_stats.memo_depth tells what the last run did.
 * "poll_sleep" n -- dataflow form: pause between two polls of a waiting tile, n x 512 cycles (default 2).
 * "beliefs_direct" 1/0 -- bn_bp_run_view: the kernels write the marginals straight into the engine's mapped host
 *   buffer (default 1, outputs up to 16 MB) instead of a copy command queued behind the run.
 * "dag" 0/1/2 -- networks whose nodes all have arity <= 4 and at most 5 parents (BASELINE configs[1], the 10 k-node random DAG; arities 2
 *   and 3 are padded to 4 with zeros, which leaves the real entries' bits alone): one
 *   launch per run with every CPT entry resident in a register; a node's child role (pi(v), lambda-messages: one wavefront of
 *   nodes / lane groups per tile) and parent role (lambda(v), pi-messages: one lane per message) run on different waves, the state
 *   lives in device memory in CSR edge order, one grid barrier per iteration.  Nodes with <= 2 parents keep the reference's
 *   operation order; with >= 3 parents the contraction is factored (sums over the two trailing parents shared by all outputs):
 *   results agree with the reference to rounding (<= 1e-12; its own products over >= 3 parents are unordered,
 *   belief_propagation.hpp:253).  Networks beyond one tile per wave run the same code walking several tiles per wave ("stream"
 *   form).  0 = never, 1 = where measured faster (default: networks with 3-5-parent nodes, and networks of <= 2-parent nodes that fit
 *   the chip at one tile per wave -- unless the one-workgroup path takes the network, or less than a quarter of the padded tables
 *   is real: binary networks of <= 2-parent nodes), 2 = wherever eligible.
 *   bn_bp_run_batch on such a network: up to 16 evidence sets share a launch and its CPT registers, taking turns inside an iteration;
 *   every set keeps the sweep count and the bits of its single run.
 *   bn_get_info "dag_eligible", "dag_blocks", "dag_tiles", "dag_stream", "dag_aborts".
 * "dagflow" 1 -- single queries on that path run in its DATAFLOW form where the plan has one (one tile per wave, more than one block, at
 *   most 64 neighbour tiles per tile): no grid barrier -- a tile starts its next iteration when the tiles it exchanges messages with
 *   have finished the previous one, one more block takes the stop decision one iteration behind, the one speculative iteration writes
 *   the other buffer.  Same sweep counts and bits as the barrier form.  0 (default): the barrier form -- measured faster on every
 *   network tried but a 64 x 64 grid (EXPERIMENTS.md R6.2).  bn_get_info "dag_flow_eligible" (known once the path has run or its plan
 *   was asked for), "dag_flow_max_nbr", "last_dag_flow".
 * "autotune" 1 -- the NEXT run first times every execution path the engine is eligible for on the evidence in force (one warm-up and
 *   two timed runs of 6 sweeps each, host wall clock) and keeps the fastest for all later runs: the built-in choice between the
 *   paths rests on thresholds measured on a handful of networks on one pool of machines.  The choice is written into the options
 *   above, which can still be set afterwards; bn_get_info "autotuned" (0 / 1) and "autotuned_path" tell.  0 clears a pending
 *   request.  Single-rank engines only.  Exchanging paths may change the last bits of networks with >= 3-parent nodes.
 * bn_bp_last_path: 0 = one launch per sweep, 2 = resident tiles (one launch per run), 3 = one workgroup, state in LDS
 *   (small networks, one launch per run), 4 = the same items over several workgroups (mid-size networks), 5 = register-resident
 *   child tiles + parent items (networks of arity <= 4 with <= 5 parents). */
int bn_set_option(bn_engine *eng, const char *name, int32_t value);
int bn_bp_last_path(bn_engine *eng);
/* Named integer properties (tests, tools): "resident_eligible", "flow_eligible", "last_flow" (1: the last run
 * used the dataflow form), "nbr_max", "nbr_chunks", "resident_blocks", "resident_aborts", "shard_flow" (in-kernel
 * exchange set up), "n_boundary_nodes", "rccl_ranks" (what the RCCL communicator of a sharded engine reports; 0: none), "small_eligible", "small_waves", "small_lds_bytes", "mid_eligible", "mid_parts", "mid_aborts", "dag_eligible", "dag_blocks", "dag_tiles", "dag_stream", "dag_aborts", "autotuned", "autotuned_path", "create_us_plan" / "create_us_small" / "create_us_mid" / "create_us_dag" / "create_us_device" (microseconds bn_create spent on the host plans -- tile layout, one-workgroup, several-workgroup, register-resident DAG -- and on the device side: allocations + uploads; bn_create builds the plan and image of the register-resident DAG path only where the defaults pick that path, elsewhere its image is filled and uploaded by the first run that wants it -- "dag" 2, "autotune", a batch), "lw_small" (1 once a sampler call has run: the straight-line sampling kernel for networks whose every node has <= 4 parents, <= 256 CPT rows and <= 4 states is in use), "lw_last_sample_kernel" (the sampling kernel the last sampler launch ran: 0 none yet; 32 + 2 P + R: the straight-line kernel, P = 1 when every arity is a power of two, R = 1 for rejection sampling; 16 + 4 W + 2 I + R: the generic kernel, W = 1 when every table has fewer than 2^24 rows, I = 1 when node ids fit 24 bits) and "lw_last_hist_kernel" (the histogram kernel launched last: 0 none yet; 2, 4, 8: one byte per state, that many accumulators; 34, 36: two bits per state, 2 or 4 accumulators; 64: the any-arity kernel for arities above 8); unknown name: BN_ERR_ARG.
 * When a one-launch path gives up a bounded wait (its workgroups were not all on the chip: another engine, stream or process uses the
 * GPU) the run is repeated on a slower path; the first such event of an engine prints ONE line on stderr, all are counted. */
int64_t bn_get_info(bn_engine *eng, const char *name);

/* Single steps of a run (tests / diagnostics): begin, one sweep (without exchange), finish.
 * bn_debug_allgather emulates the exchange between n shard engines living on ONE device. */
int bn_bp_step_begin(bn_engine *eng);
int bn_bp_step_sweep(bn_engine *eng, int32_t sweep, double eps);
/* One sweep in the two launches of a sharded run with the exchange overlapped: part 1 = the interior
 * tiles (they read nothing the previous sweep's all-gather delivers, so the engine launches them while
 * that collective is in flight), part 2 = the tiles that touch a cut edge + the residual bookkeeping
 * (launched once the collective has landed); part 0 = both in one launch (bn_bp_step_sweep). */
int bn_bp_step_sweep_part(bn_engine *eng, int32_t sweep, double eps, int32_t part);
int bn_bp_step_finish(bn_engine *eng, int32_t launched, int32_t final_batch, double eps,
                      int32_t *done_out, int32_t *sweeps_out, double *residual_out);
int bn_debug_allgather(bn_engine **engs, int32_t n, int32_t sweep);
/* The achievable HBM rate of a device, measured by the library's own streaming kernels (csrc/bn_stream.hip; 16 bytes per lane,
 * non-temporal loads and stores, HIP events on a stream of its own): mode 0 = copy (bytes read + bytes written), mode 1 = triad
 * (dst = a + s * b: 2 reads + 1 write); `bytes` = size of ONE array (take it well beyond the 256 MiB Infinity Cache); best of `reps`.
 * The yardstick SURVEY.md 8(d) asks for beside the nominal 8 TB/s; the reference has no counterpart.  device = HIP ordinal or
 * BN_DEVICE_CURRENT.  *gbs_out in GB/s. */
int bn_debug_stream(int32_t device, int32_t mode, int64_t bytes, int32_t reps, double *gbs_out);

typedef struct bn_bp_stats {
    int32_t sweeps;            /* iterations of the last run                                */
    int32_t sweep_launches;    /* sweep kernels launched (>= sweeps; extras exit at once)    */
    float sweep_kernel_ms;     /* HIP-event time over all sweep launches of the last run ("timing" on) */
    float total_ms;            /* host wall time of the last bn_bp_run_device call           */
    int64_t algorithmic_bytes_per_sweep; /* SURVEY.md 8(d) formula                           */
    int64_t layout_bytes_per_sweep;      /* bytes the sweep kernel actually requests         */
    int64_t messages_per_sweep;          /* 2E                                              */
    float sweep_devclock_ms;   /* device clock: first sweep's start -> last executed sweep's end */
    int32_t resident_aborts;   /* resident launches that gave up a bounded wait, over the engine's life: each sends
                                  the following runs down the per-sweep launches for a while (8, 16, ... runs) */
    int32_t memo_sweeps;       /* sweeps of the last run that were taken from the first-sweep image instead of being executed
                                  (option "memo0"): 0 or 1.  `sweeps` counts them all the same */
    int32_t memo_depth;        /* sweeps of the last run taken from stored images (options "memo0", "memo1"): 0, 1 or 2 */
} bn_bp_stats;
int bn_bp_last_stats(bn_engine *eng, bn_bp_stats *out);

/*
 * Likelihood weighting.
 * Replaces: likelihood_weighting::operator()(evidence, sample_num) (likelihood_weighting.hpp:28-59).
 * Returns the UN-normalised weighted histogram [sum k] (node-major) of samples
 * [sample_begin, sample_begin + n_samples) so that several GPUs / calls can be summed; the
 * caller applies the reference's normalise rule (:197-221).  Every sample id owns one
 * xoshiro128++ stream seeded by a Philox4x32-10 block keyed by (`seed`, sample id) and advanced by one step per topological position
 * (oracle/lw_oracle.c states the mapping; the reference seeds an mt19937 from std::random_device, :224-244).
 */
int bn_lw_run(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_state,
              uint64_t sample_begin, uint64_t n_samples, uint64_t seed, double *hist_out);
/* The same over every rank of the communicator (bn_comm_init): the range [sample_begin,
 * sample_begin + n_samples_total) is split evenly, each GPU draws its share, one RCCL all-reduce
 * sums the histograms; every rank receives the total in hist_out. */
int bn_lw_run_allreduce(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_state,
                        uint64_t sample_begin, uint64_t n_samples_total, uint64_t seed, double *hist_out);
/*
 * Rejection (logic) sampling.
 * Replaces: rejection_sampling::operator()(condition, generate_sample_num)
 * (rejection_sampling.hpp:33-62): forward samples are drawn in index order until n_accept of them
 * agree with every (node, state) pair; counts_out [sum k] holds the state counts of exactly those
 * n_accept samples (the caller divides by the accepted count).  The reference loops forever when
 * the condition has probability zero; here at most max_draw samples are drawn and the numbers
 * actually drawn / accepted are reported.
 */
int bn_rs_run(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_state,
              uint64_t sample_begin, uint64_t n_accept, uint64_t max_draw, uint64_t seed,
              double *counts_out, uint64_t *drawn_out, uint64_t *accepted_out);
/*
 * Maximum-likelihood CPTs from a table of joint patterns.
 * Replaces: sampler::load_sample(table) + sampler::make_cpt(graph) (bayesian/sampler.hpp:29-37,
 * 81-163) -- the consumer of likelihood_weighting::make_samples' pattern table.
 *   patterns [n_patterns][n_nodes] : state of every node in each distinct pattern
 *   counts   [n_patterns]          : occurrences of each pattern
 *   structure                      : k / in_ptr / in_idx / cpt_off / device of the model; its `cpt`
 *                                    is not read (the graph has no CPTs yet) and may be NULL
 *   cpt_out                        : the fitted flat CPTs (layout of bn_model_desc.cpt); a row no
 *                                    pattern supports is uniform (:140-146)
 * An empty table (the reference's `return false`, :83) is BN_ERR_ARG.
 */
int bn_fit_cpt(const bn_model_desc *structure, int64_t n_patterns, const uint8_t *patterns,
               const uint64_t *counts, double *cpt_out);
/* Sampled states of the first `n` samples of the last bn_lw_run, sample-major [s][node]. */
int bn_lw_states(bn_engine *eng, uint64_t n, uint8_t *states_out, double *weights_out);

/*
 * Gibbs sampling: independent Markov chains over the states of all nodes, hard evidence clamped.  The reference has no
 * counterpart.  Unlike likelihood weighting and rejection sampling, which draw from the prior, a chain moves inside the evidence:
 * it converges where P(e) is small, on networks too dense for the junction tree.
 * Runs sweeps [sweep_begin, sweep_begin + n_sweeps) of chains [chain_begin, chain_begin + n_chains) (64-bit chain ids).
 *   Start: init_states == NULL: chain c starts from the states bn_lw_run with the same `seed` and evidence draws for sample id c
 *     (the weight is ignored): bn_lw_states after a bn_lw_run of the same range returns exactly the chains' starting states.  The
 *     call uses the sampler to draw them, so it leaves the sampler's last batch as that bn_lw_run would.  init_states
 *     [n_chains][n]: those; evidence nodes are overwritten by their clamp; a state >= the node's arity elsewhere is BN_ERR_ARG.
 *   Scan order: the moral graph (a node joined to its parents, its children and its children's other parents) is coloured once
 *     per engine, whatever the evidence: nodes in ascending index, each takes the smallest colour no moral neighbour holds.  A
 *     sweep visits the colours 0, 1, ... and inside a colour every free node.  Nodes of one colour share no family: the GPU
 *     updates them at once, which equals the sequential scan in (colour, node index) order.
 *   One update of node v, fp64, no contraction: for x = 0 .. k[v] - 1
 *       w[x] = cpt_v[row_v][x] x cpt_c[row_c(x)][s_c] for every child c of v in ascending child index (one multiply each);
 *       row_c(x) is c's row with v at x, first parent most significant;
 *     T = w[0] + w[1] + ... left to right.  T not a finite number above 0: the state is kept and `stuck` goes up by one.  Else
 *     t = u x T (one multiply) and the new state is the first x with t < c_x, c_x the same running sum; none: the last x with
 *     w[x] > 0.
 *   The uniform is a pure function of (seed, chain c, sweep g, node v): ONE Philox4x32-10 block, counter {v, g, c_lo, c_hi}, key
 *     {seed_lo, seed_hi ^ 0x47494253} (the tag keeps these blocks apart from the sampler's stream seeds);
 *     U = (out0 << 21) | (out1 >> 11), u = U x 2^-53.  g is the global sweep number, below 2^32 (else BN_ERR_ARG).
 *   Kept: after sweep g with g >= burn_in and (g - burn_in) % thin == 0 every node's state (evidence nodes too) adds 1 to
 *     counts_out[node_off[v] + state]: unsigned 64-bit counts, the same whatever the order of the additions.
 *     *kept_out = kept sweeps x n_chains: marginals are counts / kept.  *stuck_out: updates that kept the state because T was
 *     not a finite number above 0 (a start that contradicts the evidence in a network with zeros).  Both may be NULL.
 *   states_out (may be NULL) [n_chains][n]: the states after the last sweep.  n_sweeps == 0: the starting states, zero counts.
 *   Continuity: sweeps [0, a) and then [a, b) from the first run's states_out (sweep_begin = a) give the states of one run of
 *     [0, b), and the two counts add up to its counts; disjoint chain ranges add up the same way (several GPUs, several calls).
 * thin == 0, an unknown evidence node or state, a node listed twice: BN_ERR_ARG.
 * Eligible (bn_get_info "gibbs_eligible"; bn_gibbs_plan_info): n <= 4096 nodes and arities summing to <= 8192 -- a chain's states and
 * a workgroup's histogram live in LDS; beyond, and on sharded engines, BN_ERR_STATE with the planner's reason in bn_last_error and
 * no launch.  BN_DEVICE_HOST_ONLY engines: BN_ERR_NO_DEVICE.  The plan is built at first use and survives bn_reload_cpt, after
 * which the runs read the new tables.  A run is split into launches of at most bn_set_option "gibbs_sweeps_per_launch" sweeps
 * (0: the default, bn_get_info "gibbs_sweeps_per_launch": up to 256, fewer where a sweep reads many table entries); the chains'
 * states rest in device memory between launches and the split changes no bit.  bn_get_info "gibbs_colours", "gibbs_lds_bytes",
 * "gibbs_last_launches", "gibbs_last_kernel_ns" (option "timing" 1: HIP events around the launches).
 */
int bn_gibbs_run(bn_engine *eng, int32_t ne, const int32_t *ev_node, const int32_t *ev_state,
                 uint64_t chain_begin, uint64_t n_chains, uint64_t sweep_begin, uint64_t n_sweeps,
                 uint64_t burn_in, uint64_t thin, uint64_t seed, const uint8_t *init_states,
                 uint64_t *counts_out, uint8_t *states_out, uint64_t *stuck_out, uint64_t *kept_out);
/* The plan of bn_gibbs_run (also on host-only engines): colour_out [n] (may be NULL) the colour of every node; dims_out[8] =
 * eligible (1), colours, threads of a workgroup, chains of a workgroup, LDS bytes of a workgroup, sweeps per launch, nodes of
 * the largest colour, table entries one chain reads per sweep.  Not eligible: BN_ERR_STATE, bn_last_error has the reason. */
int bn_gibbs_plan_info(bn_engine *eng, int32_t *colour_out, int64_t *dims_out);

/* ---- entropy and mutual information over a pattern table ----
 * Replaces: bn::evaluation::entropy / mutual_information (bayesian/evaluation/transinformation.hpp:10-84),
 * which the reference declares but cannot compile (entropy::operator() calls lower_bound / key_comp on an
 * unordered_map, :26-27).
 *   bn_info_create: uploads a table once -- patterns [n_patterns][n_vars] states, counts [n_patterns]
 *   occurrences (any uint64 whose total fits in 64 bits), k [n_vars] arities in 1..255 -- and transposes
 *   it on the device.  Null pointers, arity, n_vars <= 0, n_patterns < 0 and a zero total: BN_ERR_ARG; no
 *   device: BN_ERR_NO_DEVICE; a state >= its arity (checked on the device): BN_ERR_ARG, nothing kept.
 *   bn_info_entropy: joint entropy of a set of columns (sorted, duplicates dropped),
 *   H = -sum over non-zero cells of (c/N) log2(c/N), fp64, N the total count (:35-39).  The cells are summed
 *   in a fixed order (increasing mixed-radix key, the smallest column the most significant digit, in chunks
 *   of 4096 keys), so H does not depend on the order of the patterns.  route 0: automatic, 1: dense cells
 *   (product of the arities <= 2^22), 2: sort on the packed key.  A key over 64 bits (product of the
 *   arities > 2^64): BN_ERR_ARG.
 *   bn_info_pair_entropies: for m columns (vars == NULL: every column, m == n_vars) h [m], hxy [m][m] and,
 *   if mi_out is not NULL, mi [m][m] = h[x] + h[y] - hxy[x][y] (:60, :80; no clamping).  hxy is symmetric
 *   bit for bit, its diagonal is h, and every entry has the bits of bn_info_entropy({x, y}).  Columns of
 *   arity <= 32 go through one all-pairs int8 matrix-core kernel; pairs with a wider column through the
 *   dense route of a single call.
 *   bn_info_pair_counts: the exact joint counts of n_pairs pairs (pairs [n_pairs][2]) as the all-pairs
 *   computation made them: for pair i a k_x x k_y block, x the row, blocks back to back in counts_out.
 *   bn_info_last_pairs_ms: device time of the all-pairs kernel of the last pair call (0 if none ran).
 *   bn_info_get: "n_vars", "n_patterns", "digit_passes" (7-bit passes over the counts); "learn_count_ns", "learn_lattice_ns",
 *   "learn_score_ns": device time of the kernels of the last bn_learn_score_groups / bn_learn_score_subsets call on the table. */
typedef struct bn_info_table bn_info_table;
int bn_info_create(int64_t n_patterns, int32_t n_vars, const uint8_t *patterns, const uint64_t *counts,
                   const int32_t *k, int32_t device, bn_info_table **out);
void bn_info_destroy(bn_info_table *table);
int bn_info_entropy(bn_info_table *table, int32_t n_set, const int32_t *set, int32_t route, double *h_out);
int bn_info_pair_entropies(bn_info_table *table, int32_t m, const int32_t *vars, double *h_out, double *hxy_out,
                           double *mi_out);
int bn_info_pair_counts(bn_info_table *table, int32_t n_pairs, const int32_t *pairs, uint64_t *counts_out);
int bn_info_last_pairs_ms(const bn_info_table *table, double *ms_out);
int bn_info_get(const bn_info_table *table, const char *name, int64_t *value_out);

/* ---- all-pairs conditional entropies, maximum spanning tree, Chow-Liu and TAN trees ----
 * Not in the reference: the tree learners of bnlearn (chow.liu, tree.bayes) and pgmpy (TreeSearch "chow-liu" / "tan").
 *   bn_info_cond_pair_entropies: for a conditioning column `cond` (any arity 1..255) and m columns `vars`: hz = H(Z), hxz [m] =
 *   H(X, Z), hxyz [m][m] = H(X, Y, Z) and, if cmi_out is not NULL, cmi [m][m] = I(X; Y | Z).
 *     Summation order.  For each state s of cond in increasing order, part_s folds `part -= p * log2(p)` from 0.0 over the non-zero
 *     cells N(x, y, s), p = c / N with N the table's total; within a state the cells are taken in the order bn_info_pair_entropies
 *     uses for the pair (the lower column the more significant digit).  hxyz[x][y] = 0.0 + part_0 + part_1 + ... in state order; a
 *     state that never occurs contributes part = 0.0.  So an entry is a function of the exact counts alone.
 *     Entries.  hxyz is symmetric bit for bit; hxz[x] is its diagonal entry, H(X, Z) in the same order; hz has the bits of
 *     bn_info_entropy({cond}); cmi[x][y] = hxz[x] + hxz[y] - hxyz[x][y] - hz, evaluated left to right on the device, no clamping.
 *     Invariances.  An entry does not depend on m, on its position in vars, on duplicates in vars, on the pattern order or on the run.
 *     With a cond of arity 1, hxyz, hxz and cmi have the bits of bn_info_pair_entropies' hxy, h and mi.
 *     Arities.  x and y of arity <= 32 go through the conditional form of the all-pairs matrix-core kernel, which reads the table once
 *     per state of cond.  A pair with a wider column takes the bits of the single call bn_info_entropy({x, y, cond}) (route 0) -- whose
 *     order is that call's, not the one above -- and hxz of a wider column those of bn_info_entropy({x, cond}).
 *     Refusals, BN_ERR_ARG with a bn_last_error text and nothing launched: cond out of range, cond among vars, a null pointer (vars
 *     included; cmi_out may be NULL), m <= 0, a column out of range.
 *   bn_info_cond_pair_counts: the twin of bn_info_pair_counts: for pair i the exact block [k_cond][k_x][k_y] as the epilogue saw it,
 *   blocks back to back.  A pair with a column of arity > 32 is counted by the dense route: more than 2^22 cells, BN_ERR_ARG.
 *   Both set bn_info_last_pairs_ms; bn_info_get "cond_pairs_ns" is the kernel time of the last conditional call, "tree_ns" that of the
 *   spanning-tree kernel of the last bn_learn_tree.
 *   bn_tree_max_spanning: the maximum spanning tree of the complete graph over m nodes with the weights w [m][m] (host), oriented from
 *   `root`.  Edges are totally ordered by weight descending, then by (min(u, v), max(u, v)) ascending; -0.0 and 0.0 compare equal and
 *   +-inf is allowed.  Under this strict total order the maximum spanning tree is unique, and that tree is the result.  Only w[lo][hi],
 *   lo < hi, is read.  parent_out[v] is v's neighbour on the path to root, parent_out[root] = -1.  One workgroup runs Prim's algorithm
 *   with every node's key in LDS: m <= 4096 (beyond: BN_ERR_ARG).  m == 1: no launch.  A NaN in the upper triangle, a root out of
 *   range, a null pointer, m <= 0: BN_ERR_ARG, checked on the host.
 *   bn_learn_tree: cond == -1: the Chow-Liu tree of the columns vars, the maximum spanning tree under the `mi` matrix of
 *   bn_info_pair_entropies; cond >= 0: the tree of tree-augmented naive Bayes for the class column cond, under the `cmi` matrix of
 *   bn_info_cond_pair_entropies (the edges class -> feature are the caller's to add).  The weights have those matrices' bits and stay
 *   on the device between the two kernels.  vars NULL: every column but cond, increasing (m must be their number); root: a column of
 *   vars, -1: the lowest.  parent_out [m]: the parent COLUMN of vars[i], -1 at the root; weight_out [m]: the matrix entry of the edge
 *   (vars[i], parent), 0.0 at the root; matrix_out [m][m] (may be NULL): the weights.  Duplicates in vars, cond in vars, root not in
 *   vars, a column out of range, m <= 0, m > 4096, null outputs: BN_ERR_ARG. */
int bn_info_cond_pair_entropies(bn_info_table *table, int32_t cond, int32_t m, const int32_t *vars, double *hz_out, double *hxz_out,
                                double *hxyz_out, double *cmi_out);
int bn_info_cond_pair_counts(bn_info_table *table, int32_t cond, int32_t n_pairs, const int32_t *pairs, uint64_t *counts_out);
int bn_tree_max_spanning(int32_t m, const double *w, int32_t root, int32_t device, int32_t *parent_out);
int bn_learn_tree(bn_info_table *table, int32_t cond, int32_t m, const int32_t *vars, int32_t root, int32_t *parent_out,
                  double *weight_out, double *matrix_out);

/* ---- log-likelihood of a pattern table under the engine's network ----
 * Replaces: basic_info_criteria::calc_likelihood (bayesian/evaluation/basic_info_criteria.hpp:44-78), the term of
 * bn::evaluation::aic / mdl that depends on the data; calc_parameters (:100-117) is bn_get_info(eng, "parameters")
 * = sum over the nodes of (k[v] - 1) x product of the parents' arities (int64, exact).
 *   The log table.  L[q] = log(cpt[q]) for every flat CPT entry q (layout of bn_model_desc.cpt), taken on the HOST
 *   with libm's log in fp64 (log(0) = -inf), at the first bn_score_* call and again after bn_reload_cpt.  The device
 *   never evaluates a logarithm: every result below is a function of L, the table and the stated order of additions.
 *   bn_score_log_cpt: L [n_entries] (also on a BN_DEVICE_HOST_ONLY engine).
 *   bn_score_rows: ll_out [n_patterns], ll_out[p] = sum over the selected nodes v of
 *   L[cpt_off[v] + row_v(p) * k[v] + state_v(p)], row_v the parent assignment with the first parent most significant
 *   (the rule of bn_fit_cpt).  nodes == NULL selects every node (n_sel is not read); else `nodes` lists n_sel node ids
 *   in any order; a duplicate or an id out of range: BN_ERR_ARG; n_sel == 0: every sum is +0.0.  Order of additions:
 *   the nodes are grouped by node id >> 8 (segments of 256 consecutive ids, whatever the selection); inside a segment
 *   the selected nodes are added in increasing id starting from +0.0; the segment sums are then added in increasing
 *   segment order starting from +0.0; a segment without a selected node is skipped.  ll_out[p] therefore depends on
 *   the model, the selection and pattern p alone -- not on the other patterns, on p's position or on the launch
 *   shape.  A pattern that shows a zero-probability entry scores -inf.  The counts are not used.
 *   bn_score_nodes: ll_node_out [n_nodes], ll_node_out[v] = sum over the entries q of node v's table with N[q] != 0 of
 *   double(N[q]) * L[q]; N[q] the exact number of samples (patterns weighted by their counts) showing that parent
 *   assignment and state -- the counts bn_fit_cpt normalises.  An entry no sample shows is skipped (an unseen
 *   zero-probability entry adds nothing, not 0 * -inf).  Order of additions, with r = q - cpt_off[v]: 256 partial sums,
 *   partial t taking the terms r = t, t + 256, t + 512, ... in increasing r starting from +0.0; then the partial sums are
 *   folded by halves, for s = 128, 64, ..., 1: partial[t] += partial[t + s] for every t < s; the result is partial[0].
 *   It does not depend on the order of the patterns, on how a pattern's count is spread over equal rows or on the launch
 *   shape.  family_counts_out may be NULL; else it receives N [n_entries].
 *   Errors.  BN_ERR_ARG: a null pointer, n_vars != n_nodes, an arity that differs between engine and table, engine and
 *   table on different devices (the agreement of the arities is also what keeps every gather inside L: the table's
 *   states were checked against them at bn_info_create).  BN_ERR_NO_DEVICE: a BN_DEVICE_HOST_ONLY engine.
 *   BN_ERR_STATE: a sharded engine (a shard holds only its own nodes).
 *   bn_get_info "score_rows_ns", "score_count_ns", "score_nodes_ns": device time of the last call's row kernel(s),
 *   counting kernel and node-sum kernel; bn_set_option "score_splits": workgroups per node of the counting kernel
 *   (0, the default: chosen from the shapes; the counts are integers and do not depend on it). */
int bn_score_log_cpt(bn_engine *eng, double *out);
int bn_score_rows(bn_engine *eng, bn_info_table *table, int32_t n_sel, const int32_t *nodes, double *ll_out);
int bn_score_nodes(bn_engine *eng, bn_info_table *table, double *ll_node_out, uint64_t *family_counts_out);

/* ---- structure learning: batched family scores, and the scan of greedy / K2 (reference bayesian/learning/greedy.hpp,
 *      k2_algorithm.hpp).  AIC and MDL are decomposable: adding u -> c changes the family term of c and the parameter count. ----
 *
 *   A GROUP is a child c, a base parent list (strictly increasing node ids, c not among them) and candidates u_0 .. u_{m-1} (not
 *   in the base, not c, no duplicates; m may be 0).  It stands for m + 1 families: the base (index 0) and base + {u_j} (index
 *   1 + j).  Groups are given in CSR form: child [n_groups], base_ptr / cand_ptr [n_groups + 1], base_idx, cand_idx.
 *   bn_learn_score_groups: one counting launch and one scoring launch for the whole batch (several such passes when the count
 *   scratch would pass 256 MiB).  Per family, over the entries r of the table the fitted model would have (parents in increasing
 *   node id, first parent most significant, state least -- bn_fit_cpt's layout):
 *     N[r]   exact uint64 count of the samples showing entry r (integer atomics: independent of grouping, chunking, split, order);
 *     ll     = sum over the entries with N[r] != 0 of double(N[r]) * log(double(N[r]) / double(row total)) -- the division is
 *              bn_fit_cpt's, so the argument of the logarithm has the bits of the fitted CPT entry; log is the DEVICE's fp64 log
 *              (not libm's: ll is within a few ulp per term of bn_score_nodes on the fitted model, not bit-equal to it); the order of
 *              additions is bn_score_nodes': 256 partial sums (partial t takes r = t, t + 256, ... from +0.0), folded by halves.
 *   ll is a function of the family's counts alone: the same family scored alone, as a base, as a candidate, anywhere in any
 *   batch, has the same bits.  ll_out [n_groups + candidates] is group-major, base first; counts_out is NULL or receives every
 *   family's N back to back in that order.  The environment variable BN_LEARN_SPLITS (> 0) fixes the number of workgroups the
 *   patterns are split over (default: chosen from the shapes; no result depends on it).
 *   Limits (BN_ERR_ARG, the text names the group): at most 16 parents per family, family table <= 2^20 entries.
 *
 *   bn_learner holds a graph over the table's columns, every node's family term ll[v], the exact parameter count and the score:
 *     likelihood = 0.0; for v = 0 .. n - 1: likelihood -= ll[v];
 *     AIC (criterion 0) = likelihood + double(params); MDL (1) = likelihood + double(params) * (log2(double(total)) / 2).
 *   bn_learn_try_parents is the inner loop of greedy.hpp:39-58 / :82-97 and k2_algorithm.hpp:47-61 for one child: it walks cand in
 *   the given order; a candidate that is the child, already a parent, reachable from the child (the edge would close a cycle,
 *   graph.hpp:268-275), or whose family would exceed max_parents or the limits above is not added (accepted_out 0; the last is
 *   a difference from the reference, which has no limits); any other is accepted iff the score with it is strictly smaller than
 *   the current score.  All remaining candidates are scored against the current parents as one group; the first in order that
 *   improves is accepted and the rest re-scored: device passes per call = acceptances + 1 at most.  The starting graph may have
 *   edges (in_ptr / in_idx, any parent order); BN_ERR_ARG if it has a cycle, a duplicate edge or a family over the limits.
 *   bn_learn_structure: in_ptr_out [n + 1], in_idx_out [edges] ("edges" of bn_learn_get), parents increasing per node.
 *   bn_learn_get names: "families_scored", "passes", "count_ns", "score_ns" (device time of the two kernels, summed), "count_bytes"
 *   (what the counting kernel had to read, from the shapes: per chunk of G candidates P * (8 + base parents + 1 + G)), "edges",
 *   "parameters".  The learner borrows the table: destroy the learner first.  Work runs on the table's stream. */
int bn_learn_score_groups(bn_info_table *table, int32_t n_groups, const int32_t *child, const int32_t *base_ptr,
                          const int32_t *base_idx, const int32_t *cand_ptr, const int32_t *cand_idx, double *ll_out,
                          uint64_t *counts_out);
typedef struct bn_learner bn_learner;
int bn_learn_create(bn_info_table *table, const int32_t *in_ptr, const int32_t *in_idx, int32_t criterion, int32_t max_parents,
                    bn_learner **out);
int bn_learn_try_parents(bn_learner *L, int32_t child, int32_t n_cand, const int32_t *cand, uint8_t *accepted_out);
int bn_learn_score(const bn_learner *L, double *score_out);
int bn_learn_structure(const bn_learner *L, int32_t *in_ptr_out, int32_t *in_idx_out);
int bn_learn_get(const bn_learner *L, const char *name, int64_t *out);
void bn_learn_destroy(bn_learner *L);

/* ---- exhaustive parent-set search: the subset lattice of one child, and the reference's brute_force on top of it (reference
 *      bayesian/learning/brute_force.hpp; the between-cluster step of stepwise_structure.hpp). ----
 *
 *   bn_learn_score_subsets scores the 2^m families  base + {cand[j] : bit j of mask}  of one child: ll_out [2^m] by mask;
 *   counts_out is NULL or receives every family's N in the fitted layout, family after family in mask order.  The TOP family
 *   base + all candidates is counted once from the table; every other family's counts are made on the device by summing absent
 *   candidates out of it (uint64 adds: exact), directly in the fitted layout, and scored by the kernel bn_learn_score_groups uses.
 *   N and ll of a family are therefore, bit for bit, what bn_learn_score_groups gives for it.  base may come in any order; m = 0
 *   gives the one family.  Limits (BN_ERR_ARG, the text names the number): n_base + m <= 16; the top family <= 2^20 entries; all 2^m
 *   tables together <= 2^25 cells (one pass; there is no multi-pass lattice); ids distinct, in range, not the child.
 *
 *   bn_learn_best_parents: the best subset of cand to ADD to the child's parents.  cand is filtered as bn_learn_try_parents filters
 *   it (the child, a parent, a node the child reaches, a second listing, a family over the size limit; nothing passes when the
 *   child has max_parents parents); the m survivors are scored through the lattice -- survivors beyond its limits are an error,
 *   not a silent cut.  A subset's score is the learner's stated function with the child's ll and the parameter count replaced;
 *   subsets that would pass max_parents are not eligible.  The winner is the strictly smallest score, among equal values the
 *   first in the reference's visiting order (brute_force.hpp:104-111: "not added" before "added", cand[0] outermost -- mask order
 *   with the bit significance reversed).  The empty subset keeps the graph.  taken_out [n_cand]: 1 where the edge was added.
 *   bn_learn_terms: ll_out [n] the family terms the score is the sum of; params_out (may be NULL) the parameter count.
 *
 *   bn_learn_brute_force_hint is brute_force::learn_with_hint (:51-113): every subset of the possible edges par[i] -> child[j].
 *   When no node of child reaches a node of par in the starting graph (which also makes the two sets disjoint) no add_edge can be
 *   refused for a cycle and the edges into different children do not interact: the search is bn_learn_best_parents(child[j], par)
 *   for each distinct child in the order given.  Otherwise the literal depth-first enumeration runs on the host over the possible
 *   edges parent-major, with add_edge's refusals (an existing edge, a cycle) and max_parents, over family terms fetched once per
 *   child through the lattice; more than 20 possible edges is then BN_ERR_ARG.  A graph replaces the best on strictly smaller only.
 *
 *   bn_learn_brute_force is brute_force::operator()(graph, vertexes) (:32-44, :116-156), literally: level t tries, for each later
 *   vertex v_i, no edge / v_t -> v_i / v_i -> v_t and recurses to level t + 1 (so a graph gets at most one new edge per level).
 *   The evaluated quantity is the reference's eval_(graph, vertexes): likelihood = 0.0; likelihood -= ll[v] over vertexes IN THE
 *   GIVEN ORDER; plus the penalty on the WHOLE graph's parameters; a graph replaces the best on strictly smaller only (a graph
 *   met again is skipped: it cannot win).  One lattice call per vertex over the other vertexes.  n_v <= 8 (2 027 025 distinct
 *   graphs) and distinct vertexes, else BN_ERR_ARG.  eval_out (may be NULL) receives the best evaluated quantity;
 *   bn_learn_score afterwards gives the whole graph's score.  Both searches leave the best graph in the learner.
 *   bn_learn_get also names "lattice_ns" (device time of the lattice kernels, summed) and "subsets_scored". */
int bn_learn_score_subsets(bn_info_table *table, int32_t child, int32_t n_base, const int32_t *base, int32_t m, const int32_t *cand,
                           double *ll_out, uint64_t *counts_out);
int bn_learn_best_parents(bn_learner *L, int32_t child, int32_t n_cand, const int32_t *cand, uint8_t *taken_out);
int bn_learn_terms(const bn_learner *L, double *ll_out, int64_t *params_out);
int bn_learn_brute_force_hint(bn_learner *L, int32_t n_par, const int32_t *par, int32_t n_child, const int32_t *child);
int bn_learn_brute_force(bn_learner *L, int32_t n_v, const int32_t *vertexes, double *eval_out);

/* ---- simulated annealing as many device-resident chains over a table of family terms (reference
 *      bayesian/learning/simulated_annealing.hpp:41-115). ----
 *
 *   bn_term_table holds, for every child c and every parent set S of at most q = max_parents nodes other than c, the family
 *   term ll(c, S), resident on the device: bit for bit what bn_learn_score_groups gives for that family (it is built through it:
 *   the groups (c, base B, candidates u > max(B)) for every B of fewer than q nodes, in one batch).  Index:
 *     relabel the nodes other than c to 0 .. n - 2 by s' = s - (s > c);  for S = {s'_1 < ... < s'_j}
 *     rank = offset[j] + sum over i = 1 .. j of C(s'_i, i),   offset[j] = sum over t < j of C(n - 1, t);
 *     T(n, q) = offset[q + 1] entries per child, child c's row at c * T  (T(37, 3) = 7 807, T(64, 3) = 41 728).
 *   A family over the per-family limit of 2^20 table entries holds a quiet NaN: "not eligible".  Limits (BN_ERR_ARG, the text names
 *   the number): 1 <= max_parents <= 16; n <= 64 (the kernel gives a node a lane); n * T(n, q) <= 2^22 entries (32 MiB) -- a larger
 *   table is refused, not trimmed.  bn_terms_fetch: ll_out [T], one child's row.  bn_terms_get names: "entries" (n * T), "row_entries"
 *   (T), "nodes", "max_parents", "ineligible" (NaN entries), "families_scored", "passes", "build_ns" (device time of the counting and
 *   scoring kernels).  The term table borrows the bn_info_table: destroy the term table first.
 *
 *   bn_learn_anneal runs `chains` independent chains (1 .. 2^16) from the learner's current graph, one wave per chain, lane v = node
 *   v.  A chain's edge list starts child-major, parents increasing per child.  The loop, per iteration:
 *     method = draw(3).  0: from = draw(n), to = draw(n); add_edge(from, to) is refused when from == to or `to` reaches `from`
 *     (graph.hpp:270), when the edge exists (:284), and -- the library's limits, not the reference's -- when `to` has
 *     min(q, the learner's max_parents) parents or the new family's term is NaN; otherwise the edge is appended to the list.
 *     1, 2: with no edge the iteration ends here (`continue`: no draw, no cooling); else i = draw(edges) picks edge_list()[i],
 *     which is erased in place; 2 then adds the opposite edge at the end of the list, and when that is refused adds the original
 *     edge back AT THE END (graph.hpp:339-358): the list stays reordered and the proposal does not count as operated.
 *     A proposal that was not operated neither cools nor counts towards same_state_max.  Otherwise now = the learner's score of
 *     the proposed graph (the stated function above, node order, exact parameter count: the bits of bn_learn_score), diff = now -
 *     current; accepted iff diff <= 0, else u = uniform() and accepted iff u < exp(-now / (boltzmann * T)) (rule 0, the
 *     reference's :97: `now`, not `diff`, in the exponent) or u < exp(-diff / (boltzmann * T)) (rule 1, Metropolis); the multiply
 *     and the divide are separate operations.  Rejected: the graph AND its edge list become those of the last accepted graph
 *     (graph = best_graph, :109 -- this also undoes the reordering of refused reversals since then), same-state count + 1;
 *     accepted: same-state count = 0.  T *= decreasing_rate.
 *   The loop runs while T > final_temp && same-state count < same_state_max && iterations < max_proposals (0: 2^20; at most 2^24).
 *   Random stream of chain j: xoshiro128++ seeded by Philox4x32-10(counter {j_lo, j_hi, 0, 0}, key {seed_lo, seed_hi}), an all-zero
 *   block becoming {1, 0, 0, 0} (the sampler's stream_seed); one step per draw, 32-bit output r: draw(m) = (uint64(r) * m) >> 32,
 *   uniform() = (r + 0.5) * 2^-32.  Draw order per iteration: method; from, to or the edge index; u only for an operated proposal
 *   with diff > 0.  A chain depends on (seed, j) and the arguments only: not on `chains` or the launch shape.
 *   Arguments (BN_ERR_ARG, nothing launched): temperatures finite and > 0, 0 < decreasing_rate < 1, boltzmann finite and > 0, rule
 *   0 or 1, 1 <= chains <= 2^16, the term table built from the learner's table, no starting family over q parents.
 *   Outputs (each may be NULL): eval_out [chains] final evaluations; counts_out [chains][4] iterations, operated, accepted, flags
 *   (1: ended by temperature, 2: by same_state_max, 4: by max_proposals); masks_out [chains][n] final parent masks (bit u of word
 *   v: u -> v); n_edges_out [chains] and edges_out [chains][n * q] the final ordered edge lists, from | to << 8; trace_out
 *   [trace_cap] for chain trace_chain (-1: none), per operated proposal in order (the first trace_cap of them): the drawn edge
 *   from -> to, the method, the bits of now, accepted; winner_out the winning chain: the STRICTLY smallest final evaluation, among
 *   equal values the lowest index.  The learner's graph and terms are replaced by the winner's: bn_learn_score equals its
 *   evaluation bit for bit, bn_learn_structure / bn_learn_terms work as usual.  Runs on the table's stream; no device-wide
 *   synchronise.  bn_learn_get also names "anneal_ns" (device time of the kernel, summed), "anneal_chains", "anneal_steps"
 *   (iterations of all chains). */
typedef struct bn_term_table bn_term_table;
typedef struct bn_anneal_params {
    double initial_temp, final_temp, decreasing_rate, boltzmann;
    uint32_t same_state_max, max_proposals;
    int32_t rule, trace_chain;
    uint32_t trace_cap, pad_;
} bn_anneal_params;
typedef struct bn_anneal_trace {
    uint64_t now_bits;
    uint8_t method, from, to, accepted;
    uint32_t pad_;
} bn_anneal_trace;
int bn_terms_create(bn_info_table *table, int32_t max_parents, bn_term_table **out);
int bn_terms_get(const bn_term_table *terms, const char *name, int64_t *out);
int bn_terms_fetch(const bn_term_table *terms, int32_t child, double *ll_out);
void bn_terms_destroy(bn_term_table *terms);
int bn_learn_anneal(bn_learner *L, bn_term_table *terms, const bn_anneal_params *params, int32_t chains, uint64_t seed,
                    double *eval_out, uint32_t *counts_out, uint64_t *masks_out, int32_t *n_edges_out, uint16_t *edges_out,
                    bn_anneal_trace *trace_out, int32_t *winner_out);

/* ---- hierarchical clustering with stochastic pruning as many device-resident runs (reference
 *      bayesian/learning/stepwise_structure_hc.hpp:131-360 over greedy.hpp:67-101). ----
 *
 *   bn_learn_hc runs `runs` independent searches (1 .. 2^16), one wave per run, lane v = node v (n <= 64), over a bn_term_table
 *   built on the learner's table and a similarity matrix S [n][n], and makes the best final graph the learner's.  The learner's
 *   starting edges are ignored: the algorithm clears them (:134).
 *   Difference from the reference: it orders clusters, and the two halves of a similarity, by shared_ptr address (:199, :257),
 *   which depends on the allocator.  Here a cluster has an id: node i's initial cluster is i, the cluster made by merge number s
 *   (from 0) is n + s (at most 2n - 2), and "smaller address" reads "smaller id".
 *   State of a run: the graph; `clusters`, the ordered list of live ids, initially 0 .. n-1; per cluster its ordered node list (a
 *   merged cluster holds the parent cluster's nodes, then the child cluster's, in their stored order); `sims`, the ordered list of
 *   (a, b, value), a < b, initially every i < j in row-major order with value = make_similarity(i, j); average = 0.0, then +=
 *   value / double(n (n - 1) / 2) in that order (:171-186).
 *   make_similarity(X, Y) (:240-259): value = 0.0; for l in nodes(X) (outer), r in nodes(Y) (inner): value += S[l][r] /
 *   double(|X| |Y|): one divide and one add per pair, no tree.
 *   The loop, while more than one cluster is live and sims is not empty (:267):
 *     pick: best = 0; for i >= 1: if value[best] < value[i]: best = i -- the FIRST maximum (:220-237); that entry (a, b, old_value)
 *     leaves the list; coin = draw(2): (parent, child) = (b, a) when set, else (a, b).
 *     learn_with_hint(nodes(parent), nodes(child)) (greedy.hpp:67-101): the copy of the child nodes is shuffled (for i = len-1 ..
 *     1: j = draw(i + 1); swap(x[i], x[j])); eval_now = the learner's score; per child the copy of the parent nodes is shuffled
 *     again (the shuffles accumulate within the call) and each parent visited in order: the edge parent -> child is refused when
 *     the child has max_parents parents or the new family's term is NaN (the library's limits; the reference's own refusals, a
 *     cycle or an existing edge, cannot occur: two clusters meet once and their edges run one way between disjoint node sets);
 *     otherwise eval_next = the learner's score with the edge (the stated function, node order, exact parameter count: the bits
 *     of bn_learn_score), and the edge is kept iff eval_next < eval_now.
 *     merge (:204-217): parent and child leave `clusters` (ordered erase), the new id is appended.
 *     prune (:299-360): for each c in `clusters` order, c != new: its connections, the entries of sims that join c with parent or
 *     with child, leave the list (ordered erase); new_value = make_similarity(new, c); two connections: p = pow(alpha, new_value /
 *     average); one: p = pow(alpha, old_value / that connection's value); none: next cluster, no draw.  u = uniform(); u < p: the
 *     pair is pruned; otherwise (c, new, new_value) is appended to sims.  IEEE arithmetic as it falls: a zero average or
 *     connection gives inf or NaN, and u < NaN keeps the pair.  (The reference's closing sweep, :351-359, never finds anything.)
 *   A run's result is the learner's score of its final graph; with no merge (n == 1) that of the empty graph, where the
 *   reference returns DBL_MAX.
 *   Random stream of run j: as chain j of bn_learn_anneal.  Draw order per merge: the coin, the child shuffle, per child its parent
 *   shuffle, then one uniform per surviving cluster that has a connection, in `clusters` order.  A run depends on (seed, j) and
 *   the arguments only: not on `runs` or the launch shape.
 *   similarity NULL: S is the `mi` matrix bn_info_pair_entropies gives for every column of the learner's table, bit for bit,
 *   read as S[l][r]: made on the device from the all-pairs kernel's own entropies, on the table's stream, and left there (no
 *   host round trip; only the pairs of a column of arity > 32, which that call finishes on the host, are written from it).  Non-NULL: the caller's [n][n] matrix; one whose [x][y]
 *   and [y][x] differ in bits is refused; the diagonal is not read.
 *   Arguments (BN_ERR_ARG, the text names the limit, nothing launched): n <= 64; 1 <= runs <= 2^16; alpha finite and >= 0; 1 <=
 *   max_parents <= the term table's (a run refuses at min(max_parents, the learner's)); the term table built on the learner's
 *   table; -1 <= trace_run < runs.
 *   Outputs (each may be NULL): score_out [runs]; counts_out [runs][6]: merges, candidates that reached an evaluation, edges kept,
 *   pairs pruned, pairs kept, flags (1: one cluster left, 2: sims empty; both may be set); masks_out [runs][n] final parent masks
 *   (bit u of word v: u -> v); trace_out [trace_cap] for run trace_run, in the order things happen (the first trace_cap records;
 *   a run makes at most 2 016), n_trace_out their number: kind 0, a merge: a = parent id, b = child id, c = coin, value_bits = the
 *   bits of old_value; kind 1, a pruning visit: a = cluster id, b = connections, c = pruned, value_bits = the bits of new_value.
 *   winner_out: the run with the STRICTLY smallest score, among equals the lowest.  The learner's graph and terms become the
 *   winner's: bn_learn_score equals its score bit for bit, bn_learn_structure / bn_learn_terms work as after bn_learn_anneal.
 *   bn_learn_get also names "hc_ns" (device time of the kernel, summed), "hc_runs", "hc_merges". */
typedef struct bn_hc_params {
    double alpha;
    int32_t max_parents, trace_run;
    uint32_t trace_cap, pad_;
} bn_hc_params;
typedef struct bn_hc_trace {
    uint64_t value_bits;
    uint8_t kind, a, b, c;
    uint32_t pad_;
} bn_hc_trace;
int bn_learn_hc(bn_learner *L, bn_term_table *terms, const bn_hc_params *params, int32_t runs, uint64_t seed,
                const double *similarity, double *score_out, uint32_t *counts_out, uint64_t *masks_out, bn_hc_trace *trace_out,
                int32_t *n_trace_out, int32_t *winner_out);

/* ---- tabu hill climbing as many device-resident runs: steepest descent over add, delete and reverse moves, a tabu list over node
 *      pairs, perturbed restarts (the search of bnlearn's hc / tabu and pgmpy's HillClimbSearch; NOT IN THE REFERENCE). ----
 *
 *   bn_learn_climb runs `runs` independent searches (1 .. 2^16), one wave per run, lane v = node v (n <= 64), over a bn_term_table
 *   built on the learner's table, and makes the best graph any run saw the learner's.
 *   Graph of a run: parent masks pm[v], family terms ll[v], the exact int64 parameter count.  In-degree bound mp =
 *   min(params.max_parents, the term table's q, the learner's max_parents).  `current` is the learner's stated score of the graph
 *   (node-order sum plus penalty, exact parameter count: the bits of bn_learn_score), recomputed from the terms after every move.
 *   Moves: id = (kind * n + from) * n + to.  Kind 0 adds from -> to, 1 deletes it, 2 turns it into to -> from.  Legal:
 *     add     : from != to, the edge is absent, `to` does not reach `from`, `to` has fewer than mp parents, the new term is not NaN;
 *     delete  : the edge is present;
 *     reverse : the edge is present; with it removed `from` does not reach `to`; `from` has fewer than mp parents; the term of
 *               `from` with `to` added is not NaN.
 *   Delta of a family change of child c to a new parent set: (ll[c] - term_new); under AIC + double(p_new - p_old), under MDL
 *   + double(p_new - p_old) * penalty, under BDeu / K2 nothing; p = (k[c] - 1) * rows exactly; every operation a plain fp64 one (no
 *   fused multiply-add).  d of an add or a delete is the delta of `to`'s family; of a reverse delta(`to` without `from`) +
 *   delta(`from` with `to`), one add, in that order.  A move whose d is NaN is not legal.
 *   Tabu: a move on the unordered pair {from, to} is tabu while one of the last tabu_len (0 .. 64) APPLIED moves of this run was on
 *   that pair; perturbations do not count.
 *   Step, while steps < max_steps (0: 2^16; at most 2^20):
 *     1. the legal, non-tabu move with the smallest d (IEEE <, so -0.0 and +0.0 tie), among equal d the lowest id;
 *     2. none: flag 1, the run ends;
 *     3. !(d < 0) and worse == max_worse: flag 2 (a local optimum), the run ends;
 *     4. the move is applied, steps += 1, the pair enters the tabu ring (the oldest entry leaves it);
 *     5. current = the stated score of the new graph;
 *     6. current < best_eval strictly: the graph becomes the run's best, best_step = steps, worse = 0; otherwise worse += 1.
 *   Leaving the loop at max_steps is flag 4.  tabu_len = 0, max_worse = 0 is the classic greedy climb; with both above 0 a run walks
 *   through plateaus and over ridges and returns the best graph it saw.  (Step 3 compares with ==, as stated: a move with d < 0
 *   whose recomputed score is not smaller in bits leaves worse above a max_worse of 0, and the run goes on to max_steps.)
 *   Starts: run 0 from the learner's graph.  Run j >= 1 first makes `perturb` (0 .. 2^16) proposals from stream j, the stream of
 *   chain j of bn_learn_anneal with the same seeding: kind = draw(3), from = draw(n), to = draw(n), applied when legal under the
 *   rules above and skipped without a redraw otherwise.  The perturbed graph is the run's first best.  The climb draws nothing.  A
 *   run depends on (seed, j) and the arguments only: not on `runs` or the launch shape.
 *   Arguments (BN_ERR_ARG, the text names the limit, nothing launched): n <= 64; 1 <= runs <= 2^16; 0 <= tabu_len <= 64; max_steps <=
 *   2^20; perturb <= 2^16; max_parents >= 1; the term table built on the learner's table and of the learner's score spec; no
 *   starting family over q parents; -1 <= trace_run < runs.
 *   Outputs (each may be NULL): score_out [runs] each run's best_eval; counts_out [runs][6]: steps, steps with d < 0,
 *   perturbations applied, best_step, flags, moves that were legal but tabu at the last look; masks_out [runs][n] the best graphs'
 *   parent masks (bit u of word v: u -> v); trace_out [trace_cap] for run trace_run (-1: none), per applied step in order (the
 *   first trace_cap): kind, from, to, the bits of d, the bits of current; winner_out: the run with the STRICTLY smallest best_eval,
 *   among equals the lowest.  The learner's graph and terms become the winner's: bn_learn_score equals its score bit for bit,
 *   bn_learn_structure / bn_learn_terms work as after bn_learn_anneal.  Runs on the table's stream; no device-wide synchronise.
 *   bn_learn_get also names "climb_ns" (device time of the kernel, summed), "climb_runs", "climb_steps". */
typedef struct bn_climb_params {
    int32_t max_parents, tabu_len;
    uint32_t max_worse, max_steps, perturb;
    int32_t trace_run;
    uint32_t trace_cap, pad_;
} bn_climb_params;
typedef struct bn_climb_trace {
    uint64_t d_bits, current_bits;
    uint8_t kind, from, to, pad8_;
    uint32_t pad32_;
    uint64_t pad_;
} bn_climb_trace;
int bn_learn_climb(bn_learner *L, bn_term_table *terms, const bn_climb_params *params, int32_t runs, uint64_t seed,
                   double *score_out, uint32_t *counts_out, uint64_t *masks_out, bn_climb_trace *trace_out, int32_t *winner_out);

/* ---- exact structure learning: the DAG of globally smallest cost by dynamic programming over node subsets (Silander & Myllymaki
 *      2006; the search of pgmpy's ExhaustiveSearch; NOT IN THE REFERENCE). ----
 *
 *   bn_learn_optimal finds, over a bn_term_table built on the learner's table and of the learner's score spec, a DAG whose sum of
 *   family costs is the smallest any DAG within the bounds has, and makes it the learner's graph.  The learner's starting graph is
 *   not read.  1 <= n <= 24.  In-degree bound mp = min(params.max_parents, the term table's q, the learner's max_parents).
 *   allowed: NULL, or [n] masks: bit u of allowed[v] set means u may be a parent of v; bit v of allowed[v] is ignored.
 *   Family cost of child v with parent set S:  f(v, S) = (0.0 - ll(v, S)) + double(dp) * penalty,  dp = (k_v - 1) * rows(S) an exact
 *   int64, penalty 1.0 under AIC and log2(N) / 2 under MDL; under BDeu / K2 f(v, S) = 0.0 - term and no more.  Every step one plain
 *   fp64 operation (no fused multiply-add).  f is +inf where the term is NaN (not eligible), where |S| > mp, and where S is not
 *   inside allowed[v]; the empty set is always eligible.
 *   Step 1, for every v and every C inside V \ {v}:  bps[v][C] = min over S inside C of (f(v, S), rank(v, S)), compared
 *     lexicographically: the smaller cost, among equal costs the smaller term-table rank.  C is indexed by its mask with bit v
 *     squeezed out, c = (C & ((1 << v) - 1)) | ((C >> (v + 1)) << v), the rank tables' relabelling s' = s - (s > v).  Made as a
 *     min-zeta transform: the cell of S starts as (f, rank) where |S| <= mp and as (+inf, 0xFFFFFFFF) otherwise, then for each of the
 *     n - 1 bits b, g[c] = min(g[c], g[c ^ (1 << b)]) for every c with bit b set.  min does not round and the order is total: the
 *     result does not depend on the order of the bits or of the cells.
 *   Step 2:  R[empty] = +0.0;  for W not empty, R[W] = min over v in W, v ascending, of R[W \ v] + bps[v][squeeze(W \ v)].cost, one
 *     fp64 add per term; the first v starts the minimum and a STRICTLY smaller value replaces it, so among equals the lowest v stays;
 *     sink[W] = that v.
 *   Step 3:  W = V;  for i = n - 1 .. 0:  s = sink[W], order_out[i] = s, W ^= 1 << s, the parents of s are the set of rank
 *     bps[s][squeeze(W)].rank.
 *   Outputs (each may be NULL): value_out = R[V]; order_out [n] a topological order, parents first; masks_out [n] the parent masks
 *   (bit u of word v: u -> v).  The learner's graph, terms and parameter count become the result's, as after bn_learn_climb:
 *   bn_learn_structure / bn_learn_terms work as usual and bn_learn_score is the learner's stated score of that graph (node-order sum
 *   plus penalty on the summed parameter count).  That is another order of additions than R[V]'s: the two may differ in the last
 *   bits.
 *   Arguments (BN_ERR_ARG, the text names the limit; checked before any allocation or launch, the learner stays as it was): a null
 *   pointer; a term table built on another table or of another spec (as bn_learn_anneal); n outside 1 .. 24; max_parents < 1; a bit
 *   at or above n in a word of allowed.  Memory: n * 2^(n - 1) cells of 12 bytes and 2^n sets of 9 (2.4 GB at n = 24), allocated
 *   for the call and freed when it returns; an allocation that fails returns BN_ERR_HIP with the runtime's out-of-memory text and
 *   leaves the learner unchanged.  Runs on the table's stream, one launch per pass of step 1, per level of step 2 and for step 3,
 *   with no host wait in between.  bn_learn_get also names "optimal_ns" (device time of all launches, summed over the calls),
 *   "optimal_bps_ns" and "optimal_sink_ns" (steps 1 and 2 of it), and of the last call "optimal_cells" (n * 2^(n - 1)) and
 *   "optimal_bytes" (the device memory of the four tables). */
typedef struct bn_optimal_params {
    int32_t max_parents, pad_;
    const uint64_t *allowed;   /* NULL, or [n] */
    uint64_t pad64_;
} bn_optimal_params;
int bn_learn_optimal(bn_learner *L, bn_term_table *terms, const bn_optimal_params *params, double *value_out, int32_t *order_out,
                     uint64_t *masks_out);

/* ---- Bayesian-Dirichlet scores: BDeu and K2 (Cooper-Herskovits) as family terms of every search above ----
 *
 *   A bn_score_spec names the family term: kind 0 the log-likelihood term ll above (used with AIC / MDL), kind 2 BDeu with the
 *   equivalent sample size ess, kind 3 K2 (ess not read).  Every *_spec entry point is the entry point of the same name with the
 *   term chosen by the spec; a NULL spec or kind 0 gives the bits of the entry point without _spec.  Another kind, or a BDeu ess
 *   that is not finite and within [2^-20, 2^20], is BN_ERR_ARG and nothing is launched.
 *
 *   lgamma_pos(x), finite x > 0, every operation a plain fp64 one (no fused multiply-add), log the DEVICE's fp64 log:
 *     p = 1.0;  while (x < 16.0) { p = p * x;  x = x + 1.0; }                      (at most 16 steps)
 *     r = 1.0 / x;  r2 = r * r;
 *     s = c5; s = s * r2 + c4; s = s * r2 + c3; s = s * r2 + c2; s = s * r2 + c1; s = s * r2 + c0;  s = s * r;
 *         c0 .. c5 = the doubles nearest 1/12, -1/360, 1/1260, -1/1680, 1/1188, -691/360360
 *     v = (((x - 0.5) * log(x)) - x) + HALF_LOG_2PI + s;                          HALF_LOG_2PI = 0x3FED67F1C864BEB4 (0.9189385332046727)
 *     return (the loop ran at least once) ? v - log(p) : v;
 *
 *   The term of a family with child arity kc, R parent configurations (all of them, observed or not) and E = R * kc entries in the
 *   fitted layout:
 *     BDeu: a_r = ess / double(R), a_c = ess / double(E);    K2: a_c = 1.0, a_r = double(kc);
 *     G_r = lgamma_pos(a_r), G_c = lgamma_pos(a_c);
 *     entry r (row j, state s) with count N and row total tot:  t_r = 0.0;
 *       if N != 0:               t_r = lgamma_pos(a_c + double(N)) - G_c;
 *       if s == 0 and tot != 0:  t_r = t_r + (G_r - lgamma_pos(a_r + double(tot)));
 *     bd = the sum of the t_r in ll's order: 256 partial sums (partial t takes r = t, t + 256, ... from +0.0), folded by halves.
 *   bd is the log marginal likelihood of the family's counts; like ll it is a function of the counts and the spec alone (same bits
 *   alone, as a base, as a candidate, out of the subset lattice, in any batch, at any split).  The counts are the same exact N.
 *
 *   bn_learn_create_spec: criteria 0 and 1 take a NULL or kind-0 spec; criterion 2 (BDeu) a kind-2 spec, criterion 3 (K2) a kind-3
 *   spec.  Under criteria 2 and 3 the score is the likelihood alone, no penalty:
 *     likelihood = 0.0; for v = 0 .. n - 1: likelihood -= bd[v];  score = likelihood
 *   that is MINUS the log marginal likelihood: smaller is better, and every "accept iff strictly smaller" rule above holds as it
 *   stands (try_parents, best_parents, the brute-force searches, the chains' and runs' evaluation).  The parameter count is kept and
 *   reported as before.  bn_learn_get also names "criterion".
 *   bn_terms_create_spec: a term table of that term; bn_terms_get also names "score_kind" and "ess_bits" (the bits of ess; 0 for
 *   kinds 0 and 3).  bn_learn_anneal and bn_learn_hc refuse (BN_ERR_ARG, before any launch) a table whose spec is not the
 *   learner's: kinds equal and ess equal in bits; an AIC / MDL learner needs a kind-0 table. */
typedef struct bn_score_spec {
    int32_t kind;   /* 0 log-likelihood term, 2 BDeu, 3 K2 */
    int32_t pad;
    double ess;     /* BDeu's equivalent sample size */
} bn_score_spec;
int bn_learn_score_groups_spec(bn_info_table *table, const bn_score_spec *spec, int32_t n_groups, const int32_t *child,
                               const int32_t *base_ptr, const int32_t *base_idx, const int32_t *cand_ptr, const int32_t *cand_idx,
                               double *ll_out, uint64_t *counts_out);
int bn_learn_score_subsets_spec(bn_info_table *table, const bn_score_spec *spec, int32_t child, int32_t n_base, const int32_t *base,
                                int32_t m, const int32_t *cand, double *ll_out, uint64_t *counts_out);
int bn_learn_create_spec(bn_info_table *table, const int32_t *in_ptr, const int32_t *in_idx, int32_t criterion,
                         const bn_score_spec *spec, int32_t max_parents, bn_learner **out);
int bn_terms_create_spec(bn_info_table *table, const bn_score_spec *spec, int32_t max_parents, bn_term_table **out);

/* ---- conditional-independence tests (G^2) and constraint-based structure learning (PC-stable); not in the reference: the tests of
 *      bnlearn's ci.test "mi" / "mi-adf" and the search of its pc.stable, pgmpy's PC and pcalg. ----
 *
 *   A TEST is (x, y, S): "x independent of y given S", x != y, neither in S, |S| <= 8, S in any order (it is sorted increasing; a
 *   duplicate is BN_ERR_ARG).  Its table has k_x * k_y * prod k_S <= 2^20 cells (bn_learn_score_groups' family limit).
 *     N[s][b][a]  exact uint64 counts: s the mixed-radix index over the sorted S, first column most significant, b the state of y, a
 *                 the state of x, least significant; cell r = (s * k_y + b) * k_x + a.  They are the counts bn_learn_score_groups
 *                 makes for the group "child x, base S, candidate y", taken through the same counting launch: the library groups
 *                 the tests by (x, S) itself, and no result depends on the grouping, the order of the tests, the split
 *                 (BN_LEARN_SPLITS), the passes over the count scratch or the order of the patterns.
 *     marginals   per stratum s: N_s, row sums R[s][b] = sum over a, column sums C[s][a] = sum over b; uint64, exact.
 *     G           over the cells r with N != 0:  t_r = double(N) * log((double(N) * double(N_s)) / (double(R) * double(C))), every
 *                 operation a plain fp64 one, log the DEVICE's fp64 log; the additions are bn_score_nodes': 256 partial sums (partial
 *                 t takes r = t, t + 256, ... from +0.0), folded by halves; G = 2.0 * sum; a G that is not > 0.0 (a rounding below
 *                 zero, -0.0) is +0.0.
 *     df (int64)  df_rule 0, nominal (bnlearn "mi"):  (k_x - 1) * (k_y - 1) * prod k_S;
 *                 df_rule 1, adjusted (bnlearn "mi-adf"):  the sum over the strata with N_s != 0 of
 *                 (rows b with R != 0, minus 1) * (columns a with C != 0, minus 1).
 *     p           chisq_sf(G, df), the chi-square upper tail Q(df / 2, G / 2) as this function (plain fp64 operations, the device's
 *                 log and exp, lgamma_pos above):
 *                   if (df <= 0 || !(G > 0.0)) return 1.0;
 *                   a = 0.5 * double(df);  x = 0.5 * G;  pref = exp(((a * log(x)) - x) - lgamma_pos(a));
 *                   if (x < a + 1.0) {                                  the series for P
 *                     ap = a;  del = 1.0 / a;  sum = del;
 *                     repeat at most 100000 times { ap = ap + 1.0;  del = (del * x) / ap;  sum = sum + del;
 *                                                   if (del < sum * 2^-52) break; }
 *                     q = 1.0 - (sum * pref);
 *                   } else {                                            the continued fraction for Q, modified Lentz
 *                     b = (x + 1.0) - a;  c = 1.0 / 2^-1000;  d = 1.0 / b;  h = d;
 *                     for i = 1 .. 100000 { an = (-double(i)) * (double(i) - a);  b = b + 2.0;
 *                                           d = (an * d) + b;   if (fabs(d) < 2^-1000) d = 2^-1000;
 *                                           c = b + (an / c);   if (fabs(c) < 2^-1000) c = 2^-1000;
 *                                           d = 1.0 / d;  del = d * c;  h = h * del;
 *                                           if (fabs(del - 1.0) < 2^-52) break; }
 *                     q = pref * h;
 *                   }
 *                   if (!(q > 0.0)) return 0.0;   return q > 1.0 ? 1.0 : q;
 *                 Both loops end after about sqrt(2 a log(2^52)) steps (some 6500 at df = 2^20), far below the cap.  Never NaN; a
 *                 vanishing tail is 0.0 or a denormal.
 *     decision    the test is INDEPENDENT iff p > alpha (bnlearn's rule), 0 < alpha < 1.
 *   G, df and p of a test are functions of its counts alone: the same bits alone, twice in a batch, in any batch, inside bn_learn_pc.
 *   bn_ci_tests: tests in CSR form (x, y [n_tests], s_ptr [n_tests + 1], s_idx); stat_out, df_out, p_out [n_tests]; indep_out NULL
 *   or [n_tests] (1: independent); counts_out NULL or every test's N back to back in the order of the tests.  BN_ERR_ARG (the text
 *   names the test, nothing is launched): x == y, x or y in S, a duplicate in S, |S| > 8, an id out of range, more than 2^20 cells,
 *   df_rule not 0 or 1, alpha outside (0, 1).
 *   bn_ci_chisq_sf: p_out[i] = chisq_sf(g[i], df[i]) evaluated ON THE DEVICE (the current one); g finite and >= 0, df >= 0.
 *   bn_info_get "ci_count_ns", "ci_stat_ns": device time of the counting and statistic kernels of the last bn_ci_tests / bn_learn_pc
 *   call on the table (0 after a refused call); "ci_launches": kernels those calls have launched on the table so far.
 *   The environment variable BN_CI_SCRATCH_CELLS (> 0) lowers the cells of the count scratch per pass (default 2^25), so that small
 *   batches take several passes and bn_learn_pc's levels several chunks: a test arrangement, no result depends on it.
 *
 *   bn_learn_pc: the order-independent ("stable") PC skeleton, then orientation.  n <= 1024 columns.
 *     Start: the complete graph over the columns, or start_adj [n][n] (symmetric, the diagonal is not read).
 *     Level l = 0, 1, ..., max_cond (0 .. 8).  With A the adjacency at the START of the level: for every ordered pair (x, y) adjacent
 *     in A with |A(x) \ {y}| >= l, one test (x, y, S) for every S in A(x) \ {y} with |S| = l; at l = 0 only x < y.  The RANK of a test
 *     among those of its edge {x, y} is side * C(|A(min)| - 1, l) + the lexicographic index of S among the l-subsets of
 *     A(x) \ {y}, side 0 when x = min(x, y) and 1 otherwise (C(m, l) = 0 for m < l): increasing (side, S lexicographic).  After the
 *     level the edge is removed iff one of its tests is independent, and sepset(x, y) is the S of its LOWEST-RANK independent test
 *     (on the device one uint32 atomicMin per edge; the host reads back one rank per edge and nothing else).  Every test of a level
 *     is run.  The search stops when no ordered pair qualifies at level l or after level max_cond.
 *     A test over 2^20 cells is not run and counts as dependent; tests_skipped_out sums them.  A level that asks for more than
 *     max_tests tests (over-limit ones included; 0: the default 2^22, at most 2^26) refuses the call with BN_ERR_STATE naming the
 *     level and the number; nothing is trimmed and no output is written.
 *     Orientation (host).  v-structures: for every z, x < y in increasing (z, x, y) with x - z - y, x and y not adjacent, a recorded
 *     sepset(x, y) and z not in it: x -> z <- y; an edge already oriented the other way stays (the first orientation wins).  Then
 *     Meek's R1, R2, R3 to a fixed point: a scan visits the ordered pairs (a, b) in increasing (a, b) and turns an undirected a - b
 *     into a -> b at once if R1 (some c -> a, c and b not adjacent), else R2 (some c with a -> c -> b), else R3 (some c, d not
 *     adjacent with a - c, a - d, c -> b, d -> b) applies; scans repeat until one changes nothing.
 *     Outputs: skeleton_out, cpdag_out [n][n] uint8 marks (both [a][b] and [b][a] set: a - b; only [a][b]: a -> b); sep_len_out
 *     [n][n] (-1: none recorded: the pair is adjacent, or was not adjacent at the start), sep_idx_out [n][n][max_cond] (increasing;
 *     may be NULL when max_cond == 0); levels_out [max_cond + 1] records, *n_levels_out of them written; tests_skipped_out may be NULL.
 *   bn_pdag_to_dag: a consistent DAG extension of a PDAG in the same marks (Dor-Tarsi): while nodes remain, the LOWEST node with no
 *   outgoing directed edge to a remaining node and whose every undirected remaining neighbour is adjacent to all other remaining
 *   nodes adjacent to it takes its undirected edges as incoming and is removed.  in_ptr_out [n + 1], in_idx_out [adjacent pairs],
 *   parents increasing: what bn_learn_create takes.  No such node at some step: BN_ERR_STATE, the PDAG has no extension. */
typedef struct bn_pc_params {
    double alpha;        /* a test is independent iff p > alpha */
    int32_t max_cond;    /* the last level (largest |S|), 0 .. 8 */
    int32_t df_rule;     /* 0 nominal, 1 adjusted */
    int64_t max_tests;   /* per level; 0: 2^22 */
} bn_pc_params;
typedef struct bn_pc_level {
    int64_t tests, removed;     /* tests run at the level; edges it removed */
    double count_ns, stat_ns;   /* device time of its counting and statistic kernels */
} bn_pc_level;
int bn_ci_tests(bn_info_table *table, int32_t n_tests, const int32_t *x, const int32_t *y, const int32_t *s_ptr, const int32_t *s_idx,
                int32_t df_rule, double alpha, double *stat_out, int64_t *df_out, double *p_out, uint8_t *indep_out,
                uint64_t *counts_out);
int bn_ci_chisq_sf(int64_t n, const double *g, const int64_t *df, double *p_out);
int bn_learn_pc(bn_info_table *table, const bn_pc_params *params, const uint8_t *start_adj, uint8_t *skeleton_out, uint8_t *cpdag_out,
                int32_t *sep_len_out, int32_t *sep_idx_out, bn_pc_level *levels_out, int32_t *n_levels_out,
                int64_t *tests_skipped_out);
int bn_pdag_to_dag(int32_t n, const uint8_t *pdag, int32_t *in_ptr_out, int32_t *in_idx_out);

/* ---- layout introspection (host only; valid for BN_DEVICE_HOST_ONLY engines too) ---- */
typedef struct bn_layout_info {
    int32_t n_nodes, n_edges, n_classes, n_tiles;
    int32_t lanes_per_node_max;
    int64_t cpt_doubles, rec_doubles, node_doubles; /* striped device array sizes (one buffer) */
    int64_t algorithmic_bytes_per_sweep, layout_bytes_per_sweep, messages_per_sweep;
    int32_t rank, nranks, n_owned;  /* sharding: this rank's share */
    int32_t n_interior_tiles;       /* tiles [0, n_interior_tiles) touch no cut edge (== n_tiles on one rank) */
    int64_t n_cut_edges;            /* cut edges incident to this rank */
    int64_t segment_bytes;          /* all-gather payload per rank per sweep (residual slots included) */
    int64_t segment_used_bytes;     /* message halves this rank actually produces */
    int64_t exchange_base;          /* start of the exchange region in a record buffer, 16-byte units */
} bn_layout_info;
int bn_layout_get(bn_engine *eng, bn_layout_info *out);
/* per CSR edge: MsgRef {pi, lam} of bn_plan.hpp on this rank ({-1,0}: no owned endpoint) */
int bn_layout_edge_refs(bn_engine *eng, int32_t *pi_out, int32_t *lam_out);
/* node -> lane slot on this rank, -1 for nodes of other ranks, [n] */
int bn_layout_node_slots(bn_engine *eng, int32_t *slots_out);
/* node -> tile on this rank, -1 for nodes of other ranks, [n] */
int bn_layout_node_tiles(bn_engine *eng, int32_t *tiles_out);
/* per-class: kv, m, lanes_per_node, variant (0 = one-lane generic, 1 = register-resident template,
 * 2 = lane group (k = 4, 3-5 parents), 3 = any arities, a group of 8..64 lanes per node) */
/* dataflow tables: nbr_out [n_tiles * bn_get_info("nbr_chunks") * 64] neighbour slots (rank * 2048 + tile, -1 padded),
 * pub_out [n_tiles] bit q = the tile reports to rank q; either may be NULL */
int bn_layout_flow(bn_engine *eng, int32_t *nbr_out, uint32_t *pub_out);
int bn_layout_class(bn_engine *eng, int32_t cls, int32_t *kv, int32_t *m, int32_t *lanes_per_node,
                    int32_t *variant, int32_t *n_nodes);
/* The plan of the one-workgroup path for small networks (csrc/bn_small.hpp; tests emulate the kernel on it):
 * dims_out[12] = n, N (sum of arities), M (sum over edges of the parent's arity), S (CPT entries), T (staged terms),
 * TT (parent terms), CL (child-list entries), waves, re, rb, rc (rounds per item kind), mmax; the arrays (any may be
 * NULL) are sized from those: ent [re * 64 * waves][2], ent_cpt [re * 64 * waves], term [TT], clist [CL],
 * bslot [rb * 64 * waves][4], cslot [rc * 64 * waves][4], npi_init [N].  BN_ERR_STATE: the network is not eligible. */
int bn_small_plan_get(bn_engine *eng, int32_t *dims_out, uint32_t *ent, double *ent_cpt, uint32_t *term, uint16_t *clist,
                      uint32_t *bslot, uint32_t *cslot, double *npi_init);
/* ... of part `part` (0 .. bn_get_info "mid_parts" - 1) of the plan that spreads a mid-size network over several workgroups
 * (csrc/bn_mid.hip): same arrays; message and node-vector indices are global, staging places the part's own;
 * dims_out[14]: the twelve values above, then the part's node range [v0, v1). */
int bn_mid_plan_get(bn_engine *eng, int32_t part, int32_t *dims_out, uint32_t *ent, double *ent_cpt, uint32_t *term, uint16_t *clist,
                    uint32_t *bslot, uint32_t *cslot, double *npi_init);

/* The plan of the register-resident DAG path (csrc/bn_dag.hpp: networks of arity <= 4 with <= 5 parents per node; tests emulate the
 * kernel on it).  dims_out[8] = n, E, tiles, blocks, stream (1: some wave walks several tiles per iteration), child tiles, parent
 * tiles, doubles of the CPT image; the arrays (any may be NULL) are sized from those: tiles [tiles][8] (kind, active nodes / items,
 * first per-lane entry, first double2 of the CPT image, largest child count, 3 unused), slot_ptr [blocks * 8 + 1], cnode
 * [tiles * 64][2] (node, first in-edge), pitem [tiles * 64][4] (node, target out-edge or -1, first out-edge entry, child count |
 * target's rank << 16), oedge [max(E, 1)], cpt_img [dims_out[7]], npi_init [4 n].  BN_ERR_STATE: the network is not eligible. */
int bn_dag_plan_get(bn_engine *eng, int32_t *dims_out, int32_t *tiles, int32_t *slot_ptr, int32_t *cnode, int32_t *pitem,
                    int32_t *oedge, double *cpt_img, double *npi_init);

#ifdef __cplusplus
}
#endif
#endif /* BN_MI355X_H */
