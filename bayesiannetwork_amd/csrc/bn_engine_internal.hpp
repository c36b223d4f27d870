// bn_engine_internal.hpp -- what the translation units of the C ABI (include/bn_mi355x.h) share: the engine object and the helpers
// that more than one of them uses -- among them the one guard of the compute entry points (refuse_unusable), the one validation of
// a call's evidence sets (check_evidence_sets) and the one device image of the item tables (ItemImage, upload_items, put_items);
// mapped page-locked buffers are MappedBuf (bn_buffer.hpp): block, device alias and capacity in one owner.  bn_engine.cpp: evidence, the steps of a run with one launch per sweep, options, info, read-out,
// messages; bn_engine_create.cpp: bn_create / bn_destroy, the device set-up one step per path, the stream pool, ensure_dag;
// bn_engine_paths.cpp: the one-launch paths of a single query, their dispatch (run_device_impl) and "autotune";
// bn_engine_policy.hpp / .cpp: which path runs a query, as pure host functions of a few facts (no HIP: checked stand-alone on a
// CPU), for one query and for a batch; bn_engine_batch.cpp: several evidence sets per call -- buffers, evidence staging, the second
// (dense) engine, the entry points and their dispatch; bn_engine_batch_paths.cpp: the five runs of a batch and what they share;
// bn_batch_stage.hpp / .cpp: the layout of a batch's evidence staging block (no HIP either); bn_engine_shard.cpp: RCCL communicator
// and the in-kernel exchange of sharded engines; bn_engine_tools.cpp: plan / layout introspection, bn_reload_cpt, the samplers' and
// the fit's entry points; bn_engine_mpe.cpp, bn_engine_em.cpp, bn_engine_jt.cpp, bn_engine_jt_em.cpp, bn_engine_gibbs.cpp: max-product,
// expectation-maximisation, junction-tree propagation, exact expectation-maximisation and Gibbs sampling, each over a state of its own.  No CPU compute path exists in any of them: every result comes from the
// kernels.
#ifndef BN_ENGINE_INTERNAL_HPP
#define BN_ENGINE_INTERNAL_HPP
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include <dlfcn.h>
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#include <rccl/rccl.h>  // types only: the library is loaded lazily with dlopen (no link dependency)

#include "bn_device.hpp"
#include "bn_fit.hpp"
#include "bn_lw.hpp"
#include "bn_small.hpp"
#include "bn_dag.hpp"
#include "bn_buffer.hpp"
#include "bn_engine_policy.hpp"
#include "bn_batch_stage.hpp"
#include "bn_maxprod.hpp"
#include "bn_em.hpp"
#include "bn_jt.hpp"
#include "bn_gibbs.hpp"

using namespace bnmi;

struct bn_engine;
namespace bn_eng __attribute__((visibility("hidden"))) {
extern thread_local std::string g_err;   // bn_last_error (per thread)
int fail(int code, const std::string& msg);
}  // namespace bn_eng
using namespace bn_eng;


// Entry points run on the engine's device and leave the calling thread's current device as they
// found it (a caller may drive another GPU from the same thread).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t enter(int device) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) return e;
        if (prev == device) return hipSuccess;
        e = hipSetDevice(device);
        switched = e == hipSuccess;
        return e;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define ON_DEVICE(e)            \
    DeviceGuard guard_;         \
    HIPCHK(guard_.enter((e)->device))


#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(BN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)

// RCCL entry points, resolved at the first bn_comm_* call.  In a process that already loaded
// librccl.so.1 (e.g. through torch) the same copy is reused.
struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;   // (optional: bn_get_info "rccl_ranks")
};

// The register-resident DAG path's device image for single queries: uploaded whole by ensure_dag, or not at all.
struct DagImage {
    DeviceBuf<DagTile> tiles;
    DeviceBuf<int32_t> slotptr;
    DeviceBuf<DagChildLane> cnode;      // (tiles, parent lanes and out-edges: with state records in place of CSR ids, build_dag_device_tables)
    DeviceBuf<DagParentLaneDev> pitem;
    DeviceBuf<int32_t> oedge;
    DeviceBuf<int32_t> eperm;           // CSR edge id -> message record, node id -> slot of its vectors
    DeviceBuf<int32_t> nperm;
    DeviceBuf<double> cpt;
    DeviceBuf<double> init;
    DeviceBuf<int32_t> k;               // networks with arities below 4 (DagPlan::uniform4 == false): arity, in-edge CSR and marginal offsets for the padded form
    DeviceBuf<int32_t> inptr;
    DeviceBuf<int32_t> inidx;
    DeviceBuf<int64_t> noff;
    DeviceBuf<double> state;            // pi-/lambda-messages (CSR edge order), pi(v), lambda(v): two buffers each (bn_dag.hpp dag_off_*)
    DeviceBuf<uint8_t> frz;
    DeviceBuf<ResidentSync> sync;
    DeviceBuf<int32_t> nbr;             // dataflow form (dag_flow_ok): neighbour tiles, granule table + verdict words
    DeviceBuf<DagFlowSync> flow;
};

// The item tables of the one-workgroup and the several-workgroup kernels (bn_small.hpp) on the device: one image per plan -- the
// engine's two, and the one max-product builds for itself.  upload_items fills one, put_items hands it to a kernel's arguments.
struct ItemImage {
    DeviceBuf<SmallEntry> ent;
    DeviceBuf<double> ent_cpt;
    DeviceBuf<uint32_t> term;
    DeviceBuf<uint16_t> clist;
    DeviceBuf<SmallSlot> bslot, cslot;
    DeviceBuf<int32_t> nv_idx, nv_slot;
    DeviceBuf<double> npi_init;
    DeviceBuf<int32_t> node_off;
    DeviceBuf<MidPart> parts;           // several workgroups only: each one's share, and the first message element of a node's in-edges
    DeviceBuf<int32_t> msg_first;
};

// Scoring (bn_score.cpp): the log of the flat CPT and the model's structure as the scoring kernels read them, made at the
// first bn_score_* call; bn_reload_cpt clears `ready`, so the next call takes the logarithms of the new tables.
struct ScoreState {
    bool ready = false;
    std::vector<double> h_L;            // [entries] std::log(cpt_flat[q]) (fp64, libm)
    bool wide = false;                  // some node's table has >= 2^32 entries
    int32_t splits = 0;                 // option "score_splits": workgroups per node of the counting pass (0: chosen from the shapes)
    DeviceBuf<double> d_L;
    DeviceBuf<int32_t> d_k, d_in_ptr, d_in_idx;
    DeviceBuf<int64_t> d_cpt_off;
    float last_rows_ms = 0.0f, last_count_ms = 0.0f, last_nodes_ms = 0.0f;   // device-event times of the last calls' kernels
};

// Max-product (bn_engine_mpe.cpp, bn_maxprod.hip): everything its runs need beyond the item tables of the sum-product paths, allocated at
// the first run.  Nothing here is read or written by a bn_bp_* call, and a bn_mpe_* call touches nothing else of the engine.
struct MpeState {
    int form_option = 0;            // option "mpe_form": 0 the rule (bn_policy::mpe_form), 1 one workgroup, 2 several workgroups
    int group = kMpeDefaultGroup;   // option "mpe_group": sweep launches between two reads of the control record (several-workgroup form)
    bool small_ready = false, mid_ready = false;   // the form's kernels are prepared, its state allocated
    DeviceBuf<int32_t> d_elem_node; // [N] node of a node-vector element (the lanes that decode a node's state)
    int32_t cap_sets = 0, res_cap = 0;   // what the per-set buffers below were sized for
    MappedBuf<double> h_mm;         // [cap_sets][N] max-marginals: mapped, the kernels write them here themselves (no copy command
                                    //   behind the run: the results are there when the run's one synchronisation returns)
    MappedBuf<int32_t> h_states;    // [cap_sets][n], the same
    DeviceBuf<double> d_res_hist;   // [cap_sets][res_cap]
    MappedBuf<MpeCtl> h_ctl;        // [cap_sets], mapped: the kernels write it themselves
    MappedBuf<char> h_ev;           // the staging block of the call's evidence (bn_batch_stage.hpp), mapped: read in place
    DeviceBuf<double> d_s_state;    // one workgroup: [small_state_sets][2 M + 2 N] the state each set's run stopped in
    int32_t small_state_sets = 0;
    DeviceBuf<double> d_m_state;    // several workgroups: pi[2][M], lam[2][M], npi[2][N], nlam[2][N]
    DeviceBuf<uint8_t> d_m_frz;
    DeviceBuf<MpeMidSync> d_m_sync;
    // A network the engine has no several-workgroup plan for because ONE workgroup holds it (bn_create builds that plan only for the
    // others, and the sum-product path choice must not see one here): option "mpe_form" 2 builds a plan and tables of the max-product
    // run's own at its first use; bn_reload_cpt drops them.
    MidPlan own_mid;
    bool own_tried = false, own_uploaded = false;
    ItemImage own_img;
    uint32_t run_id = 0;
    // the last call
    bool have_run = false, last_single = false;
    int last_form = 0;
    int32_t n_sets = 0, last_groups = 0;
    int64_t last_device_ns = 0;
    std::vector<int32_t> sweeps;
};

// What the two expectation-maximisation states below share, and all that the loop of both (em_drive, bn_engine_em.cpp) works on:
// theta, the sums, the table, the scratch of family posteriors, the M-step's row array -- allocated by em_reserve.
struct EmCore {
    int64_t scratch_cells;              // option "em_scratch_cells" / "jt_em_scratch_cells": doubles of the posteriors' scratch array
    bool ready = false;                 // theta, sums, words allocated, the row array uploaded, the events created
    DeviceBuf<double> d_theta;          // [entries] flat
    DeviceBuf<double> d_E, d_partial;   // [entries] the sum, and the 256-block in hand
    DeviceBuf<unsigned long long> d_words;   // [0] runs cut by the cap, [1] skipped families, [2] delta's bit pattern, [3] L (a double)
    DeviceBuf<bn_policy::EmRow> d_row;  // [entries] bn_policy::em_rows
    DeviceBuf<uint8_t> d_patterns;      // the table of the call
    DeviceBuf<unsigned long long> d_counts;
    int64_t cap_patterns = 0;
    DeviceBuf<double> d_b;              // [rows of a launch][entries] family posteriors of the launch in hand
    int64_t cap_b = 0;
    EventOwner ev[3];                   // E-step begins, E-step ends, M-step ends
    // the last call
    int32_t last_iters = 0;
    int64_t skipped = 0, estep_ns = 0, mstep_ns = 0;
};

// Expectation-maximisation (bn_engine_em.cpp, bn_em.hip): its own images of the CPT values (the entry items' table, the roots' initial
// pi(v)) and the index maps between them and the flat array, beside the core -- allocated at the first call.  Nothing here is read or
// written by a bn_bp_* / bn_mpe_* / bn_jt_em_* call, and a bn_em_* call touches nothing else of the engine.
struct EmState {
    EmCore core{bn_policy::kEmScratchCells};
    bool ready = false;                 // kernels prepared, maps uploaded, images allocated
    std::vector<int32_t> slot_of;       // [entries] flat CPT entry -> its slot in the entry items' table
    std::vector<int32_t> init_of;       // [entries] flat CPT entry -> element of the initial pi(v) (a root's), -1: none
    DeviceBuf<int32_t> d_ent_flat;      // [slots] the inverse | (first entry of its family) << 16, -1: no entry
    DeviceBuf<int32_t> d_slot_of, d_init_of;
    DeviceBuf<double> d_cpt, d_init;    // the images the E-step kernel reads, rewritten by every M-step
    DeviceBuf<int32_t> d_sweeps;        // [patterns] of the last E-step
    int64_t cap_rows = 0;
    int64_t capped = 0;                 // the last call
};

// Junction-tree propagation (bn_engine_jt.cpp, bn_jt.hip): the plan (built at the first call that asks for it), its tables on the
// device, the base potentials, scratch and outputs -- allocated at the first run.  Nothing here is read or written by a bn_bp_* /
// bn_mpe_* / bn_em_* call, and a bn_jt_* call touches nothing else of the engine.
struct JtState {
    int form_option = 0;                // option "jt_form": 0 the rule (jt_form), 1 state in LDS, 2 state in device scratch
    int64_t scratch_cells = kJtScratchCells;   // option "jt_scratch_cells"
    JtPlan plan;
    bool tried = false;                 // the planner has run (bn_get_info "jt_eligible", the plan calls, the first run)
    bool uploaded = false;              // the item tables are on the device
    bool psi_ready = false;             // ... and the base potentials of the CPTs in force
    DeviceBuf<JtClique> d_cliques;
    DeviceBuf<JtLevel> d_levels;
    DeviceBuf<JtNode> d_nodes;
    DeviceBuf<int32_t> d_ent_clique, d_dn_map, d_sep_clique, d_c_base, d_p_base, d_c_res, d_p_res, d_up_map, d_home_nodes, d_elem_node, d_asg_ptr;
    DeviceBuf<JtAsg> d_asg;
    DeviceBuf<JtFam> d_fam;
    DeviceBuf<double> d_cpt, d_psi0;
    DeviceBuf<double> d_scratch;        // form 2: [scratch_slots][state_cells]
    int64_t scratch_slots = 0;
    DeviceBuf<int32_t> d_ev_slot;       // [ev_slots][n]
    int64_t ev_slots = 0;
    DeviceBuf<double> d_beliefs, d_scales;   // [cap_sets][N], [cap_sets][nc]
    DeviceBuf<int32_t> d_states;        // [cap_sets][n]: the assignment a max run decodes (bn_jt_mpe_run)
    int32_t cap_sets = 0;
    MappedBuf<char> h_ev;               // the staging block of the call's evidence (bn_batch_stage.hpp), mapped: read in place
    // the last call
    bool have_run = false;
    int last_form = 0;
    int last_kind = 0;                  // JtKind: 1 a sum run (bn_jt_run*), 2 a max run (bn_jt_mpe_run*)
    int32_t n_sets = 0, last_launches = 0;
    int64_t last_kernel_ns = 0;         // option "timing": HIP events around the run's launches
    std::vector<double> scales;         // [n_sets][nc]
};

// Exact expectation-maximisation (bn_engine_jt_em.cpp, jt_em_kernel of bn_jt.hip): the family tables on the device, the base
// potentials of its theta and, in form 2, the scratch of the rows' states, beside the core -- allocated at the first call.  It reads
// the junction tree's plan and item tables; nothing else of the engine is read or written, and nothing here by any other call family.
struct JtEmState {
    EmCore core{bn_policy::kJtEmScratchCells};
    bool ready = false;                 // family tables uploaded, potentials allocated
    DeviceBuf<JtFamily> d_families;
    DeviceBuf<int32_t> d_f_node, d_f_base, d_f_res;
    DeviceBuf<double> d_psi0;           // [pot_cells] the base potentials of theta
    DeviceBuf<double> d_loglik;         // [patterns] of the last E-step
    DeviceBuf<int32_t> d_skipped;       // [patterns] of the last E-step
    int64_t cap_rows = 0;
    DeviceBuf<double> d_scratch;        // form 2: [rows of a launch][state_cells]
    int64_t cap_scratch = 0;
    int32_t last_form = 0;              // the last call
    int64_t last_launches = 0;
};

// Gibbs sampling (bn_engine_gibbs.cpp, bn_gibbs.hip): the plan (built at the first call that asks for it), its tables and its own
// copy of the flat CPTs on the device, the chains' states, the histogram -- allocated at the first run.  A bn_gibbs_run call
// that starts its chains itself draws them with the sampler (bn_lw_run's state, as a bn_lw_run call of the same range leaves it);
// nothing else of the engine is read or written, and nothing here by any other call family.
struct GibbsState {
    int32_t sweeps_option = 0;          // option "gibbs_sweeps_per_launch" (0: the plan's default)
    GibbsPlan plan;
    bool tried = false;                 // the planner has run
    bool uploaded = false;              // the tables are on the device
    bool cpt_ready = false;             // ... and the CPTs in force
    DeviceBuf<int32_t> d_colour_ptr;
    DeviceBuf<GibbsSlot> d_slots;
    DeviceBuf<GibbsChild> d_children;
    DeviceBuf<GibbsTerm> d_terms;
    DeviceBuf<double> d_cpt;
    DeviceBuf<int16_t> d_clamp;         // [n]
    DeviceBuf<unsigned long long> d_words;   // [cells] the histogram, then [1] the stuck count
    DeviceBuf<uint8_t> d_states;        // [cap_chains][n]
    uint64_t cap_chains = 0;
    // the last call
    int64_t last_launches = 0, last_kernel_ns = 0;
};

struct bn_engine {
    Plan plan;
    bool host_only = true;
    int64_t create_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // bn_get_info "create_us_{plan,small,mid,dag,device}"
    bool poisoned = false;          // a bn_reload_cpt upload failed half-way: device images of mixed age, every compute call is refused
    int device = -1;
    hipStream_t stream = nullptr;
    // device images
    DeviceBuf<TileDesc> d_tiles;
    DeviceBuf<ClassDesc> d_classes;
    DeviceBuf<FlatEntry> d_flat_tab;
    DeviceBuf<double> d_cpt;
    DeviceBuf<double> d_rec[2];
    DeviceBuf<double> d_node[2];
    DeviceBuf<MsgRef> d_out;
    DeviceBuf<MsgRef> d_inrefs;
    ncclComm_t comm = nullptr;
    hipStream_t comm_stream = nullptr;   // sharded runs: the all-gathers run here, beside the interior tiles' launch
    hipEvent_t ev_swept = nullptr;       // main stream: every tile of the current sweep has been launched
    hipEvent_t ev_gathered = nullptr;    // comm stream: the current sweep's all-gather
    bool overlap = true;                 // BN_OVERLAP=0 / bn_set_option("overlap", 0): kernel and collective back to back
    DeviceBuf<uint8_t> d_frozen;
    uint8_t frozen_mark = 1;        // mark value of the evidence set in force (1..255; wrapping clears the array)
    DeviceBuf<int32_t> d_slot_node;
    DeviceBuf<int64_t> d_slot_boff;
    DeviceBuf<int32_t> d_node_tile;
    DeviceBuf<int32_t> d_node_nl;
    DeviceBuf<double> d_res_hist;
    DeviceBuf<Ctl> d_ctl;
    DeviceBuf<double> d_beliefs;
    // evidence staging: one pinned host block the device reads mapped (the evidence kernel reads it in place), sub-pointers into h_ev.dev()
    MappedBuf<char> h_ev;
    int32_t ev_ne = 0;
    int32_t ev_nval = 0;            // values of the evidence in force (sum of the observed nodes' arities)
    int32_t* d_ev_node = nullptr;
    int32_t* d_ev_off = nullptr;
    double* d_ev_val = nullptr;
    bool ev_applied_dirty = false;  // an evidence launch failed: marks unknown, clear them at the next set
    bool rows_clean = true;         // residual slots are zero (left so by the last finish kernel / the reset kernel)
    uint32_t run_id = 0;            // id of the current / last run (bn_device.hpp Ctl)
    bool nontemporal = false;
    bool timing = false;            // HIP events around each batch of sweeps (bn_bp_stats.sweep_kernel_ms); opt-in:
                                    // an event record between two launches opens a ~6 us bubble in the queue
    bn_policy::PathFacts facts;     // what the path choice reads of the plans below (path_facts_of: bn_create, and wherever a plan is rebuilt)
    bn_policy::ResidentShape shape; // the resident kernel's launch shape and eligibility on this device (plan_resident, at bn_create)
    // A launch of the resident kernel that gives up a bounded wait (its blocks were not all co-resident: another
    // process or engine held CUs) sends this and the next `resident_cooldown` runs down the per-sweep launches;
    // after that the resident path is tried again, and a repeated abort doubles the pause (<= 1024 runs).
    int32_t resident_aborts = 0;    // launches that gave up, over the engine's life (bn_bp_stats.resident_aborts)
    int32_t resident_cooldown = 0;  // runs left before the resident path is tried again
    int32_t resident_backoff = 8;   // length of the next pause
    MappedBuf<double> h_beliefs;    // pinned: bn_bp_run_view hands this out, bn_bp_run stages nothing through it
    double* beliefs_override = nullptr;  // where the kernels write the beliefs of the run in hand instead of d_beliefs
    bool beliefs_on_host_only = false;   // the last run wrote its marginals into h_beliefs, not d_beliefs (synced back on demand)
    int beliefs_direct = 1;         // option "beliefs_direct": bn_bp_run_view lets the kernels write the marginals straight into
                                    // the mapped host buffer (no copy command behind the run; 316x316 grid: 253 -> 235 us per query);
                                    // outputs above 16 MB go through the copy engine (larger PCIe payloads)
    std::vector<uint32_t> ev_seen;  // check_evidence: epoch stamp per node (no per-call allocation)
    uint32_t ev_epoch = 0;
    bool ev_upload_pending = false; // an evidence H2D from h_ev may still be in flight (no sync since)
    int resident_poll_margin = 30;  // direct form: 10 ns ticks between the predicted arrival of the last block and a block's first poll (BN_RESIDENT_DELAY)
    int resident_direct = 1;        // option "direct" / BN_RESIDENT_DIRECT: the grid barrier without a service block (bn_resident.hip wait_verdict);
                                    // measured against the service block, us per sweep: 32 x 32 grid 6.98 -> 6.46, 128 x 128 7.25 -> 6.80, 316 x 316 11.46 -> 11.04
    DeviceBuf<ResidentSync> d_rsync;
    bool rsync_dirty = true;        // the sync block must be zeroed before the next launch
    // First-sweep image of the resident path (option "memo0" / BN_MEMO0; bn_device.hpp Memo0Args, bn_engine_memo.cpp): what sweep 0
    // leaves behind, built at the first run that can use it, kept right per evidence set by the evidence launch (flush_evidence)
    struct Memo0 {
        int enabled = 1;
        bool valid = false;             // built from the CPT image in force; the slots of `applied` hold those nodes as evidence nodes
        DeviceBuf<double> d_rec, d_node, d_cv;   // records and node vectors in the layout of rec1 / node1; [n] contributions
        DeviceBuf<unsigned long long> d_words;   // [0], [1]: sweep 0's residual, written by the patch launches in turn (each leaves the
                                                 // other zero); [2]: the largest contribution of all (no evidence, nothing to restore)
        DeviceBuf<Memo0Image> d_img;    // [3] what the resident kernel reads: the two buffers and word q
        int word = 2;                   // the word that holds sweep 0's residual for the evidence the image holds
        int next_word = 0;              // the (zero) word of the next patch launch
        MappedBuf<int32_t> h_restore;   // [n] mapped: the nodes that lose their evidence, read in place by the patch launch
        std::vector<double> cv;         // [n] host copy of the contributions
        std::vector<int32_t> order;     // nodes by descending contribution
        std::vector<int32_t> applied;   // the evidence set the image holds
        std::vector<int32_t> restore;
        std::vector<uint32_t> stamp;    // membership of the set in hand (bn_policy::memo0_stamp)
        uint32_t epoch = 0;
        double const_residual = 0.0;    // largest contribution among the nodes outside `applied`
    } memo;
    // Second-sweep image (option "memo1" / BN_MEMO1; bn_device.hpp Memo1Args, bn_engine_memo.cpp): what sweep 1 leaves behind, built
    // together with the first-sweep image, kept right per evidence set by a launch behind the first-sweep patch
    struct Memo1 {
        int enabled = 1;
        bool built = false;             // the buffers hold the image of the CPTs in force, right for the evidence set `applied`
        bool holds = false;             // ... and `applied` is the set in force: a run may start at sweep 2
        int oneshot = 0;                // BN_MEMO1_ONESHOT: 1 = a set that arrives with its single run (bn_bp_run, bn_bp_run_view) patches
                                        // too; measured on the headline, the launch then costs more than the iteration it saves (EXP R20.2)
        int64_t limit = 1 << 15;        // BN_MEMO1_LIMIT: most (|E| + |R|) x (1 + max degree) a set may cost and still patch (EXP R20.4)
        DeviceBuf<double> d_rec, d_node, d_cv;   // records and node vectors in the layout of rec0 / node0; [n] contributions
        DeviceBuf<unsigned long long> d_words;   // as Memo0::d_words, for sweep 1's residual
        DeviceBuf<Memo0Image> d_img;    // [9] what the resident kernel reads: record 3 * (first-sweep word) + (second-sweep word)
        DeviceBuf<int32_t> d_adj_off, d_adj;     // node-level CSR: parents, then children
        int word = 2, next_word = 0;
        MappedBuf<int32_t> h_list;      // [n] mapped: E then R, read in place by the patch launch
        std::vector<double> cv;         // [n] host copy of the pristine contributions
        std::vector<int32_t> order;     // nodes by descending contribution
        std::vector<int32_t> adj_off, adj;
        int32_t max_degree = 0;
        std::vector<int32_t> applied;   // the evidence set the image holds (its own list: a set over the limit leaves it alone)
        std::vector<int32_t> list;
        double seed = 0.0;              // largest pristine contribution outside N[E] for the set in force
    } memo1;
    bool ev_one_shot = false;       // the evidence in force arrived in the call that runs it once (bn_bp_run, bn_bp_run_view)
    // dataflow form of the resident kernel (no grid barrier; single evidence set, more than one tile block)
    int poll_sleep = 2;             // option "poll_sleep" / BN_POLL_SLEEP: pause between two polls of a waiting tile (x 512 cycles)
    int flow = 0;                   // option "flow" / BN_RESIDENT_FLOW: 1 = dataflow form where eligible, 0 = grid barrier per sweep
                                    // (the default on one GPU: measured equal per sweep, and the lagging stop decision costs one
                                    // speculative iteration per run; sharded engines exchange through the dataflow form)
    DeviceBuf<FlowSync> d_flow;
    bool flow_dirty = true;
    uint32_t flow_gen_base = 0;
    DeviceBuf<int32_t> d_nbr;
    // sharded engines: halo exchange inside the resident kernel (bn_peer_export / bn_peer_import)
    bool shard_flow_ok = false;     // ... on every rank, and the peers' buffers are mapped: the dataflow form exchanges in-kernel
    bool fine_grained = false;      // record buffers / sync block allocated fine-grained (peers store into them)
    uint32_t shard_run_seq = 0;     // bn_bp_run_device calls on this sharded engine: every rank counts alike -> same generations
    DeviceBuf<PeerTable> d_peers;
    DeviceBuf<uint32_t> d_pub_mask;
    std::vector<uint32_t> pub_mask; // host copy (introspection)
    std::vector<void*> ipc_opened;  // hipIpcOpenMemHandle results to close
    MappedBuf<unsigned> h_abort;    // pinned + mapped: set by a kernel that gives up a bounded wait
    uint32_t gen_base = 0;          // barrier generations used so far on d_rsync
    // several evidence sets per launch (bn_bp_*_batch): per-set records, node vectors, marks, beliefs, histories
    struct Batch {
        int32_t n_sets = 0, cap_sets = 0;
        DeviceBuf<double> d_rec[2];
        DeviceBuf<double> d_node[2];
        DeviceBuf<uint8_t> d_frozen;
        DeviceBuf<double> d_beliefs;
        DeviceBuf<double> d_res_hist;
        DeviceBuf<ResidentSync> d_sync;  // resident path: [min(cap_sets, kResidentMaxSets)]
        bool sync_dirty = true;
        uint32_t gen_base = 0;
        DeviceBuf<double> d_s_state;  // one-workgroup path (bn_small.hip): [cap_sets][2 M + 2 N]
        // register-resident DAG path (bn_dag.hip), several sets per launch: [dag_sets] states, marks, barrier words (allocated at first use)
        DeviceBuf<double> d_g_state;
        DeviceBuf<uint8_t> d_g_frz;
        DeviceBuf<ResidentSync> d_g_sync;
        int32_t dag_sets = 0;
        uint8_t dag_mark = 0;
        bool dag_ev_applied = false;  // state slot q holds set q's evidence under mark dag_mark (a batch of at most kDagMaxSets sets on a network
                                      // without padding: an observed node's vectors are carried over by every sweep, so they outlive the run)
        bool dag_sync_dirty = true;
        uint32_t dag_gen_base = 0;
        bool ev_deferred = false;     // the sets' evidence sits in d_ev only (read there by that kernel); d_ev_meta: per set {count, first node / offset / value}
        int32_t* d_ev_meta = nullptr;   // (inside the staging block)
        MappedBuf<char> h_ev;           // small networks: the staging block is page-locked host memory the kernels read in place
        char* ev_base = nullptr;        // the staging block of the batch in force as the device sees it: d_ev, or h_ev.dev()
        MappedBuf<double> h_beliefs;    // small networks, bn_bp_run_batch: the kernel writes every set's marginals here (mapped) ...
        bool direct_out = false;        // ... when this is set for the run at hand
        bool beliefs_on_host = false;   // the last run's marginals are in h_beliefs, not d_beliefs
        bn_stage::BatchLayout ev_layout;   // where the arrays and each set's entries start inside the staging block
        DeviceBuf<Ctl> d_ctl;       // per-sweep launches: one control block per set
        bool rows_clean = true;     // ... and every set's residual slots are zero
        int32_t predicted_sweeps = 0;
        MappedBuf<Ctl> h_ctl;       // pinned + mapped, [cap_sets]
        DeviceBuf<char> d_ev;       // staging of every set's evidence
        size_t ev_cap = 0;
        // host copy of the evidence (sets run one after another when the network is not resident-eligible)
        std::vector<int32_t> ne, ev_node, ev_off;
        std::vector<double> ev_val;
        std::vector<int32_t> sweeps;
        std::vector<double> residual;
        bool have_run = false;
    } batch;
    bool batch_on_dense = false;    // the current batch lives in `dense`
    bool dense_refused = false;     // the dense layout would give some node's sums another order than this engine's single queries: batches stay here
    bn_engine* dense = nullptr;     // a second engine with the dense layout: batches on a network whose own layout trades
                                    // wavefront count for one query's latency (Plan::latency_rules_applied) run there
    // small networks: the whole run in ONE workgroup with the state in LDS (bn_small.hip)
    SmallPlan small;
    bool small_ok = false;
    int small_mode = 1;             // option "small": 0 never, 1 where it was measured faster than the other paths, 2 wherever eligible
    ItemImage small_img;
    DeviceBuf<double> d_s_state;    // [2 M + 2 N] the state the last launch stopped in
    // networks beyond one workgroup's LDS, spread over up to 32 (bn_mid.hip): the same items, state in device memory
    MidPlan mid;
    bool mid_ok = false;
    int mid_mode = 1;               // option "mid": 0 never, 1 where eligible and the resident tiles do not cover the network, 2 wherever eligible
    int32_t small_cooldown = 0;     // (never set: the one-workgroup path waits for nobody; the path table wants a member)
    int32_t mid_cooldown = 0, mid_aborts = 0;   // runs left on the tile kernels after a grid wait gave up; how often that happened
    ItemImage mid_img;
    DeviceBuf<double> d_m_state;    // [4 M + 4 N]: pi[2][M], lam[2][M], npi[2][N], nlam[2][N]
    DeviceBuf<uint8_t> d_m_frz;
    DeviceBuf<char> d_m_sync;       // per state slot kMidSyncBytes: the barrier counter, the three residual words, the group counters
    int32_t mid_slots = 0;          // state slots allocated (1 for single queries; batches run several sets per launch)
    int32_t n_cus = 0;
    // k = 4 networks with up to 5 parents per node (BASELINE configs[1]): child tiles with the CPT in registers + parent items on
    // waves of their own, state in device memory, one launch per run (bn_dag.hip)
    DagPlan dag;
    bool dag_ok = false;            // eligible on this device (the LIGHT plan is in e->dag)
    bool dag_flow_ok = false;       // the plan has a dataflow form (<= 64 neighbour tiles per tile, one tile per wave, > 1 block) and the service block fits
    int dag_flow = 0;               // option "dagflow" 1: single queries take the dataflow form where it exists (default 0: measured slower, EXPERIMENTS R6.2)
    int32_t dag_flow_pause = 0;     // runs left on the barrier form after a dataflow launch gave up a wait
    int32_t dag_flow_max_nbr = 0;
    int last_dag_flow = 0;
    bool dag_ready = false;         // full plan built, device tables and image uploaded (ensure_dag)
    int32_t dag_cap = 224;          // the block cap the plan was built for
    int dag_mode = 1;               // option "dag": 0 never, 1 where eligible and no other one-launch path takes the network, 2 wherever eligible
    int32_t dag_cooldown = 0, dag_aborts = 0;   // runs left on the tile kernels after a grid wait gave up; how often that happened
    DagDeviceTables dag_tables;             // (host copy, built with the plan -- also on host-only engines, where the CPU sanitizer run walks it; bn_bp_messages reads eperm)
    DagImage dag_img;
    uint8_t dag_mark = 0;           // mark value of the evidence set applied to dag_img.state / frz
    bool dag_ev_applied = false;    // ... and whether that is the set in force
    bool dag_sync_dirty = true;
    uint32_t dag_gen_base = 0;
    bool ev_deferred = false;       // the evidence in force sits in the staging block only: the one-workgroup kernel reads it there
                                    // itself (no evidence launch in front of the run); the tile buffers get it -- marks, vectors --
                                    // when another path needs them (flush_evidence)
    bool autotune_pending = false;  // option "autotune": the next run first times every eligible path on the staged evidence and keeps the fastest
    int32_t autotuned_path = -1;    // ... the path it kept (bn_bp_last_path numbering), -1: never tuned
    bool abort_reported = false;    // the one stderr line about a one-launch path that gave up a bounded wait has been printed
    int multisweep = 1;             // resident one-launch path: 0 never, 1 where it was measured faster (one block, or
                                    // >= kResidentMinTiles tiles), 2 wherever eligible (tests, experiments)
    int32_t last_path = 0;          // 0 per-sweep launches, 2 one launch for the whole run (resident tiles), 3 one workgroup, state in LDS (bn_small.hip)
    int32_t last_flow = 0;          // ... in its dataflow form
    MappedBuf<Ctl> h_ctl;           // pinned + mapped: the finishing kernels write it themselves
    // run state
    int32_t res_cap = 1 << 16;
    int32_t predicted_sweeps = 0;
    bool have_run = false;
    Ctl last_ctl{};
    bn_bp_stats stats{};
    std::vector<hipEvent_t> events;  // (begin, end) per sweep batch
    int grid_tiles = 0;              // blocks for one-wave-per-tile kernels without remap
    LwState lw;
    ScoreState score;
    MpeState mpe;
    EmState em;
    JtState jt;
    JtEmState jt_em;
    GibbsState gibbs;
};


// ---- the one-launch execution paths of a single query: one driver per path ------------------------------------------------------
// wanted(): eligible AND chosen -- by the option ("small" / "mid" / "dag" / "multisweep": 0 never, 2 wherever eligible) or, at 1, by
// the defaults measured on 20 networks (scripts/time_paths.py, profiles/r05_paths.json).  run(): BN_OK, BN_ERR_STATE (a bounded wait
// gave up: the launch's workgroups were not all on the chip), or an error.  gave_up(): the path's bookkeeping of such an abort.
struct PathDriver {
    int id;                                             // bn_bp_last_path
    bool (*wanted)(const bn_engine*);
    int (*run)(bn_engine*, double eps, int32_t max_sweeps, double* copy_to);
    int (*gave_up)(bn_engine*, const char* what);       // BN_OK: go on with the next path
    const char* what;                                   // ... the kernel's name in the one line on stderr
    void (*ran_ok)(bn_engine*);                         // may be null
    int32_t bn_engine::*cooldown;                       // runs left before the path is tried again
    bool reads_tile_evidence;                           // flush_evidence() first
};

namespace bn_eng __attribute__((visibility("hidden"))) {
extern RcclApi g_rccl;
int load_rccl();

// (both free what `dst` held first; a failed allocation leaves it empty)
template <class T, class A>
inline int upload(DeviceBuf<T>& dst, const std::vector<T, A>& src, hipStream_t s) {
    HIPCHK(dev_malloc(dst, std::max<size_t>(src.size(), 1) * sizeof(T)));
    if (!src.empty()) HIPCHK(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return BN_OK;
}

template <class T>
inline int dalloc(DeviceBuf<T>& dst, size_t count) {
    HIPCHK(dev_malloc(dst, std::max<size_t>(count, 1) * sizeof(T)));
    return BN_OK;
}


// the item tables of a one-workgroup plan / of a several-workgroup plan (g0: its first part, which carries the tables over all nodes)
inline int upload_items(ItemImage& img, const SmallPlan& sp, hipStream_t s) {
    int r;
    if ((r = upload(img.ent, sp.ent, s)) || (r = upload(img.ent_cpt, sp.ent_cpt, s)) || (r = upload(img.term, sp.term, s)) ||
        (r = upload(img.clist, sp.clist, s)) || (r = upload(img.bslot, sp.bslot, s)) || (r = upload(img.cslot, sp.cslot, s)) ||
        (r = upload(img.nv_idx, sp.nv_idx, s)) || (r = upload(img.nv_slot, sp.nv_slot, s)) || (r = upload(img.npi_init, sp.npi_init, s)) ||
        (r = upload(img.node_off, sp.node_off, s)))
        return r;
    return BN_OK;
}
inline int upload_items(ItemImage& img, const MidTables& t, const SmallPlan& g0, hipStream_t s) {
    int r;
    if ((r = upload(img.parts, t.parts, s)) || (r = upload(img.ent, t.ent, s)) || (r = upload(img.ent_cpt, t.ent_cpt, s)) ||
        (r = upload(img.term, t.term, s)) || (r = upload(img.clist, t.clist, s)) || (r = upload(img.bslot, t.bslot, s)) ||
        (r = upload(img.cslot, t.cslot, s)) || (r = upload(img.nv_idx, g0.nv_idx, s)) || (r = upload(img.nv_slot, g0.nv_slot, s)) ||
        (r = upload(img.npi_init, g0.npi_init, s)) || (r = upload(img.node_off, g0.node_off, s)) || (r = upload(img.msg_first, t.msg_first, s)))
        return r;
    return BN_OK;
}
// the pointers every item kernel's argument struct names alike (nv_idx, nv_slot, parts, msg_first: where the struct has them)
template <class Args>
inline void put_items(Args& a, const ItemImage& t) {
    a.ent = t.ent; a.ent_cpt = t.ent_cpt; a.term = t.term; a.clist = t.clist; a.bslot = t.bslot; a.cslot = t.cslot;
    a.npi_init = t.npi_init; a.node_off = t.node_off;
}

// What every compute entry point refuses: an engine without a device (host_only_code: the code that entry point returns for it,
// BN_ERR_STATE or BN_ERR_NO_DEVICE) and one a failed bn_reload_cpt left with device images of mixed age.  BN_OK: go on.
int refuse_unusable(const bn_engine* e, int host_only_code);
bn_policy::PathFacts path_facts_of(const Plan& p, const SmallPlan& small, const MidPlan& mid, const DagPlan& dag);
inline bn_policy::PathOks oks_of(const bn_engine* e) { return {e->small_ok, e->mid_ok, e->dag_ok, e->shard_flow_ok}; }
inline bn_policy::PathModes modes_of(const bn_engine* e) { return {e->multisweep, e->small_mode, e->mid_mode, e->dag_mode}; }
inline void next_run_id(bn_engine* e) {   // 0 is what a control block holds that no run has written
    ++e->run_id;
    if (e->run_id == 0) e->run_id = 1;
}
bool dag_applies(const bn_engine* e);
int ensure_dag(bn_engine* e);
SmallArgs small_args_of(bn_engine* e, const BpBuffers& b, double eps, int32_t max_sweeps, int32_t begin, Ctl* host_ctl);
int mid_launch(bn_engine* e, const MidArgs& a, int32_t n_sets, const double* copy_from, double* copy_to, bool wait = true);
MidArgs mid_args_of(bn_engine* e, const BpBuffers& b0, const SetStrides& st, Ctl* h_ctl_dev, double eps, int32_t max_sweeps,
                           int32_t begin, int32_t set_base, int32_t slot_base);
bool mid_applies(const bn_engine* e);
BpBuffers buffers_of(bn_engine* e);
// the evidence a run of the DAG path applies and where its marginals go: the engine's own (a single query), or one set of a batch
// (own = false: the engine's state arrays hold foreign evidence afterwards, so the evidence in force is applied again at its next run)
struct DagQuery {
    bn_stage::SetView ev;
    double* beliefs = nullptr;   // nullptr: where buffers_of(e) says
    bool own = true;
};
int run_dag(bn_engine* e, double eps, int32_t max_sweeps, double* copy_to);   // the evidence in force
int run_dag_query(bn_engine* e, double eps, int32_t max_sweeps, double* copy_to, const DagQuery& q);
int resident_service_blocks(int tile_blocks);
void report_abort_once(bn_engine* e, const char* what, int pause_runs);
int mid_reserve_slots(bn_engine* e, int32_t slots);
int ensure_events(bn_engine* e, size_t count);
int check_evidence(const Plan& p, int32_t ne, const int32_t* ev_node, const int32_t* ev_off,
                          std::vector<uint32_t>& seen, uint32_t& epoch);
// The evidence of a call that brings its sets with it (bn_mpe_*, bn_jt_*): every set validated like bn_bp_set_evidence does, at its
// slices of the concatenated arrays; `out`: where the sets start.  No findings at all: ev_off is not read and comes back null.
int check_evidence_sets(bn_engine* e, int32_t n_sets, const int32_t* ne, const int32_t* ev_node, const int32_t*& ev_off, const double* ev_val,
                        bn_stage::BatchLayout& out);
void free_engine(bn_engine* e);
int small_gave_up(bn_engine*, const char*);
int dag_gave_up(bn_engine* e, const char* what);
int mid_gave_up(bn_engine* e, const char* what);
int resident_gave_up(bn_engine* e, const char* what);
// several evidence sets per call: bn_engine_batch.cpp dispatches, bn_engine_batch_paths.cpp has the runs
BpBuffers batch_buffers_of(bn_engine* e, int32_t q);
inline SetStrides strides_of(const bn_engine* e) {
    const Plan& p = e->plan;
    return SetStrides{p.rec_total_doubles, p.node_doubles, int64_t(std::max(p.n_slots, 1)), p.node_off[p.n], e->res_cap};
}
int run_batch_launches(bn_engine* e, double eps, int32_t max_sweeps);
int run_batch_small(bn_engine* e, double eps, int32_t max_sweeps, double*);
int run_batch_dag(bn_engine* e, double eps, int32_t max_sweeps, double*);
int run_batch_mid(bn_engine* e, double eps, int32_t max_sweeps, double*);
int run_batch_resident(bn_engine* e, double eps, int32_t max_sweeps, double*);
// the run of a single query: bn_engine_paths.cpp dispatches, bn_engine.cpp has the evidence and the per-sweep launches
int flush_evidence(bn_engine* e);
// the first-sweep image (bn_engine_memo.cpp)
bool memo0_possible(const bn_engine* e);          // the option is on and the network runs the grid-barrier form of the resident kernel
int memo0_ensure(bn_engine* e);                   // builds the image if there is none: one launch over all nodes, then the set in force
int memo0_patch(bn_engine* e);                    // ONE launch: marks + vectors of the set in force, its slots of the image, the dropped nodes' slots
void memo0_invalidate(bn_engine* e);              // the CPTs changed, or a launch failed: rebuilt at the next run that can use it
void note_run_result(bn_engine* e);
int run_per_sweep(bn_engine* e, double eps, int32_t max_sweeps, double* copy_to);
int run_device_impl(bn_engine* e, double eps, int32_t max_sweeps, int32_t* sweeps_out, double* residual_out, double* copy_to);
void resident_ran_ok(bn_engine* e);
// the "mpe_*" names of bn_set_option / bn_get_info (bn_engine_mpe.cpp); *known = false: not one of them
int mpe_set_option(bn_engine* e, const char* name, int32_t value, bool* known);
int64_t mpe_get_info(bn_engine* e, const char* name, bool* known);
void mpe_cpt_reloaded(bn_engine* e);   // bn_reload_cpt: what max-product built from the old tables is dropped
// the "em_*" names (bn_engine_em.cpp)
int em_set_option(bn_engine* e, const char* name, int32_t value, bool* known);
int64_t em_get_info(bn_engine* e, const char* name, bool* known);
// ---- what bn_em_* and bn_jt_em_* share (bn_engine_em.cpp): one call, one E-step as the loop sees it, one loop
struct EmCall {
    int64_t n_patterns;
    const uint8_t* patterns;
    const uint64_t* counts;
    const double* theta0;     // flat, [entries]
    bool fit;                 // false: one E-step, no M-step
    int32_t max_iters;
    double tol, prior;
    double* E_out;            // the last E-step's sums (may be null)
    void* rows_out;           // ... and its per-row array, EmEstep::d_rows (may be null)
    double* cpt_out;          // (fit)
    int32_t* iters_out;
    double* delta_hist;
    double* loglik_hist;      // (the tree only)
    int32_t hist_cap;
};
// The launches return 0 or the hipError_t; `begin` and `end` may be empty.  They queue on the engine's stream and do not wait.
struct EmEstep {
    const char* what[3];                                   // begin, chunk, end: the kernel's name in "... launch failed"
    std::function<int()> begin;                            // once per iteration, before the chunks
    std::function<int(const bn_policy::EmChunk&)> chunk;   // one launch's rows: their family posteriors into EmCore::d_b
    std::function<int()> end;                              // once per iteration, behind the chunks
    const int32_t* slot_of;                                // the M-step's images (EmMstepArgs); all null: none
    const int32_t* init_of;
    double* ent_cpt;
    double* npi_init;
    const void* d_rows;                                    // [patterns] of row_bytes each: what the last E-step says of every row
    size_t row_bytes;
    bool has_L;                                            // `end` leaves L in word 3
    int64_t* capped;                                       // where word 0 of the call goes (null: nowhere)
};
int em_reserve(bn_engine* e, EmCore& m, int64_t n_patterns, const bn_policy::EmPlan& plan);
int em_drive(bn_engine* e, EmCore& m, const EmCall& c, const bn_policy::EmPlan& plan, const EmEstep& es);
int em_check_fit_args(const double* cpt_out, int32_t max_iters, double tol, double prior, bool any_hist, int32_t hist_cap);
// bn_set_option of either family: the option `own` ("em_scratch_cells" / "jt_em_scratch_cells"; 0: the default `dflt`)
int em_scratch_option(const char* own, int64_t dflt, EmCore& m, const char* name, int32_t value, bool* known);
// the "jt_*" names (bn_engine_jt.cpp)
int jt_set_option(bn_engine* e, const char* name, int32_t value, bool* known);
int64_t jt_get_info(bn_engine* e, const char* name, bool* known);
void jt_cpt_reloaded(bn_engine* e);    // bn_reload_cpt: the base potentials are computed again at the next run
// What every call that runs on the tree refuses, in the order it reports them: a sharded engine and a plan that is not eligible
// (jt_check_plan, which builds the plan, once, also on engines without a device), then a forced form 1 that does not fit and an
// engine without a device (jt_check_form; *form_out: 1 or 2).  Two steps: exact EM has a refusal of its own between them.
int jt_check_plan(bn_engine* e);
int jt_check_form(bn_engine* e, int* form_out);
int jt_ensure_tables(bn_engine* e);    // the plan's item tables on the device, once (not the base potentials)
JtTables jt_tables_of(const JtState& j, const double* psi0);   // ... as the kernels take them, with the base potentials to run on
// the "jt_em_*" names (bn_engine_jt_em.cpp)
int jt_em_set_option(bn_engine* e, const char* name, int32_t value, bool* known);
int64_t jt_em_get_info(bn_engine* e, const char* name, bool* known);
// the "gibbs_*" names (bn_engine_gibbs.cpp)
int gibbs_set_option(bn_engine* e, const char* name, int32_t value, bool* known);
int64_t gibbs_get_info(bn_engine* e, const char* name, bool* known);
void gibbs_cpt_reloaded(bn_engine* e);   // bn_reload_cpt: the tables are copied again at the next run
// The table of bn_em_* and bn_jt_em_*: its arguments, then (behind whatever else the entry point checks of its arguments) its cells
inline int em_check_table_args(const bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (n_patterns < 1) return fail(BN_ERR_ARG, "n_patterns must be at least 1");
    if (!patterns) return fail(BN_ERR_ARG, "null patterns");
    if (!counts) return fail(BN_ERR_ARG, "null counts");
    return BN_OK;
}
inline int em_check_table_cells(const bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts) {
    const Plan& p = e->plan;
    bool any = false;
    for (int64_t r = 0; r < n_patterns; ++r) {
        const uint8_t* row = patterns + r * p.n;
        for (int32_t v = 0; v < p.n; ++v)
            if (row[v] != kEmMissing && int32_t(row[v]) >= p.k[v])
                return fail(BN_ERR_ARG, "pattern " + std::to_string(r) + ": state " + std::to_string(int(row[v])) + " of node " + std::to_string(v) +
                                            " is not below its arity " + std::to_string(p.k[v]) + " (and not BN_EM_MISSING)");
        any = any || counts[r] != 0;
    }
    if (!any) return fail(BN_ERR_ARG, "the table's counts sum to zero");
    return BN_OK;
}
}  // namespace bn_eng

#endif  // BN_ENGINE_INTERNAL_HPP
