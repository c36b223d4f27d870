// bn_engine.cpp -- C ABI (include/bn_mi355x.h) over the HIP kernels: evidence, the steps of a run of belief propagation with one
// launch per sweep, options, info, read-out, messages.  Creation: bn_engine_create.cpp; the one-launch execution paths and their
// dispatch: bn_engine_paths.cpp; batches, sharding, introspection and the samplers' entry points: bn_engine_batch.cpp,
// bn_engine_shard.cpp, bn_engine_tools.cpp (bn_engine_internal.hpp has the map).
#include "bn_engine_internal.hpp"

thread_local std::string bn_eng::g_err;
RcclApi bn_eng::g_rccl;

int bn_eng::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int bn_eng::load_rccl() {
    if (g_rccl.handle) return BN_OK;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(BN_ERR_COMM, std::string("cannot load librccl: ") + dlerror());
    RcclApi a;
    a.handle = h;
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(h, "ncclAllGather"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(h, "ncclAllReduce"));
    a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(h, "ncclCommCount"));
    if (!a.AllReduce || !a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllGather || !a.GetErrorString)
        return fail(BN_ERR_COMM, "librccl lacks a required symbol");
    g_rccl = a;
    return BN_OK;
}

extern "C" const char* bn_last_error(void) { return g_err.c_str(); }
extern "C" const char* bn_version(void) { return "bn_mi355x 0.1 (gfx950)"; }

BpBuffers bn_eng::buffers_of(bn_engine* e) {
    BpBuffers b;
    b.tiles = e->d_tiles;
    b.classes = e->d_classes;
    b.flat_tab = e->d_flat_tab;
    b.n_tiles = int32_t(e->plan.tiles.size());
    b.cpt = e->d_cpt;
    b.rec0 = e->d_rec[0]; b.rec1 = e->d_rec[1];
    b.node0 = e->d_node[0]; b.node1 = e->d_node[1];
    b.out_refs = e->d_out;
    b.frozen = e->d_frozen;
    b.frozen_mark = e->frozen_mark;
    b.slot_node = e->d_slot_node;
    b.slot_boff = e->d_slot_boff;
    b.node_tile = e->d_node_tile;
    b.node_nl = e->d_node_nl;
    b.in_refs = e->d_inrefs;
    b.g_base = e->plan.g_base;
    b.seg_d2 = e->plan.seg_d2;
    b.seg_data_d2 = e->plan.seg_data_d2;
    b.rec_total_doubles = e->plan.rec_total_doubles;
    b.rank = e->plan.rank;
    b.nranks = e->plan.nranks;
    b.res_hist = e->d_res_hist;
    b.res_cap = e->res_cap;
    b.ctl = e->d_ctl;
    b.beliefs = e->beliefs_override ? e->beliefs_override : e->d_beliefs;
    return b;
}

int bn_eng::refuse_unusable(const bn_engine* e, int host_only_code) {
    if (e->host_only) return fail(host_only_code, "engine was created with BN_DEVICE_HOST_ONLY: no GPU, no compute");
    if (e->poisoned) return fail(BN_ERR_STATE, "engine unusable: bn_reload_cpt failed while uploading (destroy it and create a new one)");
    return BN_OK;
}

// `seen` / `epoch`: one stamp per node, kept by the engine so that a query costs O(ne), not O(n)
int bn_eng::check_evidence(const Plan& p, int32_t ne, const int32_t* ev_node, const int32_t* ev_off,
                          std::vector<uint32_t>& seen, uint32_t& epoch) {
    if (ne < 0) return fail(BN_ERR_ARG, "negative evidence count");
    if (ne == 0) return BN_OK;
    if (!ev_node || !ev_off) return fail(BN_ERR_ARG, "null evidence array");
    if (ev_off[0] != 0) return fail(BN_ERR_ARG, "ev_off[0] != 0");
    if (seen.size() != size_t(p.n) || epoch == 0xffffffffu) { seen.assign(size_t(p.n), 0u); epoch = 0; }
    ++epoch;
    for (int32_t j = 0; j < ne; ++j) {
        int32_t v = ev_node[j];
        if (v < 0 || v >= p.n) return fail(BN_ERR_ARG, "evidence node out of range");
        if (seen[v] == epoch) return fail(BN_ERR_ARG, "evidence node listed twice");
        seen[v] = epoch;
        if (ev_off[j + 1] - ev_off[j] != p.k[v])
            return fail(BN_ERR_ARG, "evidence vector of node " + std::to_string(v) + " must have selectable_num entries");
    }
    return BN_OK;
}

int bn_eng::check_evidence_sets(bn_engine* e, int32_t n_sets, const int32_t* ne, const int32_t* ev_node, const int32_t*& ev_off, const double* ev_val,
                                bn_stage::BatchLayout& out) {
    int64_t total = 0;
    for (int32_t q = 0; q < n_sets; ++q) {
        if (ne[q] < 0) return fail(BN_ERR_ARG, "negative evidence count");
        total += ne[q];
    }
    if (total == 0) ev_off = nullptr;   // (nothing of it is read)
    out = bn_stage::layout_of(n_sets, ne, ev_off);
    for (int32_t q = 0; q < n_sets; ++q) {
        if (ne[q] > 0 && (!ev_node || !ev_off)) return fail(BN_ERR_ARG, "null evidence array");
        if (int rc = check_evidence(e->plan, ne[q], ev_node ? ev_node + out.node_at[q] : nullptr, ev_off ? ev_off + out.off_at[q] : nullptr, e->ev_seen, e->ev_epoch))
            return rc;
        if (ne[q] > 0 && !ev_val) return fail(BN_ERR_ARG, "null ev_val");
    }
    return BN_OK;
}

int bn_eng::ensure_events(bn_engine* e, size_t count) {
    while (e->events.size() < count) {
        hipEvent_t ev;
        HIPCHK(hipEventCreate(&ev));
        e->events.push_back(ev);
    }
    return BN_OK;
}

// Evidence staging: one pinned host block [ev_node | ev_off | ev_val] -> one H2D copy, then the
// evidence is APPLIED (marks cleared, new marks and vectors written): it stays in force for every
// following run until the next call, so a run itself starts with its first sweep.
// wait: block until the upload has left the pinned staging block (bn_bp_set_evidence); bn_bp_run passes false --
// its own single synchronisation at the end of the call covers it
// The evidence in force (staging block) -> the tile buffers: ONE kernel marks the nodes with this set's mark value and writes
// their vectors (bp_evidence_kernel).  No-op when they hold it already.
int bn_eng::flush_evidence(bn_engine* e) {
    if (!e->ev_deferred) return BN_OK;
    const Plan& p = e->plan;
    if (e->ev_applied_dirty) memo0_invalidate(e);  // (what the failed launch left of the first-sweep image is unknown too)
    if (e->frozen_mark == 255 || e->ev_applied_dirty) {  // the mark values are used up (or a launch failed half-way): start over
        HIPCHK(hipMemsetAsync(e->d_frozen, 0, std::max<size_t>(p.n_slots, 1), e->stream));
        e->frozen_mark = 0;
    }
    ++e->frozen_mark;
    e->ev_applied_dirty = false;
    e->ev_deferred = false;
    if (e->memo.valid) {  // the same ONE launch also keeps the first-sweep image right for this set (bn_engine_memo.cpp)
        if (int rc = memo0_patch(e)) {
            e->ev_applied_dirty = true;
            return rc;
        }
        return BN_OK;
    }
    EvidenceArgs ea{buffers_of(e), e->ev_ne, e->d_ev_node, e->d_ev_off, e->d_ev_val};
    if (int code = launch_bp_evidence(ea, e->stream)) {
        e->ev_applied_dirty = true;
        return fail(BN_ERR_HIP, std::string("bp_evidence launch failed: ") + hipGetErrorString(hipError_t(code)));
    }
    e->ev_upload_pending = e->ev_ne > 0;
    return BN_OK;
}

static int set_evidence_impl(bn_engine* e, int32_t ne, const int32_t* ev_node, const int32_t* ev_off,
                             const double* ev_val, bool wait) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (int rc = refuse_unusable(e, BN_ERR_STATE)) return rc;
    const Plan& p = e->plan;
    int rc = check_evidence(p, ne, ev_node, ev_off, e->ev_seen, e->ev_epoch);
    if (rc) return rc;
    if (ne > 0 && !ev_val) return fail(BN_ERR_ARG, "null ev_val");
    ON_DEVICE(e);
    const int64_t nval = ne > 0 ? ev_off[ne] : 0;
    const size_t off_node = 0, off_off = size_t(ne) * 4, off_val = (off_off + size_t(ne + 1) * 4 + 7) & ~size_t(7);
    const size_t bytes = off_val + size_t(nval) * 8;
    if (e->ev_upload_pending) {  // the staging block is about to be rewritten
        HIPCHK(hipStreamSynchronize(e->stream));
        e->ev_upload_pending = false;
    }
    if (!e->h_ev) {
        // the staging block is sized ONCE, for the largest evidence set the model admits (every node observed): growing it
        // later would mean freeing page-locked memory, which waits for the whole device -- and where several shard engines share a process,
        // a rank whose kernel is already waiting for this rank's would never let that return
        HIPCHK(e->h_ev.alloc(((size_t(p.n) * 4 + size_t(p.n + 1) * 4 + 7) & ~size_t(7)) + size_t(p.node_off[p.n]) * 8 + 64));
    }
    if (bytes > e->h_ev.capacity()) return fail(BN_ERR_ARG, "evidence larger than the model");
    // ONE kernel applies a set: it reads the arrays in place from the page-locked staging block (no copy command in the
    // queue in front of the run) and marks the nodes with this set's mark value (no memset of the previous set's marks)
    if (ne > 0) {
        std::memcpy(e->h_ev + off_node, ev_node, size_t(ne) * 4);
        std::memcpy(e->h_ev + off_off, ev_off, size_t(ne + 1) * 4);
        std::memcpy(e->h_ev + off_val, ev_val, size_t(nval) * 8);
    }
    e->d_ev_node = reinterpret_cast<int32_t*>(e->h_ev.dev() + off_node);
    e->d_ev_off = reinterpret_cast<int32_t*>(e->h_ev.dev() + off_off);
    e->d_ev_val = reinterpret_cast<double*>(e->h_ev.dev() + off_val);
    e->ev_ne = ne;
    e->ev_nval = int32_t(nval);
    e->dag_ev_applied = false;
    if (e->small_ok || e->mid_ok || dag_applies(e)) {  // the item kernels read the arrays where they are; flush_evidence() serves every other path
        e->ev_deferred = true;
        e->ev_upload_pending = ne > 0;
        return BN_OK;
    }
    e->ev_deferred = true;
    e->ev_one_shot = !wait;   // (bn_bp_run / bn_bp_run_view pass wait == false: the set is run once, in this call)
    if ((rc = flush_evidence(e))) return rc;
    if (wait) {
        HIPCHK(hipStreamSynchronize(e->stream));
        e->ev_upload_pending = false;
    }
    return BN_OK;
}

extern "C" int bn_bp_set_evidence(bn_engine* e, int32_t ne, const int32_t* ev_node, const int32_t* ev_off,
                                  const double* ev_val) {
    return set_evidence_impl(e, ne, ev_node, ev_off, ev_val, true);
}

// ---- the steps of a run; bn_bp_run_device chains them, the bn_bp_step_* entry points expose
// them one by one (tests drive several shards on one GPU with an emulated all-gather).
static int step_begin(bn_engine* e) {
    // a run on the tile kernels starts here (also the single-step API): what it leaves behind -- beliefs in d_beliefs, messages
    // in the record buffers -- is what the diagnostics must read, whatever path and output buffer the previous run used
    e->beliefs_on_host_only = false;
    e->last_path = 0;
    if (int rc = flush_evidence(e)) return rc;
    next_run_id(e);
    if (!e->rows_clean) {  // the previous run did not end through a finish kernel that saw it over
        if (int code = launch_bp_reset(buffers_of(e), e->stream))
            return fail(BN_ERR_HIP, std::string("bp_reset launch failed: ") + hipGetErrorString(hipError_t(code)));
    }
    e->rows_clean = false;
    return BN_OK;
}

// part: 0 = every tile + bookkeeping (one launch); 1 = interior tiles only, no bookkeeping;
// 2 = the tiles that touch a cut edge + bookkeeping (sharded runs, see bn_plan.cpp / run loop)
static int step_sweep(bn_engine* e, int32_t sweep, double eps, int part = 0) {
    const int cur = sweep & 1;
    const int32_t nt = int32_t(e->plan.tiles.size()), ni = e->plan.n_interior_tiles;
    const int32_t t0 = part == 2 ? ni : 0, t1 = part == 1 ? ni : nt;
    const int32_t book = part == 1 ? 0 : 1;
    if (t1 - t0 + book <= 0) return BN_OK;
    SweepArgs sa{buffers_of(e), e->d_rec[cur], e->d_rec[cur ^ 1], e->d_node[cur], e->d_node[cur ^ 1], eps, sweep,
                 t0, t1, book, e->run_id, SetStrides{}};
    // one wave per tile (+ one for the bookkeeping), blocks padded to a multiple of 8 for the XCD mapping
    const int grid = ((t1 - t0 + book + kWavesPerBlock - 1) / kWavesPerBlock + 7) & ~7;
    static const bool no_light = std::getenv("BN_NO_LIGHT") != nullptr;  // A/B switch
    if (launch_bp_sweep(sa, grid, 1, e->nontemporal, e->plan.light && !no_light, e->plan.variants, e->stream))
        return fail(BN_ERR_HIP, "bp_sweep launch failed");
    return BN_OK;
}

// Halo exchange after sweep `sweep`: in-place all-gather of every rank's segment of the buffer
// that sweep wrote.  One collective per sweep; it also carries the residual slots.
static int step_exchange(bn_engine* e, int32_t sweep, hipStream_t on) {
    const Plan& p = e->plan;
    // BN_EXCHANGE_ALWAYS: issue the (then trivial) collective on a 1-rank communicator too, so the
    // RCCL call can be exercised on a single-GPU box
    if (p.nranks == 1 && !(e->comm && std::getenv("BN_EXCHANGE_ALWAYS"))) return BN_OK;
    if (!e->comm) return fail(BN_ERR_COMM, "sharded engine: call bn_comm_init before running");
    double* g = e->d_rec[(sweep + 1) & 1] + 2 * p.g_base;
    const size_t count = size_t(2 * p.seg_d2);
    ncclResult_t rc = g_rccl.AllGather(g + size_t(p.rank) * count, g, count, ncclDouble, e->comm, on);
    if (rc != ncclSuccess) return fail(BN_ERR_COMM, std::string("ncclAllGather: ") + g_rccl.GetErrorString(rc));
    return BN_OK;
}

// One iteration of a sharded run with the exchange overlapped: the interior tiles of
// iteration s read nothing the all-gather of iteration s-1 delivers, so their launch goes out first and
// runs while that collective is still in flight on the comm stream; only the launch over the tiles that
// touch a cut edge (and the residual bookkeeping, which reads every rank's slots) waits for it.
// Critical path per iteration: max(interior kernel, all-gather) + boundary kernel, instead of their sum.
static int step_sweep_overlapped(bn_engine* e, int32_t sweep, double eps, bool gather_pending) {
    int rc;
    if ((rc = step_sweep(e, sweep, eps, 1))) return rc;
    if (gather_pending) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_gathered, 0));
    if ((rc = step_sweep(e, sweep, eps, 2))) return rc;
    HIPCHK(hipEventRecord(e->ev_swept, e->stream));
    HIPCHK(hipStreamWaitEvent(e->comm_stream, e->ev_swept, 0));
    if ((rc = step_exchange(e, sweep, e->comm_stream))) return rc;
    HIPCHK(hipEventRecord(e->ev_gathered, e->comm_stream));
    return BN_OK;
}

static int step_finish(bn_engine* e, int32_t launched, bool final_batch, double eps) {
    // wave 0 writes the outcome straight into the pinned host Ctl: visible after the stream
    // synchronises, no copy command in between
    FinishArgs fa{buffers_of(e), eps, launched, final_batch ? 1 : 0, e->run_id, e->h_ctl.dev(), SetStrides{}};
    if (launch_bp_finish(fa, e->grid_tiles, 1, e->stream)) return fail(BN_ERR_HIP, "bp_finish launch failed");
    return BN_OK;
}

void bn_eng::note_run_result(bn_engine* e) {
    e->rows_clean = true;  // the finish kernel that saw the run over left the residual slots zero
    e->last_ctl = *e->h_ctl;
    e->have_run = true;
    e->predicted_sweeps = e->last_ctl.n_sweeps;
    e->stats.sweeps = e->last_ctl.n_sweeps;
    e->stats.memo_sweeps = 0;   // (run_resident says otherwise behind this)
    e->stats.memo_depth = 0;
    // device clock (100 MHz): start of sweep 0 -> start of the launch after the last executed sweep
    const unsigned long long t0 = e->last_ctl.t_first, t1 = e->last_ctl.t_last;
    e->stats.sweep_devclock_ms = t1 > t0 ? float(double(t1 - t0) * 1e-5) : 0.f;
}

// One launch per sweep (every network; what the one-launch paths of bn_engine_paths.cpp do not take, or hand back): sweeps in batches
// of the predicted count, a finish kernel behind each batch, one synchronisation per batch.
int bn_eng::run_per_sweep(bn_engine* e, double eps, int32_t max_sweeps, double* copy_to) {
    hipStream_t s = e->stream;
    int rc;
    if ((rc = step_begin(e))) return rc;
    int32_t launched = 0, batches = 0;
    // every rank takes the same decisions: they all see the same sweep counts
    int32_t batch = e->predicted_sweeps > 0 ? e->predicted_sweeps : 8;
    for (;;) {
        if (max_sweeps > 0) batch = std::min(batch, max_sweeps - launched);
        if (e->timing) {
            if ((rc = ensure_events(e, 2 * size_t(batches + 1)))) return rc;
            HIPCHK(hipEventRecord(e->events[2 * batches], s));
        }
        const bool overlapped = e->plan.nranks > 1 && e->overlap && e->comm_stream;
        for (int32_t i = 0; i < batch; ++i) {
            if (overlapped) {
                if ((rc = step_sweep_overlapped(e, launched + i, eps, launched + i > 0))) return rc;
            } else {
                if ((rc = step_sweep(e, launched + i, eps))) return rc;
                if ((rc = step_exchange(e, launched + i, s))) return rc;
            }
        }
        if (overlapped && batch > 0) HIPCHK(hipStreamWaitEvent(s, e->ev_gathered, 0));  // the finish kernel reads every rank's slots
        launched += batch;
        if (e->timing) HIPCHK(hipEventRecord(e->events[2 * batches + 1], s));
        ++batches;
        if ((rc = step_finish(e, launched, max_sweeps > 0 && launched >= max_sweeps, eps))) return rc;
        if (copy_to)  // behind the finish kernel; repeated if the predicted sweep count turns out too low
            HIPCHK(hipMemcpyAsync(copy_to, e->d_beliefs, sizeof(double) * e->plan.node_off[e->plan.n], hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        e->ev_upload_pending = false;
        if (e->h_ctl->run_id != e->run_id) return fail(BN_ERR_STATE, "finish kernel did not report (stale control block)");
        if (e->h_ctl->done != 0) break;
        batch = 8;
    }
    note_run_result(e);
    float ms = 0.f;
    for (int32_t i = 0; e->timing && i < batches; ++i) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, e->events[2 * i], e->events[2 * i + 1]));
        ms += t;
    }
    e->stats.sweep_launches = launched;
    e->stats.sweep_kernel_ms = ms;
    return BN_OK;
}

extern "C" int bn_bp_run_device(bn_engine* e, double eps, int32_t max_sweeps, int32_t* sweeps_out,
                                double* residual_out) {
    return run_device_impl(e, eps, max_sweeps, sweeps_out, residual_out, nullptr);
}

// Engine options: "timing" = 1/0 (HIP events around the sweep launches; off: sweep_kernel_ms reads 0);
// "multisweep" = 1/0 (networks small enough run all their sweeps in ONE launch; 0 forces one launch per sweep).
extern "C" int bn_set_option(bn_engine* e, const char* name, int32_t value) {
    if (!e || !name) return fail(BN_ERR_ARG, "null argument");
    if (std::strcmp(name, "timing") == 0) { e->timing = value != 0; return BN_OK; }
    if (std::strcmp(name, "overlap") == 0) { e->overlap = value != 0; return BN_OK; }
    if (std::strcmp(name, "beliefs_direct") == 0) { e->beliefs_direct = value != 0; return BN_OK; }
    if (std::strcmp(name, "flow") == 0) { e->flow = value != 0; return BN_OK; }
    if (std::strcmp(name, "direct") == 0) { e->resident_direct = value != 0; return BN_OK; }
    if (std::strcmp(name, "memo0") == 0) { e->memo.enabled = value != 0; return BN_OK; }   // (the image, once built, is kept right either way)
    if (std::strcmp(name, "memo1") == 0) {
        // (built together with the first-sweep image: where that one exists without it, both are built again by the next run)
        if (value != 0 && e->memo.valid && !e->memo1.built) memo0_invalidate(e);
        e->memo1.enabled = value != 0;
        return BN_OK;
    }
    if (std::strcmp(name, "mid") == 0) { e->mid_mode = value < 0 ? 0 : (value > 2 ? 2 : value); return BN_OK; }
    if (std::strcmp(name, "dagflow") == 0) { e->dag_flow = value != 0; return BN_OK; }
    if (std::strcmp(name, "dag") == 0) { e->dag_mode = value < 0 ? 0 : (value > 2 ? 2 : value); return BN_OK; }
    if (std::strcmp(name, "autotune") == 0) { e->autotune_pending = value != 0; if (value == 0) e->autotuned_path = -1; return BN_OK; }
    if (std::strcmp(name, "small") == 0) { e->small_mode = value < 0 ? 0 : (value > 2 ? 2 : value); return BN_OK; }
    if (std::strcmp(name, "poll_sleep") == 0) { e->poll_sleep = std::max(0, std::min(value, 64)); return BN_OK; }
    if (std::strcmp(name, "multisweep") == 0) { e->multisweep = value < 0 ? 0 : (value > 2 ? 2 : value); return BN_OK; }
    if (std::strcmp(name, "score_splits") == 0) { e->score.splits = std::max(0, std::min(value, 65535)); return BN_OK; }
    if (std::strncmp(name, "mpe_", 4) == 0) {   // max-product: "mpe_form", "mpe_group" (bn_engine_mpe.cpp)
        bool known = false;
        const int rc = mpe_set_option(e, name, value, &known);
        if (known) return rc;
    }
    if (std::strncmp(name, "em_", 3) == 0) {   // expectation-maximisation: "em_scratch_cells" (bn_engine_em.cpp)
        bool known = false;
        const int rc = em_set_option(e, name, value, &known);
        if (known) return rc;
    }
    if (std::strncmp(name, "jt_em_", 6) == 0) {   // exact expectation-maximisation: "jt_em_scratch_cells" (bn_engine_jt_em.cpp)
        bool known = false;
        const int rc = jt_em_set_option(e, name, value, &known);
        if (known) return rc;
    }
    if (std::strncmp(name, "jt_", 3) == 0) {   // junction tree: "jt_form", "jt_scratch_cells" (bn_engine_jt.cpp)
        bool known = false;
        const int rc = jt_set_option(e, name, value, &known);
        if (known) return rc;
    }
    if (std::strncmp(name, "gibbs_", 6) == 0) {   // Gibbs sampling: "gibbs_sweeps_per_launch" (bn_engine_gibbs.cpp)
        bool known = false;
        const int rc = gibbs_set_option(e, name, value, &known);
        if (known) return rc;
    }
    return fail(BN_ERR_ARG, std::string("unknown option ") + name);
}
// Introspection for tests and tools: a named integer property of the engine / its last run.
extern "C" int64_t bn_get_info(bn_engine* e, const char* name) {
    if (!e || !name) return fail(BN_ERR_ARG, "null argument");
    if (std::strcmp(name, "resident_eligible") == 0) return e->shape.resident_ok ? 1 : 0;
    if (std::strcmp(name, "flow_eligible") == 0) return e->shape.flow_ok ? 1 : 0;
    if (std::strcmp(name, "last_flow") == 0) return e->last_path == 2 ? e->last_flow : 0;
    if (std::strcmp(name, "nbr_max") == 0) return e->plan.nbr_max;
    if (std::strcmp(name, "nbr_chunks") == 0) return e->plan.nbr.empty() ? 0 : e->plan.nbr_chunks;
    if (std::strcmp(name, "shard_flow") == 0) return e->shard_flow_ok ? 1 : 0;
    if (std::strncmp(name, "create_us_", 10) == 0) {   // construction split: host plans (tile / one-workgroup / several-workgroup / DAG), device side
        static const char* const kPhase[] = {"plan", "small", "mid", "dag", "device"};
        for (int i = 0; i < 5; ++i)
            if (std::strcmp(name + 10, kPhase[i]) == 0) return e->create_us[i];
        return fail(BN_ERR_ARG, std::string("unknown info ") + name);
    }
    if (std::strcmp(name, "rccl_ranks") == 0) {   // what the communicator itself reports (0: none initialised)
        int n = 0;
        if (e->comm && g_rccl.CommCount && g_rccl.CommCount(e->comm, &n) != ncclSuccess) n = -1;
        return n;
    }
    if (std::strcmp(name, "n_boundary_nodes") == 0) return int64_t(e->plan.boundary_node.size());
    if (std::strcmp(name, "parameters") == 0) {   // basic_info_criteria::calc_parameters (basic_info_criteria.hpp:100-117): sum (k - 1) x prod k[parent]
        int64_t total = 0;
        for (int32_t v = 0; v < e->plan.n; ++v) {
            int64_t rows = e->plan.k[v] - 1;
            for (int32_t j = e->plan.in_ptr[v]; j < e->plan.in_ptr[v + 1]; ++j) rows *= e->plan.k[e->plan.in_idx[j]];
            total += rows;
        }
        return total;
    }
    if (std::strcmp(name, "score_rows_ns") == 0) return int64_t(double(e->score.last_rows_ms) * 1e6);     // device-event times of the last
    if (std::strcmp(name, "score_count_ns") == 0) return int64_t(double(e->score.last_count_ms) * 1e6);   // bn_score_rows / bn_score_nodes
    if (std::strcmp(name, "score_nodes_ns") == 0) return int64_t(double(e->score.last_nodes_ms) * 1e6);   // kernels (counting, node sums)
    if (std::strcmp(name, "resident_blocks") == 0) return e->shape.blocks;
    if (std::strcmp(name, "resident_waves") == 0) return e->shape.waves;
    if (std::strcmp(name, "resident_aborts") == 0) return e->resident_aborts;
    if (std::strcmp(name, "memo0_active") == 0) return e->memo.enabled != 0 && e->memo.valid ? 1 : 0;   // the first-sweep image exists and runs may start from it
    if (std::strcmp(name, "memo0_bytes") == 0)   // device memory the image takes (0: not built)
        return (e->memo.d_rec ? int64_t(8) * (e->plan.rec_total_doubles + e->plan.node_doubles + e->plan.n + 4) : 0) +
               (e->memo1.d_rec ? int64_t(8) * (e->plan.rec_total_doubles + e->plan.node_doubles + e->plan.n + 4) +
                                     int64_t(4) * int64_t(e->memo1.adj_off.size() + e->memo1.adj.size()) : 0);
    if (std::strcmp(name, "memo1_active") == 0)   // the second-sweep image exists, holds the evidence in force, and runs may start from it
        return e->memo.enabled != 0 && e->memo.valid && e->memo1.enabled != 0 && e->memo1.built && e->memo1.holds ? 1 : 0;
    if (std::strcmp(name, "mid_eligible") == 0) return e->mid.ok ? 1 : 0;
    if (std::strcmp(name, "mid_parts") == 0) return e->mid.ok ? int64_t(e->mid.parts.size()) : 0;
    if (std::strcmp(name, "mid_aborts") == 0) return e->mid_aborts;
    if (std::strcmp(name, "autotuned") == 0) return e->autotuned_path >= 0 ? 1 : 0;
    if (std::strcmp(name, "autotuned_path") == 0) return e->autotuned_path >= 0 ? e->autotuned_path : 0;   // (valid when "autotuned" is 1)
    if (std::strcmp(name, "dag_eligible") == 0) return e->dag.ok ? 1 : 0;
    if (std::strcmp(name, "dag_blocks") == 0) return e->dag.ok ? e->dag.blocks : 0;
    if (std::strcmp(name, "dag_tiles") == 0) return e->dag.ok ? int64_t(e->dag.tiles.size()) : 0;
    if (std::strcmp(name, "dag_stream") == 0) return e->dag.ok && e->dag.stream ? 1 : 0;
    if (std::strcmp(name, "lw_small") == 0) return e->lw.ready && e->lw.small ? 1 : 0;   // (known after the first sampler call)
    if (std::strcmp(name, "lw_last_sample_kernel") == 0) return e->lw.last_sample_kernel;   // (bn_lw.hpp launch_lw_sample: which instantiation)
    if (std::strcmp(name, "lw_last_hist_kernel") == 0) return e->lw.last_hist_kernel;
    if (std::strcmp(name, "dag_aborts") == 0) return e->dag_aborts;
    if (std::strcmp(name, "batch_dense_refused") == 0) return e->dense_refused ? 1 : 0;   // (known after the first batch of >= 2 sets)
    if (std::strcmp(name, "batch_on_dense") == 0) return e->batch_on_dense ? 1 : 0;
    if (std::strcmp(name, "dag_flow_eligible") == 0) return e->dag_flow_ok ? 1 : 0;     // (known once the path has been set up: ensure_dag)
    if (std::strcmp(name, "dag_flow_max_nbr") == 0) return e->dag_flow_max_nbr;
    if (std::strcmp(name, "last_dag_flow") == 0) return e->last_path == 5 ? e->last_dag_flow : 0;
    if (std::strcmp(name, "small_eligible") == 0) return e->small.ok ? 1 : 0;
    if (std::strcmp(name, "small_waves") == 0) return e->small.ok ? e->small.waves : 0;
    if (std::strcmp(name, "small_lds_bytes") == 0) return e->small.ok ? int64_t(e->small.lds_bytes) : 0;
    if (std::strncmp(name, "mpe_", 4) == 0) {   // max-product: "mpe_form", "mpe_last_form", ... (bn_engine_mpe.cpp)
        bool known = false;
        const int64_t v = mpe_get_info(e, name, &known);
        if (known) return v;
    }
    if (std::strncmp(name, "em_", 3) == 0) {   // expectation-maximisation: "em_eligible", "em_last_iters", ... (bn_engine_em.cpp)
        bool known = false;
        const int64_t v = em_get_info(e, name, &known);
        if (known) return v;
    }
    if (std::strncmp(name, "jt_em_", 6) == 0) {   // exact expectation-maximisation: "jt_em_last_iters", ... (bn_engine_jt_em.cpp)
        bool known = false;
        const int64_t v = jt_em_get_info(e, name, &known);
        if (known) return v;
    }
    if (std::strncmp(name, "jt_", 3) == 0) {   // junction tree: "jt_eligible", "jt_form", "jt_cliques", ... (bn_engine_jt.cpp)
        bool known = false;
        const int64_t v = jt_get_info(e, name, &known);
        if (known) return v;
    }
    if (std::strncmp(name, "gibbs_", 6) == 0) {   // Gibbs sampling: "gibbs_eligible", "gibbs_colours", ... (bn_engine_gibbs.cpp)
        bool known = false;
        const int64_t v = gibbs_get_info(e, name, &known);
        if (known) return v;
    }
    return fail(BN_ERR_ARG, std::string("unknown info ") + name);
}
// 0 per-sweep launches, 2 resident tiles (bn_resident.hip), 3 one workgroup with the state in LDS (bn_small.hip), 4 the same items over several workgroups (bn_mid.hip)
extern "C" int bn_bp_last_path(bn_engine* e) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    return e->last_path;
}

// ---- single steps (diagnostics / tests) -------------------------------------------------------
extern "C" int bn_bp_step_begin(bn_engine* e) {
    if (!e || e->host_only) return fail(BN_ERR_STATE, "no device engine");
    ON_DEVICE(e);
    return step_begin(e);
}
extern "C" int bn_bp_step_sweep(bn_engine* e, int32_t sweep, double eps) {
    if (!e || e->host_only) return fail(BN_ERR_STATE, "no device engine");
    ON_DEVICE(e);
    return step_sweep(e, sweep, eps);
}
// part 1: the interior tiles only; part 2: the tiles that touch a cut edge + the residual bookkeeping
// (together one sweep; the overlapped run launches part 1 before the previous sweep's exchange has landed)
extern "C" int bn_bp_step_sweep_part(bn_engine* e, int32_t sweep, double eps, int32_t part) {
    if (!e || e->host_only) return fail(BN_ERR_STATE, "no device engine");
    if (part < 0 || part > 2) return fail(BN_ERR_ARG, "part must be 0, 1 or 2");
    ON_DEVICE(e);
    return step_sweep(e, sweep, eps, part);
}
extern "C" int bn_bp_step_finish(bn_engine* e, int32_t launched, int32_t final_batch, double eps, int32_t* done_out,
                                 int32_t* sweeps_out, double* residual_out) {
    if (!e || e->host_only) return fail(BN_ERR_STATE, "no device engine");
    ON_DEVICE(e);
    int rc = step_finish(e, launched, final_batch != 0, eps);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->h_ctl->run_id != e->run_id) return fail(BN_ERR_STATE, "finish kernel did not report (stale control block)");
    if (done_out) *done_out = e->h_ctl->done;
    if (sweeps_out) *sweeps_out = e->h_ctl->n_sweeps;
    if (residual_out) *residual_out = e->h_ctl->last_res;
    if (e->h_ctl->done != 0) note_run_result(e);
    return BN_OK;
}
// the marginals of the last run in device memory (a bn_bp_run_view that wrote them straight to the host buffer: uploaded first)
static int beliefs_to_device(bn_engine* e) {
    if (!e->beliefs_on_host_only) return BN_OK;
    ON_DEVICE(e);
    HIPCHK(hipMemcpyAsync(e->d_beliefs, e->h_beliefs, sizeof(double) * e->plan.node_off[e->plan.n], hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->beliefs_on_host_only = false;
    return BN_OK;
}
extern "C" const double* bn_bp_beliefs_device(bn_engine* e) {
    if (!e || e->host_only) return nullptr;
    if (beliefs_to_device(e) != BN_OK) return nullptr;
    return e->d_beliefs;
}

extern "C" int bn_bp_copy_beliefs(bn_engine* e, double* beliefs_out) {
    if (!e || !beliefs_out) return fail(BN_ERR_ARG, "null argument");
    if (e->host_only || !e->have_run) return fail(BN_ERR_STATE, "no belief propagation run to copy from");
    if (e->beliefs_on_host_only) {  // the last run's marginals are in the engine's page-locked buffer
        if (beliefs_out != e->h_beliefs) std::memcpy(beliefs_out, e->h_beliefs, sizeof(double) * e->plan.node_off[e->plan.n]);
        return BN_OK;
    }
    ON_DEVICE(e);
    HIPCHK(hipMemcpyAsync(beliefs_out, e->d_beliefs, sizeof(double) * e->plan.node_off[e->plan.n],
                          hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return BN_OK;
}

// Evidence in, beliefs out, ONE stream synchronisation: the evidence upload, the evidence kernel, the run and
// the copy of the beliefs are queued back to back on the engine's stream and waited for once.
extern "C" int bn_bp_run(bn_engine* e, int32_t ne, const int32_t* ev_node, const int32_t* ev_off,
                         const double* ev_val, double eps, int32_t max_sweeps, double* beliefs_out,
                         int32_t* sweeps_out, double* residual_out) {
    if (!beliefs_out) return fail(BN_ERR_ARG, "null beliefs_out");
    int rc = set_evidence_impl(e, ne, ev_node, ev_off, ev_val, false);
    if (rc) return rc;
    return run_device_impl(e, eps, max_sweeps, sweeps_out, residual_out, beliefs_out);
}

// The same with the beliefs left in a pinned host buffer the engine owns (valid until the next run on this
// engine): the copy behind the run is one DMA into page-locked memory, and a caller that unpacks the flat
// array anyway (the C++ functor builds its map of 1 x k matrices from it) never needs a second copy.
extern "C" int bn_bp_run_view(bn_engine* e, int32_t ne, const int32_t* ev_node, const int32_t* ev_off,
                              const double* ev_val, double eps, int32_t max_sweeps, const double** beliefs_view,
                              int32_t* sweeps_out, double* residual_out) {
    if (!beliefs_view) return fail(BN_ERR_ARG, "null beliefs_view");
    *beliefs_view = nullptr;
    int rc = set_evidence_impl(e, ne, ev_node, ev_off, ev_val, false);
    if (rc) return rc;
    if (!e->h_beliefs) {
        ON_DEVICE(e);
        HIPCHK(e->h_beliefs.alloc(size_t(e->plan.node_off[e->plan.n])));
    }
    if (e->beliefs_direct && e->plan.nranks == 1 && e->plan.node_off[e->plan.n] * 8 <= (int64_t(16) << 20)) {
        e->beliefs_override = e->h_beliefs.dev();
        rc = run_device_impl(e, eps, max_sweeps, sweeps_out, residual_out, nullptr);
        e->beliefs_override = nullptr;
        e->beliefs_on_host_only = rc == BN_OK;
    } else {
        rc = run_device_impl(e, eps, max_sweeps, sweeps_out, residual_out, e->h_beliefs);
    }
    if (rc) return rc;
    *beliefs_view = e->h_beliefs;
    return BN_OK;
}

extern "C" int bn_bp_residual_history(bn_engine* e, double* out, int32_t cap) {
    if (!e || !out || cap < 0) return fail(BN_ERR_ARG, "bad argument");
    if (e->host_only || !e->have_run) return fail(BN_ERR_STATE, "no belief propagation run yet");
    int32_t cnt = std::min({cap, e->last_ctl.n_sweeps, e->res_cap});
    ON_DEVICE(e);
    if (cnt > 0) HIPCHK(hipMemcpy(out, e->d_res_hist, sizeof(double) * cnt, hipMemcpyDeviceToHost));
    return cnt;
}

extern "C" int bn_bp_messages(bn_engine* e, double* pi_msg_out, double* lambda_msg_out) {
    if (!e || !pi_msg_out || !lambda_msg_out) return fail(BN_ERR_ARG, "null argument");
    if (e->host_only || !e->have_run) return fail(BN_ERR_STATE, "no belief propagation run yet");
    ON_DEVICE(e);
    if (e->last_path == 5) {  // bn_dag.hip: CSR edge order, four doubles per edge, two buffers: the run stopped in buffer n_sweeps & 1
        const int64_t E = e->dag.E, n = e->dag.n;
        const int par = e->last_ctl.n_sweeps & 1;
        // the records (tile-major in the state, bn_dag.hpp) back in CSR edge order; arities below 4: of a padded record edge e's first
        // k(parent of e) entries exist
        std::vector<double> pm(size_t(E) * 4), lm(size_t(E) * 4);
        HIPCHK(hipMemcpy(pm.data(), e->dag_img.state + 2 * dag_off_pim(E, n, par, 0), sizeof(double) * 4 * size_t(E), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(lm.data(), e->dag_img.state + 2 * dag_off_lam(E, n, par, 0), sizeof(double) * 4 * size_t(E), hipMemcpyDeviceToHost));
        size_t at = 0;
        for (int64_t ed = 0; ed < E; ++ed) {
            const int kp = e->dag.uniform4 ? 4 : e->plan.k[e->plan.in_idx[ed]];
            const size_t rec = size_t(e->dag_tables.eperm[size_t(ed)]);
            for (int i = 0; i < kp; ++i, ++at) { pi_msg_out[at] = pm[rec * 4 + i]; lambda_msg_out[at] = lm[rec * 4 + i]; }
        }
        return BN_OK;
    }
    if (e->last_path == 4) {  // bn_mid.hip keeps them in CSR edge order, two buffers: the run stopped in buffer n_sweeps & 1
        const size_t M = size_t(e->mid.parts[0].M), par = size_t(e->last_ctl.n_sweeps & 1);
        HIPCHK(hipMemcpy(pi_msg_out, e->d_m_state + par * M, sizeof(double) * M, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(lambda_msg_out, e->d_m_state + 2 * M + par * M, sizeof(double) * M, hipMemcpyDeviceToHost));
        return BN_OK;
    }
    if (e->last_path == 3) {  // bn_small.hip leaves the messages in CSR edge order
        const size_t bytes = sizeof(double) * size_t(e->small.M);
        HIPCHK(hipMemcpy(pi_msg_out, e->d_s_state, bytes, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(lambda_msg_out, e->d_s_state + e->small.M, bytes, hipMemcpyDeviceToHost));
        return BN_OK;
    }
    std::vector<double> rec(std::max<int64_t>(e->plan.rec_total_doubles, 1));
    HIPCHK(hipMemcpy(rec.data(), e->d_rec[e->last_ctl.n_sweeps & 1], sizeof(double) * e->plan.rec_total_doubles,
                     hipMemcpyDeviceToHost));
    unstripe_messages(e->plan, rec, pi_msg_out, lambda_msg_out);
    return BN_OK;
}

extern "C" int bn_bp_last_stats(bn_engine* e, bn_bp_stats* out) {
    if (!e || !out) return fail(BN_ERR_ARG, "null argument");
    *out = e->stats;
    out->resident_aborts = e->resident_aborts;
    return BN_OK;
}

