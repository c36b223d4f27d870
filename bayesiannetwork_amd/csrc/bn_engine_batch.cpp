// bn_engine_batch.cpp -- several evidence sets on one network per call (bn_bp_set_evidence_batch / bn_bp_run_batch*): an extension beside
// the drop-in, whose API takes one query at a time.  Every set keeps the bits, the sweep count and the residual history of its single run.
// Here: the batch's buffers, the evidence staging, the second (dense) engine, the entry points and the dispatch over the batch forms of
// the one-launch paths.  The runs themselves: bn_engine_batch_paths.cpp; which path wants a batch, and the layout of the staging
// block: bn_engine_policy.cpp and bn_batch_stage.cpp (pure host functions).
#include "bn_engine_internal.hpp"

// the batch's per-set buffers for at least n_sets sets (a larger batch than any before: everything anew)
static int batch_reserve(bn_engine* e, int32_t n_sets) {
    bn_engine::Batch& bt = e->batch;
    if (n_sets <= bt.cap_sets) return BN_OK;
    const Plan& p = e->plan;
    HIPCHK(hipStreamSynchronize(e->stream));
    bt = bn_engine::Batch();
    int r;
    const size_t B = size_t(n_sets);
    for (int i = 0; i < 2; ++i) {
        if ((r = dalloc(bt.d_rec[i], B * size_t(p.rec_total_doubles)))) return r;
        if ((r = dalloc(bt.d_node[i], B * size_t(p.node_doubles)))) return r;
        HIPCHK(hipMemsetAsync(bt.d_rec[i], 0, std::max<size_t>(B * p.rec_total_doubles, 1) * 8, e->stream));
        HIPCHK(hipMemsetAsync(bt.d_node[i], 0, std::max<size_t>(B * p.node_doubles, 1) * 8, e->stream));
    }
    if ((r = dalloc(bt.d_frozen, B * size_t(std::max(p.n_slots, 1))))) return r;
    if ((r = dalloc(bt.d_beliefs, B * size_t(p.node_off[p.n])))) return r;
    if ((r = dalloc(bt.d_res_hist, B * size_t(e->res_cap)))) return r;
    if ((r = dalloc(bt.d_sync, std::min<size_t>(B, kResidentMaxSets)))) return r;
    if ((r = dalloc(bt.d_ctl, B))) return r;
    if (e->small_ok && (r = dalloc(bt.d_s_state, B * size_t(2 * e->small.M + 2 * e->small.N)))) return r;
    HIPCHK(hipMemsetAsync(bt.d_ctl, 0, sizeof(Ctl) * B, e->stream));  // done_run = 0: no run is marked done
    HIPCHK(hipMemsetAsync(bt.d_frozen, 0, B * size_t(std::max(p.n_slots, 1)), e->stream));
    HIPCHK(hipMemsetAsync(bt.d_beliefs, 0, std::max<size_t>(B * p.node_off[p.n], 1) * 8, e->stream));
    HIPCHK(bt.h_ctl.alloc(B));
    std::memset(bt.h_ctl, 0, sizeof(Ctl) * B);
    HIPCHK(hipStreamSynchronize(e->stream));
    bt.cap_sets = n_sets;
    return BN_OK;
}

// buffers of evidence set q inside the batch arrays
BpBuffers bn_eng::batch_buffers_of(bn_engine* e, int32_t q) {
    const Plan& p = e->plan;
    const bn_engine::Batch& bt = e->batch;
    BpBuffers b = buffers_of(e);
    b.rec0 = bt.d_rec[0] + size_t(q) * p.rec_total_doubles;
    b.rec1 = bt.d_rec[1] + size_t(q) * p.rec_total_doubles;
    b.node0 = bt.d_node[0] + size_t(q) * p.node_doubles;
    b.node1 = bt.d_node[1] + size_t(q) * p.node_doubles;
    b.frozen = bt.d_frozen + size_t(q) * std::max(p.n_slots, 1);
    b.frozen_mark = 1;  // batches clear their marks with a memset per call
    b.beliefs = bt.d_beliefs + size_t(q) * p.node_off[p.n];
    b.res_hist = bt.d_res_hist + size_t(q) * e->res_cap;
    b.ctl = bt.d_ctl + q;
    return b;
}

// the options a batch on the second engine runs under: this engine's
static void sync_dense_options(bn_engine* e) {
    e->dense->multisweep = e->multisweep;
    e->dense->small_mode = e->small_mode;
    e->dense->mid_mode = e->mid_mode;
    e->dense->dag_mode = e->dag_mode;
}
// one entry per node of a plan for bn_policy::dense_keeps_bits
static std::vector<bn_policy::NodeLayout> node_layouts_of(const Plan& p) {
    std::vector<bn_policy::NodeLayout> out(size_t(p.n));
    for (int32_t v = 0; v < p.n; ++v) {
        if (p.node_class[v] < 0) continue;
        const ClassDesc& c = p.classes[p.node_class[v]];
        out[v] = {p.node_class[v], c.variant, c.G, int64_t(c.kv) * c.rows};
    }
    return out;
}
// The second engine with the dense layout (lanes_per_node = 2) that answers this engine's batches where bn_policy::batch_wants_dense
// says so: built from the same model at the first such call (the networks this concerns are small, so the second copy is too), given
// up for good where its sums would differ in the last bits from this engine's single queries (bn_policy::dense_keeps_bits).
static bn_engine* dense_engine_for_batch(bn_engine* e, int32_t n_sets, int& rc) {
    rc = BN_OK;
    if (!bn_policy::batch_wants_dense(e->facts, e->shape, oks_of(e), modes_of(e), n_sets) || e->dense_refused) return nullptr;
    if (!e->dense) {
        const Plan& p = e->plan;
        bn_model_desc d;
        d.n_nodes = p.n;
        d.k = p.k.data(); d.in_ptr = p.in_ptr.data(); d.in_idx = p.in_idx.data();
        d.cpt_off = p.cpt_off.data(); d.cpt = p.cpt_flat.data();
        d.device = e->device;
        d.lanes_per_node = p.group_wide ? 4 : 2;  // same lane-group split: same bits as this engine's single queries
        rc = bn_create(&d, &e->dense);
        if (rc) { e->dense = nullptr; return nullptr; }
        const std::vector<bn_policy::NodeLayout> own = node_layouts_of(e->plan), other = node_layouts_of(e->dense->plan);
        if (!bn_policy::dense_keeps_bits(own.data(), int32_t(own.size()), other.data(), int32_t(other.size()))) {
            free_engine(e->dense);
            e->dense = nullptr;
            e->dense_refused = true;
            return nullptr;
        }
    }
    sync_dense_options(e);
    e->dense->timing = e->timing;
    return e->dense;
}
static void adopt_batch_outcome(bn_engine* e) {  // what bn_bp_stats / bn_bp_last_path report after a forwarded batch
    e->last_path = e->dense->last_path;
    const bn_bp_stats own = e->stats;
    e->stats = e->dense->stats;
    e->stats.algorithmic_bytes_per_sweep = own.algorithmic_bytes_per_sweep;
    e->stats.layout_bytes_per_sweep = own.layout_bytes_per_sweep;
    e->stats.messages_per_sweep = own.messages_per_sweep;
}

// The batch's evidence (the staging block) -> the sets' tile buffers: marks cleared, one bp_evidence_kernel per set.  No-op when done already.
static int flush_batch_evidence(bn_engine* e) {
    bn_engine::Batch& bt = e->batch;
    if (!bt.ev_deferred) return BN_OK;
    const Plan& p = e->plan;
    HIPCHK(hipMemsetAsync(bt.d_frozen, 0, size_t(bt.n_sets) * size_t(std::max(p.n_slots, 1)), e->stream));
    for (int32_t q = 0; q < bt.n_sets; ++q) {
        const bn_stage::SetView v = bt.ev_layout.set_view(bt.ev_base, q);
        EvidenceArgs ea{batch_buffers_of(e, q), v.ne, v.node, v.off, v.val};
        if (int code = launch_bp_evidence(ea, e->stream))
            return fail(BN_ERR_HIP, std::string("bp_evidence launch failed: ") + hipGetErrorString(hipError_t(code)));
    }
    bt.ev_deferred = false;
    return BN_OK;
}

extern "C" int bn_bp_set_evidence_batch(bn_engine* e, int32_t n_sets, const int32_t* ne, const int32_t* ev_node,
                                        const int32_t* ev_off, const double* ev_val) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (int rc = refuse_unusable(e, BN_ERR_STATE)) return rc;
    e->batch_on_dense = false;
    if (n_sets >= 1 && n_sets <= BN_MAX_BATCH_SETS) {
        int rc;
        if (bn_engine* de = dense_engine_for_batch(e, n_sets, rc)) {
            rc = bn_bp_set_evidence_batch(de, n_sets, ne, ev_node, ev_off, ev_val);
            e->batch_on_dense = rc == BN_OK;
            return rc;
        } else if (rc) {
            return rc;
        }
    }
    if (n_sets < 1 || n_sets > BN_MAX_BATCH_SETS) return fail(BN_ERR_ARG, "n_sets must be in 1.." + std::to_string(BN_MAX_BATCH_SETS));
    if (e->plan.nranks > 1) return fail(BN_ERR_STATE, "batched evidence sets are not available on sharded engines");
    if (!ne) return fail(BN_ERR_ARG, "null ne");
    const Plan& p = e->plan;
    // validate every set like bn_bp_set_evidence does, at its slices of the concatenated arrays
    bn_stage::BatchLayout lay = bn_stage::layout_of(n_sets, ne, ev_off);
    for (int32_t q = 0; q < n_sets; ++q) {
        if (ne[q] < 0) return fail(BN_ERR_ARG, "negative evidence count");
        if (ne[q] > 0 && (!ev_node || !ev_off || !ev_val)) return fail(BN_ERR_ARG, "null evidence array");
        int rc = check_evidence(p, ne[q], ev_node ? ev_node + lay.node_at[q] : nullptr, ev_off ? ev_off + lay.off_at[q] : nullptr, e->ev_seen, e->ev_epoch);
        if (rc) return rc;
    }
    ON_DEVICE(e);
    int rc = batch_reserve(e, n_sets);
    if (rc) return rc;
    bn_engine::Batch& bt = e->batch;
    bt.n_sets = n_sets;
    bt.have_run = false;
    bt.ne.assign(ne, ne + n_sets);
    bt.ev_node.assign(ev_node, ev_node + lay.node_at[n_sets]);
    bt.ev_off.assign(ev_off, ev_off + (lay.node_at[n_sets] > 0 || ev_off ? lay.off_at[n_sets] : 0));
    bt.ev_val.assign(ev_val, ev_val + lay.val_at[n_sets]);
    const size_t bytes = lay.bytes;
    bt.ev_layout = std::move(lay);
    bt.ev_deferred = true;
    bt.dag_ev_applied = false;
    bt.beliefs_on_host = false;
    if (e->small_ok || e->mid_ok || dag_applies(e)) {
        // Small networks: the block is page-locked host memory that the kernels read in place -- the one-workgroup kernel (one
        // workgroup per set) each set's arrays, no copy command, no evidence launch per set, no synchronisation here; the tile
        // buffers get the marks and vectors only if another path runs the batch (flush_batch_evidence).  (No kernel is in
        // flight when the block is rewritten: every run entry point synchronises before it returns.)
        HIPCHK(bt.h_ev.reserve(bytes));
        bt.ev_base = bt.h_ev.dev();   // (every time: the batch before may have been staged in d_ev -- the options decide, and they may change)
        bt.ev_layout.fill(bt.h_ev, ev_node, ev_off, ev_val);
        bt.d_ev_meta = bt.ev_layout.meta(bt.ev_base);
        return BN_OK;
    }
    // every other network: one H2D copy, then one evidence kernel per set
    if (bytes > bt.ev_cap) {
        const size_t cap = std::max<size_t>(bytes * 2, 4096);
        bt.ev_cap = 0;   // (a failed allocation leaves d_ev empty)
        HIPCHK(dev_malloc(bt.d_ev, cap));
        bt.ev_cap = cap;
    }
    bt.ev_base = bt.d_ev;
    std::vector<char> host(std::max<size_t>(bytes, 1));
    bt.ev_layout.fill(host.data(), ev_node, ev_off, ev_val);
    HIPCHK(hipMemcpyAsync(bt.d_ev, host.data(), bytes, hipMemcpyHostToDevice, e->stream));
    bt.d_ev_meta = bt.ev_layout.meta(bt.ev_base);
    if ((rc = flush_batch_evidence(e))) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));  // `host` is a local
    return BN_OK;
}

// ---- the one-launch paths of a batch (bn_bp_run_batch_device): the PathDriver table of single queries, batch forms.  Which of them
// wants the batch: bn_engine_policy.cpp, handed the engine's facts, shape and options and what only the device side knows.
static bn_policy::BatchDevice batch_device_of(const bn_engine* e) { return {e->batch.d_s_state != nullptr, e->batch.ev_base != nullptr}; }
static bool batch_small_wanted(const bn_engine* e) { return bn_policy::batch_small_wanted(e->facts, e->shape, oks_of(e), modes_of(e), batch_device_of(e)); }
static bool batch_dag_wanted(const bn_engine* e) { return bn_policy::batch_dag_wanted(e->facts, e->shape, oks_of(e), modes_of(e), batch_device_of(e)); }
static bool batch_mid_wanted(const bn_engine* e) { return bn_policy::batch_mid_wanted(e->facts, e->shape, oks_of(e), modes_of(e), batch_device_of(e)); }
static bool batch_resident_wanted(const bn_engine* e) { return bn_policy::batch_resident_wanted(e->facts, e->shape, oks_of(e), modes_of(e), batch_device_of(e)); }
static const PathDriver kBatchPaths[] = {
    {3, batch_small_wanted, run_batch_small, small_gave_up, "", nullptr, &bn_engine::small_cooldown, false},
    {5, batch_dag_wanted, run_batch_dag, dag_gave_up, "the register-resident DAG kernel (bn_dag.hip, batch)", nullptr, &bn_engine::dag_cooldown, false},
    {4, batch_mid_wanted, run_batch_mid, mid_gave_up, "the several-workgroup item kernel (bn_mid.hip, batch)", nullptr, &bn_engine::mid_cooldown, false},
    {2, batch_resident_wanted, run_batch_resident, resident_gave_up, "the resident-tile kernel (bn_resident.hip, batch)", resident_ran_ok, &bn_engine::resident_cooldown, true},
};

extern "C" int bn_bp_run_batch_device(bn_engine* e, double eps, int32_t max_sweeps, int32_t* sweeps_out, double* residual_out) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (e->batch_on_dense && e->dense) {
        sync_dense_options(e);
        const int rc = bn_bp_run_batch_device(e->dense, eps, max_sweeps, sweeps_out, residual_out);
        if (rc == BN_OK) adopt_batch_outcome(e);
        return rc;
    }
    if (int rc = refuse_unusable(e, BN_ERR_STATE)) return rc;
    if (max_sweeps < 0) return fail(BN_ERR_ARG, "max_sweeps < 0");
    bn_engine::Batch& bt = e->batch;
    if (bt.n_sets < 1) return fail(BN_ERR_STATE, "call bn_bp_set_evidence_batch first");
    const auto t_begin = std::chrono::steady_clock::now();
    ON_DEVICE(e);
    bt.sweeps.assign(bt.n_sets, 0);
    bt.residual.assign(bt.n_sets, 0.0);
    bt.beliefs_on_host = false;
    // The one-launch paths of a batch, in the order of kBatchPaths (the same drivers' table as a single query's, with the batch forms of
    // wanted / run): the first that wants the batch and is not paused runs every set; one that gives up a bounded wait pauses itself,
    // and the whole batch is run again by the next; what none of them takes runs with one launch per sweep, one set per blockIdx.y.
    int rc = BN_ERR_STATE;
    bool evidence_flushed = false, restage = false;
    for (const PathDriver& d : kBatchPaths) {
        if (!d.wanted(e)) continue;
        if (d.reads_tile_evidence && !evidence_flushed) {   // the tile kernels read the sets' evidence from their own buffers
            if ((rc = flush_batch_evidence(e))) return rc;
            evidence_flushed = true;
        }
        int32_t& cooldown = e->*(d.cooldown);
        if (cooldown > 0) { --cooldown; rc = BN_ERR_STATE; continue; }   // paused after a launch that gave up
        rc = d.run(e, eps, max_sweeps, nullptr);
        if (rc == BN_OK) {
            if (d.ran_ok) d.ran_ok(e);
            break;
        }
        if (rc != BN_ERR_STATE) return rc;
        if (int g = d.gave_up(e, d.what)) return g;   // counters, pause, one line on stderr
        bt.sweeps.assign(bt.n_sets, 0);       // the whole batch again on the next path
        bt.residual.assign(bt.n_sets, 0.0);
        restage = restage || d.reads_tile_evidence;
    }
    if (rc != BN_OK) {
        if (restage) {
            // marks / vectors possibly half-written by an aborted launch of the tile kernels: apply every set's evidence again
            std::vector<int32_t> ne = bt.ne, ev_node = bt.ev_node, ev_off = bt.ev_off;
            std::vector<double> ev_val = bt.ev_val;
            rc = bn_bp_set_evidence_batch(e, int32_t(ne.size()), ne.data(), ev_node.data(), ev_off.data(), ev_val.data());
            if (rc) return rc;
            bt.sweeps.assign(bt.n_sets, 0);
            bt.residual.assign(bt.n_sets, 0.0);
        }
        if ((rc = flush_batch_evidence(e))) return rc;
        rc = run_batch_launches(e, eps, max_sweeps);
        if (rc) return rc;
    }
    bt.have_run = true;
    e->stats.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    for (int32_t q = 0; q < bt.n_sets; ++q) {
        if (sweeps_out) sweeps_out[q] = bt.sweeps[q];
        if (residual_out) residual_out[q] = bt.residual[q];
    }
    return BN_OK;
}

extern "C" int bn_bp_copy_beliefs_batch(bn_engine* e, double* beliefs_out) {
    if (!e || !beliefs_out) return fail(BN_ERR_ARG, "null argument");
    if (e->batch_on_dense && e->dense) return bn_bp_copy_beliefs_batch(e->dense, beliefs_out);
    if (e->host_only || !e->batch.have_run) return fail(BN_ERR_STATE, "no batched run to copy from");
    if (e->batch.beliefs_on_host) {  // the last run wrote them into page-locked host memory
        std::memcpy(beliefs_out, e->batch.h_beliefs, sizeof(double) * size_t(e->batch.n_sets) * e->plan.node_off[e->plan.n]);
        return BN_OK;
    }
    ON_DEVICE(e);
    HIPCHK(hipMemcpyAsync(beliefs_out, e->batch.d_beliefs, sizeof(double) * size_t(e->batch.n_sets) * e->plan.node_off[e->plan.n],
                          hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return BN_OK;
}

extern "C" int bn_bp_residual_history_batch(bn_engine* e, int32_t set, double* out, int32_t cap) {
    if (!e || !out || cap < 0) return fail(BN_ERR_ARG, "bad argument");
    if (e->batch_on_dense && e->dense) return bn_bp_residual_history_batch(e->dense, set, out, cap);
    if (e->host_only || !e->batch.have_run) return fail(BN_ERR_STATE, "no batched run yet");
    if (set < 0 || set >= e->batch.n_sets) return fail(BN_ERR_ARG, "set index out of range");
    const int32_t cnt = std::min({cap, e->batch.sweeps[set], e->res_cap});
    ON_DEVICE(e);
    if (cnt > 0)
        HIPCHK(hipMemcpy(out, e->batch.d_res_hist + size_t(set) * e->res_cap, sizeof(double) * cnt, hipMemcpyDeviceToHost));
    return cnt;
}

extern "C" int bn_bp_run_batch(bn_engine* e, int32_t n_sets, const int32_t* ne, const int32_t* ev_node, const int32_t* ev_off,
                               const double* ev_val, double eps, int32_t max_sweeps, double* beliefs_out, int32_t* sweeps_out,
                               double* residual_out) {
    if (!beliefs_out) return fail(BN_ERR_ARG, "null beliefs_out");
    int rc = bn_bp_set_evidence_batch(e, n_sets, ne, ev_node, ev_off, ev_val);
    if (rc) return rc;
    bn_engine* on = (e->batch_on_dense && e->dense) ? e->dense : e;
    on->batch.direct_out = true;   // (the one-workgroup path writes the marginals into page-locked host memory; other paths ignore it)
    rc = bn_bp_run_batch_device(e, eps, max_sweeps, sweeps_out, residual_out);
    on->batch.direct_out = false;
    if (rc) return rc;
    return bn_bp_copy_beliefs_batch(e, beliefs_out);
}
