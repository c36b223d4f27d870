// bn_engine_batch_paths.cpp -- the runs of a batch of evidence sets (bn_bp_run_batch_device, bn_engine_batch.cpp): the batch forms of
// the one-launch paths -- resident tiles, one workgroup per set, several workgroups per set, the register-resident DAG path -- and the
// per-sweep launches with one set per blockIdx.y, with what they share: reading the sets' control blocks, the tail of a run, and the
// launches of a batch's chunks behind each other with one wait for all of them.  Every set gets the bits of its single query.
#include "bn_engine_internal.hpp"

namespace {
// what the control blocks of sets [first, first + count) report once their launches have ended: sweeps and last residual of every
// set into the batch's arrays; the span of the device clock (100 MHz) over the sets and the largest sweep count come back
struct Collected {
    unsigned long long t0 = ~0ull, t1 = 0;
    int32_t sweeps = 0;
    float devclock_ms() const { return t1 > t0 ? float(double(t1 - t0) * 1e-5) : 0.f; }
};
Collected collect_sets(bn_engine::Batch& bt, int32_t first, int32_t count) {
    Collected c;
    for (int32_t q = first; q < first + count; ++q) {
        bt.sweeps[q] = bt.h_ctl[q].n_sweeps;
        bt.residual[q] = bt.h_ctl[q].last_res;
        c.t0 = std::min(c.t0, bt.h_ctl[q].t_first);
        c.t1 = std::max(c.t1, bt.h_ctl[q].t_last);
        c.sweeps = std::max(c.sweeps, bt.h_ctl[q].n_sweeps);
    }
    return c;
}

// what bn_bp_last_path / bn_bp_stats report after a batch
void finish_batch(bn_engine* e, int path, int32_t launches, float kernel_ms, float devclock_ms, int32_t sweeps) {
    e->last_path = path;
    e->stats.sweep_launches = launches;
    e->stats.sweep_kernel_ms = kernel_ms;
    e->stats.sweep_devclock_ms = devclock_ms;
    e->stats.sweeps = sweeps;
    e->stats.memo_sweeps = 0;   // (batches run every sweep)
    e->stats.memo_depth = 0;
}

// The chunks of a batch follow each other on the stream and the host waits ONCE for all of them (a wait per chunk cost a batch of 16
// sets on the resident tiles four wake-ups and four launch latencies).  enqueue(c): chunk c's launches, no wait; collect(c): what
// the chunk reported, once the stream has drained; dirty(): the path's polled words (and whatever else an aborted or failed launch
// may have left half-done) are to be set up again.  The stream is drained also after a failed enqueue: what is on it writes into
// the batch's buffers.  The abort word -- raised by any workgroup that gave up a bounded wait -- goes before what the control blocks
// say: BN_ERR_STATE with `gave_up_text`, and the caller hands the batch to the next path.  ms: HIP events around all the launches.
template <class Enqueue, class Collect, class Dirty>
int run_chunks(bn_engine* e, int32_t n_chunks, const char* gave_up_text, int32_t& launches, float* ms, Enqueue enqueue, Collect collect, Dirty dirty) {
    hipStream_t s = e->stream;
    *e->h_abort = 0;
    if (ms) {
        if (int rc = ensure_events(e, 2)) return rc;
        HIPCHK(hipEventRecord(e->events[0], s));
    }
    int rc = BN_OK;
    int32_t enqueued = 0;
    while (enqueued < n_chunks && (rc = enqueue(enqueued)) == BN_OK) ++enqueued;
    if (ms && rc == BN_OK) HIPCHK(hipEventRecord(e->events[1], s));
    const hipError_t drained = hipStreamSynchronize(s);
    if (drained != hipSuccess && rc == BN_OK) rc = fail(BN_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(drained));
    launches += enqueued;
    if (rc == BN_OK && *e->h_abort != 0) rc = fail(BN_ERR_STATE, gave_up_text);
    if (rc == BN_OK && ms) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, e->events[0], e->events[1]));
        *ms += t;
    }
    for (int32_t c = 0; c < enqueued && rc == BN_OK; ++c) rc = collect(c);
    *e->h_abort = 0;
    if (rc != BN_OK) dirty();
    return rc;
}

// a launch of the several-workgroup or the one-workgroup kernel reads the sets' evidence in the staging block, unless the tile
// buffers hold it already (whole: every set's meta entry; otherwise set q's, which a single-set launch reads as entry blockIdx.x = 0)
template <class Args>
void stage_evidence_of(const bn_engine::Batch& bt, Args& x, int32_t meta_of_set) {
    if (!bt.ev_deferred) return;
    const bn_stage::SetView all = bt.ev_layout.set_view(bt.ev_base, 0);
    x.ev_mode = 1;
    x.ev_node = all.node; x.ev_off = all.off; x.ev_val = all.val;
    x.ev_meta = bt.d_ev_meta + bn_stage::kMetaWords * meta_of_set;
}
}  // namespace

// ---- resident tiles ------------------------------------------------------------------------------------------------------------------
// sets [first, first + count) through the resident kernel, round-robin in one launch (count <= kResidentMaxSets): enqueue only;
// consecutive launches share the barrier words -- the generations count on.
static int enqueue_batch_resident_chunk(bn_engine* e, double eps, int32_t max_sweeps, int32_t first, int32_t count, int32_t begin, uint32_t mask) {
    bn_engine::Batch& bt = e->batch;
    hipStream_t s = e->stream;
    if (bt.sync_dirty || bt.gen_base > (1u << 29)) {
        HIPCHK(hipMemsetAsync(bt.d_sync, 0, sizeof(ResidentSync) * size_t(std::min(bt.cap_sets, kResidentMaxSets)), s));
        bt.sync_dirty = false;
        bt.gen_base = 0;
    }
    for (int32_t q = 0; q < count; ++q)
        if ((mask >> q) & 1u) bt.h_ctl[first + q].run_id = 0;
    const SetStrides st = strides_of(e);
    ResidentArgs a{batch_buffers_of(e, first), eps, max_sweeps, begin, kResidentBudget, e->run_id, bt.gen_base, 5000000ull, bt.d_sync,
                   bt.h_ctl.dev() + first, e->shape.blocks, e->shape.waves, count, mask, st.rec, st.node, st.slot, st.belief, st.res_hist,
                   nullptr, nullptr, nullptr, 0, nullptr, 1, 0, e->h_abort.dev()};
    if (int code = launch_bp_resident(a, e->shape.blocks + resident_service_blocks(e->shape.blocks), e->shape.lean, s))
        return fail(BN_ERR_HIP, std::string("bp_resident launch failed: ") + hipGetErrorString(hipError_t(code)));
    bt.gen_base += kResidentBudget + 1;
    return BN_OK;
}

// after the stream has drained: what the launch of sets [first, first + count) (those in `mask`) reported.  next = the sets whose run
// goes on beyond the launch's budget of iterations.
static int collect_batch_resident_chunk(bn_engine* e, int32_t first, int32_t count, uint32_t mask, uint32_t& next, double& dev_ticks) {
    bn_engine::Batch& bt = e->batch;
    next = 0;
    for (int32_t q = 0; q < count; ++q) {
        if (!((mask >> q) & 1u)) continue;
        const Ctl& c = bt.h_ctl[first + q];
        if (c.run_id != e->run_id) return fail(BN_ERR_STATE, "resident kernel did not report (stale control block)");
        if (c.done < 0) return fail(BN_ERR_STATE, "resident kernel gave up a barrier wait");
        if (c.done == 0) next |= 1u << q;
    }
    collect_sets(bt, first, count);   // (a set not in `mask` reports what it did when its run ended)
    dev_ticks += double(bt.h_ctl[first].t_last - bt.h_ctl[first].t_first);
    return BN_OK;
}

// every set through the resident kernel: up to kResidentMaxSets per launch, further sets in further launches
int bn_eng::run_batch_resident(bn_engine* e, double eps, int32_t max_sweeps, double*) {
    bn_engine::Batch& bt = e->batch;
    next_run_id(e);
    int32_t launches = 0;
    double dev_ticks = 0.0;
    float ms = 0.f;
    struct Chunk { int32_t first, count; uint32_t next; };
    std::vector<Chunk> chunks;
    for (int32_t count : bn_policy::resident_batch_chunks(bt.n_sets)) chunks.push_back(Chunk{chunks.empty() ? 0 : chunks.back().first + chunks.back().count, count, 0u});
    const char* const gave_up = "resident kernel gave up a barrier wait";
    auto dirty = [&] { bt.sync_dirty = true; };
    int rc = run_chunks(e, int32_t(chunks.size()), gave_up, launches, e->timing ? &ms : nullptr,
        [&](int32_t c) { return enqueue_batch_resident_chunk(e, eps, max_sweeps, chunks[c].first, chunks[c].count, 0, (1u << chunks[c].count) - 1u); },
        [&](int32_t c) { return collect_batch_resident_chunk(e, chunks[c].first, chunks[c].count, (1u << chunks[c].count) - 1u, chunks[c].next, dev_ticks); },
        dirty);
    if (rc != BN_OK) return rc;
    // runs beyond one launch's budget of iterations (rare): those sets go on, chunk by chunk, a launch and a wait at a time
    for (Chunk& c : chunks) {
        for (int32_t begin = kResidentBudget; c.next != 0; begin += kResidentBudget) {
            const uint32_t mask = c.next;
            rc = run_chunks(e, 1, gave_up, launches, nullptr,
                [&](int32_t) { return enqueue_batch_resident_chunk(e, eps, max_sweeps, c.first, c.count, begin, mask); },
                [&](int32_t) { return collect_batch_resident_chunk(e, c.first, c.count, mask, c.next, dev_ticks); }, dirty);
            if (rc != BN_OK) return rc;
        }
    }
    finish_batch(e, 2, launches, ms, float(dev_ticks * 1e-5), *std::max_element(bt.sweeps.begin(), bt.sweeps.end()));
    return BN_OK;
}

// ---- one launch per sweep ------------------------------------------------------------------------------------------------------------
// Every set in each per-sweep launch (blockIdx.y = evidence set): any tile variants.  The sets share the launch
// and its latency -- what a small or latency-bound network pays for -- and the CPT lines in the caches; each keeps
// its own records, node vectors, marks, residual slots and done mark, so it stops on the sweep its single run
// stops on (a converged set's blocks return at once in the launches the others still need).
int bn_eng::run_batch_launches(bn_engine* e, double eps, int32_t max_sweeps) {
    bn_engine::Batch& bt = e->batch;
    const Plan& p = e->plan;
    hipStream_t s = e->stream;
    next_run_id(e);
    const int32_t B = bt.n_sets;
    if (!bt.rows_clean) {  // an earlier batched run did not end through its finish kernel
        for (int32_t q = 0; q < bt.cap_sets; ++q)
            if (int code = launch_bp_reset(batch_buffers_of(e, q), s))
                return fail(BN_ERR_HIP, std::string("bp_reset launch failed: ") + hipGetErrorString(hipError_t(code)));
    }
    bt.rows_clean = false;
    const SetStrides st = strides_of(e);
    const BpBuffers b0 = batch_buffers_of(e, 0);
    const int32_t nt = int32_t(p.tiles.size());
    const int grid = ((nt + 1 + kWavesPerBlock - 1) / kWavesPerBlock + 7) & ~7;
    static const bool no_light = std::getenv("BN_NO_LIGHT") != nullptr;
    int32_t launched = 0;
    int32_t batch = bt.predicted_sweeps > 0 ? bt.predicted_sweeps : (e->predicted_sweeps > 0 ? e->predicted_sweeps : 8);
    for (;;) {
        if (max_sweeps > 0) batch = std::min(batch, max_sweeps - launched);
        for (int32_t i = 0; i < batch; ++i) {
            const int32_t sweep = launched + i;
            const int cur = sweep & 1;
            SweepArgs sa{b0, bt.d_rec[cur], bt.d_rec[cur ^ 1], bt.d_node[cur], bt.d_node[cur ^ 1], eps, sweep, 0, nt, 1, e->run_id, st};
            // B == 1 runs the plain instantiation on set 0's buffers
            if (launch_bp_sweep(sa, grid, B, false, p.light && !no_light, p.variants, s)) return fail(BN_ERR_HIP, "bp_sweep launch failed");
        }
        launched += batch;
        FinishArgs fa{b0, eps, launched, (max_sweeps > 0 && launched >= max_sweeps) ? 1 : 0, e->run_id, bt.h_ctl.dev(), st};
        if (launch_bp_finish(fa, e->grid_tiles, B, s)) return fail(BN_ERR_HIP, "bp_finish launch failed");
        HIPCHK(hipStreamSynchronize(s));
        bool all_done = true;
        for (int32_t q = 0; q < B; ++q) {
            if (bt.h_ctl[q].run_id != e->run_id) return fail(BN_ERR_STATE, "finish kernel did not report (stale control block)");
            if (bt.h_ctl[q].done == 0) all_done = false;
        }
        if (all_done) break;
        batch = 8;
    }
    bt.rows_clean = true;  // every set's run ended in a finish kernel that saw it over
    const Collected c = collect_sets(bt, 0, B);
    bt.predicted_sweeps = c.sweeps;
    finish_batch(e, 0, launched, 0.f, c.devclock_ms(), c.sweeps);
    return BN_OK;
}

// ---- one workgroup per set -----------------------------------------------------------------------------------------------------------
// Small networks: one workgroup per evidence set, all sets in ONE launch, each set stopping by itself (bn_small.hip).
int bn_eng::run_batch_small(bn_engine* e, double eps, int32_t max_sweeps, double*) {
    bn_engine::Batch& bt = e->batch;
    const Plan& p = e->plan;
    hipStream_t s = e->stream;
    next_run_id(e);
    const int32_t B = bt.n_sets;
    const int64_t state_stride = 2 * int64_t(e->small.M) + 2 * int64_t(e->small.N);
    SmallArgs a = small_args_of(e, batch_buffers_of(e, 0), eps, max_sweeps, 0, bt.h_ctl.dev());
    a.state = bt.d_s_state; a.sets = strides_of(e); a.state_stride = state_stride;
    const size_t per_set = size_t(p.node_off[p.n]);
    if (bt.direct_out) {  // bn_bp_run_batch: the marginals go straight into page-locked host memory (no copy command, no second sync)
        if (size_t(B) * per_set > bt.h_beliefs.capacity()) HIPCHK(bt.h_beliefs.alloc(size_t(bt.cap_sets) * per_set));   // (for every set the batch's buffers hold)
        a.b.beliefs = bt.h_beliefs.dev();
    }
    bt.beliefs_on_host = bt.direct_out;
    stage_evidence_of(bt, a, 0);
    if (int code = launch_bp_small(a, e->small.waves, e->small.lds_bytes, B, s))
        return fail(BN_ERR_HIP, std::string("bp_small launch failed: ") + hipGetErrorString(hipError_t(code)));
    HIPCHK(hipStreamSynchronize(s));
    int32_t launches = 1;
    for (int32_t q = 0; q < B; ++q) {
        if (bt.h_ctl[q].run_id != e->run_id) return fail(BN_ERR_HIP, "bp_small kernel did not report (stale control block)");
        while (bt.h_ctl[q].done == 0) {  // a set that used up the launch's budget of iterations goes on by itself
            SmallArgs c = small_args_of(e, batch_buffers_of(e, q), eps, max_sweeps, bt.h_ctl[q].n_sweeps, bt.h_ctl.dev() + q);
            c.state = bt.d_s_state + size_t(q) * state_stride;
            if (bt.direct_out) c.b.beliefs = bt.h_beliefs.dev() + size_t(q) * per_set;
            stage_evidence_of(bt, c, q);
            if (int code = launch_bp_small(c, e->small.waves, e->small.lds_bytes, 1, s))
                return fail(BN_ERR_HIP, std::string("bp_small launch failed: ") + hipGetErrorString(hipError_t(code)));
            HIPCHK(hipStreamSynchronize(s));
            ++launches;
        }
    }
    const Collected c = collect_sets(bt, 0, B);
    bt.predicted_sweeps = c.sweeps;
    finish_batch(e, 3, launches, 0.f, c.devclock_ms(), c.sweeps);
    return BN_OK;
}

// ---- several workgroups per set ------------------------------------------------------------------------------------------------------
// Mid-size networks: every set runs exactly like a single query (same kernel, same bits), as many sets per launch as fit the
// chip with a workgroup per CU (the grid barrier needs every workgroup of a set resident).  BN_ERR_STATE: a grid wait gave up.
int bn_eng::run_batch_mid(bn_engine* e, double eps, int32_t max_sweeps, double*) {
    bn_engine::Batch& bt = e->batch;
    next_run_id(e);
    const int32_t B = bt.n_sets;
    const int32_t per_launch = bn_policy::mid_sets_per_launch(e->n_cus, int32_t(e->mid.parts.size()), B);
    if (int rc = mid_reserve_slots(e, per_launch)) return rc;
    const SetStrides st = strides_of(e);
    const BpBuffers b0 = batch_buffers_of(e, 0);
    const char* const gave_up = "a workgroup of the mid-size kernel gave up its grid wait";
    int32_t launches = 0;
    // (a chunk's sets use the state slots the previous chunk's kernel has left)
    int rc = run_chunks(e, (B + per_launch - 1) / per_launch, gave_up, launches, nullptr,
        [&](int32_t c) {
            MidArgs a = mid_args_of(e, b0, st, bt.h_ctl.dev(), eps, max_sweeps, 0, c * per_launch, 0);
            stage_evidence_of(bt, a, 0);
            return mid_launch(e, a, std::min(per_launch, B - c * per_launch), nullptr, nullptr, false);
        },
        [&](int32_t c) {
            for (int32_t q = c * per_launch; q < std::min(B, (c + 1) * per_launch); ++q) {
                if (bt.h_ctl[q].done < 0) return fail(BN_ERR_STATE, gave_up);
                if (bt.h_ctl[q].run_id != e->run_id) return fail(BN_ERR_HIP, "bp_mid kernel did not report (stale control block)");
            }
            return int(BN_OK);
        },
        [] {});
    e->ev_upload_pending = false;
    if (rc != BN_OK) return rc;
    for (int32_t q = 0; q < B; ++q) {
        while (bt.h_ctl[q].done == 0) {  // a set that used up the launch's budget of iterations goes on by itself, in its slot
            MidArgs c = mid_args_of(e, b0, st, bt.h_ctl.dev(), eps, max_sweeps, bt.h_ctl[q].n_sweeps, q, q % per_launch);
            stage_evidence_of(bt, c, 0);
            if ((rc = mid_launch(e, c, 1, nullptr, nullptr))) return rc;
            ++launches;
            if (bt.h_ctl[q].done < 0) return fail(BN_ERR_STATE, gave_up);
        }
    }
    const Collected c = collect_sets(bt, 0, B);
    bt.predicted_sweeps = c.sweeps;
    finish_batch(e, 4, launches, 0.f, c.devclock_ms(), c.sweeps);
    return BN_OK;
}

// ---- the register-resident DAG path --------------------------------------------------------------------------------------------------
// Sets [first, first + count) of the batch in ONE launch of the register-resident DAG kernel: the sets take turns inside an
// iteration, so a set's barrier completes while the others sweep, and one set of CPT registers serves them all (bn_dag.hip,
// dag_drive).  Every set has its own state, marks, barrier words, residual history and control block and keeps the bits and the
// sweep count of its single run.  Enqueue only: the next chunk's evidence lands in the state slots when the previous chunk's kernel
// has left them.  run_id: the id the chunk's control blocks must report under.
static int enqueue_batch_dag_chunk(bn_engine* e, double eps, int32_t max_sweeps, int32_t first, int32_t count, uint32_t& run_id) {
    bn_engine::Batch& bt = e->batch;
    const Plan& p = e->plan;
    const DagPlan& dp = e->dag;
    hipStream_t s = e->stream;
    const size_t state_d = size_t(dag_state_doubles(dp.E, dp.n));
    if (bt.dag_sets < kDagMaxSets) {   // first use: every set's state, marks and barrier words
        int r;
        if ((r = dalloc(bt.d_g_state, state_d * kDagMaxSets))) return r;
        if ((r = dalloc(bt.d_g_frz, size_t(dp.n) * kDagMaxSets))) return r;
        if ((r = dalloc(bt.d_g_sync, size_t(kDagMaxSets)))) return r;
        HIPCHK(hipMemsetAsync(bt.d_g_state, 0, state_d * kDagMaxSets * sizeof(double), s));
        HIPCHK(hipMemsetAsync(bt.d_g_frz, 0, size_t(dp.n) * kDagMaxSets, s));
        bt.dag_sets = kDagMaxSets;
        bt.dag_mark = 0;
        bt.dag_sync_dirty = true;
    }
    // The evidence of a batch that fits the state slots (one chunk) on a network without padding stays where the first run put it: the
    // sweeps carry an observed node's vectors over and sweep 0 reads nothing else of the old state (the single query's dag_ev_applied).
    const bool keeps = dp.uniform4 && first == 0 && count == bt.n_sets;
    const bool apply = !(keeps && bt.dag_ev_applied);
    bt.dag_ev_applied = false;   // (true again only once every launch of this chunk is on the stream: an error return below leaves no claim behind)
    if (apply) {   // pi(v) = lambda(v) = the given vector in both buffers, node marked (:68-73): every set of the chunk in one launch
        if (bt.dag_mark == 255) {  // the mark values are used up: start over
            HIPCHK(hipMemsetAsync(bt.d_g_frz, 0, size_t(dp.n) * kDagMaxSets, s));
            bt.dag_mark = 0;
        }
        ++bt.dag_mark;
        DagEvidenceBatch eb{};
        DagInitBatch ib{};
        for (int32_t q = 0; q < count; ++q) {
            const bn_stage::SetView v = bt.ev_layout.set_view(bt.ev_base, first + q);
            eb.set[q] = DagEvidenceArgs{v.ne, dp.n, dp.E, v.node, v.off, v.val, bt.d_g_state + size_t(q) * state_d,
                                        bt.d_g_frz + size_t(q) * dp.n, bt.dag_mark, e->dag_img.k, e->dag_img.nperm};
            ib.set[q] = DagInitArgs{dp.n, dp.E, e->dag_img.inptr, e->dag_img.inidx, e->dag_img.k, e->dag_img.init, bt.d_g_state + size_t(q) * state_d,
                                    bt.d_g_frz + size_t(q) * dp.n, bt.dag_mark, e->dag_img.eperm, e->dag_img.nperm};
        }
        if (int code = launch_dag_evidence_batch(eb, count, s))
            return fail(BN_ERR_HIP, std::string("dag_evidence launch failed: ") + hipGetErrorString(hipError_t(code)));
        if (!dp.uniform4) {
            if (int code = launch_dag_init_batch(ib, count, s))
                return fail(BN_ERR_HIP, std::string("dag_init launch failed: ") + hipGetErrorString(hipError_t(code)));
        }
    }
    if (bt.dag_sync_dirty || bt.dag_gen_base > (1u << 29)) {
        HIPCHK(hipMemsetAsync(bt.d_g_sync, 0, sizeof(ResidentSync) * size_t(kDagMaxSets), s));
        bt.dag_sync_dirty = false;
        bt.dag_gen_base = 0;
    }
    next_run_id(e);
    run_id = e->run_id;
    DagArgs a{};
    a.b = buffers_of(e);
    a.b.beliefs = bt.d_beliefs + size_t(first) * p.node_off[p.n];
    a.b.res_hist = bt.d_res_hist + size_t(first) * e->res_cap;
    a.eps = eps; a.max_sweeps = max_sweeps; a.sweep_begin = 0; a.budget = kDagBudget; a.run_id = e->run_id;
    a.gen_base = bt.dag_gen_base;
    a.timeout_ticks = 5000000ull;
    a.sync = bt.d_g_sync; a.host_ctl = bt.h_ctl.dev() + first; a.host_abort = e->h_abort.dev();
    a.n = dp.n; a.E = dp.E; a.n_blocks = dp.blocks;
    a.tiles = e->dag_img.tiles; a.slot_ptr = e->dag_img.slotptr; a.cnode = e->dag_img.cnode; a.pitem = e->dag_img.pitem; a.oedge = e->dag_img.oedge;
    a.cpt_img = e->dag_img.cpt; a.npi_init = e->dag_img.init; a.state = bt.d_g_state; a.frz = bt.d_g_frz; a.frz_mark = bt.dag_mark;
    static const int poll_sleep = std::getenv("BN_DAG_SLEEP") ? std::atoi(std::getenv("BN_DAG_SLEEP")) : 1;
    static const int first_delay = std::getenv("BN_DAG_DELAY") ? std::atoi(std::getenv("BN_DAG_DELAY")) : 30;
    a.poll_sleep = poll_sleep;
    a.first_poll_delay = first_delay;
    a.n_sets = count; a.set_mask = (1u << count) - 1u;
    a.state_init = dp.uniform4 ? 0 : 1; a.node_k = e->dag_img.k; a.node_off = e->dag_img.noff;
    a.state_stride = int64_t(state_d); a.frz_stride = dp.n; a.belief_stride = p.node_off[p.n]; a.res_hist_stride = e->res_cap;
    for (int32_t q = 0; q < count; ++q) bt.h_ctl[first + q].run_id = 0;
    if (int code = launch_bp_dag(a, dp.stream, s))
        return fail(BN_ERR_HIP, std::string("bp_dag launch failed: ") + hipGetErrorString(hipError_t(code)));
    bt.dag_gen_base += kDagBudget + 1;
    bt.dag_ev_applied = keeps;
    return BN_OK;
}

// The register-resident DAG path (bn_dag.hip) answers a batch up to bn_policy::dag_sets_per_launch sets a launch; a set that does not
// finish in its launch (more than kDagBudget sweeps), and a batch of one, is a single query's run that reads the set's evidence in the
// batch's staging block and writes its marginals and residual history into the set's slots.  BN_ERR_STATE: a grid wait gave up.
int bn_eng::run_batch_dag(bn_engine* e, double eps, int32_t max_sweeps, double*) {
    if (int rc0 = ensure_dag(e)) return rc0;   // (first use of the path on this engine)
    bn_engine::Batch& bt = e->batch;
    const Plan& p = e->plan;
    int32_t launches = 0, max_sw = 0;
    double dev_ms = 0.0;
    std::vector<char> left(size_t(bt.n_sets), 1);   // set q is still to be run on its own
    // (an explicit BN_DAG_SETS=0 has always meant one set per launch, like every value below 1)
    static const char* const forced_text = std::getenv("BN_DAG_SETS");
    static const int per_launch = bn_policy::dag_sets_per_launch(forced_text ? (std::atoi(forced_text) != 0 ? std::atoi(forced_text) : -1) : 0);
    if (per_launch > 1 && bt.n_sets > 1) {
        std::vector<uint32_t> run_ids(size_t((bt.n_sets + per_launch - 1) / per_launch), 0u);
        int rc = run_chunks(e, int32_t(run_ids.size()), "a block of the register-resident DAG kernel gave up its grid wait", launches, nullptr,
            [&](int32_t c) { return enqueue_batch_dag_chunk(e, eps, max_sweeps, c * per_launch, std::min(per_launch, bt.n_sets - c * per_launch), run_ids[c]); },
            [&](int32_t c) {
                const int32_t first = c * per_launch, count = std::min(per_launch, bt.n_sets - first);
                for (int32_t q = first; q < first + count; ++q)
                    if (bt.h_ctl[q].done < 0) return fail(BN_ERR_STATE, "a block of the register-resident DAG kernel gave up its grid wait");
                for (int32_t q = first; q < first + count; ++q)
                    if (bt.h_ctl[q].run_id != run_ids[c]) return fail(BN_ERR_HIP, "bp_dag kernel did not report (stale control block)");
                dev_ms += double(bt.h_ctl[first].t_last - bt.h_ctl[first].t_first) * 1e-5;
                max_sw = std::max(max_sw, collect_sets(bt, first, count).sweeps);
                for (int32_t q = first; q < first + count; ++q) left[q] = bt.h_ctl[q].done == 0;   // the budget of one launch ran out: this set goes on alone
                return int(BN_OK);
            },
            [&] { bt.dag_sync_dirty = true; bt.dag_ev_applied = false; });   // (the state slots may not hold this batch's evidence)
        if (rc != BN_OK) return rc;
    }
    bool any_left = false;
    for (int32_t q = 0; q < bt.n_sets; ++q) {
        if (!left[q]) continue;
        any_left = true;
        const DagQuery query{bt.ev_layout.set_view(bt.ev_base, q), bt.d_beliefs + size_t(q) * p.node_off[p.n], false};
        if (int rc = run_dag_query(e, eps, max_sweeps, nullptr, query)) return rc;
        bt.sweeps[q] = e->last_ctl.n_sweeps;
        bt.residual[q] = e->last_ctl.last_res;
        const int32_t cnt = std::min(e->last_ctl.n_sweeps, e->res_cap);
        if (cnt > 0)
            HIPCHK(hipMemcpyAsync(bt.d_res_hist + size_t(q) * e->res_cap, e->d_res_hist, sizeof(double) * cnt, hipMemcpyDeviceToDevice, e->stream));
        launches += e->stats.sweep_launches;
        dev_ms += e->stats.sweep_devclock_ms;
        max_sw = std::max(max_sw, e->last_ctl.n_sweeps);
    }
    if (any_left) HIPCHK(hipStreamSynchronize(e->stream));   // (the copies of the left-over sets' residual histories; the chunks were waited for above)
    bt.predicted_sweeps = max_sw;
    finish_batch(e, 5, launches, 0.f, float(dev_ms), max_sw);
    return BN_OK;
}
