// bn_engine_paths.cpp -- the one-launch execution paths of a single query (resident tiles, one workgroup, several workgroups,
// register-resident DAG): each path's run, what it does when a bounded wait gives up, the table that orders them and the dispatch
// of bn_bp_run_device over it; option "autotune".  Which path WANTS a network: bn_engine_policy.cpp.
#include "bn_engine_internal.hpp"

// blocks the barrier of a resident launch adds to the tile blocks: one, sweeping every tile block's granules
int bn_eng::resident_service_blocks(int tile_blocks) { return tile_blocks > 1 ? 1 : 0; }

namespace {
// What the four runs below share.  A run is a loop of launches (more than one only beyond the kernel's budget of iterations):
//     OneLaunchRun run(e);
//     for (;;) { arguments from run.sweep_begin;  run.begin();  launch;  run.launched();  copy behind the launch;  run.sync();
//                the path's abort handling;  run.after_sync(code, text);  if (run.done) break; }
//     run.finish(path);
// The path keeps what is its own: its arguments, the polled words and their generations, what an abort means, a shard's copy.
struct OneLaunchRun {
    bn_engine* e;
    const bool timed;               // HIP events around each launch (bn_engine::timing) -> bn_bp_stats.sweep_kernel_ms
    int32_t sweep_begin = 0;        // the iteration the next launch continues from
    int32_t launches = 0;
    bool done = false;
    float ms = 0.f;
    double dev_ticks = 0.0;

    explicit OneLaunchRun(bn_engine* e_, bool may_time = true) : e(e_), timed(may_time && e_->timing) { next_run_id(e); }
    int begin() {
        ++launches;
        if (!timed) return BN_OK;
        if (int rc = ensure_events(e, 2)) return rc;
        HIPCHK(hipEventRecord(e->events[0], e->stream));
        return BN_OK;
    }
    int launched() {
        if (timed) HIPCHK(hipEventRecord(e->events[1], e->stream));
        return BN_OK;
    }
    int sync() {
        HIPCHK(hipStreamSynchronize(e->stream));
        e->ev_upload_pending = false;
        return BN_OK;
    }
    // the launch has ended and did not give up: it must have reported under this run's id (else `stale_code`, `stale_text`)
    int after_sync(int stale_code, const char* stale_text) {
        if (e->h_ctl->run_id != e->run_id) return fail(stale_code, stale_text);
        if (timed) {
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, e->events[0], e->events[1]));
            ms += t;
        }
        dev_ticks += double(e->h_ctl->t_last - e->h_ctl->t_first);
        done = e->h_ctl->done != 0;
        if (!done) sweep_begin = e->h_ctl->n_sweeps;
        return BN_OK;
    }
    void finish(int path) {
        const bool rows_were_clean = e->rows_clean;  // these paths never touch the residual slots
        note_run_result(e);
        e->rows_clean = rows_were_clean;
        e->last_path = path;
        e->stats.sweep_launches = launches;
        e->stats.sweep_kernel_ms = ms;
        e->stats.sweep_devclock_ms = float(dev_ticks * 1e-5);
    }
};
}  // namespace

// Networks of register-resident tiles that fit the chip: ONE launch runs the whole run with the CPTs,
// references and node vectors resident in registers / LDS and a grid barrier per sweep (bn_resident.hip).
// BN_ERR_STATE = a bounded wait inside the kernel gave up: the caller redoes the run with per-sweep launches.
// copy_to: host memory the beliefs are copied into BEHIND the launch, before the run's one synchronisation
// (bn_bp_run / bn_bp_run_view); nullptr leaves them in HBM (bn_bp_run_device)
static int run_resident(bn_engine* e, double eps, int32_t max_sweeps, double* copy_to) {
    hipStream_t s = e->stream;
    const bn_policy::ResidentShape& rs = e->shape;
    OneLaunchRun run(e);
    const bool shard = e->plan.nranks > 1;  // (only called with shard_flow_ok then)
    const bool flow = shard || (rs.flow_ok && e->flow != 0);
    // The grid-barrier form starts from the stored first sweep where that is known to be safe (bn_engine_memo.cpp; the choice:
    // bn_policy::memo0_applies): the first launch begins at sweep 1 and reads the image instead of rec1 / node1.  The image is built
    // by the first run that could use it.
    bool memo = false;
    if (!flow && max_sweeps != 1 && memo0_possible(e)) {
        if (int rc = memo0_ensure(e)) return rc;
        memo = bn_policy::memo0_applies({true, e->memo.valid, flow, max_sweeps, eps, e->memo.const_residual});
    }
    // ... and from the stored second sweep where the image holds the set in force and sweep 1 is known not to end the run
    // (bn_policy::memo1_applies): sweep 2 then reads that image instead of rec0 / node0
    int depth = memo ? 1 : 0;
    if (memo && e->res_cap >= 2 && bn_policy::memo1_applies({{true, e->memo.valid, flow, max_sweeps, eps, e->memo.const_residual}, e->memo1.enabled != 0,
                                          e->memo1.built && e->memo1.holds, e->memo1.seed}))
        depth = 2;
    run.sweep_begin = depth;
    while (!run.done) {
        // polled words: generations count on from launch to launch, so they are zeroed only at creation, after an
        // aborted launch and before the 30-bit generation would wrap
        if (shard) {
            // Every rank derives the generations of a launch from the number of runs the engine has been asked for and
            // the launch's place in the run: ranks agree without talking, nothing is ever zeroed while peers may be
            // writing, and a granule left by an earlier (or an aborted) launch can never carry a wanted generation.
            if (run.launches >= 4) return fail(BN_ERR_STATE, "sharded resident run needs more than 4 launches");
            e->flow_gen_base = (((e->shard_run_seq & 0x3ffffu) << 2) + uint32_t(run.launches)) * uint32_t(kResidentBudget + 1);
        } else if (flow) {
            if (e->flow_dirty || e->flow_gen_base > (1u << 29)) {
                HIPCHK(hipMemsetAsync(e->d_flow, 0, flow_sync_bytes(1), s));
                e->flow_dirty = false;
                e->flow_gen_base = 0;
            }
        } else if (e->rsync_dirty || e->gen_base > (1u << 29)) {
            HIPCHK(hipMemsetAsync(e->d_rsync, 0, sizeof(ResidentSync), s));
            e->rsync_dirty = false;
            e->gen_base = 0;
        }
        *e->h_abort = 0;
        const bool from_image = memo && run.launches == 0;   // (as many iterations less: the launches of a long run end where they always did)
        // The kernel knows ONE image form: a launch that begins at sweep 1 and reads the image in the place of rec1 / node1.  A run behind
        // the second-sweep image is that launch with its sweeps numbered one later than the run's: the buffers of the two parities
        // exchanged, the residual history one entry further, the cap one less -- and one added to the count it reports (below).
        const bool shifted = from_image && depth == 2;
        BpBuffers bufs = buffers_of(e);
        if (shifted) {
            std::swap(bufs.rec0, bufs.rec1);
            std::swap(bufs.node0, bufs.node1);
            bufs.res_hist += 1;
            bufs.res_cap -= 1;
        }
        ResidentArgs a{bufs, eps, shifted && max_sweeps > 0 ? max_sweeps - 1 : max_sweeps, shifted ? 1 : run.sweep_begin,
                       from_image ? kResidentBudget - depth : kResidentBudget, e->run_id, flow ? e->flow_gen_base : e->gen_base,
                       // one wait: 50 ms of the 100 MHz clock; shards: 2 s (the ranks' launches start up to a host hiccup apart)
                       shard ? 200000000ull : 5000000ull, e->d_rsync, e->h_ctl.dev(),
                       rs.blocks, rs.waves, 1, 1u, 0, 0, 0, 0, 0, flow ? e->d_flow.get() : nullptr,
                       shard ? e->d_peers.get() : nullptr, shard ? e->d_pub_mask.get() : nullptr, shard ? e->plan.n_interior_tiles : 0,
                       e->d_nbr, e->plan.nbr_chunks, e->poll_sleep, e->h_abort.dev(), (!flow && !shard) ? e->resident_direct : 0, e->resident_poll_margin,
                       !from_image ? nullptr : (depth == 2 ? e->memo1.d_img + (3 * e->memo.word + e->memo1.word) : e->memo.d_img + e->memo.word)};
        if (int rc = run.begin()) return rc;
        if (int code = launch_bp_resident(a, rs.blocks + (shard ? 1 : resident_service_blocks(rs.blocks)), rs.lean, s))
            return fail(BN_ERR_HIP, std::string("bp_resident launch failed: ") + hipGetErrorString(hipError_t(code)));
        if (int rc = run.launched()) return rc;
        // (shards: the copy goes out only once the kernel has ended -- a copy into pageable memory blocks inside the runtime,
        // and where several shard engines live in one process, the thread of a rank whose kernel is still waiting for a
        // peer's would keep that peer's thread from launching)
        if (copy_to && !shard)  // a launch that stops on its budget (1024 sweeps) copies an intermediate state; the last one counts
            HIPCHK(hipMemcpyAsync(copy_to, e->d_beliefs, sizeof(double) * e->plan.node_off[e->plan.n], hipMemcpyDeviceToHost, s));
        if (int rc = run.sync()) return rc;
        if (copy_to && shard) {  // through the engine's page-locked buffer: a plain DMA, nothing that blocks inside the runtime
            const size_t bytes = sizeof(double) * e->plan.node_off[e->plan.n];
            if (copy_to != e->h_beliefs && !e->h_beliefs) {
                HIPCHK(e->h_beliefs.alloc(size_t(e->plan.node_off[e->plan.n])));
            }
            HIPCHK(hipMemcpyAsync(e->h_beliefs, e->d_beliefs, bytes, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (copy_to != e->h_beliefs) std::memcpy(copy_to, e->h_beliefs, bytes);
        }
        if (!shard) (flow ? e->flow_gen_base : e->gen_base) += kResidentBudget + 1;
        const bool gave_up = e->h_ctl->done < 0 || *e->h_abort != 0;  // any block may raise it, whatever block 0 / the service reported
        if (e->h_ctl->run_id != e->run_id || gave_up) (flow ? e->flow_dirty : e->rsync_dirty) = true;
        if (gave_up) {
            char where[96];
            std::snprintf(where, sizeof where, " (code 0x%x: wait kind %u, iteration %u, tile %u; run seq %u)", *e->h_abort, *e->h_abort & 0xffu,
                          (*e->h_abort >> 8) & 0xfffu, (*e->h_abort >> 20) & 0x7ffu, e->shard_run_seq);
            return fail(BN_ERR_STATE, std::string("resident kernel gave up a bounded wait") + where);
        }
        if (shifted && e->h_ctl->run_id == e->run_id) e->h_ctl->n_sweeps += 1;   // (the launch counted from one later)
        if (int rc = run.after_sync(BN_ERR_STATE, "resident kernel did not report (stale control block)")) return rc;
    }
    run.finish(2);
    e->stats.memo_sweeps = memo ? 1 : 0;
    e->stats.memo_depth = depth;
    e->last_flow = flow ? 1 : 0;
    return BN_OK;
}

SmallArgs bn_eng::small_args_of(bn_engine* e, const BpBuffers& b, double eps, int32_t max_sweeps, int32_t begin, Ctl* host_ctl) {
    const SmallPlan& sp = e->small;
    SmallArgs a{};
    a.b = b; a.eps = eps; a.max_sweeps = max_sweeps; a.sweep_begin = begin; a.budget = kSmallBudget; a.run_id = e->run_id;
    a.host_ctl = host_ctl;
    a.n = sp.n; a.N = sp.N; a.M = sp.M; a.S = sp.S; a.T = sp.T; a.TT = sp.TT; a.CL = sp.CL;
    a.re = sp.re; a.rb = sp.rb; a.rc = sp.rc; a.mmax = sp.mmax;
    put_items(a, e->small_img);
    a.nv_idx = e->small_img.nv_idx; a.nv_slot = e->small_img.nv_slot;
    a.state = e->d_s_state; a.sets = SetStrides{}; a.state_stride = 0;
    a.ev_mode = 0; a.ev_ne = 0; a.ev_nval = 0; a.ev_node = nullptr; a.ev_off = nullptr; a.ev_val = nullptr; a.ev_meta = nullptr;
    return a;
}

// Small networks: ONE workgroup runs every iteration with the state in LDS and writes the beliefs (bn_small.hip).
static int run_small(bn_engine* e, double eps, int32_t max_sweeps, double* copy_to) {
    hipStream_t s = e->stream;
    OneLaunchRun run(e);
    while (!run.done) {
        SmallArgs a = small_args_of(e, buffers_of(e), eps, max_sweeps, run.sweep_begin, e->h_ctl.dev());
        if (e->ev_deferred) {  // the evidence in force was never written to the tile buffers: the kernel reads the staging block
            a.ev_mode = 1; a.ev_ne = e->ev_ne; a.ev_nval = e->ev_nval; a.ev_node = e->d_ev_node; a.ev_off = e->d_ev_off; a.ev_val = e->d_ev_val;
        }
        if (int rc = run.begin()) return rc;
        if (int code = launch_bp_small(a, e->small.waves, e->small.lds_bytes, 1, s))
            return fail(BN_ERR_HIP, std::string("bp_small launch failed: ") + hipGetErrorString(hipError_t(code)));
        if (int rc = run.launched()) return rc;
        if (copy_to)  // a launch that stops on its budget copies an intermediate state; the last one counts
            HIPCHK(hipMemcpyAsync(copy_to, e->d_beliefs, sizeof(double) * e->plan.node_off[e->plan.n], hipMemcpyDeviceToHost, s));
        if (int rc = run.sync()) return rc;
        if (int rc = run.after_sync(BN_ERR_HIP, "bp_small kernel did not report (stale control block)")) return rc;
    }
    run.finish(3);
    return BN_OK;
}

// Networks spread over several workgroups (bn_mid.hip).  The arguments of a launch over the sets [set_base, set_base + n)
// of a batch (single query: set 0 of one) working in state slots [0, n).
MidArgs bn_eng::mid_args_of(bn_engine* e, const BpBuffers& b0, const SetStrides& st, Ctl* h_ctl_dev, double eps, int32_t max_sweeps,
                           int32_t begin, int32_t set_base, int32_t slot_base) {
    const SmallPlan& g0 = e->mid.parts[0];
    MidArgs a{};
    a.b = b0; a.eps = eps; a.max_sweeps = max_sweeps; a.sweep_begin = begin; a.budget = kSmallBudget; a.run_id = e->run_id;
    a.host_ctl = h_ctl_dev;
    a.n = g0.n; a.N = g0.N; a.M = g0.M; a.nparts = int32_t(e->mid.parts.size());
    put_items(a, e->mid_img);
    a.parts = e->mid_img.parts; a.nv_idx = e->mid_img.nv_idx; a.nv_slot = e->mid_img.nv_slot; a.msg_first = e->mid_img.msg_first;
    a.ev_mode = 0; a.ev_ne = 0; a.ev_node = nullptr; a.ev_off = nullptr; a.ev_val = nullptr; a.ev_meta = nullptr;
    a.state_stride = 4 * int64_t(g0.M) + 4 * int64_t(g0.N);
    a.pi = e->d_m_state; a.lam = a.pi + 2 * size_t(g0.M); a.npi = a.lam + 2 * size_t(g0.M); a.nlam = a.npi + 2 * size_t(g0.N);
    a.frz = e->d_m_frz;
    a.bar = reinterpret_cast<unsigned*>(e->d_m_sync.get());
    a.res = reinterpret_cast<unsigned long long*>(e->d_m_sync + 8);
    a.abort = e->h_abort.dev();
    a.timeout_ticks = 5000000ull;  // one wait: 50 ms of the 100 MHz clock
    // first poll of the grid barrier placed by the previous barrier's lag (arrival times in the granules, as bn_dag.hip / bn_resident.hip do):
    // BN_MID_DELAY = margin in 10 ns ticks, -1 (default) = poll from the own arrival on.  mixed10k, us per sweep: 8.30 off, 8.17 at 0,
    // 8.80 at 30, 9.08 at 60 (round 6; round 5 measured 8.5 / 8.7 / 9.1): the polling wave has nothing else to do and polls back to
    // back, so a poll placed by prediction can only be later -- at margin 0 it is within the run-to-run spread, with any margin slower
    static const int mid_first_delay = std::getenv("BN_MID_DELAY") ? std::atoi(std::getenv("BN_MID_DELAY")) : -1;
    a.first_poll_delay = mid_first_delay;
    a.sets = st; a.set_base = set_base; a.slot_base = slot_base;
    return a;
}
// launch + wait; BN_ERR_STATE: a grid wait gave up (the caller redoes the work on the tile kernels)
// wait = false: enqueue only (the chunks of a batch, bn_engine_batch.cpp: the caller clears the abort word before the first, waits once
// behind the last and looks at the abort word then)
int bn_eng::mid_launch(bn_engine* e, const MidArgs& a, int32_t n_sets, const double* copy_from, double* copy_to, bool wait) {
    hipStream_t s = e->stream;
    if (wait) *e->h_abort = 0;
    HIPCHK(hipMemsetAsync(e->d_m_sync + size_t(a.slot_base) * kMidSyncBytes, 0, size_t(n_sets) * kMidSyncBytes, s));
    if (int code = launch_bp_mid(a, e->mid.waves, e->mid.rounds, e->mid.lds_bytes, n_sets, s))
        return fail(BN_ERR_HIP, std::string("bp_mid launch failed: ") + hipGetErrorString(hipError_t(code)));
    if (copy_to) HIPCHK(hipMemcpyAsync(copy_to, copy_from, sizeof(double) * e->plan.node_off[e->plan.n], hipMemcpyDeviceToHost, s));
    if (!wait) return BN_OK;
    HIPCHK(hipStreamSynchronize(s));
    e->ev_upload_pending = false;
    if (*e->h_abort != 0) {
        *e->h_abort = 0;
        return fail(BN_ERR_STATE, "a workgroup of the mid-size kernel gave up its grid wait");
    }
    return BN_OK;
}
// one query: one launch for the whole run (more only beyond 65 536 iterations)
static int run_mid(bn_engine* e, double eps, int32_t max_sweeps, double* copy_to) {
    OneLaunchRun run(e, false);   // (no events around this path's launches: sweep_kernel_ms reads 0)
    const BpBuffers b = buffers_of(e);
    while (!run.done) {
        MidArgs a = mid_args_of(e, b, SetStrides{}, e->h_ctl.dev(), eps, max_sweeps, run.sweep_begin, 0, 0);
        if (e->ev_deferred) {  // the evidence in force was never written to the tile buffers: the kernel reads the staging block
            a.ev_mode = 1; a.ev_ne = e->ev_ne; a.ev_node = e->d_ev_node; a.ev_off = e->d_ev_off; a.ev_val = e->d_ev_val;
        }
        if (int rc = run.begin()) return rc;
        if (int rc = mid_launch(e, a, 1, b.beliefs, copy_to)) return rc;   // (launch, copy behind it, wait)
        if (e->h_ctl->done < 0) return fail(BN_ERR_STATE, "a workgroup of the mid-size kernel gave up its grid wait");
        if (int rc = run.after_sync(BN_ERR_HIP, "bp_mid kernel did not report (stale control block)")) return rc;
    }
    run.finish(4);
    return BN_OK;
}

// The evidence in force (staging block) -> the state arrays of the DAG path: marks of this set's own value, vectors in both buffers.
static int flush_dag_evidence(bn_engine* e, const DagQuery& q) {
    if (int rc = ensure_dag(e)) return rc;
    if (q.own && e->dag_ev_applied) return BN_OK;
    e->dag_ev_applied = false;
    if (e->dag_mark == 255) {  // the mark values are used up: start over
        HIPCHK(hipMemsetAsync(e->dag_img.frz, 0, size_t(e->dag.n), e->stream));
        e->dag_mark = 0;
    }
    ++e->dag_mark;
    DagEvidenceArgs ea{q.ev.ne, e->dag.n, e->dag.E, q.ev.node, q.ev.off, q.ev.val, e->dag_img.state, e->dag_img.frz, e->dag_mark, e->dag_img.k, e->dag_img.nperm};
    if (int code = launch_dag_evidence(ea, e->stream))
        return fail(BN_ERR_HIP, std::string("dag_evidence launch failed: ") + hipGetErrorString(hipError_t(code)));
    e->dag_ev_applied = q.own;
    e->ev_upload_pending = q.ev.ne > 0;
    return BN_OK;
}

// One launch runs the whole query (more only beyond kDagBudget iterations).  BN_ERR_STATE: a grid wait gave up.
int bn_eng::run_dag(bn_engine* e, double eps, int32_t max_sweeps, double* copy_to) {
    return run_dag_query(e, eps, max_sweeps, copy_to, DagQuery{{e->ev_ne, e->d_ev_node, e->d_ev_off, e->d_ev_val}, nullptr, true});
}
int bn_eng::run_dag_query(bn_engine* e, double eps, int32_t max_sweeps, double* copy_to, const DagQuery& q) {
    hipStream_t s = e->stream;
    if (int rc = ensure_dag(e)) return rc;   // (first use of the path on this engine: full plan, device tables, upload)
    const DagPlan& dp = e->dag;
    if (int rc = flush_dag_evidence(e, q)) return rc;
    OneLaunchRun run(e);
    BpBuffers b = buffers_of(e);
    if (q.beliefs) b.beliefs = q.beliefs;
    if (!dp.uniform4) {   // arities below 4: the run's initial state stands in memory (zeros in the padding), bn_dag_plan.cpp
        DagInitArgs ia{dp.n, dp.E, e->dag_img.inptr, e->dag_img.inidx, e->dag_img.k, e->dag_img.init, e->dag_img.state, e->dag_img.frz, e->dag_mark, e->dag_img.eperm, e->dag_img.nperm};
        if (int code = launch_dag_init(ia, s))
            return fail(BN_ERR_HIP, std::string("dag_init launch failed: ") + hipGetErrorString(hipError_t(code)));
    }
    while (!run.done) {
        // polled words: generations count on from launch to launch; zeroed at creation, after an abort and before they would wrap
        if (e->dag_sync_dirty || e->dag_gen_base > (1u << 29)) {
            HIPCHK(hipMemsetAsync(e->dag_img.sync, 0, sizeof(ResidentSync), s));
            if (e->dag_img.flow) HIPCHK(hipMemsetAsync(e->dag_img.flow, 0, dag_flow_sync_bytes(dp.tiles.size()), s));
            e->dag_sync_dirty = false;
            e->dag_gen_base = 0;
        }
        *e->h_abort = 0;
        DagArgs a{};
        // the dataflow form where the plan allows it ("dagflow" 1; a run that gave up a wait stays on the barrier for a while)
        const bool flow = e->dag_flow_ok && e->dag_flow != 0 && !dp.stream && dp.blocks > 1 && e->dag_flow_pause == 0;
        if (flow) {
            static const int flow_sleep = std::getenv("BN_DAG_FLOW_SLEEP") ? std::atoi(std::getenv("BN_DAG_FLOW_SLEEP")) : 4;   // x 512 cycles between polls; configs[1], us per executed iteration: 6.59 / 6.38 / 6.14 / 6.06 / 6.00 at 0 / 1 / 2 / 4 / 8
            a.flow = e->dag_img.flow; a.nbr = e->dag_img.nbr; a.n_tiles = int32_t(dp.tiles.size()); a.flow_sleep = flow_sleep;
        }
        e->last_dag_flow = flow ? 1 : 0;
        a.b = b; a.eps = eps; a.max_sweeps = max_sweeps; a.sweep_begin = run.sweep_begin; a.budget = kDagBudget; a.run_id = e->run_id;
        a.gen_base = e->dag_gen_base;
        a.timeout_ticks = 5000000ull;  // one wait: 50 ms of the 100 MHz clock
        a.sync = e->dag_img.sync; a.host_ctl = e->h_ctl.dev(); a.host_abort = e->h_abort.dev();
        a.n = dp.n; a.E = dp.E; a.n_blocks = dp.blocks;
        a.tiles = e->dag_img.tiles; a.slot_ptr = e->dag_img.slotptr; a.cnode = e->dag_img.cnode; a.pitem = e->dag_img.pitem; a.oedge = e->dag_img.oedge;
        a.cpt_img = e->dag_img.cpt; a.npi_init = e->dag_img.init; a.state = e->dag_img.state; a.frz = e->dag_img.frz; a.frz_mark = e->dag_mark;
        static const int poll_sleep = std::getenv("BN_DAG_SLEEP") ? std::atoi(std::getenv("BN_DAG_SLEEP")) : 1;
        a.poll_sleep = poll_sleep;
        static const int first_delay = std::getenv("BN_DAG_DELAY") ? std::atoi(std::getenv("BN_DAG_DELAY")) : 30;   // 10 ns ticks: measured flat from 20 to 60 (config 2: 6.9 us per sweep at 0, 6.5-6.6 there)
        a.first_poll_delay = first_delay;
        a.n_sets = 1; a.set_mask = 1u;
        a.state_init = dp.uniform4 ? 0 : 1; a.node_k = e->dag_img.k; a.node_off = e->dag_img.noff;
        if (int rc = run.begin()) return rc;
        if (int code = launch_bp_dag(a, dp.stream, s))
            return fail(BN_ERR_HIP, std::string("bp_dag launch failed: ") + hipGetErrorString(hipError_t(code)));
        if (int rc = run.launched()) return rc;
        if (copy_to)  // a launch that stops on its budget copies an intermediate state; the last one counts
            HIPCHK(hipMemcpyAsync(copy_to, e->d_beliefs, sizeof(double) * e->plan.node_off[e->plan.n], hipMemcpyDeviceToHost, s));
        if (int rc = run.sync()) return rc;
        e->dag_gen_base += kDagBudget + 1;
        const bool gave_up = e->h_ctl->done < 0 || *e->h_abort != 0;
        if (e->h_ctl->run_id != e->run_id || gave_up) e->dag_sync_dirty = true;
        if (gave_up) {
            *e->h_abort = 0;
            if (flow) e->dag_flow_pause = 64;   // (the barrier form next time the path is tried)
            return fail(BN_ERR_STATE, "a block of the register-resident DAG kernel gave up its grid wait");
        }
        if (int rc = run.after_sync(BN_ERR_HIP, "bp_dag kernel did not report (stale control block)")) return rc;
        if (!flow && e->dag_flow_pause > 0) --e->dag_flow_pause;
    }
    run.finish(5);
    return BN_OK;
}

// A one-launch path gave up a bounded wait: its workgroups were not all on the chip together -- another engine, stream or process
// holds compute units.  The run is repeated on a slower path and the result is the same, but the caller should know why its
// queries got slower: ONE line per engine on stderr (not gated by BN_DEBUG); the counters keep counting
// (bn_bp_stats.resident_aborts, bn_get_info "mid_aborts" / "dag_aborts").
void bn_eng::report_abort_once(bn_engine* e, const char* what, int pause_runs) {
    if (e->abort_reported && !std::getenv("BN_DEBUG")) return;
    e->abort_reported = true;
    std::fprintf(stderr,
                 "[bn_mi355x] %s gave up a bounded wait (%s): its workgroups were not all resident -- does another engine, stream or "
                 "process use this GPU?  This run and the next %d take a slower path (same results); further such events are counted, "
                 "not printed (bn_bp_stats.resident_aborts, bn_get_info \"mid_aborts\" / \"dag_aborts\").\n",
                 what, g_err.c_str(), pause_runs);
}

// Option "autotune": time every execution path this engine is eligible for ONCE, on the evidence in force, and keep the fastest
// for all later runs (the built-in choice between them rests on thresholds measured on a handful of networks on one pool of
// machines).  A trial is one run capped at 6 sweeps, evidence staged, host wall clock, best of two after one warm-up.  The
// choice is expressed through the engine's own options ("multisweep", "small", "mid", "dag"), so bn_set_option can still
// override it.  Paths whose >= 3-parent arithmetic differs in the last bits (bn_mi355x.h) may be exchanged by this.
static int autotune_paths(bn_engine* e, double eps) {
    struct Cand { int path, multisweep, small, mid, dag; bool ok; };
    const Cand cands[] = {
        {0, 0, 0, 0, 0, true},                               // one launch per sweep
        {2, 2, 0, 0, 0, e->shape.resident_ok},               // resident tiles
        {3, 1, 2, 0, 0, e->small_ok},                        // one workgroup, state in LDS
        {4, 1, 0, 2, 0, e->mid_ok},                          // the same items over several workgroups
        {5, 1, 0, 0, 2, e->dag_ok},                          // register-resident child tiles + parent items
    };
    const int keep[4] = {e->multisweep, e->small_mode, e->mid_mode, e->dag_mode};
    const bool keep_timing = e->timing;
    e->timing = false;
    // A trial executes every sweep it is timed for: the resident path's stored sweeps (options "memo0", "memo1") are one or two
    // sweeps of any run, but a third of a 6-sweep trial -- with them the resident tiles won trials they lose as whole queries
    // (128 x 128 grid: 132 us per query against the DAG path's 118).  The images stay as they are and are used again afterwards.
    struct ImagesOff {
        bn_engine* e;
        int keep0, keep1;
        explicit ImagesOff(bn_engine* e_) : e(e_), keep0(e_->memo.enabled), keep1(e_->memo1.enabled) { e->memo.enabled = 0; e->memo1.enabled = 0; }
        ~ImagesOff() { e->memo.enabled = keep0; e->memo1.enabled = keep1; }
    } images_off(e);
    double best = 1e300;
    int best_i = -1;
    for (int i = 0; i < 5; ++i) {
        if (!cands[i].ok) continue;
        e->multisweep = cands[i].multisweep; e->small_mode = cands[i].small; e->mid_mode = cands[i].mid; e->dag_mode = cands[i].dag;
        double t_best = 1e300;
        bool took = true;
        for (int rep = 0; rep < 3 && took; ++rep) {
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = run_device_impl(e, eps, 6, nullptr, nullptr, nullptr);
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (rc != BN_OK) { e->multisweep = keep[0]; e->small_mode = keep[1]; e->mid_mode = keep[2]; e->dag_mode = keep[3]; e->timing = keep_timing; return rc; }
            took = e->last_path == cands[i].path;        // (a path in its pause after an abort, or refused by a policy: not a candidate now)
            if (rep > 0 && took) t_best = std::min(t_best, dt);
        }
        if (took && t_best < best) { best = t_best; best_i = i; }
    }
    e->timing = keep_timing;
    if (best_i < 0) { e->multisweep = keep[0]; e->small_mode = keep[1]; e->mid_mode = keep[2]; e->dag_mode = keep[3]; return BN_OK; }
    e->multisweep = cands[best_i].multisweep; e->small_mode = cands[best_i].small; e->mid_mode = cands[best_i].mid; e->dag_mode = cands[best_i].dag;
    e->autotuned_path = cands[best_i].path;
    if (std::getenv("BN_DEBUG")) std::fprintf(stderr, "[bn_mi355x] autotune: path %d (%.1f us per 6-sweep run)\n", e->autotuned_path, best * 1e6);
    return BN_OK;
}

// ---- which path wants the network: the engine's facts, shape and options handed to the pure choice (bn_engine_policy.cpp has the
// rules and the measurements behind them)
bool bn_eng::mid_applies(const bn_engine* e) { return bn_policy::mid_applies(e->facts, e->shape, oks_of(e), modes_of(e)); }
bool bn_eng::dag_applies(const bn_engine* e) { return bn_policy::dag_applies(e->facts, e->shape, oks_of(e), modes_of(e)); }
static bool resident_wanted(const bn_engine* e) { return bn_policy::resident_wanted(e->facts, e->shape, oks_of(e), modes_of(e)); }
static bool small_wanted(const bn_engine* e) { return bn_policy::small_wanted(e->facts, e->shape, oks_of(e), modes_of(e)); }
static bool dag_first_wanted(const bn_engine* e) { return bn_policy::dag_first_wanted(e->facts, e->shape, oks_of(e), modes_of(e)); }
static bool dag_later_wanted(const bn_engine* e) { return bn_policy::dag_later_wanted(e->facts, e->shape, oks_of(e), modes_of(e)); }

int bn_eng::resident_gave_up(bn_engine* e, const char* what) {
    ++e->resident_aborts;
    if (e->plan.nranks > 1) {
        // Sharded engines: NO unilateral fall-back inside the library.  A peer whose service block had already published the
        // final verdict may have returned BN_OK: it would never enter the RCCL all-gather this rank would now wait in, and
        // peers may still be storing into this rank's exchange region.  The caller's control plane decides for ALL ranks
        // (multigpu.run_collective: all-reduce of the outcome, then "multisweep" 0 everywhere, or a collective retry);
        // nothing of the engine's state has been touched.
        const std::string why = g_err;
        return fail(BN_ERR_STATE, "the in-kernel exchange gave up a bounded wait on this rank (" + why + "): every rank must switch together -- "
                                  "set \"multisweep\" 0 on ALL ranks (RCCL exchange) or retry collectively");
    }
    // this run and the next few go down the per-sweep launches (8, 16, ... 1 024 runs), then the path is tried again
    e->resident_cooldown = e->resident_backoff;
    e->resident_backoff = std::min(e->resident_backoff * 2, 1024);
    report_abort_once(e, what, e->resident_cooldown);
    return BN_OK;
}
void bn_eng::resident_ran_ok(bn_engine* e) { e->resident_backoff = 8; }

int bn_eng::small_gave_up(bn_engine*, const char*) { return BN_OK; }   // (one workgroup: it waits for nobody)
int bn_eng::dag_gave_up(bn_engine* e, const char* what) {
    ++e->dag_aborts;
    e->dag_cooldown = 64;   // something else holds CUs: the other paths for a while
    report_abort_once(e, what, 64);
    return BN_OK;
}
int bn_eng::mid_gave_up(bn_engine* e, const char* what) {
    ++e->mid_aborts;
    e->mid_cooldown = 64;
    report_abort_once(e, what, 64);
    return BN_OK;
}

static const char kDagName[] = "the register-resident DAG kernel (bn_dag.hip)";
static const PathDriver kOneLaunchPaths[] = {
    {5, dag_first_wanted, run_dag, dag_gave_up, kDagName, nullptr, &bn_engine::dag_cooldown, false},
    {3, small_wanted, run_small, small_gave_up, "", nullptr, &bn_engine::small_cooldown, false},
    {5, dag_later_wanted, run_dag, dag_gave_up, kDagName, nullptr, &bn_engine::dag_cooldown, false},   // (its place by default: behind the one-workgroup path)
    {4, mid_applies, run_mid, mid_gave_up, "the several-workgroup item kernel (bn_mid.hip)", nullptr, &bn_engine::mid_cooldown, false},
    {2, resident_wanted, run_resident, resident_gave_up, "the resident-tile kernel (bn_resident.hip)", resident_ran_ok, &bn_engine::resident_cooldown, true},
};

int bn_eng::run_device_impl(bn_engine* e, double eps, int32_t max_sweeps, int32_t* sweeps_out, double* residual_out, double* copy_to) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (e->autotune_pending && !e->host_only && e->plan.nranks == 1) {
        e->autotune_pending = false;
        double* const keep_override = e->beliefs_override;
        e->beliefs_override = nullptr;          // (trial runs write into the engine's own buffer)
        const int rc = autotune_paths(e, eps);
        e->beliefs_override = keep_override;
        if (rc != BN_OK) return rc;
    }
    e->beliefs_on_host_only = false;  // (bn_bp_run_view sets it again when its kernels wrote to the host buffer)
    if (int rc = refuse_unusable(e, BN_ERR_STATE)) return rc;
    if (max_sweeps < 0) return fail(BN_ERR_ARG, "max_sweeps < 0");
    if (e->plan.nranks > 1 && !e->comm && !(e->shard_flow_ok && e->multisweep != 0))
        return fail(BN_ERR_COMM, "sharded engine: call bn_comm_init (RCCL exchange) or bn_peer_import (in-kernel exchange) before running");
    const auto t_begin = std::chrono::steady_clock::now();
    ON_DEVICE(e);
    int rc;
    if (e->plan.nranks > 1) ++e->shard_run_seq;
    // The one-launch paths, in the order of kOneLaunchPaths: the first one that wants the network (eligible, and chosen by the
    // options / the measured defaults) and is not paused runs the query; one that gives up a bounded wait pauses itself and
    // hands the query to the next; what none of them takes runs with one launch per sweep (below).
    bool evidence_flushed = false;
    for (const PathDriver& d : kOneLaunchPaths) {
        if (!d.wanted(e)) continue;
        if (d.reads_tile_evidence && !evidence_flushed) {   // the tile kernels read the evidence from their own buffers
            if ((rc = flush_evidence(e))) return rc;
            evidence_flushed = true;
        }
        int32_t& cooldown = e->*(d.cooldown);
        if (cooldown > 0) { --cooldown; continue; }   // paused after a launch that gave up
        rc = d.run(e, eps, max_sweeps, copy_to);
        if (rc == BN_OK) {
            if (d.ran_ok) d.ran_ok(e);
            e->stats.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
            if (sweeps_out) *sweeps_out = e->last_ctl.n_sweeps;
            if (residual_out) *residual_out = e->last_ctl.last_res;
            return BN_OK;
        }
        if (rc != BN_ERR_STATE) return rc;
        if ((rc = d.gave_up(e, d.what)) != BN_OK) return rc;   // counters, pause, one line on stderr (a shard: an error, see resident_gave_up)
    }
    if (!evidence_flushed && (rc = flush_evidence(e))) return rc;
    e->last_path = 0;
    if (e->plan.nranks > 1 && !e->comm)
        return fail(BN_ERR_COMM, "the in-kernel exchange gave up and no RCCL communicator is set up to fall back on (bn_comm_init)");
    if ((rc = run_per_sweep(e, eps, max_sweeps, copy_to))) return rc;
    e->stats.total_ms =
        std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (sweeps_out) *sweeps_out = e->last_ctl.n_sweeps;
    if (residual_out) *residual_out = e->last_ctl.last_res;
    return BN_OK;
}
