// bn_engine_create.cpp -- bn_create / bn_create_sharded / bn_destroy: the host plans, then the device side one step per path (tile
// images, resident tiles, one workgroup, several workgroups, DAG); the facts the path choice reads (path_facts_of); the pool of parked
// streams; the lazily built parts (mid_reserve_slots, ensure_dag).  bn_engine_internal.hpp has the map of the engine's files.
#include "bn_engine_internal.hpp"

#include <mutex>

// Streams of destroyed engines, kept for the next bn_create on the same device: creating a non-blocking stream costs 1.5-4 ms on an
// MI355X box (scripts/experiments/create_split.py) -- most of what constructing a functor on an ALARM-sized network takes once the
// runtime is up.  A parked stream is idle (free_engine synchronises it first); at most eight per process.
namespace {
struct ParkedStream { int device; hipStream_t stream; };
std::mutex g_stream_mu;
std::vector<ParkedStream> g_parked_streams;
hipStream_t take_parked_stream(int device) {
    std::lock_guard<std::mutex> lock(g_stream_mu);
    for (size_t i = 0; i < g_parked_streams.size(); ++i)
        if (g_parked_streams[i].device == device) {
            hipStream_t s = g_parked_streams[i].stream;
            g_parked_streams.erase(g_parked_streams.begin() + i);
            return s;
        }
    return nullptr;
}
// The FIRST device engine of a process on a device also parks a few spare streams: with another engine's stream alive, creating one more
// costs 5-11 ms (scripts/experiments/create_split_alive.py) -- nearly all of a functor's construction on an ALARM-sized network --
// while that first bn_create spends 80-240 ms bringing the runtime up anyway.
constexpr int kSpareStreams = 3;
std::vector<int> g_primed_devices;
void prime_spare_streams(int device) {
    {
        std::lock_guard<std::mutex> lock(g_stream_mu);
        for (int d : g_primed_devices)
            if (d == device) return;
        g_primed_devices.push_back(device);
    }
    if (std::getenv("BN_NO_SPARE_STREAMS")) return;
    for (int i = 0; i < kSpareStreams; ++i) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return; }
        std::lock_guard<std::mutex> lock(g_stream_mu);
        g_parked_streams.push_back(ParkedStream{device, s});
    }
}
void park_stream(int device, hipStream_t s) {
    if (hipStreamSynchronize(s) == hipSuccess) {
        std::lock_guard<std::mutex> lock(g_stream_mu);
        if (g_parked_streams.size() < 8) { g_parked_streams.push_back(ParkedStream{device, s}); return; }
    }
    (void)hipStreamDestroy(s);
}
}  // namespace

void bn_eng::free_engine(bn_engine* e) {
    if (!e) return;
    if (e->dense) { free_engine(e->dense); e->dense = nullptr; }
    if (e->host_only) { delete e; return; }
    DeviceGuard guard;   // (the buffers' owners free on the current device: `delete e` stays inside the guard)
    (void)guard.enter(e->device);
    e->lw = LwState();
    for (void* q : e->ipc_opened) (void)hipIpcCloseMemHandle(q);
    if (e->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(e->comm);
    if (e->ev_swept) (void)hipEventDestroy(e->ev_swept);
    if (e->ev_gathered) (void)hipEventDestroy(e->ev_gathered);
    if (e->comm_stream) (void)hipStreamDestroy(e->comm_stream);
    for (hipEvent_t ev : e->events) (void)hipEventDestroy(ev);
    const int device = e->device;
    hipStream_t stream = e->stream;
    delete e;   // device and page-locked memory
    if (stream) park_stream(device, stream);
}

static void debug_segv_handler(int sig) {
    void* frames[64];
    int n = backtrace(frames, 64);
    const char msg[] = "[bn_mi355x] fatal signal, native backtrace:\n";
    (void)!write(2, msg, sizeof msg - 1);
    backtrace_symbols_fd(frames, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
// bn_engine_policy.hpp restates these without including a device header: they must not drift apart
static_assert(bn_policy::kResidentWaves == kResidentWaves && bn_policy::kResidentMaxBlocks == kResidentMaxBlocks &&
              bn_policy::kFlowMaxTiles == kFlowMaxTiles && bn_policy::kMaxRanks == kMaxRanks &&
              bn_policy::kResidentMaxSets == kResidentMaxSets && bn_policy::kDagMaxSets == kDagMaxSets,
              "bn_engine_policy.hpp: a constant differs from bn_device.hpp / bn_dag.hpp");

// What the path choice reads of the plans (bn_engine_policy.hpp).  Filled at bn_create and again wherever a plan it summarises is
// rebuilt: the DAG plan for another block cap or in full (ensure_dag), the several-workgroup plan refused for the device's CU count,
// bn_reload_cpt.
static bn_policy::PathFacts::Dag dag_facts_of(const DagPlan& dag) {
    bn_policy::PathFacts::Dag d;
    d.ok = dag.ok; d.uniform4 = dag.uniform4; d.has_groups = dag.has_groups; d.fill = dag.fill; d.stream = dag.stream; d.blocks = dag.blocks;
    return d;
}
bn_policy::PathFacts bn_eng::path_facts_of(const Plan& p, const SmallPlan& small, const MidPlan& mid, const DagPlan& dag) {
    bn_policy::PathFacts f;
    f.nranks = p.nranks;
    f.latency_rules_applied = p.latency_rules_applied;
    f.n_tiles = int64_t(p.tiles.size());
    f.all_uniform = p.tiles.empty() || p.variants == (1 << kVariantUniform);
    f.tile_kv = p.tiles.empty() ? 0 : int(p.tiles[0].kv);
    for (const TileDesc& td : p.tiles) {
        f.all_uniform = f.all_uniform && td.variant == kVariantUniform;
        f.tile_cmax = std::max(f.tile_cmax, int32_t(td.cmax));
        f.tile_m = std::max(f.tile_m, int32_t(td.m));
        f.any_in_ref = f.any_in_ref || td.in_ref_base >= 0;
        f.any_cmax_gt2 = f.any_cmax_gt2 || td.cmax > 2;
        if (int(td.kv) != f.tile_kv) f.tile_kv = 0;
    }
    f.rec_total_doubles = p.rec_total_doubles;
    f.nbr_empty = p.nbr.empty();
    for (int32_t k : p.k) f.kmax = std::max(f.kmax, k);
    f.small.ok = small.ok; f.small.n = small.n; f.small.re = small.re; f.small.rb = small.rb; f.small.rc = small.rc; f.small.mmax = small.mmax;
    f.mid.ok = mid.ok; f.mid.parts = int32_t(mid.parts.size()); f.mid.est_total = mid.est_total;
    for (const SmallPlan& sp : mid.parts) f.mid.mmax = std::max(f.mid.mmax, sp.mmax);
    f.dag = dag_facts_of(dag);
    return f;
}

// state slots of the mid-size kernel (bn_mid.hip): per slot the four double-buffered state arrays, the marks, the barrier words
int bn_eng::mid_reserve_slots(bn_engine* e, int32_t slots) {
    if (slots <= e->mid_slots) return BN_OK;
    const SmallPlan& g0 = e->mid.parts[0];
    if (e->stream) HIPCHK(hipStreamSynchronize(e->stream));
    e->d_m_state.reset(); e->d_m_frz.reset(); e->d_m_sync.reset(); e->mid_slots = 0;
    int r;
    if ((r = dalloc(e->d_m_state, size_t(slots) * size_t(4 * g0.M + 4 * g0.N)))) return r;
    if ((r = dalloc(e->d_m_frz, size_t(slots) * size_t(g0.N)))) return r;
    HIPCHK(dev_malloc(e->d_m_sync, size_t(slots) * kMidSyncBytes));
    e->mid_slots = slots;
    return BN_OK;
}

// The register-resident DAG path's full plan (padded CPT image), its device tables and their upload -- at the first use of the path.
// bn_create builds the LIGHT plan only (tile tables + the features dag_applies reads): on the 316 x 316 grid, where the resident tiles
// are the default, the image alone is 51 MB and 140 ms of host work nobody asked for (missing #5).
int bn_eng::ensure_dag(bn_engine* e) {
    if (!e->dag.ok) return fail(BN_ERR_STATE, "not eligible for the register-resident DAG path: " + (e->dag.why.empty() ? std::string("disabled") : e->dag.why));
    // Everything is built into locals and moved into the engine once the last fallible step has returned: a failure leaves the
    // light plan (or the full plan with its own tables), no image and dag_ready false, and a later call starts over.
    // (Declared before `img`: on a failure the image's frees wait for the device before the copies' sources go.)
    DagPlan full;
    DagDeviceTables tables;
    const bool build = e->dag.light;
    if (build) {
        try {
            build_dag_plan(e->plan, e->dag_cap, full, false);
            if (!full.ok || full.tiles.size() != e->dag.tiles.size() || full.blocks != e->dag.blocks || full.slot_ptr != e->dag.slot_ptr)
                return fail(BN_ERR_STATE, "the register-resident DAG plan changed between its light and its full build");
            build_dag_device_tables(full, tables);
        } catch (const std::bad_alloc&) {
            return fail(BN_ERR_ALLOC, "out of host memory while building the register-resident DAG plan");
        }
        if (e->host_only) {
            e->dag = std::move(full);
            e->dag_tables = std::move(tables);
            e->facts.dag = dag_facts_of(e->dag);
        }
    }
    if (e->host_only || e->dag_ready) return BN_OK;
    ON_DEVICE(e);
    const Plan& p = e->plan;
    const DagPlan& dp = build ? full : e->dag;
    const DagDeviceTables& dt = build ? tables : e->dag_tables;
    DagImage img;
    int r2;
    if ((r2 = upload(img.slotptr, dp.slot_ptr, e->stream))) return r2;
    if ((r2 = upload(img.tiles, dt.tiles, e->stream))) return r2;
    if ((r2 = upload(img.cnode, dp.cnode, e->stream))) return r2;
    if ((r2 = upload(img.pitem, dt.pitem, e->stream))) return r2;
    if ((r2 = upload(img.oedge, dt.oedge, e->stream))) return r2;
    if ((r2 = upload(img.eperm, dt.eperm, e->stream))) return r2;
    if ((r2 = upload(img.nperm, dt.nperm, e->stream))) return r2;
    if ((r2 = upload(img.cpt, dp.cpt_img, e->stream))) return r2;
    if ((r2 = upload(img.init, dp.npi_init, e->stream))) return r2;
    if (!dp.uniform4) {
        if ((r2 = upload(img.k, p.k, e->stream))) return r2;
        if ((r2 = upload(img.inptr, p.in_ptr, e->stream))) return r2;
        if ((r2 = upload(img.inidx, p.in_idx, e->stream))) return r2;
        if ((r2 = upload(img.noff, p.node_off, e->stream))) return r2;
    }
    const size_t sd = size_t(dag_state_doubles(dp.E, dp.n));
    if ((r2 = dalloc(img.state, sd))) return r2;
    HIPCHK(hipMemsetAsync(img.state, 0, std::max<size_t>(sd, 1) * 8, e->stream));
    if ((r2 = dalloc(img.frz, size_t(dp.n)))) return r2;
    HIPCHK(hipMemsetAsync(img.frz, 0, size_t(dp.n), e->stream));
    HIPCHK(dev_malloc(img.sync, sizeof(ResidentSync)));
    // the dataflow form of a single query (bn_dag.hip): neighbour tiles, granule table + verdict words
    DagFlowTables ft;
    try { build_dag_flow_tables(dp, p, ft); } catch (const std::bad_alloc&) { ft = DagFlowTables(); }
    const bool flow_ok = ft.ok && int64_t(dp.blocks) + 1 <= int64_t(e->n_cus);   // (+ the service block: every block co-resident)
    if (flow_ok) {
        if ((r2 = upload(img.nbr, ft.nbr, e->stream))) return r2;
        HIPCHK(dev_malloc(img.flow, dag_flow_sync_bytes(dp.tiles.size())));
    }
    HIPCHK(hipStreamSynchronize(e->stream));   // (`ft`, and `full` / `tables` until they are moved, are locals)
    if (build) {
        e->dag = std::move(full);
        e->dag_tables = std::move(tables);
        e->facts.dag = dag_facts_of(e->dag);
    }
    e->dag_img = std::move(img);
    e->dag_flow_ok = flow_ok;
    e->dag_flow_max_nbr = ft.max_nbr;
    e->dag_sync_dirty = true;
    e->dag_ev_applied = false;
    e->dag_ready = true;
    return BN_OK;
}

constexpr int32_t kDagDefaultCap = 224;  // 0.9 x 256 CUs, a multiple of 8 (rebuilt in setup_dag when the device has another count)

namespace {
// bn_get_info "create_us_*": where the construction of this engine went
struct PhaseClock {
    bn_engine* e;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(int which) {
        const auto now = std::chrono::steady_clock::now();
        e->create_us[which] += std::chrono::duration_cast<std::chrono::microseconds>(now - t).count();
        t = now;
    }
};
// BN_CREATE_TIMING: where the device side of bn_create goes, one line per step on stderr
struct DevLap {
    const bool on = std::getenv("BN_CREATE_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[bn_create] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t0).count());
        t0 = now;
    }
};
}  // namespace

// The host side of bn_create: the tile layout and the plans of the one-launch paths (no device needed: BN_DEVICE_HOST_ONLY stops here).
static int build_host_plans(bn_engine* e, const bn_model_desc* desc, const ShardSpec& shard, PhaseClock& clock) {
    std::string err;
    try {
        err = build_plan(*desc, shard, e->plan);
    } catch (const std::bad_alloc&) {
        return fail(BN_ERR_ALLOC, "out of host memory while building the layout plan");
    }
    if (!err.empty()) return fail(BN_ERR_ARG, err);
    const Plan& p = e->plan;
    clock.lap(0);
    e->grid_tiles = std::max(1, (int(p.tiles.size()) + kWavesPerBlock - 1) / kWavesPerBlock);
    // one wave past the tiles does the residual bookkeeping -> at least one spare wave
    e->stats.algorithmic_bytes_per_sweep = p.algorithmic_bytes;
    e->stats.layout_bytes_per_sweep = p.layout_bytes;
    e->stats.messages_per_sweep = p.messages_per_sweep;
    if (p.nranks == 1 && !std::getenv("BN_NO_SMALL")) {  // one-workgroup path for small networks (bn_small.hpp)
        try {
            build_small_plan(p, e->small);
        } catch (const std::bad_alloc&) {
            return fail(BN_ERR_ALLOC, "out of host memory while building the small-network plan");
        }
    }
    clock.lap(1);
    if (p.nranks == 1 && !e->small.ok && !std::getenv("BN_NO_MID")) {  // ... spread over several workgroups (bn_mid.hip)
        try {
            build_mid_plan(p, e->mid);
        } catch (const std::bad_alloc&) {
            return fail(BN_ERR_ALLOC, "out of host memory while building the mid-size plan");
        }
    }
    clock.lap(2);
    if (p.nranks == 1 && !std::getenv("BN_NO_DAG")) {  // k = 4, <= 5 parents: register-resident child tiles + parent items (bn_dag.hpp)
        try {
            // LIGHT: the tile tables and the features the default-path policy reads (dag_applies) -- not the padded CPT image, not the
            // device tables: those come with the first use of the path (ensure_dag), at once in create_device where it is the default
            build_dag_plan(p, kDagDefaultCap, e->dag, true);
            e->dag_cap = kDagDefaultCap;
        } catch (const std::bad_alloc&) {   // the other paths can still run the network
            e->dag = DagPlan();
            e->dag.why = "out of host memory while building the plan";
        }
    }
    e->facts = path_facts_of(p, e->small, e->mid, e->dag);
    clock.lap(3);
    return BN_OK;
}

// The tile kernels' tables and image, the state buffers and the control block every path reports through.
static int setup_tile_images(bn_engine* e, DevLap& dev_lap) {
    const Plan& p = e->plan;
    int r;
    if ((r = upload(e->d_tiles, p.tiles, e->stream))) return r;
    if ((r = upload(e->d_classes, p.classes, e->stream))) return r;
    if ((r = upload(e->d_flat_tab, p.flat_tab, e->stream))) return r;
    if ((r = upload(e->d_cpt, p.cpt_striped, e->stream))) return r;
    if ((r = upload(e->d_out, p.out_refs, e->stream))) return r;
    if ((r = upload(e->d_inrefs, p.in_refs, e->stream))) return r;
    if ((r = upload(e->d_slot_node, p.slot_node, e->stream))) return r;
    if ((r = upload(e->d_slot_boff, p.slot_boff, e->stream))) return r;
    if ((r = upload(e->d_node_tile, p.node_tile, e->stream))) return r;
    if ((r = upload(e->d_node_nl, p.node_nl, e->stream))) return r;
    dev_lap("tile tables + image upload");
    // shards: peers store cut-edge halves straight into these buffers from inside their kernels -> fine-grained
    // (system-coherent) allocations; BN_SHARD_COARSE=1 keeps plain hipMalloc (A/B on one device)
    e->fine_grained = p.nranks > 1 && !std::getenv("BN_SHARD_COARSE");
    for (int i = 0; i < 2; ++i) {
        if (e->fine_grained) {
            HIPCHK(dev_malloc_fine(e->d_rec[i], std::max<size_t>(p.rec_total_doubles, 1) * 8));
        } else if ((r = dalloc(e->d_rec[i], size_t(p.rec_total_doubles)))) return r;
        if ((r = dalloc(e->d_node[i], size_t(p.node_doubles)))) return r;
        HIPCHK(hipMemsetAsync(e->d_rec[i], 0, std::max<size_t>(p.rec_total_doubles, 1) * 8, e->stream));
        HIPCHK(hipMemsetAsync(e->d_node[i], 0, std::max<size_t>(p.node_doubles, 1) * 8, e->stream));
    }
    if ((r = dalloc(e->d_frozen, size_t(p.n_slots)))) return r;
    HIPCHK(hipMemsetAsync(e->d_frozen, 0, std::max<size_t>(p.n_slots, 1), e->stream));
    // store policy: working sets beyond the Infinity Cache stream their outputs non-temporally
    e->nontemporal = 8 * (p.cpt_doubles + 2 * p.rec_doubles + 2 * p.node_doubles) > (int64_t(192) << 20);
    if ((r = dalloc(e->d_res_hist, size_t(e->res_cap)))) return r;
    if ((r = dalloc(e->d_ctl, 1))) return r;
    HIPCHK(hipMemsetAsync(e->d_ctl, 0, sizeof(Ctl), e->stream));  // done_run = 0: no run is marked done
    if ((r = dalloc(e->d_beliefs, size_t(p.node_off[p.n])))) return r;
    HIPCHK(hipMemsetAsync(e->d_beliefs, 0, std::max<size_t>(p.node_off[p.n], 1) * 8, e->stream));
    dev_lap("state buffers");
    HIPCHK(e->h_ctl.alloc(1));
    std::memset(e->h_ctl, 0, sizeof(Ctl));
    dev_lap("h_ctl (mapped host)");
    return BN_OK;
}

// The resident path's launch shape for this device (bn_engine_policy.cpp plan_resident), its polled words, the abort word every
// one-launch path shares, and a sharded engine's staging and exchange words.
static int setup_resident(bn_engine* e, DevLap& dev_lap) {
    const Plan& p = e->plan;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, e->device));
    dev_lap("hipGetDeviceProperties");
    e->n_cus = prop.multiProcessorCount;
    const char* w = std::getenv("BN_RESIDENT_WAVES");
    e->shape = bn_policy::plan_resident(e->facts, e->n_cus, w ? std::atoi(w) : 0);
    if (e->shape.resident_ok) HIPCHK(dev_malloc(e->d_rsync, sizeof(ResidentSync)));
    HIPCHK(e->h_abort.alloc(64 / sizeof(unsigned)));
    std::memset(e->h_abort, 0, 64);
    if (e->shape.flow_ok) {
        HIPCHK(dev_malloc(e->d_flow, flow_sync_bytes(1)));
        int r2;
        if ((r2 = upload(e->d_nbr, p.nbr, e->stream))) return r2;
    }
    if (p.nranks > 1) {
        // shards allocate their page-locked staging now: no allocation call may fall between two ranks' launches of a run
        // (several shard engines in one process: such calls can wait for the whole device)
        HIPCHK(e->h_ev.alloc(((size_t(p.n) * 4 + size_t(p.n + 1) * 4 + 7) & ~size_t(7)) + size_t(p.node_off[p.n]) * 8 + 64));
        HIPCHK(e->h_beliefs.alloc(size_t(p.node_off[p.n])));
    }
    if (e->shape.shard_shapes_ok) {  // zeroed HERE, once: peers write into it from their kernels whenever they run
        if (e->fine_grained)
            HIPCHK(dev_malloc_fine(e->d_flow, flow_sync_bytes(p.nranks)));
        else
            HIPCHK(dev_malloc(e->d_flow, flow_sync_bytes(p.nranks)));
        HIPCHK(hipMemsetAsync(e->d_flow, 0, flow_sync_bytes(p.nranks), e->stream));
    }
    if (const char* f = std::getenv("BN_RESIDENT_FLOW")) e->flow = std::atoi(f) != 0;
    if (const char* f = std::getenv("BN_RESIDENT_DIRECT")) e->resident_direct = std::atoi(f) != 0;
    if (const char* f = std::getenv("BN_MEMO0")) e->memo.enabled = std::atoi(f) != 0;
    if (const char* f = std::getenv("BN_MEMO1")) e->memo1.enabled = std::atoi(f) != 0;
    if (const char* f = std::getenv("BN_MEMO1_ONESHOT")) e->memo1.oneshot = std::atoi(f) != 0;
    if (const char* f = std::getenv("BN_MEMO1_LIMIT")) e->memo1.limit = std::max<int64_t>(0, std::atoll(f));
    if (const char* f = std::getenv("BN_RESIDENT_DELAY")) e->resident_poll_margin = std::max(-1, std::min(std::atoi(f), 1000));
    if (const char* z = std::getenv("BN_POLL_SLEEP")) e->poll_sleep = std::max(0, std::min(std::atoi(z), 64));
    dev_lap("resident setup");
    return BN_OK;
}

static int setup_small(bn_engine* e, DevLap& dev_lap) {
    if (e->small.ok) {
        const SmallPlan& sp = e->small;
        int r2;
        if ((r2 = upload_items(e->small_img, sp, e->stream))) return r2;
        if ((r2 = dalloc(e->d_s_state, size_t(2 * sp.M + 2 * sp.N)))) return r2;
        if (int code = prepare_bp_small())
            return fail(BN_ERR_HIP, std::string("bp_small attribute: ") + hipGetErrorString(hipError_t(code)));
        e->small_ok = true;
    }
    dev_lap("small path");
    return BN_OK;
}

static int setup_mid(bn_engine* e, DevLap& dev_lap) {
    if (e->mid.ok && !bn_policy::mid_fits(e->facts, e->n_cus)) {
        e->mid.ok = false;  // the workgroups of a run wait for each other: one per CU, with room to spare
        e->mid.why = "more workgroups than 0.9 x the device's CUs";
        e->facts = path_facts_of(e->plan, e->small, e->mid, e->dag);
    }
    if (e->mid.ok) {
        MidTables t;   // (a local: mid_reserve_slots waits for the stream before it goes)
        build_mid_tables(e->mid, e->plan, t);
        int r2;
        if ((r2 = upload_items(e->mid_img, t, e->mid.parts[0], e->stream))) return r2;   // (the first part carries the tables over all nodes)
        if ((r2 = mid_reserve_slots(e, 1))) return r2;
        if (int code = prepare_bp_mid())
            return fail(BN_ERR_HIP, std::string("bp_mid attribute: ") + hipGetErrorString(hipError_t(code)));
        if (const char* mm = std::getenv("BN_MID")) e->mid_mode = std::atoi(mm) != 0;
        e->mid_ok = true;
    }
    dev_lap("mid path");
    return BN_OK;
}

// The light DAG plan for this device's block cap; image and tables come with ensure_dag.
static int setup_dag(bn_engine* e) {
    if (e->dag.ok) {
        int32_t cap = bn_policy::dag_cap(e->n_cus);
        if (const char* c = std::getenv("BN_DAG_CAP")) cap = std::max(8, std::min(cap, std::atoi(c) & ~7));   // experiments: fewer blocks
        if (cap != kDagDefaultCap) {
            try {
                build_dag_plan(e->plan, cap, e->dag, true);
                e->dag_cap = cap;
            } catch (const std::bad_alloc&) {
                e->dag = DagPlan();
                e->dag.why = "out of host memory while building the plan";
            }
            e->facts.dag = dag_facts_of(e->dag);
        }
    }
    if (e->dag.ok) {
        if (const char* dm = std::getenv("BN_DAG")) e->dag_mode = std::max(0, std::min(2, std::atoi(dm)));
        if (const char* df = std::getenv("BN_DAG_FLOW")) e->dag_flow = std::atoi(df) != 0;
        e->dag_ok = true;   // eligible on this device; image and tables: ensure_dag
    }
    return BN_OK;
}

// The device side of bn_create, one step per path.
static int create_device(bn_engine* e, int device_wanted, int ndev, DeviceGuard& guard, PhaseClock& clock) {
    DevLap dev_lap;
    if (device_wanted >= 0) {
        if (device_wanted >= ndev) return fail(BN_ERR_ARG, "device ordinal out of range");
        e->device = device_wanted;
    } else {
        HIPCHK(hipGetDevice(&e->device));
    }
    HIPCHK(guard.enter(e->device));
    dev_lap("device + guard");
    e->stream = take_parked_stream(e->device);
    if (!e->stream) HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    dev_lap("stream");
    if (e->plan.nranks > 1) {
        HIPCHK(hipStreamCreateWithFlags(&e->comm_stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&e->ev_swept, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&e->ev_gathered, hipEventDisableTiming));
        if (const char* o = std::getenv("BN_OVERLAP")) e->overlap = std::atoi(o) != 0;
    }
    int r;
    if ((r = setup_tile_images(e, dev_lap))) return r;
    if ((r = setup_resident(e, dev_lap))) return r;
    if ((r = setup_small(e, dev_lap))) return r;
    if ((r = setup_mid(e, dev_lap))) return r;
    if ((r = setup_dag(e))) return r;
    if (const char* m = std::getenv("BN_MULTISWEEP")) e->multisweep = std::max(0, std::min(2, std::atoi(m)));
    clock.lap(4);
    // the register-resident DAG path where the defaults pick it: built and uploaded now (a functor's first query pays nothing);
    // everywhere else with the first run that wants it ("dag" 2, "autotune", a batch)
    if (dag_applies(e) && !std::getenv("BN_LAZY_ALL")) {
        if ((r = ensure_dag(e))) return r;
    }
    clock.lap(3);
    dev_lap("dag path");
    HIPCHK(hipStreamSynchronize(e->stream));
    dev_lap("final synchronise");
    if (e->plan.nranks == 1) prime_spare_streams(e->device);   // (first engine of the process on this device only)
    dev_lap("spare streams");
    BigVec().swap(e->plan.cpt_striped);  // the image now lives in HBM
    clock.lap(4);
    return BN_OK;
}

static int create_impl(const bn_model_desc* desc, const ShardSpec& shard, bn_engine** out) {
    if (!desc || !out) return fail(BN_ERR_ARG, "null argument");
    if (std::getenv("BN_DEBUG")) signal(SIGSEGV, debug_segv_handler);
    *out = nullptr;
    bn_engine* e = new (std::nothrow) bn_engine();
    if (!e) return fail(BN_ERR_ALLOC, "out of host memory");
    if (const char* t = std::getenv("BN_TIMING")) e->timing = std::atoi(t) != 0;  // default off, see bn_engine::timing
    PhaseClock clock{e};
    if (int rc = build_host_plans(e, desc, shard, clock)) {
        delete e;
        return rc;
    }
    if (desc->device == BN_DEVICE_HOST_ONLY) {
        *out = e;
        return BN_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        delete e;
        return fail(BN_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    }
    e->host_only = false;
    DeviceGuard guard;
    const int rc = create_device(e, desc->device, ndev, guard, clock);
    if (rc != BN_OK) {
        std::string keep = g_err;
        free_engine(e);
        g_err = keep;
        return rc;
    }
    *out = e;
    return BN_OK;
}

extern "C" int bn_create(const bn_model_desc* desc, bn_engine** out) { return create_impl(desc, ShardSpec(), out); }

extern "C" int bn_create_sharded(const bn_model_desc* desc, int32_t rank, int32_t nranks, const int32_t* owner,
                                 bn_engine** out) {
    ShardSpec sh;
    sh.rank = rank;
    sh.nranks = nranks;
    sh.owner = owner;
    return create_impl(desc, sh, out);
}

extern "C" void bn_destroy(bn_engine* eng) { free_engine(eng); }
