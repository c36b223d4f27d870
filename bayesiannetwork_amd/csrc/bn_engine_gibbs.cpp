// bn_engine_gibbs.cpp -- Gibbs sampling: bn_gibbs_run and bn_gibbs_plan_info over the kernel of bn_gibbs.hip (the contract:
// bn_gibbs.hpp; the planner: bn_gibbs_plan.hpp).  The plan is built at the first call that asks for it -- bn_get_info
// "gibbs_eligible", bn_gibbs_plan_info, a run -- also on engines without a device; tables, the copy of the flat CPTs, the chains'
// states and the histogram are the GibbsState's own and allocated at the first run.  Chains that the caller does not start are
// started by the sampler: lw_run draws the range [chain_begin, chain_begin + n_chains) with the call's seed and evidence and its
// state matrix is transposed into the chains' states, so bn_lw_states after a bn_lw_run of that range shows the very same bytes.
#include "bn_engine_internal.hpp"

namespace {

const char kSharded[] = "Gibbs sampling is not available on sharded engines";
// chains of one pass over the sweeps: their states rest in one device array, and a sampler batch draws their start in one launch
constexpr uint64_t kPassChains = uint64_t(1) << 20;
constexpr uint64_t kPassBytes = uint64_t(1) << 28;

void ensure_plan(bn_engine* e) {
    GibbsState& g = e->gibbs;
    if (g.tried) return;
    g.tried = true;
    const Plan& p = e->plan;
    if (p.nranks > 1) { g.plan = GibbsPlan(); g.plan.why = kSharded; return; }
    try {
        build_gibbs_plan(p.n, p.k.data(), p.in_ptr.data(), p.in_idx.data(), p.cpt_off.data(), g.plan);
    } catch (const std::bad_alloc&) {   // a fact of the plan, not a failure of the engine
        g.plan = GibbsPlan();
        g.plan.why = "out of host memory while building the Gibbs plan";
    }
}

std::string refusal(const bn_engine* e) { return "not eligible for Gibbs sampling: " + e->gibbs.plan.why; }

int64_t sweeps_per_launch(const GibbsState& g) { return g.sweeps_option > 0 ? g.sweeps_option : g.plan.default_sweeps; }

// the tables, once; the CPTs, once per set of them
int ensure_device(bn_engine* e) {
    GibbsState& g = e->gibbs;
    const GibbsPlan& P = g.plan;
    hipStream_t s = e->stream;
    int r;
    if (!g.uploaded) {
        if ((r = upload(g.d_colour_ptr, P.colour_ptr, s))) return r;
        if ((r = upload(g.d_slots, P.slots, s))) return r;
        if ((r = upload(g.d_children, P.children, s))) return r;
        if ((r = upload(g.d_terms, P.terms, s))) return r;
        if ((r = dalloc(g.d_cpt, size_t(e->plan.cpt_off[e->plan.n])))) return r;
        if ((r = dalloc(g.d_clamp, size_t(P.n)))) return r;
        if ((r = dalloc(g.d_words, size_t(P.cells) + 1))) return r;
        HIPCHK(hipStreamSynchronize(s));
        g.uploaded = true;
        g.cpt_ready = false;
    }
    if (!g.cpt_ready) {
        const size_t entries = size_t(e->plan.cpt_off[e->plan.n]);
        if (entries) HIPCHK(hipMemcpyAsync(g.d_cpt, e->plan.cpt_flat.data(), entries * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        g.cpt_ready = true;
    }
    return BN_OK;
}

}  // namespace

extern "C" int bn_gibbs_run(bn_engine* e, int32_t ne, const int32_t* ev_node, const int32_t* ev_state, uint64_t chain_begin, uint64_t n_chains,
                            uint64_t sweep_begin, uint64_t n_sweeps, uint64_t burn_in, uint64_t thin, uint64_t seed, const uint8_t* init_states,
                            uint64_t* counts_out, uint8_t* states_out, uint64_t* stuck_out, uint64_t* kept_out) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (!counts_out) return fail(BN_ERR_ARG, "null counts_out");
    if (ne < 0 || (ne > 0 && (!ev_node || !ev_state))) return fail(BN_ERR_ARG, "bad evidence arguments");
    if (thin == 0) return fail(BN_ERR_ARG, "thin must be at least 1");
    if (sweep_begin > (uint64_t(1) << 32) || n_sweeps > (uint64_t(1) << 32) - sweep_begin)
        return fail(BN_ERR_ARG, "sweep numbers must stay below 2^32 (the uniform's counter holds 32 bits of them)");
    if (chain_begin + n_chains < chain_begin) return fail(BN_ERR_ARG, "chain ids must stay below 2^64");
    const Plan& p = e->plan;
    const size_t n = size_t(p.n);
    std::vector<int16_t> clamp(std::max<size_t>(n, 1), int16_t(-1));
    for (int32_t j = 0; j < ne; ++j) {
        const int32_t v = ev_node[j];
        if (v < 0 || v >= p.n) return fail(BN_ERR_ARG, "evidence node out of range");
        if (ev_state[j] < 0 || ev_state[j] >= p.k[v]) return fail(BN_ERR_ARG, "evidence state out of range");
        if (clamp[size_t(v)] >= 0) return fail(BN_ERR_ARG, "evidence node listed twice");
        clamp[size_t(v)] = int16_t(ev_state[j]);
    }
    if (p.nranks > 1) return fail(BN_ERR_STATE, kSharded);
    ensure_plan(e);
    GibbsState& g = e->gibbs;
    const GibbsPlan& P = g.plan;
    if (!P.ok) return fail(BN_ERR_STATE, refusal(e));
    if (int rc = refuse_unusable(e, BN_ERR_NO_DEVICE)) return rc;
    if (init_states)
        for (uint64_t c = 0; c < n_chains; ++c)
            for (size_t v = 0; v < n; ++v)
                if (clamp[v] < 0 && int32_t(init_states[c * n + v]) >= p.k[v])
                    return fail(BN_ERR_ARG, "init_states: state " + std::to_string(int(init_states[c * n + v])) + " of node " + std::to_string(v) + " in chain " +
                                                std::to_string(c) + " is not below its arity " + std::to_string(p.k[v]));
    const size_t cells = size_t(P.cells);
    std::fill(counts_out, counts_out + cells, uint64_t(0));
    if (stuck_out) *stuck_out = 0;
    if (kept_out) *kept_out = gibbs_kept_sweeps(sweep_begin, n_sweeps, burn_in, thin) * n_chains;
    g.last_launches = 0;
    g.last_kernel_ns = 0;
    if (n == 0 || n_chains == 0) return BN_OK;

    ON_DEVICE(e);
    if (int rc = ensure_device(e)) return rc;
    hipStream_t s = e->stream;
    const uint64_t pass = std::max<uint64_t>(1, std::min<uint64_t>({n_chains, kPassChains, kPassBytes / n}));
    if (pass > g.cap_chains) {
        g.cap_chains = 0;
        if (int rc = dalloc(g.d_states, size_t(pass) * n)) return rc;
        g.cap_chains = pass;
    }
    HIPCHK(hipMemcpyAsync(g.d_clamp, clamp.data(), n * sizeof(int16_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(g.d_words, 0, (cells + 1) * sizeof(unsigned long long), s));
    HIPCHK(hipStreamSynchronize(s));   // (`clamp` is pageable: the copy has read it)
    std::vector<uint8_t> start;
    const int64_t cap = sweeps_per_launch(g);
    const bool timed = e->timing;
    if (timed)
        if (int erc = ensure_events(e, 2)) return erc;
    double kernel_ms = 0.0;
    for (uint64_t first = 0; first < n_chains; first += pass) {
        const uint64_t cnt = std::min(pass, n_chains - first);
        if (init_states) {   // the caller's start, evidence nodes at their clamp
            start.assign(init_states + first * n, init_states + (first + cnt) * n);
            for (uint64_t c = 0; c < cnt; ++c)
                for (size_t v = 0; v < n; ++v)
                    if (clamp[v] >= 0) start[c * n + v] = uint8_t(clamp[v]);
            HIPCHK(hipMemcpyAsync(g.d_states, start.data(), cnt * n, hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
        } else {             // the sampler's draw of the same ids (the weights are not looked at)
            std::string err;
            if (int rc = lw_run(e->lw, p, s, ne, ev_node, ev_state, chain_begin + first, cnt, seed, nullptr, err)) return fail(rc, err);
            if (launch_lw_transpose(e->lw.d_states, g.d_states, p.n, e->lw.stride, e->lw.small, cnt, s))
                return fail(BN_ERR_HIP, "transpose kernel launch failed");
        }
        GibbsArgs a{};
        a.n = P.n; a.cells = P.cells; a.n_colours = P.n_colours; a.state_stride = P.state_stride;
        a.lanes_log2 = __builtin_ctz(unsigned(P.lanes_per_chain));
        a.colour_ptr = g.d_colour_ptr; a.slots = g.d_slots; a.children = g.d_children; a.terms = g.d_terms;
        a.cpt = g.d_cpt; a.clamp = g.d_clamp; a.states = g.d_states;
        a.counts = g.d_words; a.stuck = g.d_words + cells;
        a.chain_begin = chain_begin + first; a.n_chains = cnt;
        a.burn_in = burn_in; a.thin = thin; a.seed = seed;
        int rc = BN_OK;
        if (timed) HIPCHK(hipEventRecord(e->events[0], s));
        // the launches of a pass follow each other on the stream: the states rest in device memory between them
        for (uint64_t done = 0; done < n_sweeps && rc == BN_OK;) {
            const GibbsLaunch L = gibbs_launch_at(sweep_begin, n_sweeps, cap, done);
            a.sweep_begin = L.begin;
            a.n_sweeps = uint32_t(L.count);
            if (int code = launch_gibbs(a, gibbs_blocks(cnt, P.chains_per_block), P.lds_bytes, s))
                rc = fail(BN_ERR_HIP, std::string("gibbs launch failed: ") + hipGetErrorString(hipError_t(code)));
            done += L.count;
            ++g.last_launches;
        }
        if (timed && rc == BN_OK && hipEventRecord(e->events[1], s) != hipSuccess) rc = fail(BN_ERR_HIP, "hipEventRecord failed");
        if (rc == BN_OK && states_out && hipMemcpyAsync(states_out + first * n, g.d_states, cnt * n, hipMemcpyDeviceToHost, s) != hipSuccess)
            rc = fail(BN_ERR_HIP, "copy of the states failed");
        const hipError_t drained = hipStreamSynchronize(s);   // (also after a failed launch: what is on the stream writes into the buffers)
        if (drained != hipSuccess && rc == BN_OK) rc = fail(BN_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(drained));
        if (rc != BN_OK) return rc;
        if (timed) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e->events[0], e->events[1]));
            kernel_ms += double(ms);
        }
    }
    std::vector<unsigned long long> words(cells + 1);
    HIPCHK(hipMemcpyAsync(words.data(), g.d_words, (cells + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::copy(words.begin(), words.begin() + cells, counts_out);
    if (stuck_out) *stuck_out = words[cells];
    g.last_kernel_ns = int64_t(kernel_ms * 1e6);
    return BN_OK;
}

// dims_out[8] = eligible, colours, threads of a workgroup, chains of a workgroup, LDS bytes of a workgroup, sweeps per launch,
// slots of the largest colour, table entries one chain reads per sweep
extern "C" int bn_gibbs_plan_info(bn_engine* e, int32_t* colour_out, int64_t* dims_out) {
    if (!e || !dims_out) return fail(BN_ERR_ARG, "null argument");
    ensure_plan(e);
    const GibbsPlan& P = e->gibbs.plan;
    if (!P.ok) return fail(BN_ERR_STATE, refusal(e));
    const int64_t d[8] = {1, P.n_colours, P.threads, P.chains_per_block, P.lds_bytes, sweeps_per_launch(e->gibbs), P.max_class, P.reads_per_sweep};
    std::copy(d, d + 8, dims_out);
    if (colour_out) std::copy(P.colour.begin(), P.colour.end(), colour_out);
    return BN_OK;
}

// bn_set_option / bn_get_info hand the "gibbs_*" names here (bn_engine.cpp)
int bn_eng::gibbs_set_option(bn_engine* e, const char* name, int32_t value, bool* known) {
    *known = true;
    if (std::strcmp(name, "gibbs_sweeps_per_launch") == 0) {   // 0: the plan's default
        if (value < 0 || value > kGibbsMaxSweepsPerLaunch)
            return fail(BN_ERR_ARG, "gibbs_sweeps_per_launch must be in 0 (the default).." + std::to_string(kGibbsMaxSweepsPerLaunch));
        e->gibbs.sweeps_option = value;
        return BN_OK;
    }
    *known = false;
    return BN_OK;
}

int64_t bn_eng::gibbs_get_info(bn_engine* e, const char* name, bool* known) {
    *known = true;
    GibbsState& g = e->gibbs;
    if (std::strcmp(name, "gibbs_last_launches") == 0) return g.last_launches;
    if (std::strcmp(name, "gibbs_last_kernel_ns") == 0) return g.last_kernel_ns;   // option "timing" 1: events around the launches
    // the facts of the plan: asking builds it
    auto is = [&](const char* what) {
        if (std::strcmp(name, what) != 0) return false;
        ensure_plan(e);
        return true;
    };
    if (is("gibbs_eligible")) return g.plan.ok ? 1 : 0;
    if (is("gibbs_colours")) return g.plan.n_colours;
    if (is("gibbs_lds_bytes")) return g.plan.lds_bytes;
    if (is("gibbs_sweeps_per_launch")) return g.plan.ok ? sweeps_per_launch(g) : 0;
    *known = false;
    return 0;
}

void bn_eng::gibbs_cpt_reloaded(bn_engine* e) { e->gibbs.cpt_ready = false; }
