// bn_engine_mpe.cpp -- most probable explanation: the bn_mpe_* entry points over the max-product kernels (bn_maxprod.hip; the
// algorithm and its rules: bn_maxprod.hpp).  Which form runs a network: bn_policy::mpe_form.  Everything a run needs beyond the item
// tables the engine uploaded for the sum-product paths -- staging block, state, outputs, control records -- is the MpeState's own and
// allocated at the first run: a max-product run reads the engine's tables and touches nothing the bn_bp_* calls use (the evidence in
// force, the batch staging, the state bn_bp_messages reads, last_path all stay as they were).
#include "bn_engine_internal.hpp"

namespace {

// The several-workgroup plan a max-product run uses: the engine's, or -- on a network ONE workgroup holds, for which bn_create builds none --
// a plan of its own, built when option "mpe_form" 2 first asks for it (pure host work: also on engines without a device).
const MidPlan& mid_of(const bn_engine* e) { return e->mid.ok ? e->mid : e->mpe.own_mid; }
void ensure_own_mid(bn_engine* e) {
    MpeState& m = e->mpe;
    if (e->mid.ok || m.form_option != 2 || e->plan.nranks != 1 || m.own_tried) return;
    m.own_tried = true;
    try {
        build_mid_plan(e->plan, m.own_mid);
    } catch (const std::bad_alloc&) {
        m.own_mid = MidPlan();
        m.own_mid.why = "out of host memory while building the plan";
    }
}
// what the path choice reads: the engine's facts, with the own plan in place of a several-workgroup plan the engine does not have
bn_policy::PathFacts facts_of(const bn_engine* e) {
    bn_policy::PathFacts f = e->facts;
    if (!e->mid.ok && e->mpe.own_mid.ok) {
        f.mid.ok = true;
        f.mid.parts = int32_t(e->mpe.own_mid.parts.size());
    }
    return f;
}
int form_of(bn_engine* e) {
    ensure_own_mid(e);
    return bn_policy::mpe_form(facts_of(e), e->n_cus, e->mpe.form_option);
}

// why no form takes the network: the limits of the two plans, in the planners' own words
std::string no_form_text(const bn_engine* e, int forced) {
    const std::string one = e->small.ok ? std::string("eligible") : e->small.why;
    const MidPlan& mp = mid_of(e);
    const std::string several = mp.ok ? (bn_policy::mid_fits(facts_of(e), e->n_cus) ? std::string("eligible") : std::string("more workgroups than 0.9 x the device's CUs"))
                                      : (mp.why.empty() ? e->mid.why : mp.why);
    if (forced == 1) return "option mpe_form = 1, but the network is not eligible for the one-workgroup form: " + one;
    if (forced == 2) return "option mpe_form = 2, but the network is not eligible for the several-workgroup form: " + several;
    return "max-product runs networks of at most " + std::to_string(kSmallMaxParents) + " parents per node that fit one workgroup or at most " +
           std::to_string(kMidMaxParts) + " of them; this one: one workgroup: " + one + "; several workgroups: " + several;
}

// buffers of the first run, and of the first run with more sets / a higher cap than any before
int reserve(bn_engine* e, int form, int32_t n_sets, int32_t res_cap, size_t ev_bytes) {
    MpeState& m = e->mpe;
    const Plan& p = e->plan;
    const size_t N = size_t(p.node_off[p.n]), n = size_t(p.n);
    int r;
    if (!m.d_elem_node) {
        std::vector<int32_t> elem_node(std::max<size_t>(N, 1), 0);
        for (int32_t v = 0; v < p.n; ++v)
            for (int64_t y = p.node_off[v]; y < p.node_off[v + 1]; ++y) elem_node[size_t(y)] = v;
        if ((r = upload(m.d_elem_node, elem_node, e->stream))) return r;
        HIPCHK(hipStreamSynchronize(e->stream));   // (`elem_node` is a local)
    }
    if (form == 1 && !m.small_ready) {
        if (int code = prepare_mpe_small()) return fail(BN_ERR_HIP, std::string("mpe_small attribute: ") + hipGetErrorString(hipError_t(code)));
        m.small_ready = true;
    }
    if (form == 2 && !e->mid.ok && !m.own_uploaded) {   // the tables of the own plan (bn_engine_create.cpp setup_mid has the engine's)
        MidTables t;
        build_mid_tables(m.own_mid, p, t);
        if ((r = upload_items(m.own_img, t, m.own_mid.parts[0], e->stream))) return r;
        HIPCHK(hipStreamSynchronize(e->stream));   // (`t` is a local)
        m.own_uploaded = true;
    }
    if (form == 2 && !m.mid_ready) {
        const SmallPlan& g0 = mid_of(e).parts[0];
        if (int code = prepare_mpe_mid()) return fail(BN_ERR_HIP, std::string("mpe_mid attribute: ") + hipGetErrorString(hipError_t(code)));
        if ((r = dalloc(m.d_m_state, 4 * size_t(g0.M) + 4 * size_t(g0.N)))) return r;
        if ((r = dalloc(m.d_m_frz, size_t(g0.N)))) return r;
        if ((r = dalloc(m.d_m_sync, 1))) return r;
        m.mid_ready = true;
    }
    if (n_sets > m.cap_sets || res_cap > m.res_cap) {
        const size_t B = size_t(std::max(n_sets, m.cap_sets));
        const int32_t rc = std::max(res_cap, m.res_cap);
        m.cap_sets = 0;
        HIPCHK(m.h_mm.alloc(B * N));
        HIPCHK(m.h_states.alloc(B * n));
        if ((r = dalloc(m.d_res_hist, B * size_t(rc)))) return r;
        HIPCHK(m.h_ctl.alloc(B));
        m.small_state_sets = 0;
        m.cap_sets = int32_t(B);
        m.res_cap = rc;
    }
    if (form == 1 && m.small_state_sets < m.cap_sets) {
        if ((r = dalloc(m.d_s_state, size_t(m.cap_sets) * (2 * size_t(e->small.M) + 2 * size_t(e->small.N))))) return r;
        m.small_state_sets = m.cap_sets;
    }
    HIPCHK(m.h_ev.reserve(ev_bytes));
    return BN_OK;
}

// one workgroup per evidence set, the whole run in one launch (more only beyond the kernel's budget of iterations)
int run_small(bn_engine* e, const bn_stage::BatchLayout& lay, int32_t n_sets, double eps, int32_t cap) {
    MpeState& m = e->mpe;
    const SmallPlan& sp = e->small;
    MpeSmallArgs a{};
    a.eps = eps; a.max_sweeps = cap; a.sweep_begin = 0; a.budget = kSmallBudget; a.run_id = m.run_id;
    a.host_ctl = m.h_ctl.dev();
    a.n = sp.n; a.N = sp.N; a.M = sp.M; a.T = sp.T; a.TT = sp.TT; a.CL = sp.CL; a.re = sp.re; a.rb = sp.rb; a.rc = sp.rc;
    put_items(a, e->small_img);
    a.elem_node = m.d_elem_node;
    a.ev_node = reinterpret_cast<const int32_t*>(m.h_ev.dev() + lay.b_node);
    a.ev_off = reinterpret_cast<const int32_t*>(m.h_ev.dev() + lay.b_off);
    a.ev_val = reinterpret_cast<const double*>(m.h_ev.dev() + lay.b_val);
    a.ev_meta = lay.meta(m.h_ev.dev());
    a.max_marginals = m.h_mm.dev(); a.states = m.h_states.dev(); a.res_hist = m.d_res_hist; a.state = m.d_s_state; a.res_cap = m.res_cap;
    // a set that stops leaves done != 0; a launch that ends on its budget continues every set from the smallest sweep count reached --
    // only a cap above kSmallBudget sweeps gets there, and then with a single set (a batch's sets would not stay in step)
    for (;;) {
        if (int code = launch_mpe_small(a, sp.waves, sp.lds_bytes, n_sets, e->stream))
            return fail(BN_ERR_HIP, std::string("mpe_small launch failed: ") + hipGetErrorString(hipError_t(code)));
        HIPCHK(hipStreamSynchronize(e->stream));
        bool all_done = true;
        for (int32_t q = 0; q < n_sets; ++q) {
            if (m.h_ctl[q].run_id != m.run_id) return fail(BN_ERR_HIP, "mpe_small kernel did not report (stale control record)");
            all_done = all_done && m.h_ctl[q].done != 0;
        }
        if (all_done) return BN_OK;
        if (n_sets != 1) return fail(BN_ERR_STATE, "a batched max-product run takes at most " + std::to_string(kSmallBudget) + " sweeps per set");
        a.sweep_begin = m.h_ctl[0].n_sweeps;
    }
}

// one set after the other: initial state, evidence, then groups of sweep launches with a finishing launch behind each; the control
// record is read once per group
int run_mid(bn_engine* e, const bn_stage::BatchLayout& lay, int32_t n_sets, double eps, int32_t cap) {
    MpeState& m = e->mpe;
    const MidPlan& mp = mid_of(e);
    const ItemImage& t = e->mid.ok ? e->mid_img : m.own_img;
    const SmallPlan& g0 = mp.parts[0];
    const size_t M = size_t(g0.M), N = size_t(g0.N);
    MpeMidArgs a{};
    a.eps = eps; a.max_sweeps = cap; a.run_id = m.run_id;
    a.n = g0.n; a.N = g0.N; a.M = g0.M; a.nparts = int32_t(mp.parts.size());
    put_items(a, t);
    a.parts = t.parts; a.elem_node = m.d_elem_node;
    a.pi = m.d_m_state; a.lam = a.pi + 2 * M; a.npi = a.lam + 2 * M; a.nlam = a.npi + 2 * N;
    a.frz = m.d_m_frz; a.sync = m.d_m_sync; a.res_cap = m.res_cap;
    const int32_t group = std::max(1, std::min(m.group, kMpeMaxGroup));
    for (int32_t q = 0; q < n_sets; ++q) {
        const bn_stage::SetView v = lay.set_view(m.h_ev.dev(), q);
        a.host_ctl = m.h_ctl.dev() + q;
        a.ev_ne = v.ne; a.ev_node = v.node; a.ev_off = v.off; a.ev_val = v.val;
        a.max_marginals = m.h_mm.dev() + size_t(q) * N; a.states = m.h_states.dev() + size_t(q) * size_t(g0.n); a.res_hist = m.d_res_hist + size_t(q) * size_t(m.res_cap);
        int code = launch_mpe_mid_init(a, e->stream);
        if (!code) code = launch_mpe_mid_evidence(a, e->stream);
        if (code) return fail(BN_ERR_HIP, std::string("mpe_mid set-up launch failed: ") + hipGetErrorString(hipError_t(code)));
        int32_t launched = 0;
        for (;;) {
            const int32_t g = std::min(group, cap - launched);
            for (int32_t i = 0; i < g && !code; ++i) code = launch_mpe_mid_sweep(a, launched + i, false, mp.waves, mp.rounds, mp.lds_bytes, e->stream);
            launched += g;
            if (!code) code = launch_mpe_mid_sweep(a, launched, true, mp.waves, mp.rounds, mp.lds_bytes, e->stream);
            if (code) return fail(BN_ERR_HIP, std::string("mpe_mid launch failed: ") + hipGetErrorString(hipError_t(code)));
            HIPCHK(hipStreamSynchronize(e->stream));
            ++m.last_groups;
            if (m.h_ctl[q].done != 0) break;
            if (launched >= cap) return fail(BN_ERR_HIP, "mpe_mid kernels did not report the end of a capped run");
        }
        if (m.h_ctl[q].run_id != m.run_id) return fail(BN_ERR_HIP, "mpe_mid kernels did not report (stale control record)");
    }
    return BN_OK;
}

int mpe_run_impl(bn_engine* e, bool single, int32_t n_sets, const int32_t* ne, const int32_t* ev_node, const int32_t* ev_off, const double* ev_val,
                 double eps, int32_t max_sweeps, double* max_marginals_out, int32_t* states_out, int32_t* sweeps_out, double* residual_out,
                 int32_t* converged_out) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (!max_marginals_out) return fail(BN_ERR_ARG, "null max_marginals_out");
    if (!states_out) return fail(BN_ERR_ARG, "null states_out");
    if (n_sets < 1 || n_sets > BN_MAX_BATCH_SETS) return fail(BN_ERR_ARG, "n_sets must be in 1.." + std::to_string(BN_MAX_BATCH_SETS));
    if (!ne) return fail(BN_ERR_ARG, "null ne");
    const Plan& p = e->plan;
    bn_stage::BatchLayout lay;
    if (int rc = check_evidence_sets(e, n_sets, ne, ev_node, ev_off, ev_val, lay)) return rc;
    if (max_sweeps < 0) return fail(BN_ERR_ARG, "max_sweeps < 0");
    if (p.nranks > 1) return fail(BN_ERR_STATE, "max-product is not available on sharded engines");
    MpeState& m = e->mpe;
    const int form = form_of(e);
    if (form == 0) return fail(BN_ERR_STATE, no_form_text(e, m.form_option));
    if (int rc = refuse_unusable(e, BN_ERR_STATE)) return rc;
    if ((form == 1 && !e->small_ok) || (form == 2 && e->mid.ok && !e->mid_ok)) return fail(BN_ERR_STATE, "the item tables of this form were not set up on the device");
    const int32_t cap = max_sweeps == 0 ? kMpeDefaultCap : max_sweeps;   // never unbounded (bn_maxprod.hpp)
    ON_DEVICE(e);
    m.have_run = false;
    if (int rc = reserve(e, form, n_sets, std::min(cap, e->res_cap), lay.bytes)) return rc;
    // (no kernel is in flight when the staging block is rewritten: every entry point here synchronises before it returns)
    lay.fill(m.h_ev, ev_node, ev_off, ev_val);
    ++m.run_id;
    if (m.run_id == 0) m.run_id = 1;
    std::memset(m.h_ctl, 0, size_t(n_sets) * sizeof(MpeCtl));
    m.last_groups = 0;
    if (int rc = form == 1 ? run_small(e, lay, n_sets, eps, cap) : run_mid(e, lay, n_sets, eps, cap)) return rc;
    const size_t N = size_t(p.node_off[p.n]);
    // (the kernels wrote the results into mapped page-locked memory, and the run has synchronised)
    std::memcpy(max_marginals_out, m.h_mm, sizeof(double) * size_t(n_sets) * N);
    std::memcpy(states_out, m.h_states, sizeof(int32_t) * size_t(n_sets) * size_t(p.n));
    m.sweeps.assign(size_t(n_sets), 0);
    unsigned long long ticks = 0;
    for (int32_t q = 0; q < n_sets; ++q) {
        const MpeCtl& c = m.h_ctl[q];
        m.sweeps[size_t(q)] = c.n_sweeps;
        if (sweeps_out) sweeps_out[q] = c.n_sweeps;
        if (residual_out) residual_out[q] = c.last_res;
        if (converged_out) converged_out[q] = c.done == 1 ? 1 : 0;
        if (q == 0 || form == 2) ticks += c.t_last > c.t_first ? c.t_last - c.t_first : 0;   // (one workgroup per set: the sets run side by side)
    }
    m.last_device_ns = int64_t(ticks) * 10;
    m.n_sets = n_sets;
    m.last_single = single;
    m.last_form = form;
    m.have_run = true;
    return BN_OK;
}

}  // namespace

extern "C" int bn_mpe_run(bn_engine* e, int32_t ne, const int32_t* ev_node, const int32_t* ev_off, const double* ev_val, double eps, int32_t max_sweeps,
                          double* max_marginals_out, int32_t* states_out, int32_t* sweeps_out, double* residual_out, int32_t* converged_out) {
    return mpe_run_impl(e, true, 1, &ne, ev_node, ev_off, ev_val, eps, max_sweeps, max_marginals_out, states_out, sweeps_out, residual_out, converged_out);
}

extern "C" int bn_mpe_run_batch(bn_engine* e, int32_t n_sets, const int32_t* ne, const int32_t* ev_node, const int32_t* ev_off, const double* ev_val,
                                double eps, int32_t max_sweeps, double* max_marginals_out, int32_t* states_out, int32_t* sweeps_out,
                                double* residual_out, int32_t* converged_out) {
    return mpe_run_impl(e, false, n_sets, ne, ev_node, ev_off, ev_val, eps, max_sweeps, max_marginals_out, states_out, sweeps_out, residual_out,
                        converged_out);
}

extern "C" int bn_mpe_residual_history(bn_engine* e, int32_t set, double* out, int32_t cap) {
    if (!e || !out || cap < 0) return fail(BN_ERR_ARG, "bad argument");
    if (e->host_only || !e->mpe.have_run) return fail(BN_ERR_STATE, "no max-product run yet");
    const MpeState& m = e->mpe;
    if (set < 0 || set >= m.n_sets) return fail(BN_ERR_ARG, "set index out of range");
    const int32_t cnt = std::min({cap, m.sweeps[size_t(set)], m.res_cap});
    ON_DEVICE(e);
    if (cnt > 0) HIPCHK(hipMemcpy(out, m.d_res_hist + size_t(set) * size_t(m.res_cap), sizeof(double) * cnt, hipMemcpyDeviceToHost));
    return cnt;
}

extern "C" int bn_mpe_messages(bn_engine* e, double* pi_msg_out, double* lambda_msg_out) {
    if (!e || !pi_msg_out || !lambda_msg_out) return fail(BN_ERR_ARG, "null argument");
    if (e->host_only || !e->mpe.have_run || !e->mpe.last_single) return fail(BN_ERR_STATE, "no single max-product run (bn_mpe_run) to read the messages of");
    const MpeState& m = e->mpe;
    ON_DEVICE(e);
    if (m.last_form == 1) {   // the one-workgroup kernel leaves the state it stopped in: pi-messages, lambda-messages, CSR edge order
        const size_t bytes = sizeof(double) * size_t(e->small.M);
        HIPCHK(hipMemcpy(pi_msg_out, m.d_s_state, bytes, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(lambda_msg_out, m.d_s_state + e->small.M, bytes, hipMemcpyDeviceToHost));
        return BN_OK;
    }
    // several workgroups: two buffers, the run stopped in buffer n_sweeps & 1
    const size_t M = size_t(mid_of(e).parts[0].M), par = size_t(m.sweeps[0] & 1);
    HIPCHK(hipMemcpy(pi_msg_out, m.d_m_state + par * M, sizeof(double) * M, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lambda_msg_out, m.d_m_state + 2 * M + par * M, sizeof(double) * M, hipMemcpyDeviceToHost));
    return BN_OK;
}

// bn_set_option / bn_get_info hand the "mpe_*" names here (bn_engine.cpp)
int bn_eng::mpe_set_option(bn_engine* e, const char* name, int32_t value, bool* known) {
    *known = true;
    if (std::strcmp(name, "mpe_form") == 0) {
        if (value < 0 || value > 2) return fail(BN_ERR_ARG, "mpe_form must be 0 (auto), 1 (one workgroup) or 2 (several workgroups)");
        e->mpe.form_option = value;
        return BN_OK;   // (2 on a network without a several-workgroup plan: the plan is built when the form is first asked for)
    }
    if (std::strcmp(name, "mpe_group") == 0) { e->mpe.group = std::max(1, std::min(value, kMpeMaxGroup)); return BN_OK; }
    *known = false;
    return BN_OK;
}
int64_t bn_eng::mpe_get_info(bn_engine* e, const char* name, bool* known) {
    *known = true;
    if (std::strcmp(name, "mpe_form") == 0) return form_of(e);   // the form the next run takes
    if (std::strcmp(name, "mpe_parts") == 0) { ensure_own_mid(e); return mid_of(e).ok ? int64_t(mid_of(e).parts.size()) : 0; }   // workgroups of form 2
    if (std::strcmp(name, "mpe_last_form") == 0) return e->mpe.have_run ? e->mpe.last_form : 0;
    if (std::strcmp(name, "mpe_group") == 0) return e->mpe.group;
    if (std::strcmp(name, "mpe_last_groups") == 0) return e->mpe.last_groups;          // several-workgroup form: reads of the control record
    if (std::strcmp(name, "mpe_last_device_ns") == 0) return e->mpe.last_device_ns;    // device clock, first sweep's start -> the run's end
    *known = false;
    return 0;
}

void bn_eng::mpe_cpt_reloaded(bn_engine* e) {
    MpeState& m = e->mpe;
    m.own_mid = MidPlan();
    m.own_tried = false;
    m.own_uploaded = false;
    DeviceGuard guard;        // (device memory is released on the engine's device; no kernel is in flight: every entry point synchronises)
    if (!e->host_only) (void)guard.enter(e->device);
    m.own_img = ItemImage();
}
