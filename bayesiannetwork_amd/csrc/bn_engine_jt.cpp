// bn_engine_jt.cpp -- exact inference: the bn_jt_* entry points (marginals: bn_jt_run*; exact MPE: bn_jt_mpe_run*) over the
// junction-tree kernels (bn_jt.hip; the rules of the arithmetic: bn_jt.hpp; the planner: bn_jt_plan.hpp).  The plan is built at
// the first call that asks for it -- bn_get_info "jt_eligible", bn_jt_plan_dims / _dump, a run -- also on engines without a
// device; tables, base potentials, scratch and outputs are the JtState's own and allocated at the first run: a junction-tree run
// reads the engine's model and touches nothing the bn_bp_* / bn_mpe_* / bn_em_* calls use.
#include <cmath>

#include "bn_engine_internal.hpp"

namespace {

const char kSharded[] = "junction-tree propagation is not available on sharded engines";

void ensure_plan(bn_engine* e) {
    JtState& j = e->jt;
    if (j.tried) return;
    j.tried = true;
    const Plan& p = e->plan;
    if (p.nranks > 1) { j.plan = JtPlan(); j.plan.why = kSharded; return; }
    try {
        build_jt_plan(p.n, p.k.data(), p.in_ptr.data(), p.in_idx.data(), p.cpt_off.data(), j.scratch_cells, j.plan);
    } catch (const std::bad_alloc&) {   // a fact of the plan, not a failure of the engine
        j.plan = JtPlan();
        j.plan.why = "out of host memory while building the junction tree";
    }
}

std::string refusal(const bn_engine* e) { return "not eligible for junction-tree propagation: " + e->jt.plan.why; }

// the item tables, once
int ensure_tables(bn_engine* e) {
    JtState& j = e->jt;
    const JtPlan& P = j.plan;
    hipStream_t s = e->stream;
    int r;
    if (!j.uploaded) {
        if ((r = upload(j.d_cliques, P.cliques, s))) return r;
        if ((r = upload(j.d_levels, P.levels, s))) return r;
        if ((r = upload(j.d_nodes, P.nodes, s))) return r;
        if ((r = upload(j.d_ent_clique, P.ent_clique, s))) return r;
        if ((r = upload(j.d_dn_map, P.dn_map, s))) return r;
        if ((r = upload(j.d_sep_clique, P.sep_clique, s))) return r;
        if ((r = upload(j.d_c_base, P.c_base, s))) return r;
        if ((r = upload(j.d_p_base, P.p_base, s))) return r;
        if ((r = upload(j.d_c_res, P.c_res, s))) return r;
        if ((r = upload(j.d_p_res, P.p_res, s))) return r;
        if ((r = upload(j.d_up_map, P.up_map, s))) return r;
        if ((r = upload(j.d_home_nodes, P.home_nodes, s))) return r;
        if ((r = upload(j.d_elem_node, P.elem_node, s))) return r;
        if ((r = upload(j.d_asg_ptr, P.asg_ptr, s))) return r;
        if ((r = upload(j.d_asg, P.asg, s))) return r;
        if ((r = upload(j.d_fam, P.fam, s))) return r;
        if ((r = dalloc(j.d_psi0, size_t(P.pot_cells)))) return r;
        if ((r = dalloc(j.d_cpt, size_t(e->plan.cpt_off[e->plan.n])))) return r;
        HIPCHK(hipStreamSynchronize(s));
        j.uploaded = true;
        j.psi_ready = false;
    }
    return BN_OK;
}

// ... and the base potentials, once per set of CPTs
int ensure_device(bn_engine* e) {
    JtState& j = e->jt;
    const JtPlan& P = j.plan;
    hipStream_t s = e->stream;
    if (int r = ensure_tables(e)) return r;
    if (!j.psi_ready) {
        const size_t entries = size_t(e->plan.cpt_off[e->plan.n]);
        if (entries) HIPCHK(hipMemcpyAsync(j.d_cpt, e->plan.cpt_flat.data(), entries * sizeof(double), hipMemcpyHostToDevice, s));
        const JtBaseArgs b{int32_t(P.pot_cells), j.d_cliques, j.d_ent_clique, j.d_asg_ptr, j.d_asg, j.d_fam, j.d_cpt, j.d_psi0};
        if (int code = launch_jt_base(b, s)) return fail(BN_ERR_HIP, std::string("jt_base launch failed: ") + hipGetErrorString(hipError_t(code)));
        HIPCHK(hipStreamSynchronize(s));   // (the copy read the plan's host array)
        j.psi_ready = true;
    }
    return BN_OK;
}

// a sum run (kJtSum: beliefs, log P(e)) or a max run (kJtMax: max-marginals, the decoded states, log max_x P(x, e)): the same
// checks, buffers and launches, the kernel apart
int jt_run_impl(bn_engine* e, int kind, int32_t n_sets, const int32_t* ne, const int32_t* ev_node, const int32_t* ev_off, const double* ev_val,
                double* beliefs_out, int32_t* states_out, double* log_evidence_out) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (!beliefs_out) return fail(BN_ERR_ARG, kind == kJtMax ? "null max_marginals_out" : "null beliefs_out");
    if (kind == kJtMax && !states_out) return fail(BN_ERR_ARG, "null states_out");
    if (n_sets < 1 || n_sets > BN_JT_MAX_BATCH_SETS) return fail(BN_ERR_ARG, "n_sets must be in 1.." + std::to_string(BN_JT_MAX_BATCH_SETS));
    if (!ne) return fail(BN_ERR_ARG, "null ne");
    bn_stage::BatchLayout lay;
    if (int rc = check_evidence_sets(e, n_sets, ne, ev_node, ev_off, ev_val, lay)) return rc;
    int form = 0;
    if (int rc = jt_check_plan(e)) return rc;
    if (int rc = jt_check_form(e, &form)) return rc;
    JtState& j = e->jt;
    const JtPlan& P = j.plan;
    ON_DEVICE(e);
    j.have_run = false;
    if (int rc = ensure_device(e)) return rc;
    const size_t N = size_t(P.N), nc = size_t(P.nc), n = size_t(P.n);
    const int32_t per_launch = form == 1 ? n_sets : int32_t(std::min<int64_t>(n_sets, std::max<int64_t>(1, j.scratch_cells / P.state_cells)));
    int r;
    if (form == 2 && per_launch > j.scratch_slots) {
        j.scratch_slots = 0;
        if ((r = dalloc(j.d_scratch, size_t(per_launch) * size_t(P.state_cells)))) return r;
        j.scratch_slots = per_launch;
    }
    if (per_launch > j.ev_slots) {
        j.ev_slots = 0;
        if ((r = dalloc(j.d_ev_slot, size_t(per_launch) * size_t(P.n)))) return r;
        j.ev_slots = per_launch;
    }
    if (n_sets > j.cap_sets) {
        j.cap_sets = 0;
        if ((r = dalloc(j.d_beliefs, size_t(n_sets) * N))) return r;
        if ((r = dalloc(j.d_scales, size_t(n_sets) * nc))) return r;
        if ((r = dalloc(j.d_states, size_t(n_sets) * n))) return r;
        j.cap_sets = n_sets;
    }
    HIPCHK(j.h_ev.reserve(lay.bytes));
    // (no kernel is in flight when the staging block is rewritten: every entry point here synchronises before it returns)
    lay.fill(j.h_ev, ev_node, ev_off, ev_val);
    JtArgs a{};
    a.t = jt_tables_of(j, j.d_psi0);
    a.ev_node = reinterpret_cast<const int32_t*>(j.h_ev.dev() + lay.b_node);
    a.ev_off = reinterpret_cast<const int32_t*>(j.h_ev.dev() + lay.b_off);
    a.ev_val = reinterpret_cast<const double*>(j.h_ev.dev() + lay.b_val);
    a.ev_meta = lay.meta(j.h_ev.dev());
    a.ev_slot = j.d_ev_slot; a.scratch = j.d_scratch; a.beliefs = j.d_beliefs; a.scales = j.d_scales;
    a.states = j.d_states;
    // the launches of a batch follow each other on the stream (they share the scratch slots) and the host waits once for all of them
    hipStream_t s = e->stream;
    if (e->timing) {   // option "timing": HIP events around the launches (bn_get_info "jt_last_kernel_ns")
        if (int erc = ensure_events(e, 2)) return erc;
        HIPCHK(hipEventRecord(e->events[0], s));
    }
    int rc = BN_OK;
    int32_t launches = 0;
    for (int32_t first = 0; first < n_sets && rc == BN_OK; first += per_launch, ++launches) {
        a.set_base = first;
        if (int code = launch_jt(a, form, kind, std::min(per_launch, n_sets - first), s))
            rc = fail(BN_ERR_HIP, std::string("jt launch failed: ") + hipGetErrorString(hipError_t(code)));
    }
    if (e->timing && rc == BN_OK && hipEventRecord(e->events[1], s) != hipSuccess) rc = fail(BN_ERR_HIP, "hipEventRecord failed");
    j.scales.resize(size_t(n_sets) * nc);
    if (rc == BN_OK && hipMemcpyAsync(beliefs_out, j.d_beliefs, sizeof(double) * size_t(n_sets) * N, hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(BN_ERR_HIP, "copy of the beliefs failed");
    if (rc == BN_OK && kind == kJtMax &&
        hipMemcpyAsync(states_out, j.d_states, sizeof(int32_t) * size_t(n_sets) * n, hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(BN_ERR_HIP, "copy of the states failed");
    if (rc == BN_OK && hipMemcpyAsync(j.scales.data(), j.d_scales, sizeof(double) * size_t(n_sets) * nc, hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(BN_ERR_HIP, "copy of the scales failed");
    const hipError_t drained = hipStreamSynchronize(s);   // (also after a failed launch: what is on the stream writes into the buffers)
    if (drained != hipSuccess && rc == BN_OK) rc = fail(BN_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(drained));
    if (rc != BN_OK) return rc;
    j.last_kernel_ns = 0;
    if (e->timing) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->events[0], e->events[1]));
        j.last_kernel_ns = int64_t(double(ms) * 1e6);
    }
    // log P(e) (a max run: log max_x P(x, e)) = the scales' logarithms added in array order: -inf as soon as one factor is 0
    // (a set's logarithms first, then their sum: a sum carried across the calls of std::log goes through the stack at every term,
    // once or twice as the compiler happens to place it -- 12 us of a batch of 256 sets' 330 us between two builds of this loop)
    if (log_evidence_out) {
        std::vector<double> logs(nc);
        for (int32_t q = 0; q < n_sets; ++q) {
            for (size_t c = 0; c < nc; ++c) logs[c] = std::log(j.scales[size_t(q) * nc + c]);
            double lg = 0.0;
            for (size_t c = 0; c < nc; ++c) lg += logs[c];
            log_evidence_out[q] = lg;
        }
    }
    j.n_sets = n_sets;
    j.last_form = form;
    j.last_kind = kind;
    j.last_launches = launches;
    j.have_run = true;
    return BN_OK;
}

}  // namespace

extern "C" int bn_jt_run(bn_engine* e, int32_t ne, const int32_t* ev_node, const int32_t* ev_off, const double* ev_val, double* beliefs_out,
                         double* log_evidence_out) {
    return jt_run_impl(e, kJtSum, 1, &ne, ev_node, ev_off, ev_val, beliefs_out, nullptr, log_evidence_out);
}

extern "C" int bn_jt_run_batch(bn_engine* e, int32_t n_sets, const int32_t* ne, const int32_t* ev_node, const int32_t* ev_off, const double* ev_val,
                               double* beliefs_out, double* log_evidence_out) {
    return jt_run_impl(e, kJtSum, n_sets, ne, ev_node, ev_off, ev_val, beliefs_out, nullptr, log_evidence_out);
}

extern "C" int bn_jt_mpe_run(bn_engine* e, int32_t ne, const int32_t* ev_node, const int32_t* ev_off, const double* ev_val,
                             double* max_marginals_out, int32_t* states_out, double* log_p_out) {
    return jt_run_impl(e, kJtMax, 1, &ne, ev_node, ev_off, ev_val, max_marginals_out, states_out, log_p_out);
}

extern "C" int bn_jt_mpe_run_batch(bn_engine* e, int32_t n_sets, const int32_t* ne, const int32_t* ev_node, const int32_t* ev_off,
                                   const double* ev_val, double* max_marginals_out, int32_t* states_out, double* log_p_out) {
    return jt_run_impl(e, kJtMax, n_sets, ne, ev_node, ev_off, ev_val, max_marginals_out, states_out, log_p_out);
}

extern "C" int bn_jt_scales(bn_engine* e, int32_t set, double* out, int32_t cap) {
    if (!e || !out || cap < 0) return fail(BN_ERR_ARG, "bad argument");
    const JtState& j = e->jt;
    if (!j.have_run) return fail(BN_ERR_STATE, "no junction-tree run yet");
    if (set == -1) {   // every set of the last run, [n_sets][cliques]
        const int64_t all = int64_t(j.n_sets) * j.plan.nc;
        if (cap < all) return fail(BN_ERR_ARG, "bn_jt_scales: set -1 needs room for n_sets x cliques values");
        std::copy(j.scales.begin(), j.scales.end(), out);
        return int(all);
    }
    if (set < 0 || set >= j.n_sets) return fail(BN_ERR_ARG, "set index out of range");
    const int32_t cnt = std::min(cap, j.plan.nc);
    std::copy_n(j.scales.begin() + size_t(set) * size_t(j.plan.nc), cnt, out);
    return cnt;
}

// dims_out[12] = eligible, cliques, levels, potential entries, separator entries, state cells, largest clique table, its variables,
// sum of the cliques' variable counts, sum of the separators', terms per run of a two-level sum, the form of the next run
extern "C" int bn_jt_plan_dims(bn_engine* e, int64_t* dims_out) {
    if (!e || !dims_out) return fail(BN_ERR_ARG, "null argument");
    ensure_plan(e);
    const JtPlan& P = e->jt.plan;
    if (!P.built) return fail(BN_ERR_STATE, refusal(e));
    const int64_t d[12] = {P.ok ? 1 : 0, P.nc, P.nlev, P.pot_cells, P.sep_cells, P.state_cells, P.max_clique, P.max_clique_vars,
                           int64_t(P.vars.size()), int64_t(P.sep_vars.size()), kJtRun, jt_form(P, e->jt.form_option)};
    std::copy(d, d + 12, dims_out);
    return BN_OK;
}

extern "C" int bn_jt_plan_dump(bn_engine* e, int32_t* order, int32_t* parent, int32_t* level, int32_t* var_ptr, int32_t* vars, int32_t* sep_ptr,
                               int32_t* sep_vars, int32_t* cpt_clique, int32_t* home) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    ensure_plan(e);
    const JtPlan& P = e->jt.plan;
    if (!P.built) return fail(BN_ERR_STATE, refusal(e));
    auto put = [](const std::vector<int32_t>& v, int32_t* out) { if (out) std::copy(v.begin(), v.end(), out); };
    put(P.order, order); put(P.parent, parent); put(P.level, level); put(P.var_ptr, var_ptr); put(P.vars, vars); put(P.sep_ptr, sep_ptr);
    put(P.sep_vars, sep_vars); put(P.cpt_clique, cpt_clique); put(P.home, home);
    return BN_OK;
}

// bn_set_option / bn_get_info hand the "jt_*" names here (bn_engine.cpp)
int bn_eng::jt_set_option(bn_engine* e, const char* name, int32_t value, bool* known) {
    *known = true;
    JtState& j = e->jt;
    if (std::strcmp(name, "jt_form") == 0) {
        if (value < 0 || value > 2) return fail(BN_ERR_ARG, "jt_form must be 0 (auto), 1 (state in LDS) or 2 (state in device scratch)");
        j.form_option = value;
        return BN_OK;
    }
    if (std::strcmp(name, "jt_scratch_cells") == 0) {   // 0: the default
        if (value < 0) return fail(BN_ERR_ARG, "jt_scratch_cells must not be negative");
        j.scratch_cells = value == 0 ? kJtScratchCells : std::min<int64_t>(value, kJtMaxScratchCells);
        // a plan that stopped at the budget has no tables: it is built again at its next use; a complete one is judged again
        if (j.tried && j.plan.built && j.plan.cliques.empty() && j.plan.state_cells <= j.scratch_cells) j.tried = false;
        else jt_apply_budget(j.plan, j.scratch_cells);
        return BN_OK;
    }
    *known = false;
    return BN_OK;
}

int64_t bn_eng::jt_get_info(bn_engine* e, const char* name, bool* known) {
    *known = true;
    JtState& j = e->jt;
    if (std::strcmp(name, "jt_last_form") == 0) return j.have_run ? j.last_form : 0;
    if (std::strcmp(name, "jt_last_kind") == 0) return j.have_run ? j.last_kind : 0;   // 1: a sum run, 2: a max run
    if (std::strcmp(name, "jt_last_launches") == 0) return j.have_run ? j.last_launches : 0;
    if (std::strcmp(name, "jt_scratch_cells") == 0) return j.scratch_cells;
    if (std::strcmp(name, "jt_last_kernel_ns") == 0) return j.have_run ? j.last_kernel_ns : 0;   // option "timing" 1: events around the launches
    // the facts of the plan: asking builds it
    const JtPlan& P = j.plan;
    auto is = [&](const char* what) {
        if (std::strcmp(name, what) != 0) return false;
        ensure_plan(e);
        return true;
    };
    if (is("jt_eligible")) return P.ok ? 1 : 0;
    if (is("jt_form")) return jt_form(P, j.form_option);   // the form the next run takes, 0: none
    if (is("jt_cliques")) return P.nc;
    if (is("jt_max_clique")) return P.max_clique;
    if (is("jt_state_cells")) return P.state_cells;
    if (is("jt_levels")) return P.nlev;
    *known = false;
    return 0;
}

void bn_eng::jt_cpt_reloaded(bn_engine* e) { e->jt.psi_ready = false; }
int bn_eng::jt_ensure_tables(bn_engine* e) { return ensure_tables(e); }

int bn_eng::jt_check_plan(bn_engine* e) {
    if (e->plan.nranks > 1) return fail(BN_ERR_STATE, kSharded);
    ensure_plan(e);
    if (!e->jt.plan.ok) return fail(BN_ERR_STATE, refusal(e));
    return BN_OK;
}

int bn_eng::jt_check_form(bn_engine* e, int* form_out) {
    const JtPlan& P = e->jt.plan;
    *form_out = jt_form(P, e->jt.form_option);
    if (*form_out == 0)
        return fail(BN_ERR_STATE, "option jt_form = 1, but the state of one evidence set, " + std::to_string(P.state_cells) + " doubles, does not fit the " +
                                      std::to_string(kJtLdsCells) + " doubles of LDS that form 1 keeps it in");
    return refuse_unusable(e, BN_ERR_NO_DEVICE);
}

JtTables bn_eng::jt_tables_of(const JtState& j, const double* psi0) {
    const JtPlan& P = j.plan;
    return {P.n, P.N, P.nc, P.nlev, int32_t(P.pot_cells), int32_t(P.sep_cells), int32_t(P.state_cells),
            j.d_cliques, j.d_levels, j.d_nodes, j.d_ent_clique, j.d_dn_map, j.d_sep_clique, j.d_c_base, j.d_p_base, j.d_c_res, j.d_p_res,
            j.d_up_map, j.d_home_nodes, j.d_elem_node, psi0};
}
