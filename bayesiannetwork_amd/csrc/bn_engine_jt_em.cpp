// bn_engine_jt_em.cpp -- exact expectation-maximisation: the bn_jt_em_* entry points over jt_em_kernel (bn_jt.hip; the rules:
// bn_jt.hpp, "Exact EM") and the sums of bn_em.hip.  The E-step is the junction tree's sum run, one workgroup per pattern row, with
// the family posteriors read from the cliques the CPTs were assigned to; the sums, the M-step and the loop are bn_engine_em.cpp's
// (em_reserve, em_drive), which this file hands its E-step as an EmEstep.  How the rows are cut into launches:
// bn_policy::jt_em_plan.  Theta, the base potentials of theta, the table, the scratch arrays and the sums are the JtEmState's own:
// a call reads the junction tree's plan and item tables and touches nothing the bn_bp_* / bn_mpe_* / bn_em_* / bn_jt_* calls use --
// not the engine's potentials, not the last run's scales.
#include "bn_engine_internal.hpp"

namespace {

static_assert(BN_EM_MISSING == kJtEmMissing && kJtEmMissing == kEmMissing, "bn_mi355x.h / bn_em.hpp: a constant differs from bn_jt.hpp");

// this path's own part (the shared one: em_reserve): the family tables, the potentials, the rows' outputs, the form-2 states
int reserve(bn_engine* e, int64_t n_patterns, const bn_policy::EmPlan& plan, int form) {
    JtEmState& m = e->jt_em;
    const JtPlan& P = e->jt.plan;
    hipStream_t s = e->stream;
    int r;
    if (!m.ready) {
        if ((r = upload(m.d_families, P.families, s))) return r;
        if ((r = upload(m.d_f_node, P.f_node, s))) return r;
        if ((r = upload(m.d_f_base, P.f_base, s))) return r;
        if ((r = upload(m.d_f_res, P.f_res, s))) return r;
        if ((r = dalloc(m.d_psi0, size_t(P.pot_cells)))) return r;
        HIPCHK(hipStreamSynchronize(s));
        m.ready = true;
    }
    if (n_patterns > m.cap_rows) {
        m.cap_rows = 0;
        if ((r = dalloc(m.d_loglik, size_t(n_patterns)))) return r;
        if ((r = dalloc(m.d_skipped, size_t(n_patterns)))) return r;
        m.cap_rows = n_patterns;
    }
    const int64_t state = form == 2 ? int64_t(plan.chunk) * P.state_cells : 0;
    if (state > m.cap_scratch) {
        m.cap_scratch = 0;
        if ((r = dalloc(m.d_scratch, size_t(state)))) return r;
        m.cap_scratch = state;
    }
    return BN_OK;
}

// what both entry points check behind their arguments: the plan's eligibility, the form, the device.  *form_out: 1 or 2
int check_engine(bn_engine* e, int* form_out) {
    if (int rc = jt_check_plan(e)) return rc;
    if (e->jt.plan.families.empty()) return fail(BN_ERR_STATE, "exact expectation-maximisation: the CPT array has 2^31 entries or more");
    return jt_check_form(e, form_out);
}

int run(bn_engine* e, const EmCall& c, int form) {
    JtEmState& m = e->jt_em;
    JtState& j = e->jt;
    const Plan& p = e->plan;
    const JtPlan& P = j.plan;
    const int32_t S = int32_t(p.cpt_off[p.n]);
    const bn_policy::EmPlan plan = bn_policy::jt_em_plan(c.n_patterns, S, m.core.scratch_cells, form, P.state_cells, j.scratch_cells);
    ON_DEVICE(e);
    if (int rc = jt_ensure_tables(e)) return rc;
    if (int rc = em_reserve(e, m.core, c.n_patterns, plan)) return rc;
    if (int rc = reserve(e, c.n_patterns, plan, form)) return rc;
    hipStream_t s = e->stream;

    const JtBaseArgs base{int32_t(P.pot_cells), j.d_cliques, j.d_ent_clique, j.d_asg_ptr, j.d_asg, j.d_fam, m.core.d_theta, m.d_psi0};
    JtEmArgs a{};
    a.t = jt_tables_of(j, m.d_psi0);
    a.S = S; a.families = m.d_families; a.f_node = m.d_f_node; a.f_base = m.d_f_base; a.f_res = m.d_f_res;
    a.scratch = m.d_scratch; a.b = m.core.d_b;
    const JtEmTotalArgs tot{c.n_patterns, m.core.d_counts, m.d_loglik, m.d_skipped, reinterpret_cast<double*>(m.core.d_words + 3), m.core.d_words + 1};
    EmEstep es{};
    es.what[0] = "jt_base"; es.what[1] = "jt_em"; es.what[2] = "jt_em_total";
    es.begin = [&] { return launch_jt_base(base, s); };   // the potentials of theta
    es.chunk = [&](const bn_policy::EmChunk& k) {
        a.patterns = m.core.d_patterns + size_t(k.first) * size_t(p.n);
        a.loglik = m.d_loglik + k.first;
        a.skipped = m.d_skipped + k.first;
        return launch_jt_em(a, form, k.count, s);
    };
    es.end = [&] { return launch_jt_em_total(tot, s); };
    es.d_rows = m.d_loglik; es.row_bytes = sizeof(double);
    es.has_L = true;
    m.last_form = form; m.last_launches = plan.n_chunks;
    return em_drive(e, m.core, c, plan, es);
}

}  // namespace

extern "C" int bn_jt_em_expected_counts(bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts, double* ecounts_out,
                                        double* row_loglik_out) {
    if (int rc = em_check_table_args(e, n_patterns, patterns, counts)) return rc;
    if (int rc = em_check_table_cells(e, n_patterns, patterns, counts)) return rc;
    if (!ecounts_out) return fail(BN_ERR_ARG, "null ecounts_out");
    int form = 0;
    if (int rc = check_engine(e, &form)) return rc;
    EmCall c{};
    c.n_patterns = n_patterns; c.patterns = patterns; c.counts = counts;
    c.theta0 = e->plan.cpt_flat.data();
    c.fit = false; c.E_out = ecounts_out; c.rows_out = row_loglik_out;
    return run(e, c, form);
}

extern "C" int bn_jt_em_fit(bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts, const bn_jt_em_options* opt,
                            const double* cpt_init, double* cpt_out, int32_t* iters_out, double* delta_hist_out, double* loglik_hist_out,
                            int32_t hist_cap) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (!opt) return fail(BN_ERR_ARG, "null options");
    if (int rc = em_check_table_args(e, n_patterns, patterns, counts)) return rc;
    if (int rc = em_check_table_cells(e, n_patterns, patterns, counts)) return rc;
    if (int rc = em_check_fit_args(cpt_out, opt->max_iters, opt->tol, opt->prior, delta_hist_out || loglik_hist_out, hist_cap)) return rc;
    int form = 0;
    if (int rc = check_engine(e, &form)) return rc;
    EmCall c{};
    c.n_patterns = n_patterns; c.patterns = patterns; c.counts = counts;
    c.theta0 = cpt_init ? cpt_init : e->plan.cpt_flat.data();
    c.fit = true; c.max_iters = opt->max_iters; c.tol = opt->tol; c.prior = opt->prior;
    c.cpt_out = cpt_out; c.iters_out = iters_out; c.delta_hist = delta_hist_out; c.loglik_hist = loglik_hist_out; c.hist_cap = hist_cap;
    return run(e, c, form);
}

// bn_set_option / bn_get_info hand the "jt_em_*" names here (bn_engine.cpp)
int bn_eng::jt_em_set_option(bn_engine* e, const char* name, int32_t value, bool* known) {
    return em_scratch_option("jt_em_scratch_cells", bn_policy::kJtEmScratchCells, e->jt_em.core, name, value, known);
}
int64_t bn_eng::jt_em_get_info(bn_engine* e, const char* name, bool* known) {
    *known = true;
    const EmCore& m = e->jt_em.core;
    if (std::strcmp(name, "jt_em_last_iters") == 0) return m.last_iters;
    if (std::strcmp(name, "jt_em_skipped") == 0) return m.skipped;
    if (std::strcmp(name, "jt_em_estep_ns") == 0) return m.estep_ns;
    if (std::strcmp(name, "jt_em_mstep_ns") == 0) return m.mstep_ns;
    if (std::strcmp(name, "jt_em_last_form") == 0) return e->jt_em.last_form;
    if (std::strcmp(name, "jt_em_last_launches") == 0) return e->jt_em.last_launches;
    if (std::strcmp(name, "jt_em_scratch_cells") == 0) return m.scratch_cells;
    *known = false;
    return 0;
}
