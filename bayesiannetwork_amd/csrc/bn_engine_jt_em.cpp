// bn_engine_jt_em.cpp -- exact expectation-maximisation: the bn_jt_em_* entry points over jt_em_kernel (bn_jt.hip; the rules:
// bn_jt.hpp, "Exact EM") and the sums of bn_em.hip.  The E-step is the junction tree's sum run, one workgroup per pattern row, with
// the family posteriors read from the cliques the CPTs were assigned to; the sums, the M-step's arithmetic and the loop are
// bn_engine_em.cpp's.  How the rows are cut into launches: bn_policy::jt_em_plan.  Theta, the base potentials of theta, the table,
// the scratch arrays and the sums are the JtEmState's own: a call reads the junction tree's plan and item tables and touches
// nothing the bn_bp_* / bn_mpe_* / bn_em_* / bn_jt_* calls use -- not the engine's potentials, not the last run's scales.
#include <cmath>

#include "bn_engine_internal.hpp"

namespace {

static_assert(BN_EM_MISSING == kJtEmMissing && kJtEmMissing == kEmMissing, "bn_mi355x.h / bn_em.hpp: a constant differs from bn_jt.hpp");

int reserve(bn_engine* e, int64_t n_patterns, const bn_policy::EmPlan& plan, int form) {
    JtEmState& m = e->jt_em;
    const JtPlan& P = e->jt.plan;
    const size_t S = size_t(e->plan.cpt_off[e->plan.n]);
    hipStream_t s = e->stream;
    int r;
    if (!m.ready) {
        if ((r = upload(m.d_families, P.families, s))) return r;
        if ((r = upload(m.d_f_node, P.f_node, s))) return r;
        if ((r = upload(m.d_f_base, P.f_base, s))) return r;
        if ((r = upload(m.d_f_res, P.f_res, s))) return r;
        if ((r = dalloc(m.d_theta, S))) return r;
        if ((r = dalloc(m.d_psi0, size_t(P.pot_cells)))) return r;
        if ((r = dalloc(m.d_E, S))) return r;
        if ((r = dalloc(m.d_partial, S))) return r;
        if ((r = dalloc(m.d_words, 3))) return r;
        for (EventOwner& ev : m.ev) HIPCHK(hipEventCreate(ev.put()));
        HIPCHK(hipStreamSynchronize(s));
        m.ready = true;
    }
    if (n_patterns > m.cap_patterns) {
        m.cap_patterns = 0;
        if ((r = dalloc(m.d_patterns, size_t(n_patterns) * size_t(e->plan.n)))) return r;
        if ((r = dalloc(m.d_counts, size_t(n_patterns)))) return r;
        if ((r = dalloc(m.d_loglik, size_t(n_patterns)))) return r;
        if ((r = dalloc(m.d_skipped, size_t(n_patterns)))) return r;
        m.cap_patterns = n_patterns;
    }
    if (plan.scratch > m.cap_b) {
        m.cap_b = 0;
        if ((r = dalloc(m.d_b, size_t(plan.scratch)))) return r;
        m.cap_b = plan.scratch;
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

struct JtEmCall {
    int64_t n_patterns;
    const uint8_t* patterns;
    const uint64_t* counts;
    const double* theta0;     // flat, [entries]
    int form;
    bool fit;                 // false: one E-step, no M-step
    int32_t max_iters;
    double tol, prior;
    double* E_out;            // the last E-step's sums (may be null)
    double* row_loglik_out;   // ... and its rows' log-likelihoods (may be null)
    double* cpt_out;          // (fit)
    int32_t* iters_out;
    double* delta_hist;
    double* loglik_hist;
    int32_t hist_cap;
};

int run(bn_engine* e, const JtEmCall& c) {
    JtEmState& m = e->jt_em;
    JtState& j = e->jt;
    const Plan& p = e->plan;
    const JtPlan& P = j.plan;
    const int32_t S = int32_t(p.cpt_off[p.n]);
    const bn_policy::EmPlan plan = bn_policy::jt_em_plan(c.n_patterns, S, m.scratch_cells, c.form, P.state_cells, j.scratch_cells);
    ON_DEVICE(e);
    if (int rc = jt_ensure_tables(e)) return rc;
    if (int rc = reserve(e, c.n_patterns, plan, c.form)) return rc;
    hipStream_t s = e->stream;
    HIPCHK(hipMemcpyAsync(m.d_patterns, c.patterns, size_t(c.n_patterns) * size_t(p.n), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m.d_counts, c.counts, size_t(c.n_patterns) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m.d_theta, c.theta0, size_t(S) * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(m.d_words, 0, 3 * sizeof(unsigned long long), s));
    HIPCHK(hipStreamSynchronize(s));   // (the caller's arrays are pageable)

    const JtBaseArgs base{int32_t(P.pot_cells), j.d_cliques, j.d_ent_clique, j.d_asg_ptr, j.d_asg, j.d_fam, m.d_theta, m.d_psi0};
    JtEmArgs a{};
    a.t = jt_tables_of(j, m.d_psi0);
    a.S = S; a.families = m.d_families; a.f_node = m.d_f_node; a.f_base = m.d_f_base; a.f_res = m.d_f_res;
    a.scratch = m.d_scratch; a.b = m.d_b;
    EmAccArgs acc{};
    acc.S = S; acc.n_patterns = c.n_patterns; acc.b = m.d_b; acc.counts = m.d_counts; acc.partial = m.d_partial; acc.E = m.d_E;
    const JtEmTotalArgs tot{c.n_patterns, m.d_counts, m.d_loglik, m.d_skipped, reinterpret_cast<double*>(m.d_words + 1), m.d_words};
    JtEmMstepArgs ms{};
    ms.S = S; ms.prior = c.prior; ms.E = m.d_E; ms.families = m.d_families; ms.nodes = j.d_nodes; ms.f_node = m.d_f_node;
    ms.theta = m.d_theta; ms.delta_bits = m.d_words + 2;

    m.last_iters = 0; m.skipped = 0; m.estep_ns = 0; m.mstep_ns = 0; m.last_form = c.form; m.last_launches = plan.n_chunks;
    int32_t iters = 0;
    const int32_t max_iters = c.fit ? c.max_iters : 1;
    for (;;) {
        // ---- E-step: the potentials of theta, then launch after launch its rows' posteriors added before the next overwrites them
        HIPCHK(hipMemsetAsync(m.d_E, 0, size_t(S) * sizeof(double), s));
        HIPCHK(hipMemsetAsync(m.d_partial, 0, size_t(S) * sizeof(double), s));
        HIPCHK(hipEventRecord(m.ev[0], s));
        if (int code = launch_jt_base(base, s)) return fail(BN_ERR_HIP, std::string("jt_base launch failed: ") + hipGetErrorString(hipError_t(code)));
        for (int64_t ch = 0; ch < plan.n_chunks; ++ch) {
            const bn_policy::EmChunk k = bn_policy::em_chunk(plan, c.n_patterns, ch);
            a.patterns = m.d_patterns + size_t(k.first) * size_t(p.n);
            a.loglik = m.d_loglik + k.first;
            a.skipped = m.d_skipped + k.first;
            if (int code = launch_jt_em(a, c.form, k.count, s))
                return fail(BN_ERR_HIP, std::string("jt_em launch failed: ") + hipGetErrorString(hipError_t(code)));
            acc.first = k.first; acc.chunk = k.count;
            if (int code = launch_em_accumulate(acc, s))
                return fail(BN_ERR_HIP, std::string("em_accumulate launch failed: ") + hipGetErrorString(hipError_t(code)));
        }
        if (int code = launch_jt_em_total(tot, s)) return fail(BN_ERR_HIP, std::string("jt_em_total launch failed: ") + hipGetErrorString(hipError_t(code)));
        HIPCHK(hipEventRecord(m.ev[1], s));
        ++iters;
        if (!c.fit) {
            HIPCHK(hipStreamSynchronize(s));
            float ms_e = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms_e, m.ev[0], m.ev[1]));
            m.estep_ns += int64_t(double(ms_e) * 1e6);
            break;
        }
        // ---- M-step; L and delta are the iteration's one trip to the host
        HIPCHK(hipMemsetAsync(m.d_words + 2, 0, sizeof(unsigned long long), s));
        if (int code = launch_jt_em_mstep(ms, s)) return fail(BN_ERR_HIP, std::string("jt_em_mstep launch failed: ") + hipGetErrorString(hipError_t(code)));
        HIPCHK(hipEventRecord(m.ev[2], s));
        double back[2] = {0.0, 0.0};   // L, delta
        HIPCHK(hipMemcpyAsync(back, m.d_words + 1, sizeof back, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms_e = 0.0f, ms_m = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms_e, m.ev[0], m.ev[1]));
        HIPCHK(hipEventElapsedTime(&ms_m, m.ev[1], m.ev[2]));
        m.estep_ns += int64_t(double(ms_e) * 1e6);
        m.mstep_ns += int64_t(double(ms_m) * 1e6);
        if (c.loglik_hist && iters <= c.hist_cap) c.loglik_hist[iters - 1] = back[0];
        if (c.delta_hist && iters <= c.hist_cap) c.delta_hist[iters - 1] = back[1];
        if (back[1] < c.tol || iters >= max_iters) break;   // strict <: tol = 0 never stops early
    }
    unsigned long long skipped = 0;
    HIPCHK(hipMemcpy(&skipped, m.d_words, sizeof skipped, hipMemcpyDeviceToHost));
    if (c.E_out) HIPCHK(hipMemcpy(c.E_out, m.d_E, size_t(S) * sizeof(double), hipMemcpyDeviceToHost));
    if (c.row_loglik_out) HIPCHK(hipMemcpy(c.row_loglik_out, m.d_loglik, size_t(c.n_patterns) * sizeof(double), hipMemcpyDeviceToHost));
    if (c.cpt_out) HIPCHK(hipMemcpy(c.cpt_out, m.d_theta, size_t(S) * sizeof(double), hipMemcpyDeviceToHost));
    if (c.iters_out) *c.iters_out = iters;
    m.last_iters = iters;
    m.skipped = int64_t(skipped);
    return BN_OK;
}

}  // namespace

extern "C" int bn_jt_em_expected_counts(bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts, double* ecounts_out,
                                        double* row_loglik_out) {
    if (int rc = em_check_table_args(e, n_patterns, patterns, counts)) return rc;
    if (int rc = em_check_table_cells(e, n_patterns, patterns, counts)) return rc;
    if (!ecounts_out) return fail(BN_ERR_ARG, "null ecounts_out");
    JtEmCall c{};
    if (int rc = check_engine(e, &c.form)) return rc;
    c.n_patterns = n_patterns; c.patterns = patterns; c.counts = counts;
    c.theta0 = e->plan.cpt_flat.data();
    c.fit = false; c.E_out = ecounts_out; c.row_loglik_out = row_loglik_out;
    return run(e, c);
}

extern "C" int bn_jt_em_fit(bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts, const bn_jt_em_options* opt,
                            const double* cpt_init, double* cpt_out, int32_t* iters_out, double* delta_hist_out, double* loglik_hist_out,
                            int32_t hist_cap) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (!opt) return fail(BN_ERR_ARG, "null options");
    if (int rc = em_check_table_args(e, n_patterns, patterns, counts)) return rc;
    if (int rc = em_check_table_cells(e, n_patterns, patterns, counts)) return rc;
    if (!cpt_out) return fail(BN_ERR_ARG, "null cpt_out");
    if (opt->max_iters < 1 || opt->max_iters > kEmMaxIters) return fail(BN_ERR_ARG, "max_iters must be in 1.." + std::to_string(kEmMaxIters));
    if (std::isnan(opt->tol)) return fail(BN_ERR_ARG, "tol is not a number");
    if (!(opt->prior >= 0.0) || !std::isfinite(opt->prior)) return fail(BN_ERR_ARG, "prior must be finite and >= 0");
    if ((delta_hist_out || loglik_hist_out) && hist_cap < 0) return fail(BN_ERR_ARG, "hist_cap < 0");
    JtEmCall c{};
    if (int rc = check_engine(e, &c.form)) return rc;
    c.n_patterns = n_patterns; c.patterns = patterns; c.counts = counts;
    c.theta0 = cpt_init ? cpt_init : e->plan.cpt_flat.data();
    c.fit = true; c.max_iters = opt->max_iters; c.tol = opt->tol; c.prior = opt->prior;
    c.cpt_out = cpt_out; c.iters_out = iters_out; c.delta_hist = delta_hist_out; c.loglik_hist = loglik_hist_out; c.hist_cap = hist_cap;
    return run(e, c);
}

// bn_set_option / bn_get_info hand the "jt_em_*" names here (bn_engine.cpp)
int bn_eng::jt_em_set_option(bn_engine* e, const char* name, int32_t value, bool* known) {
    *known = true;
    if (std::strcmp(name, "jt_em_scratch_cells") == 0) {   // 0: the default
        if (value < 0) return fail(BN_ERR_ARG, "jt_em_scratch_cells must be >= 0");
        e->jt_em.scratch_cells = value == 0 ? bn_policy::kJtEmScratchCells : value;
        return BN_OK;
    }
    *known = false;
    return BN_OK;
}
int64_t bn_eng::jt_em_get_info(bn_engine* e, const char* name, bool* known) {
    *known = true;
    const JtEmState& m = e->jt_em;
    if (std::strcmp(name, "jt_em_last_iters") == 0) return m.last_iters;
    if (std::strcmp(name, "jt_em_skipped") == 0) return m.skipped;
    if (std::strcmp(name, "jt_em_estep_ns") == 0) return m.estep_ns;
    if (std::strcmp(name, "jt_em_mstep_ns") == 0) return m.mstep_ns;
    if (std::strcmp(name, "jt_em_last_form") == 0) return m.last_form;
    if (std::strcmp(name, "jt_em_last_launches") == 0) return m.last_launches;
    if (std::strcmp(name, "jt_em_scratch_cells") == 0) return m.scratch_cells;
    *known = false;
    return 0;
}
