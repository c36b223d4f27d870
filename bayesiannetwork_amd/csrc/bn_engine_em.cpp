// bn_engine_em.cpp -- expectation-maximisation: the bn_em_* entry points over the kernels of bn_em.hip (the rules: bn_em.hpp).  How
// the table's rows are cut into launches: bn_policy::em_plan.  Everything a call needs beyond the item tables the engine uploaded for
// the one-workgroup path is the EmState's own and allocated at the first call: an EM call reads the engine's tables and touches nothing
// the bn_bp_* / bn_mpe_* calls use (evidence in force, batch staging, the state bn_bp_messages reads, last_path, the CPT images).
// Also here, once for this file and for bn_engine_jt_em.cpp (exact EM: the same loop over the junction tree's E-step): the shared
// buffers (em_reserve over an EmCore), the loop itself (em_drive: uploads, E-step launches and sums, M-step, the one trip to the host
// per iteration, the stopping rule, the read-backs), the checks of a fit's options and the handler of the scratch option.  An E-step
// is handed to the loop as an EmEstep: what to launch before, for and behind the chunks, and what the M-step and the read-backs need.
#include <cmath>

#include "bn_engine_internal.hpp"

namespace {

static_assert(bn_policy::kEmBlock == bnmi::kEmBlock && BN_EM_MISSING == kEmMissing, "bn_engine_policy.hpp / bn_mi355x.h: a constant differs from bn_em.hpp");

// why the network has no one-workgroup plan, in the planner's own words
std::string not_eligible_text(const bn_engine* e) {
    if (e->plan.nranks > 1) return "expectation-maximisation is not available on sharded engines";
    return "expectation-maximisation runs networks of at most " + std::to_string(kSmallMaxParents) +
           " parents per node that fit one workgroup; this one: " + (e->small.why.empty() ? std::string("no one-workgroup plan") : e->small.why);
}

// The index maps between the entry items' table and the flat CPT array, from the plan's own order (bn_small_plan.cpp: nodes by
// falling parent count, stable; a node's entries in table order), checked against the values the plan holds.
int build_maps(bn_engine* e, std::vector<int32_t>& ent_flat) {
    EmState& m = e->em;
    const Plan& p = e->plan;
    const SmallPlan& sp = e->small;
    const int32_t n = p.n;
    const size_t S = size_t(p.cpt_off[n]);
    std::vector<int> order(size_t(n), 0);
    for (int v = 0; v < n; ++v) order[size_t(v)] = v;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p.in_ptr[a + 1] - p.in_ptr[a] > p.in_ptr[b + 1] - p.in_ptr[b]; });
    ent_flat.assign(sp.ent.size(), -1);
    m.slot_of.assign(S, 0);
    m.init_of.assign(S, -1);
    size_t slot = 0;
    for (int v : order) {
        const int64_t c0 = p.cpt_off[v], c1 = p.cpt_off[v + 1];
        for (int64_t q = c0; q < c1; ++q, ++slot) {
            if (slot >= sp.ent.size() || !((sp.ent[slot].y >> 24) & 1u) || std::memcmp(&sp.ent_cpt[slot], &p.cpt_flat[size_t(q)], sizeof(double)) != 0)
                return fail(BN_ERR_STATE, "expectation-maximisation: the one-workgroup plan's entry order is not the expected one");
            ent_flat[slot] = int32_t(q) | (q == c0 ? 1 << 16 : 0);
            m.slot_of[size_t(q)] = int32_t(slot);
            if (p.in_ptr[v + 1] == p.in_ptr[v]) m.init_of[size_t(q)] = int32_t(p.node_off[v] + (q - c0));
        }
    }
    return BN_OK;
}

// this path's own part (the shared one: em_reserve): the maps, the images, the rows' sweep counts
int reserve(bn_engine* e, int64_t n_patterns) {
    EmState& m = e->em;
    const SmallPlan& sp = e->small;
    int r;
    if (!m.ready) {
        if (int code = prepare_em_small()) return fail(BN_ERR_HIP, std::string("em_small attribute: ") + hipGetErrorString(hipError_t(code)));
        std::vector<int32_t> ent_flat;
        if ((r = build_maps(e, ent_flat))) return r;
        if ((r = upload(m.d_ent_flat, ent_flat, e->stream))) return r;
        if ((r = upload(m.d_slot_of, m.slot_of, e->stream))) return r;
        if ((r = upload(m.d_init_of, m.init_of, e->stream))) return r;
        HIPCHK(hipStreamSynchronize(e->stream));   // (`ent_flat` is a local)
        if ((r = dalloc(m.d_cpt, sp.ent_cpt.size()))) return r;
        if ((r = dalloc(m.d_init, sp.npi_init.size()))) return r;
        m.ready = true;
    }
    if (n_patterns > m.cap_rows) {
        m.cap_rows = 0;
        if ((r = dalloc(m.d_sweeps, size_t(n_patterns)))) return r;
        m.cap_rows = n_patterns;
    }
    return BN_OK;
}

// the checks of the table and of what both entry points share, in the order bn_mi355x.h gives: arguments, eligibility, device
int check_call(bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts, double bp_eps, int32_t bp_max_sweeps) {
    if (int rc = em_check_table_args(e, n_patterns, patterns, counts)) return rc;
    if (std::isnan(bp_eps)) return fail(BN_ERR_ARG, "bp_eps is not a number");
    if (bp_max_sweeps < 0) return fail(BN_ERR_ARG, "bp_max_sweeps < 0");
    return em_check_table_cells(e, n_patterns, patterns, counts);
}
int check_engine(bn_engine* e) {
    if (e->plan.nranks > 1 || !e->small.ok) return fail(BN_ERR_STATE, not_eligible_text(e));
    if (int rc = refuse_unusable(e, BN_ERR_NO_DEVICE)) return rc;
    if (!e->small_ok) return fail(BN_ERR_STATE, "the item tables of the one-workgroup path were not set up on the device");
    return BN_OK;
}

// bp_eps, cap: what a call says to the one-workgroup E-step alone (cap > 0)
int run(bn_engine* e, const EmCall& c, double bp_eps, int32_t cap) {
    EmState& m = e->em;
    const Plan& p = e->plan;
    const SmallPlan& sp = e->small;
    const int32_t S = int32_t(p.cpt_off[p.n]);
    const bn_policy::EmPlan plan = bn_policy::em_plan(c.n_patterns, S, m.core.scratch_cells);
    ON_DEVICE(e);
    if (int rc = em_reserve(e, m.core, c.n_patterns, plan)) return rc;
    if (int rc = reserve(e, c.n_patterns)) return rc;
    hipStream_t s = e->stream;
    // the starting tables as the two images the E-step kernel reads (em_drive waits for the stream before it starts: locals)
    std::vector<double> img(sp.ent_cpt.size(), 0.0), init(sp.npi_init.size(), 1.0);
    for (int32_t q = 0; q < S; ++q) {
        img[size_t(m.slot_of[size_t(q)])] = c.theta0[q];
        if (m.init_of[size_t(q)] >= 0) init[size_t(m.init_of[size_t(q)])] = c.theta0[q];
    }
    HIPCHK(hipMemcpyAsync(m.d_cpt, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m.d_init, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice, s));

    EmSmallArgs a{};
    a.eps = bp_eps; a.max_sweeps = cap;
    a.n = sp.n; a.N = sp.N; a.M = sp.M; a.S = S; a.T = sp.T; a.TT = sp.TT; a.CL = sp.CL; a.re = sp.re; a.rb = sp.rb; a.rc = sp.rc;
    put_items(a, e->small_img);
    a.ent_cpt = m.d_cpt; a.npi_init = m.d_init;   // (the images the M-step rewrites, not the engine's)
    a.ent_flat = m.d_ent_flat;
    a.b = m.core.d_b; a.counters = m.core.d_words;
    EmEstep es{};
    es.what[1] = "em_small";
    es.chunk = [&](const bn_policy::EmChunk& k) {
        a.patterns = m.core.d_patterns + size_t(k.first) * size_t(p.n);
        a.sweeps = m.d_sweeps + k.first;
        return launch_em_small(a, sp.waves, sp.lds_bytes, k.count, s);
    };
    es.slot_of = m.d_slot_of; es.init_of = m.d_init_of; es.ent_cpt = m.d_cpt; es.npi_init = m.d_init;
    es.d_rows = m.d_sweeps; es.row_bytes = sizeof(int32_t);
    es.capped = &m.capped;
    return em_drive(e, m.core, c, plan, es);
}

}  // namespace

// ---- what both call families share ------------------------------------------------------------------------------------------------

int bn_eng::em_check_fit_args(const double* cpt_out, int32_t max_iters, double tol, double prior, bool any_hist, int32_t hist_cap) {
    if (!cpt_out) return fail(BN_ERR_ARG, "null cpt_out");
    if (max_iters < 1 || max_iters > kEmMaxIters) return fail(BN_ERR_ARG, "max_iters must be in 1.." + std::to_string(kEmMaxIters));
    if (std::isnan(tol)) return fail(BN_ERR_ARG, "tol is not a number");
    if (!(prior >= 0.0) || !std::isfinite(prior)) return fail(BN_ERR_ARG, "prior must be finite and >= 0");
    if (any_hist && hist_cap < 0) return fail(BN_ERR_ARG, "hist_cap < 0");
    return BN_OK;
}

int bn_eng::em_scratch_option(const char* own, int64_t dflt, EmCore& m, const char* name, int32_t value, bool* known) {
    *known = std::strcmp(name, own) == 0;
    if (!*known) return BN_OK;
    if (value < 0) return fail(BN_ERR_ARG, std::string(own) + " must be >= 0");
    m.scratch_cells = value == 0 ? dflt : value;
    return BN_OK;
}

int bn_eng::em_reserve(bn_engine* e, EmCore& m, int64_t n_patterns, const bn_policy::EmPlan& plan) {
    const Plan& p = e->plan;
    const size_t S = size_t(p.cpt_off[p.n]);
    int r;
    if (!m.ready) {
        const std::vector<bn_policy::EmRow> row = bn_policy::em_rows(p.n, p.cpt_off.data(), p.k.data());
        if ((r = upload(m.d_row, row, e->stream))) return r;
        HIPCHK(hipStreamSynchronize(e->stream));   // (`row` is a local)
        if ((r = dalloc(m.d_theta, S))) return r;
        if ((r = dalloc(m.d_E, S))) return r;
        if ((r = dalloc(m.d_partial, S))) return r;
        if ((r = dalloc(m.d_words, 4))) return r;
        for (EventOwner& ev : m.ev) HIPCHK(hipEventCreate(ev.put()));
        m.ready = true;
    }
    if (n_patterns > m.cap_patterns) {
        m.cap_patterns = 0;
        if ((r = dalloc(m.d_patterns, size_t(n_patterns) * size_t(p.n)))) return r;
        if ((r = dalloc(m.d_counts, size_t(n_patterns)))) return r;
        m.cap_patterns = n_patterns;
    }
    if (plan.scratch > m.cap_b) {
        m.cap_b = 0;
        if ((r = dalloc(m.d_b, size_t(plan.scratch)))) return r;
        m.cap_b = plan.scratch;
    }
    return BN_OK;
}

// The loop of bn_em.hpp over either E-step, on the engine's stream and the calling thread's current device (the engine's); the
// buffers are em_reserve's.  One trip to the host per iteration.
int bn_eng::em_drive(bn_engine* e, EmCore& m, const EmCall& c, const bn_policy::EmPlan& plan, const EmEstep& es) {
    const Plan& p = e->plan;
    const int32_t S = int32_t(p.cpt_off[p.n]);
    hipStream_t s = e->stream;
    const auto launch_failed = [](const char* what, int code) {
        return fail(BN_ERR_HIP, std::string(what) + " launch failed: " + hipGetErrorString(hipError_t(code)));
    };
    HIPCHK(hipMemcpyAsync(m.d_patterns, c.patterns, size_t(c.n_patterns) * size_t(p.n), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m.d_counts, c.counts, size_t(c.n_patterns) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m.d_theta, c.theta0, size_t(S) * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(m.d_words, 0, 4 * sizeof(unsigned long long), s));
    HIPCHK(hipStreamSynchronize(s));   // (the caller's arrays are pageable)

    EmAccArgs acc{};
    acc.S = S; acc.n_patterns = c.n_patterns; acc.b = m.d_b; acc.counts = m.d_counts; acc.partial = m.d_partial; acc.E = m.d_E;
    EmMstepArgs ms{};
    ms.S = S; ms.prior = c.prior; ms.E = m.d_E; ms.row = m.d_row; ms.slot_of = es.slot_of; ms.init_of = es.init_of;
    ms.theta = m.d_theta; ms.ent_cpt = es.ent_cpt; ms.npi_init = es.npi_init; ms.delta_bits = m.d_words + 2;

    m.last_iters = 0; m.skipped = 0; m.estep_ns = 0; m.mstep_ns = 0;
    if (es.capped) *es.capped = 0;
    int32_t iters = 0;
    const int32_t max_iters = c.fit ? c.max_iters : 1;
    for (;;) {
        // ---- E-step: every launch's posteriors are added before the next launch overwrites the scratch array (one stream: in order)
        HIPCHK(hipMemsetAsync(m.d_E, 0, size_t(S) * sizeof(double), s));
        HIPCHK(hipMemsetAsync(m.d_partial, 0, size_t(S) * sizeof(double), s));
        HIPCHK(hipEventRecord(m.ev[0], s));
        if (es.begin)
            if (int code = es.begin()) return launch_failed(es.what[0], code);
        for (int64_t ch = 0; ch < plan.n_chunks; ++ch) {
            const bn_policy::EmChunk k = bn_policy::em_chunk(plan, c.n_patterns, ch);
            if (int code = es.chunk(k)) return launch_failed(es.what[1], code);
            acc.first = k.first; acc.chunk = k.count;
            if (int code = launch_em_accumulate(acc, s)) return launch_failed("em_accumulate", code);
        }
        if (es.end)
            if (int code = es.end()) return launch_failed(es.what[2], code);
        HIPCHK(hipEventRecord(m.ev[1], s));
        ++iters;
        if (!c.fit) {
            HIPCHK(hipStreamSynchronize(s));
            float ms_e = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms_e, m.ev[0], m.ev[1]));
            m.estep_ns += int64_t(double(ms_e) * 1e6);
            break;
        }
        // ---- M-step; delta (and L, where the E-step has one) is the iteration's one trip to the host
        HIPCHK(hipMemsetAsync(m.d_words + 2, 0, sizeof(unsigned long long), s));
        if (int code = launch_em_mstep(ms, s)) return launch_failed("em_mstep", code);
        HIPCHK(hipEventRecord(m.ev[2], s));
        double back[2] = {0.0, 0.0};   // delta, L
        HIPCHK(hipMemcpyAsync(back, m.d_words + 2, (es.has_L ? 2 : 1) * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms_e = 0.0f, ms_m = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms_e, m.ev[0], m.ev[1]));
        HIPCHK(hipEventElapsedTime(&ms_m, m.ev[1], m.ev[2]));
        m.estep_ns += int64_t(double(ms_e) * 1e6);
        m.mstep_ns += int64_t(double(ms_m) * 1e6);
        if (c.loglik_hist && iters <= c.hist_cap) c.loglik_hist[iters - 1] = back[1];
        if (c.delta_hist && iters <= c.hist_cap) c.delta_hist[iters - 1] = back[0];
        if (back[0] < c.tol || iters >= max_iters) break;   // strict <: tol = 0 never stops early
    }
    unsigned long long words[2] = {0, 0};   // runs cut by the cap, skipped families
    HIPCHK(hipMemcpy(words, m.d_words, sizeof words, hipMemcpyDeviceToHost));
    if (c.E_out) HIPCHK(hipMemcpy(c.E_out, m.d_E, size_t(S) * sizeof(double), hipMemcpyDeviceToHost));
    if (c.rows_out) HIPCHK(hipMemcpy(c.rows_out, es.d_rows, size_t(c.n_patterns) * es.row_bytes, hipMemcpyDeviceToHost));
    if (c.cpt_out) HIPCHK(hipMemcpy(c.cpt_out, m.d_theta, size_t(S) * sizeof(double), hipMemcpyDeviceToHost));
    if (c.iters_out) *c.iters_out = iters;
    m.last_iters = iters;
    if (es.capped) *es.capped = int64_t(words[0]);
    m.skipped = int64_t(words[1]);
    return BN_OK;
}

// ---- the bn_em_* entry points -----------------------------------------------------------------------------------------------------

extern "C" int bn_em_expected_counts(bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts, double bp_eps,
                                     int32_t bp_max_sweeps, double* ecounts_out, int32_t* sweeps_out) {
    if (int rc = check_call(e, n_patterns, patterns, counts, bp_eps, bp_max_sweeps)) return rc;
    if (!ecounts_out) return fail(BN_ERR_ARG, "null ecounts_out");
    if (int rc = check_engine(e)) return rc;
    EmCall c{};
    c.n_patterns = n_patterns; c.patterns = patterns; c.counts = counts;
    c.theta0 = e->plan.cpt_flat.data();
    c.fit = false; c.E_out = ecounts_out; c.rows_out = sweeps_out;
    return run(e, c, bp_eps, bp_max_sweeps == 0 ? kMpeDefaultCap : bp_max_sweeps);   // never unbounded (bn_em.hpp)
}

extern "C" int bn_em_fit(bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts, const bn_em_options* opt,
                         const double* cpt_init, double* cpt_out, int32_t* iters_out, double* delta_hist_out, int32_t hist_cap) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (!opt) return fail(BN_ERR_ARG, "null options");
    if (int rc = check_call(e, n_patterns, patterns, counts, opt->bp_eps, opt->bp_max_sweeps)) return rc;
    if (int rc = em_check_fit_args(cpt_out, opt->max_iters, opt->tol, opt->prior, delta_hist_out != nullptr, hist_cap)) return rc;
    if (int rc = check_engine(e)) return rc;
    EmCall c{};
    c.n_patterns = n_patterns; c.patterns = patterns; c.counts = counts;
    c.theta0 = cpt_init ? cpt_init : e->plan.cpt_flat.data();
    c.fit = true; c.max_iters = opt->max_iters; c.tol = opt->tol; c.prior = opt->prior;
    c.cpt_out = cpt_out; c.iters_out = iters_out; c.delta_hist = delta_hist_out; c.hist_cap = hist_cap;
    return run(e, c, opt->bp_eps, opt->bp_max_sweeps == 0 ? kMpeDefaultCap : opt->bp_max_sweeps);
}

// bn_set_option / bn_get_info hand the "em_*" names here (bn_engine.cpp)
int bn_eng::em_set_option(bn_engine* e, const char* name, int32_t value, bool* known) {
    return em_scratch_option("em_scratch_cells", bn_policy::kEmScratchCells, e->em.core, name, value, known);
}
int64_t bn_eng::em_get_info(bn_engine* e, const char* name, bool* known) {
    *known = true;
    const EmCore& m = e->em.core;
    if (std::strcmp(name, "em_eligible") == 0) return e->plan.nranks == 1 && e->small.ok ? 1 : 0;
    if (std::strcmp(name, "em_last_iters") == 0) return m.last_iters;
    if (std::strcmp(name, "em_capped") == 0) return e->em.capped;
    if (std::strcmp(name, "em_skipped") == 0) return m.skipped;
    if (std::strcmp(name, "em_estep_ns") == 0) return m.estep_ns;
    if (std::strcmp(name, "em_mstep_ns") == 0) return m.mstep_ns;
    if (std::strcmp(name, "em_scratch_cells") == 0) return m.scratch_cells;
    *known = false;
    return 0;
}
