// bn_engine_em.cpp -- expectation-maximisation: the bn_em_* entry points over the kernels of bn_em.hip (the rules: bn_em.hpp).  How
// the table's rows are cut into launches: bn_policy::em_plan.  Everything a call needs beyond the item tables the engine uploaded for
// the one-workgroup path is the EmState's own and allocated at the first call: an EM call reads the engine's tables and touches nothing
// the bn_bp_* / bn_mpe_* calls use (evidence in force, batch staging, the state bn_bp_messages reads, last_path, the CPT images).
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
int build_maps(bn_engine* e, std::vector<int32_t>& ent_flat, std::vector<uint32_t>& row) {
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
    row.assign(S, 0u);
    size_t slot = 0;
    for (int v : order) {
        const int64_t c0 = p.cpt_off[v], c1 = p.cpt_off[v + 1];
        const int32_t kv = p.k[v];
        for (int64_t q = c0; q < c1; ++q, ++slot) {
            if (slot >= sp.ent.size() || !((sp.ent[slot].y >> 24) & 1u) || std::memcmp(&sp.ent_cpt[slot], &p.cpt_flat[size_t(q)], sizeof(double)) != 0)
                return fail(BN_ERR_STATE, "expectation-maximisation: the one-workgroup plan's entry order is not the expected one");
            ent_flat[slot] = int32_t(q) | (q == c0 ? 1 << 16 : 0);
            m.slot_of[size_t(q)] = int32_t(slot);
            row[size_t(q)] = uint32_t(c0 + (q - c0) / kv * kv) | uint32_t(kv) << 16;
            if (p.in_ptr[v + 1] == p.in_ptr[v]) m.init_of[size_t(q)] = int32_t(p.node_off[v] + (q - c0));
        }
    }
    return BN_OK;
}

int reserve(bn_engine* e, int64_t n_patterns, const bn_policy::EmPlan& plan) {
    EmState& m = e->em;
    const Plan& p = e->plan;
    const SmallPlan& sp = e->small;
    const size_t S = size_t(p.cpt_off[p.n]);
    int r;
    if (!m.ready) {
        if (int code = prepare_em_small()) return fail(BN_ERR_HIP, std::string("em_small attribute: ") + hipGetErrorString(hipError_t(code)));
        std::vector<int32_t> ent_flat;
        std::vector<uint32_t> row;
        if ((r = build_maps(e, ent_flat, row))) return r;
        if ((r = upload(m.d_ent_flat, ent_flat, e->stream))) return r;
        if ((r = upload(m.d_slot_of, m.slot_of, e->stream))) return r;
        if ((r = upload(m.d_init_of, m.init_of, e->stream))) return r;
        if ((r = upload(m.d_row, row, e->stream))) return r;
        HIPCHK(hipStreamSynchronize(e->stream));   // (`ent_flat` and `row` are locals)
        if ((r = dalloc(m.d_cpt, sp.ent_cpt.size()))) return r;
        if ((r = dalloc(m.d_init, sp.npi_init.size()))) return r;
        if ((r = dalloc(m.d_theta, S))) return r;
        if ((r = dalloc(m.d_E, S))) return r;
        if ((r = dalloc(m.d_partial, S))) return r;
        if ((r = dalloc(m.d_words, 3))) return r;
        for (EventOwner& ev : m.ev) HIPCHK(hipEventCreate(ev.put()));
        m.ready = true;
    }
    if (n_patterns > m.cap_patterns) {
        m.cap_patterns = 0;
        if ((r = dalloc(m.d_patterns, size_t(n_patterns) * size_t(p.n)))) return r;
        if ((r = dalloc(m.d_counts, size_t(n_patterns)))) return r;
        if ((r = dalloc(m.d_sweeps, size_t(n_patterns)))) return r;
        m.cap_patterns = n_patterns;
    }
    if (plan.scratch > m.cap_b) {
        m.cap_b = 0;
        if ((r = dalloc(m.d_b, size_t(plan.scratch)))) return r;
        m.cap_b = plan.scratch;
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

struct EmCall {
    int64_t n_patterns;
    const uint8_t* patterns;
    const uint64_t* counts;
    double bp_eps;
    int32_t cap;
    const double* theta0;     // flat, [entries]
    bool fit;                 // false: one E-step, no M-step
    int32_t max_iters;
    double tol, prior;
    double* E_out;            // the last E-step's sums (may be null)
    int32_t* sweeps_out;      // ... and its sweep counts (may be null)
    double* cpt_out;          // (fit)
    int32_t* iters_out;
    double* hist;
    int32_t hist_cap;
};

int run(bn_engine* e, const EmCall& c) {
    EmState& m = e->em;
    const Plan& p = e->plan;
    const SmallPlan& sp = e->small;
    const int32_t S = int32_t(p.cpt_off[p.n]);
    const bn_policy::EmPlan plan = bn_policy::em_plan(c.n_patterns, S, m.scratch_cells);
    ON_DEVICE(e);
    if (int rc = reserve(e, c.n_patterns, plan)) return rc;
    hipStream_t s = e->stream;
    // the table, and the starting tables as the flat array and as the two images the E-step kernel reads
    std::vector<double> img(sp.ent_cpt.size(), 0.0), init(sp.npi_init.size(), 1.0);
    for (int32_t q = 0; q < S; ++q) {
        img[size_t(m.slot_of[size_t(q)])] = c.theta0[q];
        if (m.init_of[size_t(q)] >= 0) init[size_t(m.init_of[size_t(q)])] = c.theta0[q];
    }
    HIPCHK(hipMemcpyAsync(m.d_patterns, c.patterns, size_t(c.n_patterns) * size_t(p.n), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m.d_counts, c.counts, size_t(c.n_patterns) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m.d_theta, c.theta0, size_t(S) * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m.d_cpt, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(m.d_init, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(m.d_words, 0, 3 * sizeof(unsigned long long), s));
    HIPCHK(hipStreamSynchronize(s));   // (`img` and `init` are locals; the caller's arrays are pageable)

    EmSmallArgs a{};
    a.eps = c.bp_eps; a.max_sweeps = c.cap;
    a.n = sp.n; a.N = sp.N; a.M = sp.M; a.S = S; a.T = sp.T; a.TT = sp.TT; a.CL = sp.CL; a.re = sp.re; a.rb = sp.rb; a.rc = sp.rc;
    put_items(a, e->small_img);
    a.ent_cpt = m.d_cpt; a.npi_init = m.d_init;   // (the images the M-step rewrites, not the engine's)
    a.ent_flat = m.d_ent_flat;
    a.b = m.d_b; a.counters = m.d_words;
    EmAccArgs acc{};
    acc.S = S; acc.n_patterns = c.n_patterns; acc.b = m.d_b; acc.counts = m.d_counts; acc.partial = m.d_partial; acc.E = m.d_E;
    EmMstepArgs ms{};
    ms.S = S; ms.prior = c.prior; ms.E = m.d_E; ms.row = m.d_row; ms.slot_of = m.d_slot_of; ms.init_of = m.d_init_of;
    ms.theta = m.d_theta; ms.ent_cpt = m.d_cpt; ms.npi_init = m.d_init; ms.delta_bits = m.d_words + 2;

    m.last_iters = 0; m.capped = 0; m.skipped = 0; m.estep_ns = 0; m.mstep_ns = 0;
    int32_t iters = 0;
    const int32_t max_iters = c.fit ? c.max_iters : 1;
    for (;;) {
        // ---- E-step: every launch's posteriors are added before the next launch overwrites the scratch array (one stream: in order)
        HIPCHK(hipMemsetAsync(m.d_E, 0, size_t(S) * sizeof(double), s));
        HIPCHK(hipMemsetAsync(m.d_partial, 0, size_t(S) * sizeof(double), s));
        HIPCHK(hipEventRecord(m.ev[0], s));
        for (int64_t ch = 0; ch < plan.n_chunks; ++ch) {
            const bn_policy::EmChunk k = bn_policy::em_chunk(plan, c.n_patterns, ch);
            a.patterns = m.d_patterns + size_t(k.first) * size_t(p.n);
            a.sweeps = m.d_sweeps + k.first;
            if (int code = launch_em_small(a, sp.waves, sp.lds_bytes, k.count, s))
                return fail(BN_ERR_HIP, std::string("em_small launch failed: ") + hipGetErrorString(hipError_t(code)));
            acc.first = k.first; acc.chunk = k.count;
            if (int code = launch_em_accumulate(acc, s))
                return fail(BN_ERR_HIP, std::string("em_accumulate launch failed: ") + hipGetErrorString(hipError_t(code)));
        }
        HIPCHK(hipEventRecord(m.ev[1], s));
        ++iters;
        if (!c.fit) {
            HIPCHK(hipStreamSynchronize(s));
            float ms_e = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms_e, m.ev[0], m.ev[1]));
            m.estep_ns += int64_t(double(ms_e) * 1e6);
            break;
        }
        // ---- M-step; delta is the iteration's one trip to the host
        HIPCHK(hipMemsetAsync(m.d_words + 2, 0, sizeof(unsigned long long), s));
        if (int code = launch_em_mstep(ms, s)) return fail(BN_ERR_HIP, std::string("em_mstep launch failed: ") + hipGetErrorString(hipError_t(code)));
        HIPCHK(hipEventRecord(m.ev[2], s));
        double delta = 0.0;
        HIPCHK(hipMemcpyAsync(&delta, m.d_words + 2, sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms_e = 0.0f, ms_m = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms_e, m.ev[0], m.ev[1]));
        HIPCHK(hipEventElapsedTime(&ms_m, m.ev[1], m.ev[2]));
        m.estep_ns += int64_t(double(ms_e) * 1e6);
        m.mstep_ns += int64_t(double(ms_m) * 1e6);
        if (c.hist && iters <= c.hist_cap) c.hist[iters - 1] = delta;
        if (delta < c.tol || iters >= max_iters) break;   // strict <: tol = 0 never stops early
    }
    unsigned long long words[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(words, m.d_words, sizeof words, hipMemcpyDeviceToHost));
    if (c.E_out) HIPCHK(hipMemcpy(c.E_out, m.d_E, size_t(S) * sizeof(double), hipMemcpyDeviceToHost));
    if (c.sweeps_out) HIPCHK(hipMemcpy(c.sweeps_out, m.d_sweeps, size_t(c.n_patterns) * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (c.cpt_out) HIPCHK(hipMemcpy(c.cpt_out, m.d_theta, size_t(S) * sizeof(double), hipMemcpyDeviceToHost));
    if (c.iters_out) *c.iters_out = iters;
    m.last_iters = iters;
    m.capped = int64_t(words[0]);
    m.skipped = int64_t(words[1]);
    return BN_OK;
}

}  // namespace

extern "C" int bn_em_expected_counts(bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts, double bp_eps,
                                     int32_t bp_max_sweeps, double* ecounts_out, int32_t* sweeps_out) {
    if (int rc = check_call(e, n_patterns, patterns, counts, bp_eps, bp_max_sweeps)) return rc;
    if (!ecounts_out) return fail(BN_ERR_ARG, "null ecounts_out");
    if (int rc = check_engine(e)) return rc;
    EmCall c{};
    c.n_patterns = n_patterns; c.patterns = patterns; c.counts = counts; c.bp_eps = bp_eps;
    c.cap = bp_max_sweeps == 0 ? kMpeDefaultCap : bp_max_sweeps;   // never unbounded (bn_em.hpp)
    c.theta0 = e->plan.cpt_flat.data();
    c.fit = false; c.E_out = ecounts_out; c.sweeps_out = sweeps_out;
    return run(e, c);
}

extern "C" int bn_em_fit(bn_engine* e, int64_t n_patterns, const uint8_t* patterns, const uint64_t* counts, const bn_em_options* opt,
                         const double* cpt_init, double* cpt_out, int32_t* iters_out, double* delta_hist_out, int32_t hist_cap) {
    if (!e) return fail(BN_ERR_ARG, "null engine");
    if (!opt) return fail(BN_ERR_ARG, "null options");
    if (int rc = check_call(e, n_patterns, patterns, counts, opt->bp_eps, opt->bp_max_sweeps)) return rc;
    if (!cpt_out) return fail(BN_ERR_ARG, "null cpt_out");
    if (opt->max_iters < 1 || opt->max_iters > kEmMaxIters) return fail(BN_ERR_ARG, "max_iters must be in 1.." + std::to_string(kEmMaxIters));
    if (std::isnan(opt->tol)) return fail(BN_ERR_ARG, "tol is not a number");
    if (!(opt->prior >= 0.0) || !std::isfinite(opt->prior)) return fail(BN_ERR_ARG, "prior must be finite and >= 0");
    if (delta_hist_out && hist_cap < 0) return fail(BN_ERR_ARG, "hist_cap < 0");
    if (int rc = check_engine(e)) return rc;
    EmCall c{};
    c.n_patterns = n_patterns; c.patterns = patterns; c.counts = counts; c.bp_eps = opt->bp_eps;
    c.cap = opt->bp_max_sweeps == 0 ? kMpeDefaultCap : opt->bp_max_sweeps;
    c.theta0 = cpt_init ? cpt_init : e->plan.cpt_flat.data();
    c.fit = true; c.max_iters = opt->max_iters; c.tol = opt->tol; c.prior = opt->prior;
    c.cpt_out = cpt_out; c.iters_out = iters_out; c.hist = delta_hist_out; c.hist_cap = hist_cap;
    return run(e, c);
}

// bn_set_option / bn_get_info hand the "em_*" names here (bn_engine.cpp)
int bn_eng::em_set_option(bn_engine* e, const char* name, int32_t value, bool* known) {
    *known = true;
    if (std::strcmp(name, "em_scratch_cells") == 0) {   // 0: the default
        if (value < 0) return fail(BN_ERR_ARG, "em_scratch_cells must be >= 0");
        e->em.scratch_cells = value == 0 ? bn_policy::kEmScratchCells : value;
        return BN_OK;
    }
    *known = false;
    return BN_OK;
}
int64_t bn_eng::em_get_info(bn_engine* e, const char* name, bool* known) {
    *known = true;
    const EmState& m = e->em;
    if (std::strcmp(name, "em_eligible") == 0) return e->plan.nranks == 1 && e->small.ok ? 1 : 0;
    if (std::strcmp(name, "em_last_iters") == 0) return m.last_iters;
    if (std::strcmp(name, "em_capped") == 0) return m.capped;
    if (std::strcmp(name, "em_skipped") == 0) return m.skipped;
    if (std::strcmp(name, "em_estep_ns") == 0) return m.estep_ns;
    if (std::strcmp(name, "em_mstep_ns") == 0) return m.mstep_ns;
    if (std::strcmp(name, "em_scratch_cells") == 0) return m.scratch_cells;
    *known = false;
    return 0;
}
