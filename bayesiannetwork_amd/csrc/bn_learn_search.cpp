// bn_learn_search.cpp -- the device-resident structure searches over a term table (bn_learn_terms.cpp): bn_learn_anneal runs the
// reference's simulated_annealing.hpp as many chains (bn_learn_anneal.hip), bn_learn_hc its stepwise_structure_hc.hpp as many runs
// (bn_learn_hc.hip), bn_learn_climb tabu hill climbing as many runs (bn_learn_climb.hip).  All end alike: the run with the smallest
// score becomes the learner's graph (finish_search).
#include "bn_learn_internal.hpp"
#include "bn_learn_anneal.hpp"
#include "bn_learn_climb.hpp"
#include "bn_learn_hc.hpp"

namespace {

// a search over a term table reads the table's terms as the learner's: they must be the same function
int check_table_spec(const char* who, const bn_learner* L, const bn_term_table* tt) {
    if (same_spec(L->spec, tt->spec)) return BN_OK;
    std::string what = std::string(who) + ": the term table holds " + spec_name(tt->spec) + " terms, the learner scores by " + spec_name(L->spec);
    if (L->spec.kind == 2 && tt->spec.kind == 2) what += " with another ess (" + std::to_string(tt->spec.ess) + " against " + std::to_string(L->spec.ess) + ")";
    return fail(BN_ERR_ARG, what);
}

// the winner's graph and terms become the learner's (score = score_with(-1, 0.0, params): the kernels' evaluation is that function)
void adopt_winner(bn_learner* L, const std::vector<uint64_t>& win_mask, const std::vector<double>& win_ll, double score) {
    const int32_t n = L->n;
    for (int32_t v = 0; v < n; ++v) {
        L->parents[size_t(v)].clear();
        L->children[size_t(v)].clear();
    }
    L->params = 0;
    for (int32_t v = 0; v < n; ++v) {
        for (int32_t u = 0; u < n; ++u)
            if ((win_mask[size_t(v)] >> u) & 1) {
                L->parents[size_t(v)].push_back(u);
                L->children[size_t(u)].push_back(v);
            }
        L->ll[size_t(v)] = win_ll[size_t(v)];
        L->params += L->family_params(v, L->rows_of(v));
    }
    L->score = score;
}

// The tail of every search, entered once the kernel and the event pair (ev0, ev1) around it are on the stream and the per-run scores
// are on the host: the winner is the run of the smallest score, strictly (ties stay with the lowest index); its row of `d_masks`
// and `d_ll` ([runs][n]) and, where asked for, every run's masks are downloaded together with what `more()` enqueues; the
// kernel's time is added to `ns`; the winner becomes the learner's graph.
template <class More>
int finish_search(bn_learner* L, hipStream_t s, const std::vector<double>& score, const DeviceBuf<uint64_t>& d_masks, const DeviceBuf<double>& d_ll,
                  uint64_t* masks_out, hipEvent_t ev0, hipEvent_t ev1, double& ns, int32_t* winner_out, More more) {
    const size_t n = size_t(L->n), runs = score.size();
    size_t winner = 0;
    for (size_t j = 0; j < runs; ++j)
        if (score[j] < score[winner]) winner = j;
    std::vector<uint64_t> win_mask(n);
    std::vector<double> win_ll(n);
    HIPCHK(hipMemcpyAsync(win_mask.data(), d_masks.get() + winner * n, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(win_ll.data(), d_ll.get() + winner * n, n * 8, hipMemcpyDeviceToHost, s));
    if (masks_out) HIPCHK(hipMemcpyAsync(masks_out, d_masks, runs * n * 8, hipMemcpyDeviceToHost, s));
    if (int r = more()) return r;
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    ns += double(ms) * 1e6;
    if (winner_out) *winner_out = int32_t(winner);
    adopt_winner(L, win_mask, win_ll, score[winner]);
    return BN_OK;
}

}  // namespace

static_assert(sizeof(bn_anneal_trace) == sizeof(AnnealTrace) && sizeof(AnnealTrace) == 16, "the trace record is the ABI's");
static_assert(sizeof(AnnealRecord) == 32, "one record per chain");

extern "C" int bn_learn_anneal(bn_learner* L, bn_term_table* tt, const bn_anneal_params* p, int32_t chains, uint64_t seed, double* eval_out,
                               uint32_t* counts_out, uint64_t* masks_out, int32_t* n_edges_out, uint16_t* edges_out,
                               bn_anneal_trace* trace_out, int32_t* winner_out) {
    if (!L || !tt || !p) return fail(BN_ERR_ARG, "null argument");
    if (tt->t != L->t) return fail(BN_ERR_ARG, "anneal: the term table was built from another table than the learner's");
    if (int r = check_table_spec("anneal", L, tt)) return r;
    auto positive = [](double x) { return std::isfinite(x) && x > 0.0; };
    if (!positive(p->initial_temp) || !positive(p->final_temp)) return fail(BN_ERR_ARG, "anneal: the temperatures must be finite and positive");
    if (!(p->decreasing_rate > 0.0 && p->decreasing_rate < 1.0)) return fail(BN_ERR_ARG, "anneal: decreasing_rate must be in (0, 1)");
    if (!positive(p->boltzmann)) return fail(BN_ERR_ARG, "anneal: boltzmann must be finite and positive");
    if (p->rule != 0 && p->rule != 1) return fail(BN_ERR_ARG, "anneal: rule 0 (the reference's) or 1 (Metropolis)");
    if (chains < 1 || chains > kAnnealMaxChains) return fail(BN_ERR_ARG, "anneal: " + std::to_string(chains) + " chains (1 .. 65536)");
    if (p->max_proposals > kAnnealMaxProposals)
        return fail(BN_ERR_ARG, "anneal: max_proposals " + std::to_string(p->max_proposals) + " (at most 2^24 = " + std::to_string(kAnnealMaxProposals) + ")");
    if (p->trace_chain < -1 || p->trace_chain >= chains) return fail(BN_ERR_ARG, "anneal: trace_chain out of range");
    const bool tracing = p->trace_chain >= 0 && trace_out && p->trace_cap > 0;
    const int32_t n = L->n, q = tt->q;
    std::vector<uint64_t> pmask(size_t(n), 0);
    std::vector<int64_t> rows(size_t(n), 1);
    std::vector<uint16_t> edges;
    for (int32_t v = 0; v < n; ++v) {
        if (int32_t(L->parents[size_t(v)].size()) > q)
            return fail(BN_ERR_ARG, "anneal: node " + std::to_string(v) + " starts with " + std::to_string(L->parents[size_t(v)].size()) +
                                        " parents (the term table holds at most " + std::to_string(q) + ")");
        for (int32_t u : L->parents[size_t(v)]) {
            pmask[size_t(v)] |= uint64_t(1) << u;
            edges.push_back(uint16_t(u | (v << 8)));
        }
        rows[size_t(v)] = L->rows_of(v);
    }
    const int32_t stride = std::max(n * q, 1);
    bn_info_table* t = L->t;
    ON_DEVICE(t);
    hipStream_t s = t->stream;
    DeviceBuf<uint64_t> d_pmask, d_masks;
    DeviceBuf<int64_t> d_rows;
    DeviceBuf<double> d_ll0, d_ll;
    DeviceBuf<uint16_t> d_edges0, d_edges;
    DeviceBuf<AnnealRecord> d_rec;
    DeviceBuf<AnnealTrace> d_trace;
    EventOwner ev0, ev1;
    int r;
    if ((r = upload(d_pmask, pmask, s)) || (r = upload(d_rows, rows, s)) || (r = upload(d_ll0, L->ll, s)) || (r = upload(d_edges0, edges, s)) ||
        (r = dalloc(d_rec, size_t(chains))) || (r = dalloc(d_masks, size_t(chains) * size_t(n))) || (r = dalloc(d_ll, size_t(chains) * size_t(n))))
        return r;
    if (edges_out && (r = dalloc(d_edges, size_t(chains) * size_t(stride)))) return r;
    if (tracing && (r = dalloc(d_trace, size_t(p->trace_cap)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    AnnealArgs a{};
    a.terms = tt->d_terms;
    a.tab = tt->d_tab;
    a.T = tt->T;
    a.k = tt->d_k;
    a.pmask0 = d_pmask;
    a.rows0 = d_rows;
    a.ll0 = d_ll0;
    a.edges0 = d_edges0;
    a.n_edges0 = int32_t(edges.size());
    a.n = n;
    a.q = q;
    a.max_parents = std::min(q, L->max_parents);
    a.criterion = L->criterion;
    a.rule = p->rule;
    a.params0 = L->params;
    a.penalty = L->penalty;
    a.initial_temp = p->initial_temp;
    a.final_temp = p->final_temp;
    a.rate = p->decreasing_rate;
    a.boltzmann = p->boltzmann;
    a.same_state_max = p->same_state_max;
    a.max_proposals = p->max_proposals == 0 ? (1u << 20) : p->max_proposals;
    a.seed_lo = uint32_t(seed);
    a.seed_hi = uint32_t(seed >> 32);
    a.chains = chains;
    a.trace_chain = tracing ? p->trace_chain : -1;
    a.trace_cap = tracing ? p->trace_cap : 0;
    a.rec = d_rec;
    a.masks = d_masks;
    a.ll = d_ll;
    a.edges = edges_out ? d_edges.get() : nullptr;
    a.edge_stride = stride;
    a.trace = tracing ? d_trace.get() : nullptr;
    HIPCHK(hipEventRecord(ev0, s));
    if (int err = learn_launch_anneal(a, s)) return fail(BN_ERR_HIP, std::string("annealing kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev1, s));
    std::vector<AnnealRecord> rec(static_cast<size_t>(chains));
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, size_t(chains) * sizeof(AnnealRecord), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<double> score(static_cast<size_t>(chains));
    for (int32_t j = 0; j < chains; ++j) score[size_t(j)] = rec[size_t(j)].eval;
    auto more = [&]() -> int {
        if (edges_out) HIPCHK(hipMemcpyAsync(edges_out, d_edges, size_t(chains) * size_t(stride) * 2, hipMemcpyDeviceToHost, s));
        if (tracing) {
            const size_t len = std::min<size_t>(rec[size_t(p->trace_chain)].operated, p->trace_cap);
            if (len > 0) HIPCHK(hipMemcpyAsync(trace_out, d_trace, len * sizeof(AnnealTrace), hipMemcpyDeviceToHost, s));
        }
        return BN_OK;
    };
    if (int err = finish_search(L, s, score, d_masks, d_ll, masks_out, ev0, ev1, L->times.anneal_ns, winner_out, more)) return err;
    L->times.anneal_chains += chains;
    for (int32_t j = 0; j < chains; ++j) {
        const AnnealRecord& x = rec[size_t(j)];
        L->times.anneal_steps += x.proposals;
        if (eval_out) eval_out[j] = x.eval;
        if (counts_out) {
            counts_out[4 * j] = x.proposals;
            counts_out[4 * j + 1] = x.operated;
            counts_out[4 * j + 2] = x.accepted;
            counts_out[4 * j + 3] = x.flags;
        }
        if (n_edges_out) n_edges_out[j] = int32_t(x.n_edges);
    }
    return BN_OK;
}

// ---- hierarchical clustering with stochastic pruning (reference bayesian/learning/stepwise_structure_hc.hpp) ------------------------

static_assert(sizeof(bn_hc_trace) == sizeof(HcTrace) && sizeof(HcTrace) == 16, "the trace record is the ABI's");
static_assert(sizeof(HcRecord) == 40, "one record per run");

extern "C" int bn_learn_hc(bn_learner* L, bn_term_table* tt, const bn_hc_params* p, int32_t runs, uint64_t seed, const double* similarity,
                           double* score_out, uint32_t* counts_out, uint64_t* masks_out, bn_hc_trace* trace_out, int32_t* n_trace_out,
                           int32_t* winner_out) {
    if (!L || !tt || !p) return fail(BN_ERR_ARG, "null argument");
    if (tt->t != L->t) return fail(BN_ERR_ARG, "hc: the term table was built from another table than the learner's");
    if (int r = check_table_spec("hc", L, tt)) return r;
    const int32_t n = L->n, q = tt->q;
    if (n > kAnnealMaxNodes) return fail(BN_ERR_ARG, "hc: " + std::to_string(n) + " nodes (at most 64: a node has a lane)");
    if (runs < 1 || runs > kHcMaxRuns) return fail(BN_ERR_ARG, "hc: " + std::to_string(runs) + " runs (1 .. 65536)");
    if (!(std::isfinite(p->alpha) && p->alpha >= 0.0)) return fail(BN_ERR_ARG, "hc: alpha must be finite and >= 0");
    if (p->max_parents < 1 || p->max_parents > q)
        return fail(BN_ERR_ARG, "hc: max_parents " + std::to_string(p->max_parents) + " (1 .. " + std::to_string(q) + ", the term table's bound)");
    if (p->trace_run < -1 || p->trace_run >= runs) return fail(BN_ERR_ARG, "hc: trace_run out of range");
    const bool tracing = p->trace_run >= 0 && trace_out && p->trace_cap > 0;
    bn_info_table* t = L->t;
    std::vector<double> S(size_t(n) * size_t(n), 0.0);
    if (similarity) {
        for (int32_t x = 0; x < n; ++x)
            for (int32_t y = x + 1; y < n; ++y)
                if (std::memcmp(similarity + size_t(x) * n + y, similarity + size_t(y) * n + x, 8) != 0)
                    return fail(BN_ERR_ARG, "hc: similarity[" + std::to_string(x) + "][" + std::to_string(y) + "] and [" + std::to_string(y) +
                                                "][" + std::to_string(x) + "] differ in bits (the matrix must be symmetric)");
        std::copy(similarity, similarity + S.size(), S.begin());
    }
    int64_t params0 = 0;
    for (int32_t v = 0; v < n; ++v) params0 += L->family_params(v, 1);
    ON_DEVICE(t);
    hipStream_t s = t->stream;
    DeviceBuf<double> d_S, d_ll;
    DeviceBuf<uint64_t> d_masks;
    DeviceBuf<HcRecord> d_rec;
    DeviceBuf<HcTrace> d_trace;
    EventOwner ev0, ev1;
    int r;
    if (similarity) {
        if ((r = upload(d_S, S, s))) return r;
    } else {
        // the all-pairs mutual information stays where the kernel made it; the host sees it only for `average`
        if ((r = dalloc(d_S, S.size())) || (r = info_pair_mi_device(t, d_S, S))) return r;
    }
    // :171-186: the average of the initial similarities, one divide and one add per pair in row-major order
    double average = 0.0;
    const double pairs = double(int64_t(n) * (n - 1) / 2);
    for (int32_t x = 0; x < n; ++x)
        for (int32_t y = x + 1; y < n; ++y) average += (0.0 + S[size_t(x) * n + y] / 1.0) / pairs;
    if ((r = dalloc(d_rec, size_t(runs))) || (r = dalloc(d_masks, size_t(runs) * size_t(n))) || (r = dalloc(d_ll, size_t(runs) * size_t(n))))
        return r;
    if (tracing && (r = dalloc(d_trace, size_t(p->trace_cap)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    HcArgs a{};
    a.terms = tt->d_terms;
    a.tab = tt->d_tab;
    a.T = tt->T;
    a.k = tt->d_k;
    a.S = d_S;
    a.n = n;
    a.q = q;
    a.max_parents = std::min(p->max_parents, L->max_parents);
    a.criterion = L->criterion;
    a.params0 = params0;
    a.penalty = L->penalty;
    a.alpha = p->alpha;
    a.average = average;
    a.seed_lo = uint32_t(seed);
    a.seed_hi = uint32_t(seed >> 32);
    a.runs = runs;
    a.trace_run = tracing ? p->trace_run : -1;
    a.trace_cap = tracing ? p->trace_cap : 0;
    a.rec = d_rec;
    a.masks = d_masks;
    a.ll = d_ll;
    a.trace = tracing ? d_trace.get() : nullptr;
    HIPCHK(hipEventRecord(ev0, s));
    if (int err = learn_launch_hc(a, s)) return fail(BN_ERR_HIP, std::string("hierarchical-clustering kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev1, s));
    std::vector<HcRecord> rec(static_cast<size_t>(runs));
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, size_t(runs) * sizeof(HcRecord), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<double> score(static_cast<size_t>(runs));
    for (int32_t j = 0; j < runs; ++j) score[size_t(j)] = rec[size_t(j)].score;
    size_t n_trace = 0;
    auto more = [&]() -> int {
        if (tracing) {
            const HcRecord& x = rec[size_t(p->trace_run)];
            n_trace = std::min<size_t>(size_t(x.merges) + x.visits, p->trace_cap);
            if (n_trace > 0) HIPCHK(hipMemcpyAsync(trace_out, d_trace, n_trace * sizeof(HcTrace), hipMemcpyDeviceToHost, s));
        }
        return BN_OK;
    };
    if (int err = finish_search(L, s, score, d_masks, d_ll, masks_out, ev0, ev1, L->times.hc_ns, winner_out, more)) return err;
    L->times.hc_runs += runs;
    for (int32_t j = 0; j < runs; ++j) {
        const HcRecord& x = rec[size_t(j)];
        L->times.hc_merges += x.merges;
        if (score_out) score_out[j] = x.score;
        if (counts_out) {
            uint32_t* c = counts_out + 6 * size_t(j);
            c[0] = x.merges; c[1] = x.tried; c[2] = x.kept; c[3] = x.pruned; c[4] = x.pairs_kept; c[5] = x.flags;
        }
    }
    if (n_trace_out) *n_trace_out = int32_t(n_trace);
    return BN_OK;
}

// ---- tabu hill climbing: steepest descent over add, delete and reverse moves, a tabu list, perturbed restarts -------------------------

static_assert(sizeof(bn_climb_trace) == sizeof(ClimbTrace) && sizeof(ClimbTrace) == 32, "the trace record is the ABI's");
static_assert(sizeof(ClimbRecord) == 32, "one record per run");

extern "C" int bn_learn_climb(bn_learner* L, bn_term_table* tt, const bn_climb_params* p, int32_t runs, uint64_t seed, double* score_out,
                              uint32_t* counts_out, uint64_t* masks_out, bn_climb_trace* trace_out, int32_t* winner_out) {
    if (!L || !tt || !p) return fail(BN_ERR_ARG, "null argument");
    const int32_t n = L->n, q = tt->q;
    if (n > kAnnealMaxNodes) return fail(BN_ERR_ARG, "climb: " + std::to_string(n) + " nodes (at most 64: a node has a lane)");
    if (tt->t != L->t) return fail(BN_ERR_ARG, "climb: the term table was built from another table than the learner's");
    if (int r = check_table_spec("climb", L, tt)) return r;
    if (runs < 1 || runs > kClimbMaxRuns) return fail(BN_ERR_ARG, "climb: " + std::to_string(runs) + " runs (1 .. 65536)");
    if (p->tabu_len < 0 || p->tabu_len > kClimbMaxTabu) return fail(BN_ERR_ARG, "climb: tabu_len " + std::to_string(p->tabu_len) + " (0 .. 64)");
    if (p->max_steps > kClimbMaxSteps)
        return fail(BN_ERR_ARG, "climb: max_steps " + std::to_string(p->max_steps) + " (at most 2^20 = " + std::to_string(kClimbMaxSteps) + ")");
    if (p->perturb > kClimbMaxPerturb)
        return fail(BN_ERR_ARG, "climb: perturb " + std::to_string(p->perturb) + " (at most 2^16 = " + std::to_string(kClimbMaxPerturb) + ")");
    if (p->max_parents < 1) return fail(BN_ERR_ARG, "climb: max_parents " + std::to_string(p->max_parents) + " (at least 1)");
    if (p->trace_run < -1 || p->trace_run >= runs) return fail(BN_ERR_ARG, "climb: trace_run out of range");
    const bool tracing = p->trace_run >= 0 && trace_out && p->trace_cap > 0;
    std::vector<uint64_t> pmask(size_t(n), 0);
    std::vector<int64_t> rows(size_t(n), 1);
    for (int32_t v = 0; v < n; ++v) {
        if (int32_t(L->parents[size_t(v)].size()) > q)
            return fail(BN_ERR_ARG, "climb: node " + std::to_string(v) + " starts with " + std::to_string(L->parents[size_t(v)].size()) +
                                        " parents (the term table holds at most " + std::to_string(q) + ")");
        for (int32_t u : L->parents[size_t(v)]) pmask[size_t(v)] |= uint64_t(1) << u;
        rows[size_t(v)] = L->rows_of(v);
    }
    bn_info_table* t = L->t;
    ON_DEVICE(t);
    hipStream_t s = t->stream;
    DeviceBuf<uint64_t> d_pmask, d_masks;
    DeviceBuf<int64_t> d_rows;
    DeviceBuf<double> d_ll0, d_ll;
    DeviceBuf<ClimbRecord> d_rec;
    DeviceBuf<ClimbTrace> d_trace;
    EventOwner ev0, ev1;
    int r;
    if ((r = upload(d_pmask, pmask, s)) || (r = upload(d_rows, rows, s)) || (r = upload(d_ll0, L->ll, s)) || (r = dalloc(d_rec, size_t(runs))) ||
        (r = dalloc(d_masks, size_t(runs) * size_t(n))) || (r = dalloc(d_ll, size_t(runs) * size_t(n))))
        return r;
    if (tracing && (r = dalloc(d_trace, size_t(p->trace_cap)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    ClimbArgs a{};
    a.terms = tt->d_terms;
    a.tab = tt->d_tab;
    a.T = tt->T;
    a.k = tt->d_k;
    a.pmask0 = d_pmask;
    a.rows0 = d_rows;
    a.ll0 = d_ll0;
    a.n = n;
    a.q = q;
    a.max_parents = std::min(p->max_parents, std::min(q, L->max_parents));
    a.criterion = L->criterion;
    a.params0 = L->params;
    a.penalty = L->penalty;
    a.tabu_len = p->tabu_len;
    a.max_worse = p->max_worse;
    a.max_steps = p->max_steps == 0 ? (1u << 16) : p->max_steps;
    a.perturb = p->perturb;
    a.seed_lo = uint32_t(seed);
    a.seed_hi = uint32_t(seed >> 32);
    a.runs = runs;
    a.trace_run = tracing ? p->trace_run : -1;
    a.trace_cap = tracing ? p->trace_cap : 0;
    a.rec = d_rec;
    a.masks = d_masks;
    a.ll = d_ll;
    a.trace = tracing ? d_trace.get() : nullptr;
    HIPCHK(hipEventRecord(ev0, s));
    if (int err = learn_launch_climb(a, s)) return fail(BN_ERR_HIP, std::string("hill-climbing kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev1, s));
    std::vector<ClimbRecord> rec(static_cast<size_t>(runs));
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, size_t(runs) * sizeof(ClimbRecord), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<double> score(static_cast<size_t>(runs));
    for (int32_t j = 0; j < runs; ++j) score[size_t(j)] = rec[size_t(j)].best_eval;
    auto more = [&]() -> int {
        if (tracing) {
            const size_t len = std::min<size_t>(rec[size_t(p->trace_run)].steps, p->trace_cap);
            if (len > 0) HIPCHK(hipMemcpyAsync(trace_out, d_trace, len * sizeof(ClimbTrace), hipMemcpyDeviceToHost, s));
        }
        return BN_OK;
    };
    if (int err = finish_search(L, s, score, d_masks, d_ll, masks_out, ev0, ev1, L->times.climb_ns, winner_out, more)) return err;
    L->times.climb_runs += runs;
    for (int32_t j = 0; j < runs; ++j) {
        const ClimbRecord& x = rec[size_t(j)];
        L->times.climb_steps += x.steps;
        if (score_out) score_out[j] = x.best_eval;
        if (counts_out) {
            uint32_t* c = counts_out + 6 * size_t(j);
            c[0] = x.steps; c[1] = x.improving; c[2] = x.perturbed; c[3] = x.best_step; c[4] = x.flags; c[5] = x.tabu_legal;
        }
    }
    return BN_OK;
}
