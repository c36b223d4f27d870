// bn_learn_search.cpp -- the device-resident structure searches over a term table (bn_learn_terms.cpp): bn_learn_anneal runs the
// reference's simulated_annealing.hpp as many chains (bn_learn_anneal.hip), bn_learn_hc its stepwise_structure_hc.hpp as many runs
// (bn_learn_hc.hip), bn_learn_climb tabu hill climbing as many runs (bn_learn_climb.hip).  All begin and end alike (SearchRun): the
// same checks, buffers and arguments, and the run with the smallest score becomes the learner's graph.  bn_learn_optimal is the
// exact search (bn_learn_optimal.hip): no runs, one graph, installed in the learner by the same tail.
#include "bn_learn_internal.hpp"
#include "bn_learn_anneal.hpp"
#include "bn_learn_climb.hpp"
#include "bn_learn_hc.hpp"
#include "bn_learn_optimal_plan.hpp"

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

// What a search is called in messages, the sizes of its per-run record and its trace entry, and where its kernel time and run
// count are kept.
struct SearchKind {
    const char *who, *runs_word, *trace_arg, *kernel;
    size_t rec_bytes, trace_bytes;
    double LearnTimes::*ns;
    int64_t LearnTimes::*runs;
};
constexpr SearchKind kAnneal{"anneal", "chains", "trace_chain", "annealing kernel", sizeof(AnnealRecord), sizeof(AnnealTrace),
                             &LearnTimes::anneal_ns, &LearnTimes::anneal_chains};
constexpr SearchKind kHc{"hc", "runs", "trace_run", "hierarchical-clustering kernel", sizeof(HcRecord), sizeof(HcTrace), &LearnTimes::hc_ns,
                         &LearnTimes::hc_runs};
constexpr SearchKind kClimb{"climb", "runs", "trace_run", "hill-climbing kernel", sizeof(ClimbRecord), sizeof(ClimbTrace), &LearnTimes::climb_ns,
                            &LearnTimes::climb_runs};

// The frame of one call of a search: open() makes the checks all three make, prepare() puts everything but the search's own
// arguments on the device, launch() runs the kernel between the event pair and brings the per-run records back, finish() makes the
// winner the learner's graph.  Between them an entry checks its own parameters, fills its own arguments and maps its records to its
// outputs.
class SearchRun {
public:
    explicit SearchRun(const SearchKind& kind) : kind_(kind) {}

    bn_learner* L = nullptr;
    bn_term_table* tt = nullptr;
    int32_t n = 0, q = 0, runs = 0;
    hipStream_t s = nullptr;
    size_t n_trace = 0;   // the trace records finish() copied out

    // in this order: null, nodes, "another table", spec, runs
    int open(bn_learner* L_, bn_term_table* tt_, const void* p, int32_t runs_) {
        if (!L_ || !tt_ || !p) return fail(BN_ERR_ARG, "null argument");
        L = L_, tt = tt_, n = L->n, q = tt->q, runs = runs_;
        if (n > kTermMaxNodes) return fail(BN_ERR_ARG, who() + std::to_string(n) + " nodes (at most 64: a node has a lane)");
        if (tt->t != L->t) return fail(BN_ERR_ARG, who() + "the term table was built from another table than the learner's");
        if (int r = check_table_spec(kind_.who, L, tt)) return r;
        if (runs < 1 || runs > kSearchMaxRuns) return fail(BN_ERR_ARG, who() + std::to_string(runs) + " " + kind_.runs_word + " (1 .. 65536)");
        return BN_OK;
    }

    // The trace range check; then, on the learner's device: the learner's graph as the starting graph (where `start` is given; a node
    // with more parents than the table holds is refused), a record per run, the masks and terms of every run, the trace where one
    // is asked for, the event pair -- and the frame's part of the arguments.
    int prepare(SearchArgs& a, StartGraph* start, int32_t max_parents, int64_t params0, uint64_t seed, int32_t trace_run, uint32_t trace_cap,
                void* trace_out) {
        if (trace_run < -1 || trace_run >= runs) return fail(BN_ERR_ARG, who() + kind_.trace_arg + " out of range");
        const bool tracing = trace_run >= 0 && trace_out && trace_cap > 0;
        trace_run_ = tracing ? trace_run : -1;
        trace_cap_ = tracing ? trace_cap : 0;
        trace_out_ = trace_out;
        std::vector<uint64_t> pmask(size_t(n), 0);
        std::vector<int64_t> rows(size_t(n), 1);
        for (int32_t v = 0; start && v < n; ++v) {
            if (int32_t(L->parents[size_t(v)].size()) > q)
                return fail(BN_ERR_ARG, who() + "node " + std::to_string(v) + " starts with " + std::to_string(L->parents[size_t(v)].size()) +
                                            " parents (the term table holds at most " + std::to_string(q) + ")");
            for (int32_t u : L->parents[size_t(v)]) pmask[size_t(v)] |= uint64_t(1) << u;
            rows[size_t(v)] = L->rows_of(v);
        }
        HIPCHK(guard_.enter(L->t->device));
        s = L->t->stream;
        int r;
        if (start) {
            if ((r = upload(d_pmask_, pmask, s)) || (r = upload(d_rows_, rows, s)) || (r = upload(d_ll0_, L->ll, s))) return r;
            *start = StartGraph{d_pmask_, d_rows_, d_ll0_};
        }
        if ((r = dalloc(d_rec_, size_t(runs) * kind_.rec_bytes)) || (r = dalloc(d_masks_, size_t(runs) * size_t(n))) || (r = dalloc(d_ll_, size_t(runs) * size_t(n))))
            return r;
        if (tracing && (r = dalloc(d_trace_, size_t(trace_cap) * kind_.trace_bytes))) return r;
        HIPCHK(hipEventCreate(ev0_.put()));
        HIPCHK(hipEventCreate(ev1_.put()));
        a = SearchArgs{tt->d_terms, tt->d_tab, tt->T, tt->d_k, n, q, max_parents, L->criterion, params0, L->penalty, uint32_t(seed),
                       uint32_t(seed >> 32), runs, trace_run_, trace_cap_, d_masks_, d_ll_};   // (in the struct's order)
        return BN_OK;
    }
    template <class Rec>
    Rec* d_rec() { return reinterpret_cast<Rec*>(d_rec_.get()); }
    template <class Trace>
    Trace* d_trace() { return trace_run_ >= 0 ? reinterpret_cast<Trace*>(d_trace_.get()) : nullptr; }

    // fn(stream): the search's launch function
    template <class Fn>
    int launch(Fn fn) {
        HIPCHK(hipEventRecord(ev0_, s));
        if (int err = fn(s)) return fail(BN_ERR_HIP, std::string(kind_.kernel) + ": " + hipGetErrorString(hipError_t(err)));
        HIPCHK(hipEventRecord(ev1_, s));
        rec_.resize(size_t(runs) * kind_.rec_bytes);
        HIPCHK(hipMemcpyAsync(rec_.data(), d_rec_, rec_.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return BN_OK;
    }
    template <class Rec>
    Rec rec(int32_t j) const {
        Rec x;
        std::memcpy(&x, rec_.data() + size_t(j) * sizeof(Rec), sizeof(Rec));
        return x;
    }

    // The tail, entered with the records on the host.  score_of(j): run j's score; the winner is the run of the smallest, strictly
    // (ties stay with the lowest index).  Its row of the masks and terms and, where asked for, every run's masks are downloaded
    // together with the first trace_len_of(traced run) entries of the trace (at most its capacity) and what extra() enqueues; the kernel's
    // time and the runs are added to the learner's counters; the winner becomes the learner's graph.
    template <class ScoreOf, class TraceLenOf, class Extra>
    int finish(ScoreOf score_of, TraceLenOf trace_len_of, Extra extra, uint64_t* masks_out, int32_t* winner_out) {
        int32_t winner = 0;
        for (int32_t j = 0; j < runs; ++j)
            if (score_of(j) < score_of(winner)) winner = j;
        const size_t nn = size_t(n);
        std::vector<uint64_t> win_mask(nn);
        std::vector<double> win_ll(nn);
        HIPCHK(hipMemcpyAsync(win_mask.data(), d_masks_.get() + size_t(winner) * nn, nn * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(win_ll.data(), d_ll_.get() + size_t(winner) * nn, nn * 8, hipMemcpyDeviceToHost, s));
        if (masks_out) HIPCHK(hipMemcpyAsync(masks_out, d_masks_, size_t(runs) * nn * 8, hipMemcpyDeviceToHost, s));
        if (trace_run_ >= 0) {
            n_trace = std::min<size_t>(trace_len_of(trace_run_), trace_cap_);
            if (n_trace > 0) HIPCHK(hipMemcpyAsync(trace_out_, d_trace_, n_trace * kind_.trace_bytes, hipMemcpyDeviceToHost, s));
        }
        if (int r = extra()) return r;
        HIPCHK(hipStreamSynchronize(s));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ev0_, ev1_));
        L->times.*kind_.ns += double(ms) * 1e6;
        L->times.*kind_.runs += runs;
        if (winner_out) *winner_out = winner;
        adopt_winner(L, win_mask, win_ll, score_of(winner));
        return BN_OK;
    }

private:
    std::string who() const { return std::string(kind_.who) + ": "; }

    const SearchKind& kind_;
    DeviceGuard guard_;   // (before the buffers: they are freed on the learner's device)
    DeviceBuf<uint64_t> d_pmask_, d_masks_;
    DeviceBuf<int64_t> d_rows_;
    DeviceBuf<double> d_ll0_, d_ll_;
    DeviceBuf<unsigned char> d_rec_, d_trace_;
    EventOwner ev0_, ev1_;
    std::vector<unsigned char> rec_;
    int32_t trace_run_ = -1;
    uint32_t trace_cap_ = 0;
    void* trace_out_ = nullptr;
};

}  // namespace

static_assert(sizeof(bn_anneal_trace) == sizeof(AnnealTrace) && sizeof(AnnealTrace) == 16, "the trace record is the ABI's");
static_assert(sizeof(AnnealRecord) == 32, "one record per chain");

extern "C" int bn_learn_anneal(bn_learner* L, bn_term_table* tt, const bn_anneal_params* p, int32_t chains, uint64_t seed, double* eval_out,
                               uint32_t* counts_out, uint64_t* masks_out, int32_t* n_edges_out, uint16_t* edges_out,
                               bn_anneal_trace* trace_out, int32_t* winner_out) {
    SearchRun run(kAnneal);
    if (int r = run.open(L, tt, p, chains)) return r;
    auto positive = [](double x) { return std::isfinite(x) && x > 0.0; };
    if (!positive(p->initial_temp) || !positive(p->final_temp)) return fail(BN_ERR_ARG, "anneal: the temperatures must be finite and positive");
    if (!(p->decreasing_rate > 0.0 && p->decreasing_rate < 1.0)) return fail(BN_ERR_ARG, "anneal: decreasing_rate must be in (0, 1)");
    if (!positive(p->boltzmann)) return fail(BN_ERR_ARG, "anneal: boltzmann must be finite and positive");
    if (p->rule != 0 && p->rule != 1) return fail(BN_ERR_ARG, "anneal: rule 0 (the reference's) or 1 (Metropolis)");
    if (p->max_proposals > kAnnealMaxProposals)
        return fail(BN_ERR_ARG, "anneal: max_proposals " + std::to_string(p->max_proposals) + " (at most 2^24 = " + std::to_string(kAnnealMaxProposals) + ")");
    const int32_t n = run.n, q = run.q;
    AnnealArgs a{};
    if (int r = run.prepare(a, &a, std::min(q, L->max_parents), L->params, seed, p->trace_chain, p->trace_cap, trace_out)) return r;
    // the ordered edge list a chain starts from, and where asked for the lists the chains end with
    std::vector<uint16_t> edges;
    for (int32_t v = 0; v < n; ++v)
        for (int32_t u : L->parents[size_t(v)]) edges.push_back(uint16_t(u | (v << 8)));
    const int32_t stride = std::max(n * q, 1);
    DeviceBuf<uint16_t> d_edges0, d_edges;
    if (int r = upload(d_edges0, edges, run.s)) return r;
    if (edges_out)
        if (int r = dalloc(d_edges, size_t(chains) * size_t(stride))) return r;
    a.edges0 = d_edges0;
    a.n_edges0 = int32_t(edges.size());
    a.rule = p->rule;
    a.initial_temp = p->initial_temp;
    a.final_temp = p->final_temp;
    a.rate = p->decreasing_rate;
    a.boltzmann = p->boltzmann;
    a.same_state_max = p->same_state_max;
    a.max_proposals = p->max_proposals == 0 ? (1u << 20) : p->max_proposals;
    a.rec = run.d_rec<AnnealRecord>();
    a.edges = edges_out ? d_edges.get() : nullptr;
    a.edge_stride = stride;
    a.trace = run.d_trace<AnnealTrace>();
    if (int r = run.launch([&](hipStream_t s) { return learn_launch_anneal(a, s); })) return r;
    auto rec = [&](int32_t j) { return run.rec<AnnealRecord>(j); };
    auto edges_back = [&]() -> int {
        if (edges_out) HIPCHK(hipMemcpyAsync(edges_out, d_edges, size_t(chains) * size_t(stride) * 2, hipMemcpyDeviceToHost, run.s));
        return BN_OK;
    };
    if (int r = run.finish([&](int32_t j) { return rec(j).eval; }, [&](int32_t j) { return rec(j).operated; }, edges_back, masks_out, winner_out))
        return r;
    for (int32_t j = 0; j < chains; ++j) {
        const AnnealRecord x = rec(j);
        L->times.anneal_steps += x.proposals;
        if (eval_out) eval_out[j] = x.eval;
        if (counts_out) {
            uint32_t* c = counts_out + 4 * size_t(j);
            c[0] = x.proposals; c[1] = x.operated; c[2] = x.accepted; c[3] = x.flags;
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
    SearchRun run(kHc);
    if (int r = run.open(L, tt, p, runs)) return r;
    const int32_t n = run.n, q = run.q;
    if (!(std::isfinite(p->alpha) && p->alpha >= 0.0)) return fail(BN_ERR_ARG, "hc: alpha must be finite and >= 0");
    if (p->max_parents < 1 || p->max_parents > q)
        return fail(BN_ERR_ARG, "hc: max_parents " + std::to_string(p->max_parents) + " (1 .. " + std::to_string(q) + ", the term table's bound)");
    std::vector<double> S(size_t(n) * size_t(n), 0.0);
    if (similarity) {
        for (int32_t x = 0; x < n; ++x)
            for (int32_t y = x + 1; y < n; ++y)
                if (std::memcmp(similarity + size_t(x) * n + y, similarity + size_t(y) * n + x, 8) != 0)
                    return fail(BN_ERR_ARG, "hc: similarity[" + std::to_string(x) + "][" + std::to_string(y) + "] and [" + std::to_string(y) +
                                                "][" + std::to_string(x) + "] differ in bits (the matrix must be symmetric)");
        std::copy(similarity, similarity + S.size(), S.begin());
    }
    int64_t params0 = 0;   // of the empty graph, where a run starts
    for (int32_t v = 0; v < n; ++v) params0 += L->family_params(v, 1);
    HcArgs a{};
    if (int r = run.prepare(a, nullptr, std::min(p->max_parents, L->max_parents), params0, seed, p->trace_run, p->trace_cap, trace_out))
        return r;
    DeviceBuf<double> d_S;
    if (similarity) {
        if (int r = upload(d_S, S, run.s)) return r;
    } else {
        // the all-pairs mutual information stays where the kernel made it; the host sees it only for `average`
        int r;
        if ((r = dalloc(d_S, S.size())) || (r = info_pair_mi_device(L->t, d_S, S))) return r;
    }
    // :171-186: the average of the initial similarities, one divide and one add per pair in row-major order
    double average = 0.0;
    const double pairs = double(int64_t(n) * (n - 1) / 2);
    for (int32_t x = 0; x < n; ++x)
        for (int32_t y = x + 1; y < n; ++y) average += (0.0 + S[size_t(x) * n + y] / 1.0) / pairs;
    a.S = d_S;
    a.alpha = p->alpha;
    a.average = average;
    a.rec = run.d_rec<HcRecord>();
    a.trace = run.d_trace<HcTrace>();
    if (int r = run.launch([&](hipStream_t s) { return learn_launch_hc(a, s); })) return r;
    auto rec = [&](int32_t j) { return run.rec<HcRecord>(j); };
    auto trace_len = [&](int32_t j) { return size_t(rec(j).merges) + rec(j).visits; };
    if (int r = run.finish([&](int32_t j) { return rec(j).score; }, trace_len, [] { return BN_OK; }, masks_out, winner_out)) return r;
    for (int32_t j = 0; j < runs; ++j) {
        const HcRecord x = rec(j);
        L->times.hc_merges += x.merges;
        if (score_out) score_out[j] = x.score;
        if (counts_out) {
            uint32_t* c = counts_out + 6 * size_t(j);
            c[0] = x.merges; c[1] = x.tried; c[2] = x.kept; c[3] = x.pruned; c[4] = x.pairs_kept; c[5] = x.flags;
        }
    }
    if (n_trace_out) *n_trace_out = int32_t(run.n_trace);
    return BN_OK;
}

// ---- tabu hill climbing: steepest descent over add, delete and reverse moves, a tabu list, perturbed restarts -------------------------

static_assert(sizeof(bn_climb_trace) == sizeof(ClimbTrace) && sizeof(ClimbTrace) == 32, "the trace record is the ABI's");
static_assert(sizeof(ClimbRecord) == 32, "one record per run");

extern "C" int bn_learn_climb(bn_learner* L, bn_term_table* tt, const bn_climb_params* p, int32_t runs, uint64_t seed, double* score_out,
                              uint32_t* counts_out, uint64_t* masks_out, bn_climb_trace* trace_out, int32_t* winner_out) {
    SearchRun run(kClimb);
    if (int r = run.open(L, tt, p, runs)) return r;
    if (p->tabu_len < 0 || p->tabu_len > kClimbMaxTabu) return fail(BN_ERR_ARG, "climb: tabu_len " + std::to_string(p->tabu_len) + " (0 .. 64)");
    if (p->max_steps > kClimbMaxSteps)
        return fail(BN_ERR_ARG, "climb: max_steps " + std::to_string(p->max_steps) + " (at most 2^20 = " + std::to_string(kClimbMaxSteps) + ")");
    if (p->perturb > kClimbMaxPerturb)
        return fail(BN_ERR_ARG, "climb: perturb " + std::to_string(p->perturb) + " (at most 2^16 = " + std::to_string(kClimbMaxPerturb) + ")");
    if (p->max_parents < 1) return fail(BN_ERR_ARG, "climb: max_parents " + std::to_string(p->max_parents) + " (at least 1)");
    ClimbArgs a{};
    if (int r = run.prepare(a, &a, std::min(p->max_parents, std::min(run.q, L->max_parents)), L->params, seed, p->trace_run, p->trace_cap,
                            trace_out))
        return r;
    a.tabu_len = p->tabu_len;
    a.max_worse = p->max_worse;
    a.max_steps = p->max_steps == 0 ? (1u << 16) : p->max_steps;
    a.perturb = p->perturb;
    a.rec = run.d_rec<ClimbRecord>();
    a.trace = run.d_trace<ClimbTrace>();
    if (int r = run.launch([&](hipStream_t s) { return learn_launch_climb(a, s); })) return r;
    auto rec = [&](int32_t j) { return run.rec<ClimbRecord>(j); };
    if (int r = run.finish([&](int32_t j) { return rec(j).best_eval; }, [&](int32_t j) { return rec(j).steps; }, [] { return BN_OK; }, masks_out,
                           winner_out))
        return r;
    for (int32_t j = 0; j < runs; ++j) {
        const ClimbRecord x = rec(j);
        L->times.climb_steps += x.steps;
        if (score_out) score_out[j] = x.best_eval;
        if (counts_out) {
            uint32_t* c = counts_out + 6 * size_t(j);
            c[0] = x.steps; c[1] = x.improving; c[2] = x.perturbed; c[3] = x.best_step; c[4] = x.flags; c[5] = x.tabu_legal;
        }
    }
    return BN_OK;
}

// ---- the exact search: the DAG of smallest cost by dynamic programming over node subsets (Silander & Myllymaki 2006) --------------

static_assert(sizeof(bn_optimal_params) == 24, "the parameter block is the ABI's");

extern "C" int bn_learn_optimal(bn_learner* L, bn_term_table* tt, const bn_optimal_params* p, double* value_out, int32_t* order_out,
                                uint64_t* masks_out) {
    if (!L || !tt || !p) return fail(BN_ERR_ARG, "null argument");
    if (tt->t != L->t) return fail(BN_ERR_ARG, "optimal: the term table was built from another table than the learner's");
    if (int r = check_table_spec("optimal", L, tt)) return r;
    OptimalPlan plan;
    if (int r = plan_optimal(L->n, p->max_parents, tt->q, L->max_parents, p->allowed, plan)) return r;
    const int32_t n = L->n;
    const size_t nn = size_t(n);
    std::vector<uint64_t> allowed(nn, ~uint64_t(0));
    if (p->allowed) std::copy(p->allowed, p->allowed + n, allowed.begin());
    DeviceGuard guard;   // (before the buffers: they are freed on the learner's device)
    HIPCHK(guard.enter(L->t->device));
    hipStream_t s = L->t->stream;
    DeviceBuf<double> d_cost, d_R, d_ll, d_value;
    DeviceBuf<uint32_t> d_rank;
    DeviceBuf<uint8_t> d_sink;
    DeviceBuf<uint64_t> d_allowed, d_masks;
    DeviceBuf<int32_t> d_order;
    EventOwner ev[4];
    int r;
    if ((r = dalloc(d_cost, size_t(plan.cells))) || (r = dalloc(d_rank, size_t(plan.cells))) || (r = dalloc(d_R, size_t(plan.sets))) ||
        (r = dalloc(d_sink, size_t(plan.sets))) || (r = dalloc(d_ll, nn)) || (r = dalloc(d_value, 1)) || (r = dalloc(d_masks, nn)) ||
        (r = dalloc(d_order, nn)) || (r = upload(d_allowed, allowed, s)))
        return r;
    for (EventOwner& e : ev) HIPCHK(hipEventCreate(e.put()));
    auto launched = [](const char* what, int err) {
        return err ? fail(BN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(hipError_t(err))) : BN_OK;
    };
    // step 1: the best parent set inside every candidate set, one launch per pass of the schedule
    HIPCHK(hipEventRecord(ev[0], s));
    OptimalBpsArgs b{tt->d_terms, tt->d_tab, tt->T, tt->d_k, d_allowed, n, tt->q, plan.mp, L->criterion < 2 ? 1 : 0, L->penalty, d_cost, d_rank, {}};
    for (const OptimalPass& pass : plan.passes) {
        b.pass = pass;
        if ((r = launched("best-parent-set kernel", learn_launch_optimal_bps(b, s)))) return r;
    }
    HIPCHK(hipEventRecord(ev[1], s));
    // step 2: the best sink of every set, level by level on the stream (R[empty] = +0.0)
    HIPCHK(hipMemsetAsync(d_R, 0, sizeof(double), s));
    for (int32_t level = 1; level <= n; ++level)
        if ((r = launched("best-sink kernel", learn_launch_optimal_sink(OptimalSinkArgs{d_cost, d_R, d_sink, n, level}, s)))) return r;
    HIPCHK(hipEventRecord(ev[2], s));
    // step 3: the walk back from V
    if ((r = launched("backtracking kernel",
                      learn_launch_optimal_back(OptimalBackArgs{tt->d_terms, tt->d_tab, tt->T, d_rank, d_R, d_sink, n, tt->q, d_order, d_masks, d_ll, d_value}, s))))
        return r;
    HIPCHK(hipEventRecord(ev[3], s));
    std::vector<uint64_t> win_mask(nn);
    std::vector<double> win_ll(nn);
    std::vector<int32_t> order(nn);
    double value = 0.0;
    HIPCHK(hipMemcpyAsync(win_mask.data(), d_masks, nn * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(win_ll.data(), d_ll, nn * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(order.data(), d_order, nn * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&value, d_value, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms_all = 0.0f, ms_bps = 0.0f, ms_sink = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms_all, ev[0], ev[3]));
    HIPCHK(hipEventElapsedTime(&ms_bps, ev[0], ev[1]));
    HIPCHK(hipEventElapsedTime(&ms_sink, ev[1], ev[2]));
    L->times.optimal_ns += double(ms_all) * 1e6;
    L->times.optimal_bps_ns += double(ms_bps) * 1e6;
    L->times.optimal_sink_ns += double(ms_sink) * 1e6;
    L->times.optimal_cells = plan.cells;
    L->times.optimal_bytes = plan.bytes;
    adopt_winner(L, win_mask, win_ll, 0.0);
    L->score = L->score_with(-1, 0.0, L->params);   // the learner's own arithmetic on the graph: may differ from `value` in the last bits
    if (value_out) *value_out = value;
    if (order_out) std::copy(order.begin(), order.end(), order_out);
    if (masks_out) std::copy(win_mask.begin(), win_mask.end(), masks_out);
    return BN_OK;
}
