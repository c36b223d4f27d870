// bn_learn.cpp -- the learner object of structure learning (include/bn_mi355x.h, bn_learn_create .. bn_learn_terms), reference
// bayesian/learning/greedy.hpp and k2_algorithm.hpp.  bn_learner holds a graph, every node's family term and the score;
// bn_learn_try_parents is the reference's inner loop for one child with one device pass per ACCEPTED edge (plus one) instead of one
// fit and one score of the whole graph per candidate.  The batches run in bn_learn_batch.cpp; shared declarations: bn_learn_internal.hpp.
#include "bn_learn_internal.hpp"

static int learn_create(bn_info_table* t, const int32_t* in_ptr, const int32_t* in_idx, int32_t criterion, const bn_score_spec& spec,
                        int32_t max_parents, bn_learner** out);

extern "C" int bn_learn_create(bn_info_table* t, const int32_t* in_ptr, const int32_t* in_idx, int32_t criterion, int32_t max_parents,
                               bn_learner** out) {
    if (!out) return fail(BN_ERR_ARG, "null argument");
    *out = nullptr;
    if (!t || !in_ptr) return fail(BN_ERR_ARG, "null argument");
    if (criterion != 0 && criterion != 1) return fail(BN_ERR_ARG, "criterion: 0 AIC, 1 MDL");
    return learn_create(t, in_ptr, in_idx, criterion, kLogLikSpec, max_parents, out);
}

extern "C" int bn_learn_create_spec(bn_info_table* t, const int32_t* in_ptr, const int32_t* in_idx, int32_t criterion, const bn_score_spec* spec_in,
                                    int32_t max_parents, bn_learner** out) {
    if (!out) return fail(BN_ERR_ARG, "null argument");
    *out = nullptr;
    if (criterion < 0 || criterion > 3) return fail(BN_ERR_ARG, "criterion: 0 AIC, 1 MDL, 2 BDeu, 3 K2");
    bn_score_spec spec;
    if (int r = check_spec(spec_in, spec)) return r;
    if (spec.kind != (criterion >= 2 ? criterion : 0))
        return fail(BN_ERR_ARG, "criterion " + std::to_string(criterion) + " takes a score spec of kind " + std::to_string(criterion >= 2 ? criterion : 0) +
                                    ", not " + std::to_string(spec.kind) + (criterion >= 2 && !spec_in ? " (no spec given)" : ""));
    return learn_create(t, in_ptr, in_idx, criterion, spec, max_parents, out);
}

static int learn_create(bn_info_table* t, const int32_t* in_ptr, const int32_t* in_idx, int32_t criterion, const bn_score_spec& spec,
                        int32_t max_parents, bn_learner** out) {
    if (!t || !in_ptr) return fail(BN_ERR_ARG, "null argument");
    if (max_parents < 0 || max_parents > kLearnMaxParents) return fail(BN_ERR_ARG, "max_parents must be in 0..16");
    const int32_t n = t->n;
    if (in_ptr[0] != 0) return fail(BN_ERR_ARG, "in_ptr must start at 0");
    for (int32_t v = 0; v < n; ++v)
        if (in_ptr[v + 1] < in_ptr[v]) return fail(BN_ERR_ARG, "in_ptr must not decrease");
    if (in_ptr[n] > 0 && !in_idx) return fail(BN_ERR_ARG, "null argument");
    std::unique_ptr<bn_learner> L(new (std::nothrow) bn_learner);
    if (!L) return fail(BN_ERR_ALLOC, "host allocation failed");
    L->t = t;
    L->n = n;
    L->criterion = criterion;
    L->spec = spec;
    L->max_parents = max_parents;
    L->penalty = criterion == 1 ? std::log2(t->Nd) / 2 : 1.0;
    L->parents.resize(size_t(n));
    L->children.resize(size_t(n));
    L->listed.assign(size_t(n), 0);
    for (int32_t v = 0; v < n; ++v) {
        std::vector<int32_t>& p = L->parents[size_t(v)];
        p.assign(in_idx + in_ptr[v], in_idx + in_ptr[v + 1]);
        for (int32_t u : p)
            if (u < 0 || u >= n || u == v) return fail(BN_ERR_ARG, "node " + std::to_string(v) + ": parent id " + std::to_string(u) + " out of range or the node itself");
        std::sort(p.begin(), p.end());
        if (std::adjacent_find(p.begin(), p.end()) != p.end()) return fail(BN_ERR_ARG, "node " + std::to_string(v) + ": a parent listed twice");
        for (int32_t u : p) L->children[size_t(u)].push_back(v);
    }
    {   // acyclic: every node leaves a queue of nodes without unvisited parents
        std::vector<int32_t> left(static_cast<size_t>(n)), queue;
        for (int32_t v = 0; v < n; ++v)
            if ((left[size_t(v)] = int32_t(L->parents[size_t(v)].size())) == 0) queue.push_back(v);
        for (size_t i = 0; i < queue.size(); ++i)
            for (int32_t c : L->children[size_t(queue[i])])
                if (--left[size_t(c)] == 0) queue.push_back(c);
        if (int32_t(queue.size()) != n) return fail(BN_ERR_ARG, "the starting graph has a cycle");
    }
    std::vector<GroupIn> groups(static_cast<size_t>(n));
    for (int32_t v = 0; v < n; ++v) groups[size_t(v)] = GroupIn{v, L->parents[size_t(v)].data(), int32_t(L->parents[size_t(v)].size()), nullptr, 0};
    L->ll.assign(size_t(n), 0.0);
    if (int r = run_groups(t, spec, groups, L->ll.data(), nullptr, &L->times)) return r;   // (names the node as "group v" when over a limit)
    for (int32_t v = 0; v < n; ++v) L->params += L->family_params(v, L->rows_of(v));
    L->score = L->score_with(-1, 0.0, L->params);
    *out = L.release();
    return BN_OK;
}

extern "C" void bn_learn_destroy(bn_learner* L) { delete L; }

extern "C" int bn_learn_try_parents(bn_learner* L, int32_t child, int32_t n_cand, const int32_t* cand, uint8_t* accepted_out) {
    if (!L || n_cand < 0 || (n_cand > 0 && (!cand || !accepted_out))) return fail(BN_ERR_ARG, "null argument or n_cand < 0");
    const int32_t n = L->n;
    if (child < 0 || child >= n) return fail(BN_ERR_ARG, "child id " + std::to_string(child) + " out of range");
    for (int32_t i = 0; i < n_cand; ++i)
        if (cand[i] < 0 || cand[i] >= n) return fail(BN_ERR_ARG, "candidate id " + std::to_string(cand[i]) + " out of range");
    std::fill(accepted_out, accepted_out + n_cand, uint8_t(0));
    // what the child reaches: an edge from there would close a cycle.  Edges INTO the child add no path that starts at it, so the
    // set holds for the whole call.
    Reach reached;
    reached.run(L->children, child);
    const std::vector<int32_t>& par = L->parents[size_t(child)];
    std::vector<int32_t> uniq, uniq_at;
    std::vector<double> ll;
    int32_t pos = 0;
    while (pos < n_cand) {
        if (int32_t(par.size()) >= L->max_parents || int32_t(par.size()) >= kLearnMaxParents) break;
        const int64_t rows = L->rows_of(child);
        L->addable(child, reached, rows, cand, pos, n_cand, uniq, uniq_at);
        if (uniq.empty()) break;
        const std::vector<GroupIn> group{GroupIn{child, par.data(), int32_t(par.size()), uniq.data(), int32_t(uniq.size())}};
        ll.assign(uniq.size() + 1, 0.0);
        if (int r = run_groups(L->t, L->spec, group, ll.data(), nullptr, &L->times)) return r;
        int32_t taken = -1;
        for (size_t j = 0; j < uniq.size() && taken < 0; ++j) {
            const int64_t params_next = L->params - L->family_params(child, rows) + L->family_params(child, rows * L->t->k[size_t(uniq[j])]);
            const double score_next = L->score_with(child, ll[j + 1], params_next);
            if (score_next < L->score) {   // strict (greedy.hpp:47, k2_algorithm.hpp:54)
                taken = uniq_at[j];
                L->ll[size_t(child)] = ll[j + 1];
                L->params = params_next;
                L->score = score_next;
            }
        }
        if (taken < 0) break;
        L->add_parent(cand[taken], child);
        accepted_out[taken] = 1;
        pos = taken + 1;
    }
    return BN_OK;
}

extern "C" int bn_learn_score(const bn_learner* L, double* score_out) {
    if (!L || !score_out) return fail(BN_ERR_ARG, "null argument");
    *score_out = L->score;
    return BN_OK;
}

extern "C" int bn_learn_structure(const bn_learner* L, int32_t* in_ptr_out, int32_t* in_idx_out) {
    if (!L || !in_ptr_out) return fail(BN_ERR_ARG, "null argument");
    int32_t at = 0;
    in_ptr_out[0] = 0;
    for (int32_t v = 0; v < L->n; ++v) {
        for (int32_t u : L->parents[size_t(v)]) {
            if (!in_idx_out) return fail(BN_ERR_ARG, "null argument");
            in_idx_out[at++] = u;
        }
        in_ptr_out[v + 1] = at;
    }
    return BN_OK;
}

extern "C" int bn_learn_get(const bn_learner* L, const char* name, int64_t* out) {
    if (!L || !name || !out) return fail(BN_ERR_ARG, "null argument");
    const std::string s(name);
    if (s == "families_scored") *out = L->times.families;
    else if (s == "passes") *out = L->times.passes;
    else if (s == "count_ns") *out = int64_t(L->times.count_ns);
    else if (s == "score_ns") *out = int64_t(L->times.score_ns);
    else if (s == "count_bytes") *out = L->times.count_bytes;
    else if (s == "lattice_ns") *out = int64_t(L->times.lattice_ns);
    else if (s == "subsets_scored") *out = L->times.subsets;
    else if (s == "anneal_ns") *out = int64_t(L->times.anneal_ns);
    else if (s == "anneal_chains") *out = L->times.anneal_chains;
    else if (s == "anneal_steps") *out = L->times.anneal_steps;
    else if (s == "hc_ns") *out = int64_t(L->times.hc_ns);
    else if (s == "hc_runs") *out = L->times.hc_runs;
    else if (s == "hc_merges") *out = L->times.hc_merges;
    else if (s == "climb_ns") *out = int64_t(L->times.climb_ns);
    else if (s == "climb_runs") *out = L->times.climb_runs;
    else if (s == "climb_steps") *out = L->times.climb_steps;
    else if (s == "optimal_ns") *out = int64_t(L->times.optimal_ns);
    else if (s == "optimal_bps_ns") *out = int64_t(L->times.optimal_bps_ns);
    else if (s == "optimal_sink_ns") *out = int64_t(L->times.optimal_sink_ns);
    else if (s == "optimal_cells") *out = L->times.optimal_cells;
    else if (s == "optimal_bytes") *out = L->times.optimal_bytes;
    else if (s == "edges") {
        *out = 0;
        for (const auto& p : L->parents) *out += int64_t(p.size());
    } else if (s == "parameters") *out = L->params;
    else if (s == "criterion") *out = L->criterion;
    else return fail(BN_ERR_ARG, "unknown name (criterion, families_scored, passes, count_ns, score_ns, count_bytes, lattice_ns, subsets_scored, anneal_ns, anneal_chains, anneal_steps, hc_ns, hc_runs, hc_merges, climb_ns, climb_runs, climb_steps, optimal_ns, optimal_bps_ns, optimal_sink_ns, optimal_cells, optimal_bytes, edges, parameters)");
    return BN_OK;
}

extern "C" int bn_learn_terms(const bn_learner* L, double* ll_out, int64_t* params_out) {
    if (!L || !ll_out) return fail(BN_ERR_ARG, "null argument");
    std::copy(L->ll.begin(), L->ll.end(), ll_out);
    if (params_out) *params_out = L->params;
    return BN_OK;
}
