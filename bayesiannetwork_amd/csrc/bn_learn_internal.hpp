// bn_learn_internal.hpp -- what the translation units of structure learning (include/bn_mi355x.h, bn_learn_* and bn_terms_*) share.
// bn_learn_plan.cpp: the host-only planning of a batch; bn_learn_batch.cpp: run_groups / run_subsets on the device and the
// bn_learn_score_* entry points; bn_learn.cpp: the bn_learner object and bn_learn_try_parents (reference greedy.hpp, k2_algorithm.hpp);
// bn_learn_exhaustive.cpp: bn_learn_best_parents and the brute-force searches (brute_force.hpp); bn_learn_terms.cpp: bn_term_table;
// bn_learn_search.cpp: the device-resident searches over a term table, bn_learn_anneal, bn_learn_hc, bn_learn_climb and
// bn_learn_optimal.
#ifndef BN_LEARN_INTERNAL_HPP
#define BN_LEARN_INTERNAL_HPP
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>

#include "bn_engine_internal.hpp"
#include "bn_info_table.hpp"
#include "bn_learn.hpp"
#include "bn_learn_plan.hpp"
#include "../../include/bn_mi355x.h"

#pragma GCC visibility push(hidden)   // (internal to the library: the surface is the C ABI)

struct LearnTimes {
    double count_ns = 0.0, score_ns = 0.0;
    int64_t families = 0;
    int64_t passes = 0;        // batch calls (one per run_groups / run_subsets call, however many passes over the scratch it took)
    int64_t count_bytes = 0;   // what the counting kernel has to read, from the shapes: per chunk P * (8 + base + 1 + candidates)
    double lattice_ns = 0.0;   // the subset lattice's kernel(s)
    int64_t subsets = 0;       // families made by the lattice (the top family included)
    double anneal_ns = 0.0;    // the annealing kernel
    int64_t anneal_chains = 0, anneal_steps = 0;
    double hc_ns = 0.0;        // the hierarchical-clustering kernel
    int64_t hc_runs = 0, hc_merges = 0;
    double climb_ns = 0.0;     // the hill-climbing kernel
    int64_t climb_runs = 0, climb_steps = 0;
    double optimal_ns = 0.0;   // the exact search's launches; of these, the best-parent-set passes and the best-sink levels
    double optimal_bps_ns = 0.0, optimal_sink_ns = 0.0;
    int64_t optimal_cells = 0, optimal_bytes = 0;   // of the last call: n * 2^(n - 1), the device memory it took
};

// The family term: kind 0 the log-likelihood term (AIC / MDL), 2 BDeu, 3 K2.  Held normalised (ess 0.0 where the kind does not
// read it), so two specs are the same function iff kind and the bits of ess agree.
constexpr bn_score_spec kLogLikSpec{0, 0, 0.0};

inline int check_spec(const bn_score_spec* in, bn_score_spec& out) {
    out = kLogLikSpec;
    if (!in) return BN_OK;
    if (in->kind != 0 && in->kind != 2 && in->kind != 3)
        return fail(BN_ERR_ARG, "score spec: unknown kind " + std::to_string(in->kind) + " (0 log-likelihood term, 2 BDeu, 3 K2)");
    out.kind = in->kind;
    if (in->kind == 2) {
        if (!(std::isfinite(in->ess) && in->ess >= 0x1p-20 && in->ess <= 0x1p20))
            return fail(BN_ERR_ARG, "score spec: BDeu's ess must be finite and within [2^-20, 2^20]");
        out.ess = in->ess;
    }
    return BN_OK;
}

inline bool same_spec(const bn_score_spec& x, const bn_score_spec& y) { return x.kind == y.kind && std::memcmp(&x.ess, &y.ess, 8) == 0; }

inline const char* spec_name(const bn_score_spec& x) { return x.kind == 0 ? "the log-likelihood term (AIC / MDL)" : x.kind == 2 ? "BDeu" : "K2"; }

namespace bn_eng __attribute__((visibility("hidden"))) {
// ll_out [families], group-major, base first; counts_out: null, or every family's counts back to back in the fitted layout
int run_groups(bn_info_table* t, const bn_score_spec& spec, const std::vector<GroupIn>& groups, double* ll_out, uint64_t* counts_out,
               LearnTimes* times);
// ll_out [2^m] in mask order (bit j: cand[j] is a parent); counts_out: null, or every family's counts in the fitted layout, mask order
int run_subsets(bn_info_table* t, const bn_score_spec& spec, int32_t child, int32_t n_base, const int32_t* base, int32_t m, const int32_t* cand,
                double* ll_out, uint64_t* counts_out, LearnTimes* times);
// workgroups the counting launch splits the patterns over per chunk (bn_learn_batch.cpp; bn_learn_pc.cpp counts the same way)
int count_splits(const bn_info_table* t, int32_t n_chunks);
}  // namespace bn_eng

// What a node reaches over a `children` adjacency (graph.hpp:270, is_able_trace); the marks and the stack are kept between searches.
struct Reach {
    std::vector<int32_t> stamp, stack;
    int32_t now = 0;
    // marks every node with a path from `from`, `from` included, and stops early when it comes to `stop` (-1: never): true then
    bool run(const std::vector<std::vector<int32_t>>& children, int32_t from, int32_t stop = -1) {
        if (stamp.size() != children.size()) {
            stamp.assign(children.size(), 0);
            now = 0;
        }
        ++now;
        stack.assign(1, from);
        stamp[size_t(from)] = now;
        while (!stack.empty()) {
            const int32_t v = stack.back();
            stack.pop_back();
            if (v == stop) return true;
            for (int32_t c : children[size_t(v)])
                if (stamp[size_t(c)] != now) { stamp[size_t(c)] = now; stack.push_back(c); }
        }
        return false;
    }
    bool has(int32_t v) const { return stamp[size_t(v)] == now; }   // of the last search (a full one)
};

struct bn_learner {
    bn_info_table* t = nullptr;
    int32_t n = 0, criterion = 0, max_parents = 0;
    std::vector<std::vector<int32_t>> parents, children;   // parents increasing per node
    std::vector<double> ll;                                // family term of every node
    int64_t params = 0;
    double penalty = 1.0;    // per parameter: 1 (AIC), log2(total) / 2 (MDL); criteria 2 (BDeu) and 3 (K2) have none
    double score = 0.0;
    bn_score_spec spec = kLogLikSpec;   // the family term: kind 0 under AIC / MDL, else the criterion
    LearnTimes times;
    std::vector<uint8_t> listed;        // addable's marks: [n], zero between calls

    int64_t family_params(int32_t v, int64_t rows) const { return int64_t(t->k[size_t(v)] - 1) * rows; }
    int64_t rows_of(int32_t v) const {
        int64_t rows = 1;
        for (int32_t u : parents[size_t(v)]) rows *= t->k[size_t(u)];
        return rows;
    }
    // evaluation.py's arithmetic, the one host copy (the kernels': evaluate_terms, bn_learn_dev.hpp)
    double penalised(double likelihood, int64_t params_now) const {
        return criterion >= 2 ? likelihood : criterion == 0 ? likelihood + double(params_now) : likelihood + double(params_now) * penalty;
    }
    // likelihood = 0.0; likelihood -= ll[v] in node order, node c's term replaced by ll_c
    double score_with(int32_t c, double ll_c, int64_t params_now) const {
        double likelihood = 0.0;
        for (int32_t v = 0; v < n; ++v) likelihood -= v == c ? ll_c : ll[size_t(v)];
        return penalised(likelihood, params_now);
    }
    // the edge u -> c
    void add_parent(int32_t u, int32_t c) {
        std::vector<int32_t>& par = parents[size_t(c)];
        par.insert(std::lower_bound(par.begin(), par.end(), u), u);
        children[size_t(u)].push_back(c);
    }
    // The candidates of list[begin, end) that may still be added to `child`, in walking order, the first listing of each: not the
    // child or what it reaches (`reached`: a full search from child), not a parent, the family within 2^20 entries (rows: rows_of(child)).
    void addable(int32_t child, const Reach& reached, int64_t rows, const int32_t* list, int32_t begin, int32_t end, std::vector<int32_t>& ids,
                 std::vector<int32_t>& at) {
        const std::vector<int32_t>& par = parents[size_t(child)];
        const int32_t kc = t->k[size_t(child)];
        ids.clear();
        at.clear();
        for (int32_t i = begin; i < end; ++i) {
            const int32_t u = list[i];
            if (reached.has(u) || listed[size_t(u)] || std::binary_search(par.begin(), par.end(), u)) continue;
            if (rows * t->k[size_t(u)] * kc > kLearnMaxEntries) continue;
            listed[size_t(u)] = 1;
            ids.push_back(u);
            at.push_back(i);
        }
        for (int32_t u : ids) listed[size_t(u)] = 0;
    }
};

struct bn_term_table {
    bn_info_table* t = nullptr;
    int device = 0;
    int32_t n = 0, q = 0;
    int64_t T = 0;                       // entries per child
    std::vector<uint32_t> tab;           // the rank tables (bn_learn_terms.hpp)
    DeviceBuf<double> d_terms;
    DeviceBuf<uint32_t> d_tab;
    DeviceBuf<int32_t> d_k;
    int64_t ineligible = 0;
    bn_score_spec spec = kLogLikSpec;    // the family term the entries hold
    LearnTimes times;

    // sorted parents, none of them c
    int64_t rank(int32_t c, const int32_t* par, int32_t j) const;
    ~bn_term_table() {
        DeviceGuard g;
        (void)g.enter(device);
        d_terms.reset(); d_tab.reset(); d_k.reset();
    }
};

inline int check_ids(const bn_learner* L, const char* what, int32_t count, const int32_t* ids) {
    if (count < 0 || (count > 0 && !ids)) return fail(BN_ERR_ARG, std::string("null argument or negative count: ") + what);
    for (int32_t i = 0; i < count; ++i)
        if (ids[i] < 0 || ids[i] >= L->n) return fail(BN_ERR_ARG, std::string(what) + " id " + std::to_string(ids[i]) + " out of range");
    return BN_OK;
}

#pragma GCC visibility pop

#endif  // BN_LEARN_INTERNAL_HPP
