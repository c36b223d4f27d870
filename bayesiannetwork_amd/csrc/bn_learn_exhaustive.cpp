// bn_learn_exhaustive.cpp -- the exhaustive searches of structure learning on the subset lattice (run_subsets, bn_learn_batch.cpp),
// reference bayesian/learning/brute_force.hpp: bn_learn_best_parents takes the best subset of a candidate list for one child;
// bn_learn_brute_force_hint and bn_learn_brute_force walk the reference's enumerations over a Walk, the learner's graph plus the
// candidate edges in hand, whose family terms all come from one lattice call per node.
#include "bn_learn_internal.hpp"

namespace {

// One node whose parent set an enumeration varies: its candidates (nodes that are neither the node nor a parent of it in the
// starting graph, each once), the family term of every subset of them on top of the starting parents, and the subset in hand.
struct Slot {
    int32_t node = 0, mask = 0, best_mask = 0;
    std::vector<int32_t> cand;
    std::vector<double> ll;   // [2^cand.size()], mask order
    int32_t bit_of(int32_t u) const {
        for (size_t j = 0; j < cand.size(); ++j)
            if (cand[j] == u) return int32_t(j);
        return -1;
    }
};

// The graph an enumeration walks: the learner's, plus the candidate edges in hand.  add_edge's refusals (graph.hpp:268-275: the
// edge exists or closes a cycle) and the library's limit on the number of parents.
struct Walk {
    bn_learner* L;
    std::vector<Slot> slots;
    std::vector<int32_t> slot_of;                  // per node, or -1
    std::vector<std::vector<int32_t>> children;    // the learner's, plus the edges in hand (added and removed last in, first out)
    std::vector<int32_t> n_par;
    std::vector<double> ll;                        // family term of every node in the graph in hand
    Reach reach;
    int64_t params = 0;

    explicit Walk(bn_learner* learner)
        : L(learner), slot_of(size_t(learner->n), -1), children(learner->children), n_par(size_t(learner->n)), ll(learner->ll),
          params(learner->params) {
        for (int32_t v = 0; v < L->n; ++v) n_par[size_t(v)] = int32_t(L->parents[size_t(v)].size());
    }

    // a slot for `node` with the nodes of `from` as candidates; one lattice call
    int add_slot(int32_t node, int32_t count, const int32_t* from) {
        if (slot_of[size_t(node)] >= 0) return BN_OK;
        Slot sl;
        sl.node = node;
        const std::vector<int32_t>& par = L->parents[size_t(node)];
        for (int32_t i = 0; i < count; ++i) {
            const int32_t u = from[i];
            if (u == node || std::binary_search(par.begin(), par.end(), u) || sl.bit_of(u) >= 0) continue;
            sl.cand.push_back(u);
        }
        if (sl.cand.size() > size_t(kLearnMaxParents))
            return fail(BN_ERR_ARG, "node " + std::to_string(node) + ": " + std::to_string(sl.cand.size()) + " candidate parents (at most " +
                                        std::to_string(kLearnMaxParents) + " minus its parents)");
        sl.ll.assign(size_t(1) << sl.cand.size(), 0.0);
        if (int r = run_subsets(L->t, L->spec, node, int32_t(par.size()), par.data(), int32_t(sl.cand.size()), sl.cand.data(), sl.ll.data(), nullptr,
                                 &L->times))
            return r;
        slot_of[size_t(node)] = int32_t(slots.size());
        slots.push_back(std::move(sl));
        return BN_OK;
    }

    // graph.add_edge(u, c): false when refused
    bool add(int32_t u, int32_t c) {
        const int32_t si = slot_of[size_t(c)];
        if (si < 0) return false;
        Slot& sl = slots[size_t(si)];
        const int32_t b = sl.bit_of(u);   // (-1: the node itself, or a parent in the starting graph)
        if (b < 0 || ((sl.mask >> b) & 1)) return false;
        if (n_par[size_t(c)] >= std::min(L->max_parents, kLearnMaxParents)) return false;
        if (reach.run(children, c, u)) return false;
        flip(sl, b, u, c, true);
        return true;
    }
    void erase(int32_t u, int32_t c) {
        Slot& sl = slots[size_t(slot_of[size_t(c)])];
        flip(sl, sl.bit_of(u), u, c, false);
    }
    void flip(Slot& sl, int32_t b, int32_t u, int32_t c, bool on) {
        int64_t rows = 1;   // the family's rows without u
        for (int32_t x : L->parents[size_t(c)]) rows *= L->t->k[size_t(x)];
        for (size_t j = 0; j < sl.cand.size(); ++j)
            if (int32_t(j) != b && ((sl.mask >> j) & 1)) rows *= L->t->k[size_t(sl.cand[j])];
        const int64_t with = L->family_params(c, rows * L->t->k[size_t(u)]), without = L->family_params(c, rows);
        if (on) {
            sl.mask |= int32_t(1) << b;
            children[size_t(u)].push_back(c);
            ++n_par[size_t(c)];
            params += with - without;
        } else {
            sl.mask &= ~(int32_t(1) << b);
            children[size_t(u)].pop_back();
            --n_par[size_t(c)];
            params -= with - without;
        }
        ll[size_t(c)] = sl.ll[size_t(sl.mask)];
    }
    double penalised(double likelihood) const { return L->penalised(likelihood, params); }
    void keep() {
        for (Slot& sl : slots) sl.best_mask = sl.mask;
    }
    // the best graph becomes the learner's
    void commit() {
        for (const Slot& sl : slots) {
            const int32_t c = sl.node;
            const int64_t before = L->family_params(c, L->rows_of(c));
            for (size_t j = 0; j < sl.cand.size(); ++j)
                if ((sl.best_mask >> j) & 1) L->add_parent(sl.cand[j], c);
            L->ll[size_t(c)] = sl.ll[size_t(sl.best_mask)];
            L->params += L->family_params(c, L->rows_of(c)) - before;
        }
        L->score = L->score_with(-1, 0.0, L->params);
    }
};

}  // namespace

extern "C" int bn_learn_best_parents(bn_learner* L, int32_t child, int32_t n_cand, const int32_t* cand, uint8_t* taken_out) {
    if (!L || n_cand < 0 || (n_cand > 0 && (!cand || !taken_out))) return fail(BN_ERR_ARG, "null argument or n_cand < 0");
    if (child < 0 || child >= L->n) return fail(BN_ERR_ARG, "child id " + std::to_string(child) + " out of range");
    if (int r = check_ids(L, "candidate", n_cand, cand)) return r;
    std::fill(taken_out, taken_out + n_cand, uint8_t(0));
    Reach reached;
    reached.run(L->children, child);
    const std::vector<int32_t>& par = L->parents[size_t(child)];
    const int64_t rows = L->rows_of(child);
    const int32_t room = std::min(L->max_parents, kLearnMaxParents) - int32_t(par.size());
    // bn_learn_try_parents' filter, and no candidate at all where the child has no room for a parent
    std::vector<int32_t> surv, surv_at;
    if (room > 0) L->addable(child, reached, rows, cand, 0, n_cand, surv, surv_at);
    const int32_t m = int32_t(surv.size());
    if (m == 0) return BN_OK;
    if (m > kLearnMaxParents)
        return fail(BN_ERR_ARG, std::to_string(m) + " candidates may be added (at most " + std::to_string(kLearnMaxParents) + " minus the parents)");
    std::vector<double> ll(size_t(1) << m);
    if (int r = run_subsets(L->t, L->spec, child, int32_t(par.size()), par.data(), m, surv.data(), ll.data(), nullptr, &L->times)) return r;
    // the reference's visiting order (brute_force.hpp:104-111): "not added" before "added", cand[0] outermost
    int32_t best_mask = 0;
    int64_t best_params = L->params;
    double best = L->score_with(child, ll[0], L->params);
    for (int32_t r = 1; r < (int32_t(1) << m); ++r) {
        int32_t mask = 0, size = 0;
        int64_t rows_r = rows;
        for (int32_t j = 0; j < m; ++j)
            if ((r >> (m - 1 - j)) & 1) {
                mask |= int32_t(1) << j;
                ++size;
                rows_r *= L->t->k[size_t(surv[size_t(j)])];
            }
        if (size > room) continue;
        const int64_t params_r = L->params - L->family_params(child, rows) + L->family_params(child, rows_r);
        const double score_r = L->score_with(child, ll[size_t(mask)], params_r);
        if (score_r < best) {
            best = score_r;
            best_mask = mask;
            best_params = params_r;
        }
    }
    if (best_mask == 0) return BN_OK;   // the empty subset keeps the graph
    for (int32_t j = 0; j < m; ++j)
        if ((best_mask >> j) & 1) {
            L->add_parent(surv[size_t(j)], child);
            taken_out[surv_at[size_t(j)]] = 1;
        }
    L->ll[size_t(child)] = ll[size_t(best_mask)];
    L->params = best_params;
    L->score = best;
    return BN_OK;
}

extern "C" int bn_learn_brute_force_hint(bn_learner* L, int32_t n_par, const int32_t* par, int32_t n_child, const int32_t* child) {
    if (!L) return fail(BN_ERR_ARG, "null argument");
    if (int r = check_ids(L, "parent", n_par, par)) return r;
    if (int r = check_ids(L, "child", n_child, child)) return r;
    // no add_edge can be refused for a cycle when no child reaches a parent node (a child itself included): every new edge starts
    // at a parent node, so a path from a child to a parent node would have to exist already
    std::vector<uint8_t> is_par(size_t(L->n), 0);
    for (int32_t i = 0; i < n_par; ++i) is_par[size_t(par[i])] = 1;
    bool decomposed = true;
    Reach reached;
    for (int32_t i = 0; i < n_child && decomposed; ++i) {
        reached.run(L->children, child[i]);
        for (int32_t v = 0; v < L->n && decomposed; ++v)
            if (reached.has(v) && is_par[size_t(v)]) decomposed = false;
    }
    if (decomposed) {
        // per child the other children's edges are fixed terms of the sum, so the depth-first search is one search per child; a
        // child listed again finds its best subset in place
        std::vector<uint8_t> taken(size_t(std::max(n_par, 1)));
        std::vector<uint8_t> done(size_t(L->n), 0);
        for (int32_t i = 0; i < n_child; ++i) {
            if (done[size_t(child[i])]) continue;
            done[size_t(child[i])] = 1;
            if (int r = bn_learn_best_parents(L, child[i], n_par, par, taken.data())) return r;
        }
        return BN_OK;
    }
    const int64_t edges = int64_t(n_par) * n_child;
    if (edges > 20)
        return fail(BN_ERR_ARG, std::to_string(edges) + " possible edges with a child that reaches a parent node: the literal enumeration takes at most 20");
    Walk w(L);
    for (int32_t i = 0; i < n_child; ++i)
        if (int r = w.add_slot(child[i], n_par, par)) return r;
    double best = L->score;
    // brute_force.hpp:85-113, the possible edges parent-major (:61-67)
    struct Rec {
        Walk& w;
        const int32_t *par, *child;
        int32_t n_child;
        int64_t edges;
        double& best;
        void run(int64_t e) {
            if (e == edges) {
                double likelihood = 0.0;
                for (double x : w.ll) likelihood -= x;
                const double now = w.penalised(likelihood);
                if (now < best) {
                    best = now;
                    w.keep();
                }
                return;
            }
            run(e + 1);
            const int32_t u = par[e / n_child], c = child[e % n_child];
            if (w.add(u, c)) {
                run(e + 1);
                w.erase(u, c);
            }
        }
    } rec{w, par, child, n_child, edges, best};
    rec.run(0);
    w.commit();
    return BN_OK;
}

extern "C" int bn_learn_brute_force(bn_learner* L, int32_t n_v, const int32_t* vertexes, double* eval_out) {
    if (!L) return fail(BN_ERR_ARG, "null argument");
    if (int r = check_ids(L, "vertex", n_v, vertexes)) return r;
    if (n_v > 8) return fail(BN_ERR_ARG, std::to_string(n_v) + " vertexes (at most 8: 2 027 025 graphs)");
    for (int32_t i = 0; i < n_v; ++i)
        for (int32_t j = 0; j < i; ++j)
            if (vertexes[i] == vertexes[j]) return fail(BN_ERR_ARG, "vertex " + std::to_string(vertexes[i]) + " listed twice");
    Walk w(L);
    for (int32_t i = 0; i < n_v; ++i)
        if (int r = w.add_slot(vertexes[i], n_v, vertexes)) return r;
    // eval_(graph, vertexes): the likelihood over `vertexes` in the given order, the parameters of the whole graph
    auto eval = [&]() {
        double likelihood = 0.0;
        for (int32_t i = 0; i < n_v; ++i) likelihood -= w.ll[size_t(vertexes[i])];
        return w.penalised(likelihood);
    };
    double best = eval();
    // brute_force.hpp:116-156.  Level t tries per later vertex: no edge, v_t -> v_i, v_i -> v_t.  "No edge" gives the same graph for
    // every i, so it is walked for the first i only: a graph seen again cannot win under <.
    struct Rec {
        Walk& w;
        const int32_t* v;
        int32_t n_v;
        double& best;
        decltype(eval)& eval_;
        void run(int32_t t) {
            if (t == n_v - 1) {
                const double now = eval_();
                if (now < best) {
                    best = now;
                    w.keep();
                }
                return;
            }
            for (int32_t i = t + 1; i < n_v; ++i) {
                if (i == t + 1) run(t + 1);
                if (w.add(v[t], v[i])) {
                    run(t + 1);
                    w.erase(v[t], v[i]);
                }
                if (w.add(v[i], v[t])) {
                    run(t + 1);
                    w.erase(v[i], v[t]);
                }
            }
        }
    } rec{w, vertexes, n_v, best, eval};
    if (n_v > 0) rec.run(0);
    w.commit();
    if (eval_out) *eval_out = best;
    return BN_OK;
}
