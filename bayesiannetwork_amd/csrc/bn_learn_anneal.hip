// bn_learn_anneal.hip -- simulated annealing over network structures (reference bayesian/learning/simulated_annealing.hpp:41-115) as
// many independent chains resident on the device.  AIC / MDL are decomposable and the in-degree is bounded by q, so every family
// term a chain can ask for is in the term table (bn_learn_terms.hpp) before it starts: a step is a few random draws, a cycle
// check, one or two table lookups and a sum.
//
// One WAVE per chain, lane v = node v (n <= 64); four waves per workgroup, which share nothing but the rank tables in LDS.
//   lane v     : node v's parent mask, family term ll[v], exact int64 row product (for the parameter count), arity
//   wave       : temperature, evaluation, counters and the random stream -- wave-uniform, the stream and the counters in SGPRs
//   LDS        : the graph's ORDERED edge list (the reference draws edges[i] of edge_list(), insertion order) and the list of the
//                last accepted graph, 2 x 1 024 entries of two bytes per chain
// The loop is the reference's, quirks included:
//   method 0   : from, to drawn; add_edge refuses from == to or `to` reaching `from` (graph.hpp:270), an existing edge (:284),
//                and -- the library's limits -- a full parent set or a NaN term
//   method 1, 2: no edge: `continue` (no draw, no cooling); else an edge index is drawn; 1 erases the edge (ordered erase, :314);
//                2 erases it and adds the opposite edge at the END of the list; when that is refused the original edge is added
//                back at the END (:339-358) and the proposal does not count as operated -- the list stays reordered
//   not operated: `continue`: no cooling, no same-state count
//   operated   : now = the learner's score of the proposed graph; diff = now - current; accepted iff diff <= 0, else a uniform u
//                is drawn and accepted iff u < exp(-now / (boltzmann * T))  (rule 0, :97: `now`, not `diff`) or
//                exp(-diff / (boltzmann * T)) (rule 1, Metropolis); T *= rate
//   accepted   : best_graph = graph (:102): the lanes take the proposed terms, the list is copied to the accepted list
//   rejected   : graph = best_graph (:109): the accepted list is copied back.  This is NOT the inverse of the proposal: a refused
//                reversal since the last acceptance reordered graph's list and not best_graph's, and the copy undoes that too
// and ends when T <= final_temp, after same_state_max rejections in a row, or -- ours -- after max_proposals loop iterations.
//
// Cycle check: "does a reach b" walks the frontier F from a: next = ballot((parents & F) != 0) & ~reached, at most n rounds of one
// compare and one ballot each; nothing goes through LDS.  (The same wave-wide OR over child masks would cost a 64-bit cross-lane
// reduction per round; the parent masks give it as one ballot, so no child mask is kept.)
// Term lookup: the child's lane ranks its proposed parent mask (<= 16 binomials from the LDS table) and loads the one 8-byte term
// -- a dependent load, the step's critical path.
// Evaluation: likelihood = 0.0; likelihood -= ll[v] for v = 0 .. n-1 through lane reads IN NODE ORDER (no tree), then the AIC / MDL
// penalty from the exact parameter count: the bits of bn_learn_score on that graph.
// Random stream: chain j owns xoshiro128++ seeded by Philox4x32-10({j_lo, j_hi, 0, 0}, {seed_lo, seed_hi}) (bn_rng_dev.hpp); one
// step per draw: integer in [0, m): (uint64(r) * m) >> 32; real: (r + 0.5) * 2^-32.  Order per iteration: method; from, to (add) or
// the edge index (erase, reverse; only with an edge); u only for an operated proposal with diff > 0.
// Vector stores only, no atomics: every output word has one writer.
#include <hip/hip_runtime.h>

#include "bn_learn_anneal.hpp"
#include "bn_learn_dev.hpp"

namespace bnmi {

namespace {

// does a path lead from `a` to `b` (a == b: yes)?  pm: every lane's parent mask
__device__ __forceinline__ bool reaches(uint64_t pm, int n, int a, int b) {
    if (a == b) return true;
    uint64_t reached = uint64_t(1) << a, frontier = reached;
    for (int r = 0; r < n; ++r) {
        const uint64_t next = __ballot((pm & frontier) != 0) & ~reached;
        if ((next >> b) & 1) return true;
        if (next == 0) return false;
        reached |= next;
        frontier = next;
    }
    return false;
}

}  // namespace

__global__ __launch_bounds__(kAnnealWaves * 64) void learn_anneal_kernel(AnnealArgs a) {
    __shared__ uint32_t s_tab[kTermTabWords];
    __shared__ uint16_t s_list[kAnnealWaves][2][kAnnealMaxEdges];
    const SearchWave w = search_enter<kAnnealWaves>(s_tab, a);
    if (w.surplus) return;
    const int lane = w.lane, chain = w.run;
    uint16_t* list = s_list[w.wave][0];
    uint16_t* kept = s_list[w.wave][1];
    const int n = a.n;

    uint64_t pm;
    int64_t rows;
    double ll;
    int32_t kk;
    load_family(a, a.k, n, lane, pm, rows, ll, kk);
    int ne = a.n_edges0;
    for (int i = lane; i < ne; i += 64) list[i] = kept[i] = a.edges0[i];
    wave_sync();

    uint4 g = seed_stream(chain, a.seed_lo, a.seed_hi);

    // the learner's score of the graph whose family terms the lanes hold in x
    auto evaluate = [&](double x, int64_t params) { return evaluate_terms(x, params, n, a.criterion, a.penalty); };
    auto append = [&](int from, int to) {
        if (lane == 0) list[ne] = uint16_t(from | (to << 8));
        ++ne;
        wave_sync();
    };

    int64_t params = a.params0;
    double current = evaluate(ll, params), temp = a.initial_temp;
    uint32_t no_changed = 0, proposals = 0, operated = 0, accepted = 0;
    const bool traced = chain == a.trace_run && a.trace != nullptr;

    while (temp > a.final_temp && no_changed < a.same_state_max && proposals < a.max_proposals) {
        ++proposals;
        const uint32_t method = draw_below(g, 3u);
        int from, to;
        bool ok;
        // the proposal: what the lanes of the changed families would hold
        uint64_t pm_new = pm;
        int64_t rows_new = rows;
        bool changed = false;
        if (method == 0) {
            from = int(draw_below(g, uint32_t(n)));
            to = int(draw_below(g, uint32_t(n)));
            const uint32_t k_from = lane_u32(uint32_t(kk), from);
            ok = !reaches(pm, n, to, from);
            if (ok) {
                const uint64_t pm_to = lane_u64(pm, to);
                ok = !((pm_to >> from) & 1) && __popcll(pm_to) < a.max_parents;
            }
            if (ok && lane == to) {
                with_parent(pm, rows, from, k_from, pm_new, rows_new);
                changed = true;
            }
        } else {
            if (ne == 0) continue;
            const int at = int(draw_below(g, uint32_t(ne)));
            const int e = uni(int(list[at]));
            from = e & 255;
            to = e >> 8;
            // the ordered erase (graph.hpp:314)
            for (int base = at; base < ne - 1; base += 64) {
                const int j = base + lane;
                const uint16_t x = j < ne - 1 ? list[j + 1] : uint16_t(0);
                wave_sync();
                if (j < ne - 1) list[j] = x;
                wave_sync();
            }
            --ne;
            const uint64_t without = lane == to ? pm & ~(uint64_t(1) << from) : pm;
            const uint32_t k_from = lane_u32(uint32_t(kk), from), k_to = lane_u32(uint32_t(kk), to);
            ok = true;
            if (method == 2) {   // add_edge(to, from) on the graph without from -> to
                ok = !reaches(without, n, from, to) && __popcll(lane_u64(pm, from)) < a.max_parents;
                if (ok && lane == from) {
                    with_parent(pm, rows, to, k_to, pm_new, rows_new);
                    changed = true;
                }
            }
            if (ok && lane == to) {
                pm_new = without;
                rows_new = rows_without(rows, k_from);
                changed = true;
            }
        }
        double ll_new = ll;
        if (changed) ll_new = term_of(a.terms, a.T, s_tab, lane, pm_new);
        if (ok && method != 1) {   // a family over the per-family limit: a NaN term, add_edge refuses
            const double added = lane_f64(ll_new, method == 0 ? to : from);
            ok = added == added;
        }
        if (method == 2) append(ok ? to : from, ok ? from : to);
        else if (method == 0 && ok) append(from, to);
        if (!ok) continue;
        ++operated;

        const int64_t params_new = params + params_delta(kk, rows, rows_new, to, from, method == 2);
        const double now = evaluate(ll_new, params_new);
        const double diff = now - current;
        bool accept = diff <= 0;
        if (!accept) {
            const double u = (double(xoshiro_next(g)) + 0.5) * 0x1p-32;
            const double scale = a.boltzmann * temp;
            const double p = exp(-(a.rule == 0 ? now : diff) / scale);
            accept = u < p;
        }
        if (traced && operated - 1 < a.trace_cap && lane == 0)
            a.trace[operated - 1] = AnnealTrace{uint64_t(__double_as_longlong(now)), uint8_t(method), uint8_t(from), uint8_t(to), uint8_t(accept ? 1 : 0), 0u};
        if (accept) {
            pm = pm_new;
            rows = rows_new;
            ll = ll_new;
            params = params_new;
            current = now;
            no_changed = 0;
            ++accepted;
            for (int i = lane; i < ne; i += 64) kept[i] = list[i];
        } else {
            ne = ne - (method == 0 ? 1 : 0) + (method == 1 ? 1 : 0);   // the accepted graph's edge count
            for (int i = lane; i < ne; i += 64) list[i] = kept[i];
            ++no_changed;
        }
        wave_sync();
        temp *= a.rate;
    }

    uint32_t flags = 0;
    if (!(temp > a.final_temp)) flags |= kAnnealEndTemp;
    if (!(no_changed < a.same_state_max)) flags |= kAnnealEndSame;
    if (!(proposals < a.max_proposals)) flags |= kAnnealEndCap;
    if (lane == 0) a.rec[chain] = AnnealRecord{current, proposals, operated, accepted, flags, uint32_t(ne), 0u};
    store_graph(a, chain, lane, pm, ll);
    if (a.edges)
        for (int i = lane; i < ne; i += 64) a.edges[int64_t(chain) * a.edge_stride + i] = list[i];
}

int learn_launch_anneal(const AnnealArgs& a, void* stream) { return launch_search<kAnnealWaves>(learn_anneal_kernel, a, stream); }

}  // namespace bnmi
