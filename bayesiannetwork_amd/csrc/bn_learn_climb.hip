// bn_learn_climb.hip -- tabu hill climbing over network structures as many independent runs resident on the device: steepest
// descent over the add, delete and reverse moves of a graph, a tabu list over node pairs, perturbed restarts (the search of
// bnlearn's hc / tabu and pgmpy's HillClimbSearch; include/bn_mi355x.h states the contract).  Every family term a run can ask for
// is in the term table (bn_learn_terms.hpp) before it starts.
//
// One WAVE per run, lane v = node v (n <= 64); four waves per workgroup, which share nothing but the rank tables in LDS.
//   lane v     : node v's parent mask, family term ll[v], row product, arity; its ancestor mask anc[v] (who reaches v) and its
//                descendant mask desc[v]; the tabu mask (bit w: the pair {v, w} is tabu); the best graph's mask and term
//   lane i     : entry i of the tabu ring (tabu_len <= 64), the pair applied at a step = i mod tabu_len
//   wave       : score, counters and the random stream, wave-uniform
// A step looks at every move at once: lane u is the candidate `from`, the wave walks to = 0 .. n-1 with node to's family read across
// the lanes.  Where u -> to is absent the lane weighs the ADD (legal iff `to` is no ancestor of u, `to` is below the in-degree
// bound and the new term is a number), where it is present the DELETE and the REVERSE (legal iff no other parent of `to` descends
// from u, u is below the bound and u's new term is a number).  The changed parent set is ranked by the lane (rank_of) and its term
// loaded, four `to` at a time so that their loads are in flight together (the loads are unconditional: a lane with nothing to
// weigh reads entry 0); nothing is cached, so every delta is made from the terms of the graph as it stands.  Each lane keeps the
// smallest (d, id) it saw; six exchange rounds then give the wave's.  (d, id) is a total order -- d compared with <, equal d by
// the smaller id -- so the shape of the reduction cannot change the result.
// After an applied move the masks are rebuilt from the parent masks: anc[v] |= anc[p] | bit(p) over v's parents, every lane at
// once, until a ballot says no lane changed (at most n rounds); desc is anc transposed through n lane reads.
// Delta of a family change of child c: (ll[c] - term_new), + double(p_new - p_old) under AIC, + double(p_new - p_old) * penalty
// under MDL; plain fp64 operations, no contraction.  The score after a move is evaluate_terms of the new graph (node order, exact
// parameter count: the bits of bn_learn_score), never current + d.
// Random stream: run j owns the stream of chain j of bn_learn_anneal.hip; only the perturbation of runs j >= 1 draws from it.
// Vector stores only, no atomics: every output word has one writer.
#include <hip/hip_runtime.h>

#include "bn_learn_climb.hpp"
#include "bn_learn_dev.hpp"

namespace bnmi {

namespace {

constexpr int kNoMove = 0x7fffffff;
constexpr int kClimbBatch = 4;   // the `to` whose term loads a step has in flight together

// (d, id) before (e, ie)?  kNoMove: no move at all
__device__ __forceinline__ bool before(double d, int id, double e, int ie) {
    return id != kNoMove && (ie == kNoMove || d < e || (d == e && id < ie));
}

}  // namespace

__global__ __launch_bounds__(kClimbWaves * 64) void learn_climb_kernel(ClimbArgs a) {
    __shared__ uint32_t s_tab[kTermTabWords];
    const SearchWave w = search_enter<kClimbWaves>(s_tab, a);
    if (w.surplus) return;
    const int lane = w.lane, run = w.run;
    const int n = a.n, mp = a.max_parents;
    const bool node = lane < n;
    const uint64_t me = uint64_t(1) << lane;

    uint64_t pm;
    int64_t rows;
    double ll;
    int32_t kk;
    load_family(a, a.k, n, lane, pm, rows, ll, kk);
    uint64_t anc = 0, desc = 0, tmask = 0;
    uint32_t ring = 0xFFFFu;
    int64_t params = a.params0;

    auto rebuild = [&]() {
        uint64_t x = 0;
        for (int r = 0; r < n; ++r) {
            uint64_t m = pm, more = 0;
            while (__ballot(m != 0)) {
                const int p = m ? __ffsll((long long)m) - 1 : lane;
                const uint64_t xp = from_lane_u64(x, p);
                if (m) more |= xp | (uint64_t(1) << p);
                m &= m - 1;
            }
            const bool grew = (more & ~x) != 0;
            x |= more;
            if (!__ballot(grew)) break;
        }
        anc = x;
        uint64_t y = 0;
        for (int v = 0; v < n; ++v) y |= ((lane_u64(x, v) >> lane) & 1) << v;
        desc = y;
    };
    // the penalty's part of a delta: double(dp) under AIC, double(dp) * penalty under MDL (not added under BDeu / K2)
    auto penalty_of = [&](int64_t dp) { return a.criterion == 0 ? double(dp) : double(dp) * a.penalty; };
    auto delta = [&](double ll_old, double term_new, double pen) {
        const double d = ll_old - term_new;
        return a.criterion <= 1 ? d + pen : d;
    };
    // This lane as `from`, towards `to`, in two halves so that a step can have the loads of several `to` in flight at once.
    // probe: has: the edge is there; want0 / at0: the add (edge absent) or the delete (present) is to be weighed and the entry
    // of the term table it needs; want2 / at2: the same for the reverse.  An entry that is not wanted is entry 0: the load is
    // unconditional.  weigh: (ok0, d0) and (ok2, d2) from the loaded terms t0 and t2.
    struct Probe {
        bool has, want0, want2;
        int64_t at0, at2;
        double pen0, pen2, ll_to;
    };
    auto probe = [&](int to, bool live) {
        Probe p{false, false, false, 0, 0, 0.0, 0.0, 0.0};
        const uint64_t pm_to = lane_u64(pm, to), bit_to = uint64_t(1) << to;
        const int32_t k_to = int32_t(lane_u32(uint32_t(kk), to));
        const int64_t rows_to = int64_t(lane_u64(uint64_t(rows), to));
        p.ll_to = lane_f64(ll, to);
        const bool mine = live && node && lane != to;
        p.has = mine && (pm_to & me) != 0;
        if (mine && !p.has) {
            if (!(anc & bit_to) && __popcll(pm_to) < mp) {
                p.want0 = true;
                p.at0 = int64_t(to) * a.T + rank_of(s_tab, to, pm_to | me);
                p.pen0 = penalty_of(int64_t(k_to - 1) * (rows_to * kk - rows_to));
            }
        } else if (p.has) {
            const int64_t rows_less = rows_without(rows_to, uint32_t(kk));
            p.want0 = true;
            p.at0 = int64_t(to) * a.T + rank_of(s_tab, to, pm_to & ~me);
            p.pen0 = penalty_of(int64_t(k_to - 1) * (rows_less - rows_to));
            if (!(pm_to & ~me & desc) && __popcll(pm) < mp) {
                p.want2 = true;
                p.at2 = int64_t(lane) * a.T + rank_of(s_tab, lane, pm | bit_to);
                p.pen2 = penalty_of(int64_t(kk - 1) * (rows * k_to - rows));
            }
        }
        return p;
    };
    auto weigh = [&](const Probe& p, double t0, double t2, bool& ok0, double& d0, bool& ok2, double& d2) {
        ok0 = ok2 = false;
        d0 = d2 = 0.0;
        if (p.want0) {
            d0 = delta(p.ll_to, t0, p.pen0);
            ok0 = t0 == t0 && d0 == d0;
        }
        if (p.want2) {
            d2 = d0 + delta(ll, t2, p.pen2);
            ok2 = t2 == t2 && d2 == d2;
        }
    };
    auto apply = [&](int kind, int from, int to) {
        const uint32_t k_from = lane_u32(uint32_t(kk), from), k_to = lane_u32(uint32_t(kk), to);
        const int64_t rows_was = rows;
        bool changed = false;
        if (lane == to) {
            if (kind == 0) with_parent(pm, rows, from, k_from, pm, rows);
            else without_parent(pm, rows, from, k_from, pm, rows);
            changed = true;
        }
        if (kind == 2 && lane == from) {
            with_parent(pm, rows, to, k_to, pm, rows);
            changed = true;
        }
        if (changed) ll = term_of(a.terms, a.T, s_tab, lane, pm);
        params += params_delta(kk, rows_was, rows, to, from, kind == 2);
        rebuild();
    };

    rebuild();
    uint32_t perturbed = 0;
    if (run >= 1 && a.perturb > 0) {
        uint4 g = seed_stream(run, a.seed_lo, a.seed_hi);
        for (uint32_t i = 0; i < a.perturb; ++i) {
            const int kind = int(draw_below(g, 3u));
            const int from = int(draw_below(g, uint32_t(n)));
            const int to = int(draw_below(g, uint32_t(n)));
            bool ok0, ok2;
            double d0, d2;
            const Probe p = probe(to, true);
            weigh(p, a.terms[p.at0], a.terms[p.at2], ok0, d0, ok2, d2);
            const uint32_t f = lane_u32((p.has ? 1u : 0u) | (ok0 ? 2u : 0u) | (ok2 ? 4u : 0u), from);
            const bool ok = kind == 0 ? (f & 3u) == 2u : kind == 1 ? (f & 3u) == 3u : (f & 4u) != 0;
            if (!ok) continue;
            apply(kind, from, to);
            ++perturbed;
        }
    }

    double current = evaluate_terms(ll, params, n, a.criterion, a.penalty);
    double best_eval = current;
    uint64_t best_pm = pm;
    double best_ll = ll;
    uint32_t steps = 0, improving = 0, best_step = 0, worse = 0, flags = 0, tabu_legal = 0;
    const bool traced = run == a.trace_run && a.trace != nullptr;

    while (steps < a.max_steps) {
        double bd = 0.0;
        int bid = kNoMove;
        uint32_t tl = 0;
        for (int base = 0; base < n; base += kClimbBatch) {
            Probe p[kClimbBatch];
            double t0[kClimbBatch], t2[kClimbBatch];
#pragma unroll
            for (int j = 0; j < kClimbBatch; ++j) p[j] = probe(min(base + j, n - 1), base + j < n);
#pragma unroll
            for (int j = 0; j < kClimbBatch; ++j) {
                t0[j] = a.terms[p[j].at0];
                t2[j] = a.terms[p[j].at2];
            }
#pragma unroll
            for (int j = 0; j < kClimbBatch; ++j) {
                const int to = base + j;   // (past n - 1: nothing is wanted, nothing is ok)
                bool ok0, ok2;
                double d0, d2;
                weigh(p[j], t0[j], t2[j], ok0, d0, ok2, d2);
                const bool tabu = ((tmask >> (to & 63)) & 1) != 0;
                const int id0 = ((p[j].has ? n : 0) + lane) * n + to, id2 = (2 * n + lane) * n + to;
                tl += (tabu && ok0 ? 1u : 0u) + (tabu && ok2 ? 1u : 0u);
                if (ok0 && !tabu && before(d0, id0, bd, bid)) { bd = d0; bid = id0; }
                if (ok2 && !tabu && before(d2, id2, bd, bid)) { bd = d2; bid = id2; }
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __longlong_as_double((long long)from_lane_u64(uint64_t(__double_as_longlong(bd)), lane ^ off));
            const int oi = int(from_lane_u32(uint32_t(bid), lane ^ off));
            const uint32_t ot = from_lane_u32(tl, lane ^ off);
            if (before(od, oi, bd, bid)) { bd = od; bid = oi; }
            tl += ot;
        }
        const int id = uni(bid);
        const double d = lane_f64(bd, 0);
        tabu_legal = uint32_t(uni(int(tl)));
        if (id == kNoMove) { flags = kClimbEndNoMove; break; }
        if (!(d < 0) && worse == a.max_worse) { flags = kClimbEndOptimum; break; }
        const int kind = id / (n * n), from = (id / n) % n, to = id % n;
        apply(kind, from, to);
        if (a.tabu_len > 0) {
            const int at = int(steps % uint32_t(a.tabu_len));
            const uint32_t old = lane_u32(ring, at);
            if (old != 0xFFFFu) {   // the pair that leaves the ring: it is in it once, a tabu pair is never applied
                const int x = int(old & 255u), y = int(old >> 8);
                if (lane == x) tmask &= ~(uint64_t(1) << y);
                if (lane == y) tmask &= ~(uint64_t(1) << x);
            }
            if (lane == at) ring = uint32_t(from | (to << 8));
            if (lane == from) tmask |= uint64_t(1) << to;
            if (lane == to) tmask |= uint64_t(1) << from;
        }
        ++steps;
        if (d < 0) ++improving;
        current = evaluate_terms(ll, params, n, a.criterion, a.penalty);
        if (traced && steps - 1 < a.trace_cap && lane == 0)
            a.trace[steps - 1] = ClimbTrace{uint64_t(__double_as_longlong(d)), uint64_t(__double_as_longlong(current)), uint8_t(kind), uint8_t(from),
                                            uint8_t(to), 0, 0u, 0u};
        if (current < best_eval) {
            best_eval = current;
            best_pm = pm;
            best_ll = ll;
            best_step = steps;
            worse = 0;
        } else {
            ++worse;
        }
    }
    if (flags == 0) flags = kClimbEndCap;

    if (lane == 0) a.rec[run] = ClimbRecord{best_eval, steps, improving, perturbed, best_step, flags, tabu_legal};
    store_graph(a, run, lane, best_pm, best_ll);
}

int learn_launch_climb(const ClimbArgs& a, void* stream) { return launch_search<kClimbWaves>(learn_climb_kernel, a, stream); }

}  // namespace bnmi
