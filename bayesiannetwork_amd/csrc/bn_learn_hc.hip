// bn_learn_hc.hip -- hierarchical-clustering stepwise structure search (reference bayesian/learning/stepwise_structure_hc.hpp:131-360
// over greedy.hpp:67-101) as many independent runs resident on the device.  Everything a run reads exists before it starts: the
// similarity matrix S (the all-pairs mutual information, or the caller's) and the term table of every family of at most q parents
// (bn_learn_terms.hpp).  A run is table lookups, random draws and list maintenance; no pass over the samples.
//
// One WAVE per run, lane v = node v (n <= 64); two waves per workgroup, which share nothing but the rank tables in LDS.
//   lane v     : node v's parent mask, family term ll[v], exact int64 row product, arity
//   wave       : the stream, the counters, eval_now, the list lengths -- wave-uniform
//   LDS        : the ordered list of live cluster ids; per id the start and length of its node list in a byte array (a merged
//                cluster's list is the parent's then the child's, appended; 2 176 bytes hold every list a run can make); the
//                ordered similarity list, at most C(64, 2) = 2 016 entries of two one-byte ids and one fp64 value; per id
//                the value of its entry with the parent and with the child of the current merge
//   global     : S, 32 KiB at most and read by every run of every workgroup: it stays in L2
// A cluster has an id where the reference has an address: node i's cluster is i, merge number s makes n + s.
// The loop, while more than one cluster lives and the list is not empty:
//   pick       : the FIRST maximum of the list (std::max_element with <): a lane-strided scan, then a butterfly that prefers the
//                lower index among equal keys; a NaN never replaces and is never replaced, so it wins at index 0 only (key
//                +inf there, -inf elsewhere).  coin = draw(2): (parent, child) = (b, a) when set, else (a, b)
//   learn      : learn_with_hint: the child's nodes, then per child the parent's nodes, shuffled in registers (Fisher-Yates, a lane
//                per element, the parent shuffles accumulating); per candidate parent -> child: refused at max_parents parents
//                or a NaN term; else eval_next = the learner's score with the edge, kept iff eval_next < eval_now.  No cycle
//                and no existing-edge check: two clusters meet once and their edges run one way between disjoint node sets
//   merge      : the two ids leave the cluster list (stable compaction), the new id is appended
//   prune      : ONE stable compaction takes out the merged pair and every entry that joins a live cluster with the parent or
//                the child, noting per live cluster the values it lost (the reference erases them cluster by cluster; the result
//                is the same list, and its closing sweep finds nothing).  Then a lane per live cluster c: new_value =
//                make_similarity(new, c), one divide and one add per node pair, new's nodes outer; two connections: p =
//                pow(alpha, new_value / average); one: p = pow(alpha, old_value / that connection's value); none: no draw.
//                The uniforms are drawn in cluster order, one per cluster with a connection; u < p prunes, otherwise (c, new,
//                new_value) is appended, in cluster order.  IEEE arithmetic as it falls: u < NaN keeps the pair
// Random stream: run j owns xoshiro128++ seeded by Philox4x32-10({j_lo, j_hi, 0, 0}, {seed_lo, seed_hi}) (bn_rng_dev.hpp); one
// step per draw.  Order per merge: the coin, the child shuffle, per child its parent shuffle, the uniforms.
// Vector stores only, no atomics: every output word has one writer.
#include <hip/hip_runtime.h>

#include <climits>

#include "bn_learn_dev.hpp"
#include "bn_learn_hc.hpp"

namespace bnmi {

namespace {

// Fisher-Yates over the first `len` lanes of x: for i = len - 1 .. 1: j = draw(i + 1); swap(x[i], x[j])
__device__ __forceinline__ int shuffle_lanes(uint4& g, int x, int len, int lane) {
    for (int i = len - 1; i >= 1; --i) {
        const int j = uni(int(draw_below(g, uint32_t(i + 1))));
        const int xi = int(lane_u32(uint32_t(x), i)), xj = int(lane_u32(uint32_t(x), j));
        x = lane == i ? xj : lane == j ? xi : x;
    }
    return x;
}

}  // namespace

__global__ __launch_bounds__(kHcWaves * 64) void learn_hc_kernel(HcArgs a) {
    __shared__ uint32_t s_tab[kTermTabWords];
    __shared__ double s_val[kHcWaves][kHcMaxSims];
    __shared__ double s_cval[kHcWaves][2][kHcMaxIds];
    __shared__ uint16_t s_start[kHcWaves][kHcMaxIds];
    __shared__ uint8_t s_sa[kHcWaves][kHcMaxSims], s_sb[kHcWaves][kHcMaxSims];
    __shared__ uint8_t s_nodes[kHcWaves][kHcNodeBytes];
    __shared__ uint8_t s_len[kHcWaves][kHcMaxIds], s_ccnt[kHcWaves][2][kHcMaxIds], s_clusters[kHcWaves][64];
    const SearchWave w = search_enter<kHcWaves>(s_tab, a);
    if (w.surplus) return;
    const int wave = w.wave, lane = w.lane, run = w.run;
    double* val = s_val[wave];
    uint8_t *sa = s_sa[wave], *sb = s_sb[wave], *nodes = s_nodes[wave], *len = s_len[wave], *clusters = s_clusters[wave];
    uint16_t* start = s_start[wave];
    const int n = a.n;
    const bool node = lane < n;
    const uint64_t below = (uint64_t(1) << lane) - 1;

    // the empty graph (:134)
    uint64_t pm = 0;
    int64_t rows = 1;
    double ll = node ? a.terms[int64_t(lane) * a.T] : 0.0;
    const int32_t kk = node ? a.k[lane] : 1;
    int64_t params = a.params0;

    // one cluster per node, every pair i < j in row-major order (:148-188)
    if (node) {
        clusters[lane] = uint8_t(lane);
        nodes[lane] = uint8_t(lane);
        start[lane] = uint16_t(lane);
        len[lane] = 1;
    }
    int nc = n, top = n, m = 0;
    for (int i = 0; i + 1 < n; ++i) {
        const int j = i + 1 + lane;
        if (j < n) {
            sa[m + lane] = uint8_t(i);
            sb[m + lane] = uint8_t(j);
            val[m + lane] = 0.0 + a.S[i * n + j] / 1.0;
        }
        m += n - 1 - i;
    }
    wave_sync();

    uint4 g = seed_stream(run, a.seed_lo, a.seed_hi);

    double current = evaluate_terms(ll, params, n, a.criterion, a.penalty);
    uint32_t merges = 0, tried = 0, kept = 0, pruned = 0, pairs_kept = 0, visits = 0;
    const bool traced = run == a.trace_run && a.trace != nullptr;
    auto trace = [&](uint32_t at, double value, int kind, int x, int y, int z) {
        if (at < a.trace_cap) a.trace[at] = HcTrace{uint64_t(__double_as_longlong(value)), uint8_t(kind), uint8_t(x), uint8_t(y), uint8_t(z), 0u};
    };

    while (nc != 1 && m != 0) {
        // ---- the first maximum of the list
        double best_key = 0.0;
        int best = INT_MAX;
        for (int i = lane; i < m; i += 64) {
            const double v = val[i];
            const double key = v != v ? (i == 0 ? __builtin_inf() : -__builtin_inf()) : v;
            if (best == INT_MAX || key > best_key) {
                best_key = key;
                best = i;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double other_key = __shfl_xor(best_key, off);
            const int other = __shfl_xor(best, off);
            if (other != INT_MAX && (best == INT_MAX || other_key > best_key || (other_key == best_key && other < best))) {
                best_key = other_key;
                best = other;
            }
        }
        best = uni(best);
        const int id_a = uni(int(sa[best])), id_b = uni(int(sb[best]));
        const double old_value = lane_f64(val[best], 0);
        const int coin = uni(int(draw_below(g, 2u)));
        const int parent = coin ? id_b : id_a, child = coin ? id_a : id_b;
        const int new_id = n + int(merges);
        if (traced && lane == 0) trace(merges + visits, old_value, 0, parent, child, coin);

        // ---- learn_with_hint(nodes(parent), nodes(child))
        const int p_start = uni(int(start[parent])), p_len = uni(int(len[parent]));
        const int c_start = uni(int(start[child])), c_len = uni(int(len[child]));
        int xs = lane < c_len ? int(nodes[c_start + lane]) : 0;
        int ys = lane < p_len ? int(nodes[p_start + lane]) : 0;
        xs = shuffle_lanes(g, xs, c_len, lane);
        for (int ci = 0; ci < c_len; ++ci) {
            const int c = int(lane_u32(uint32_t(xs), ci));
            ys = shuffle_lanes(g, ys, p_len, lane);
            for (int pi = 0; pi < p_len; ++pi) {
                const int p = int(lane_u32(uint32_t(ys), pi));
                if (__popcll(lane_u64(pm, c)) >= a.max_parents) continue;
                const uint32_t k_p = lane_u32(uint32_t(kk), p);
                uint64_t pm_new = pm;
                int64_t rows_new = rows;
                double ll_new = ll;
                if (lane == c) {
                    with_parent(pm, rows, p, k_p, pm_new, rows_new);
                    ll_new = term_of(a.terms, a.T, s_tab, lane, pm_new);
                }
                const double added = lane_f64(ll_new, c);
                if (added != added) continue;   // a family over the per-family limit
                ++tried;
                const int64_t params_new = params + params_delta(kk, rows, rows_new, c, c, false);
                const double next = evaluate_terms(ll_new, params_new, n, a.criterion, a.penalty);
                if (next < current) {
                    pm = pm_new;
                    rows = rows_new;
                    ll = ll_new;
                    params = params_new;
                    current = next;
                    ++kept;
                }
            }
        }

        // ---- merge: the new cluster's nodes are the parent's then the child's, in their stored order (:204-217)
        const int new_len = p_len + c_len;
        if (lane < p_len) nodes[top + lane] = nodes[p_start + lane];
        if (lane < c_len) nodes[top + p_len + lane] = nodes[c_start + lane];
        if (lane == 0) {
            start[new_id] = uint16_t(top);
            len[new_id] = uint8_t(new_len);
        }
        const int new_start = top;
        top += new_len;
        {
            const int id = lane < nc ? int(clusters[lane]) : -1;
            const bool keep = lane < nc && id != parent && id != child;
            const uint64_t mask = __ballot(keep);
            wave_sync();
            if (keep) clusters[__popcll(mask & below)] = uint8_t(id);
            nc -= 2;
            if (lane == 0) clusters[nc] = uint8_t(new_id);
            ++nc;
        }
        ++merges;
        for (int i = lane; i < kHcMaxIds; i += 64) s_ccnt[wave][0][i] = s_ccnt[wave][1][i] = 0;
        wave_sync();

        // ---- prune (:299-348): one stable compaction of the list ...
        int out = 0;
        for (int base = 0; base < m; base += 64) {
            const int j = base + lane;
            const bool in = j < m;
            const int ea = in ? int(sa[j]) : 0, eb = in ? int(sb[j]) : 0;
            const double ev = in ? val[j] : 0.0;
            const bool dead_a = in && (ea == parent || ea == child), dead_b = in && (eb == parent || eb == child);
            const bool keep = in && !dead_a && !dead_b;
            if (dead_a != dead_b) {   // (both: the merged pair itself)
                const int other = dead_a ? eb : ea, which = (dead_a ? ea : eb) == parent ? 0 : 1;
                s_ccnt[wave][which][other] = 1;
                s_cval[wave][which][other] = ev;
            }
            const uint64_t mask = __ballot(keep);
            const int at = out + __popcll(mask & below);
            wave_sync();   // (every lane has read its entry: a kept one moves to a place at or before its own)
            if (keep) {
                sa[at] = uint8_t(ea);
                sb[at] = uint8_t(eb);
                val[at] = ev;
            }
            out += __popcll(mask);
            wave_sync();
        }
        m = out;

        // ... then a lane per live cluster other than the new one
        const int n_visits = nc - 1;
        const bool visiting = lane < n_visits;
        const int c_id = visiting ? int(clusters[lane]) : 0;
        int connections = 0;
        double new_value = 0.0, prob = 0.0;
        if (visiting) {
            const int o_start = int(start[c_id]), o_len = int(len[c_id]);
            const double count = double(new_len * o_len);
            for (int x = 0; x < new_len; ++x) {
                const double* row = a.S + int(nodes[new_start + x]) * n;
                for (int y = 0; y < o_len; ++y) new_value += row[int(nodes[o_start + y])] / count;
            }
            const int with_parent = int(s_ccnt[wave][0][c_id]), with_child = int(s_ccnt[wave][1][c_id]);
            connections = with_parent + with_child;
            if (connections == 2) prob = pow(a.alpha, new_value / a.average);
            else if (connections == 1) prob = pow(a.alpha, old_value / s_cval[wave][with_parent ? 0 : 1][c_id]);
        }
        const bool drawing = connections > 0;
        const uint64_t draw_mask = __ballot(drawing);
        const int n_draws = __popcll(draw_mask), my_draw = __popcll(draw_mask & below);
        double u = 0.0;
        for (int t = 0; t < n_draws; ++t) {
            const uint32_t r = xoshiro_next(g);
            if (my_draw == t) u = (double(r) + 0.5) * 0x1p-32;
        }
        const bool cut = drawing && u < prob, keep_pair = drawing && !cut;
        const uint64_t keep_mask = __ballot(keep_pair);
        const int at = m + __popcll(keep_mask & below);
        if (keep_pair && at < kHcMaxSims) {   // (at most C(live clusters, 2) entries: never over; the bound guards the array)
            sa[at] = uint8_t(c_id);
            sb[at] = uint8_t(new_id);
            val[at] = new_value;
        }
        m = min(m + __popcll(keep_mask), kHcMaxSims);
        pruned += uint32_t(__popcll(__ballot(cut)));
        pairs_kept += uint32_t(__popcll(keep_mask));
        if (traced && visiting) trace(merges + visits + uint32_t(lane), new_value, 1, c_id, connections, cut ? 1 : 0);
        visits += uint32_t(n_visits);
        wave_sync();
    }

    const uint32_t flags = (nc == 1 ? kHcOneCluster : 0u) | (m == 0 ? kHcNoSimilarity : 0u);
    if (lane == 0) a.rec[run] = HcRecord{current, merges, tried, kept, pruned, pairs_kept, flags, visits, 0u};
    store_graph(a, run, lane, pm, ll);
}

int learn_launch_hc(const HcArgs& a, void* stream) { return launch_search<kHcWaves>(learn_hc_kernel, a, stream); }

}  // namespace bnmi
