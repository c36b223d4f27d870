// bn_learn_pc.cpp -- constraint-based structure learning on the device: run_ci counts a batch of test groups through the family
// counting launch and its planner (bn_learn_kernels.hip, bn_learn_plan.cpp, both as they are) and takes statistic, degrees of freedom,
// p-value and decision per test (bn_ci.hip); bn_ci_tests is that for a caller's list of tests, bn_learn_pc the PC-stable skeleton level
// by level (bn_ci_plan.cpp plans a level, the device decides it, the host reads back one rank per edge) followed by the orientation
// rules (bn_ci_orient.cpp).  C ABI: bn_ci_tests, bn_ci_chisq_sf, bn_learn_pc, bn_pdag_to_dag (include/bn_mi355x.h).
#include "bn_ci.hpp"
#include "bn_ci_orient.hpp"
#include "bn_ci_plan.hpp"
#include "bn_learn_internal.hpp"

namespace {

// cells of the count scratch per pass.  BN_CI_SCRATCH_CELLS > 0 lowers it (a test arrangement: small batches then take several
// passes / chunks; no result depends on it).
int64_t ci_scratch_cells() {
    int64_t cap = kLearnMaxScratchCells;
    if (const char* env = std::getenv("BN_CI_SCRATCH_CELLS")) {
        const long long v = std::atoll(env);
        if (v > 0) cap = std::min<int64_t>(cap, v);
    }
    return cap;
}

std::vector<GroupIn> groups_of(const CiGroups& g, int32_t g0, int32_t g1) {
    std::vector<GroupIn> out;
    out.reserve(size_t(g1 - g0));
    for (int32_t i = g0; i < g1; ++i)
        out.push_back(GroupIn{g.child[size_t(i)], g.base_idx.data() + g.base_ptr[size_t(i)], g.base_ptr[size_t(i) + 1] - g.base_ptr[size_t(i)],
                              g.cand_idx.data() + g.cand_ptr[size_t(i)], g.cand_ptr[size_t(i) + 1] - g.cand_ptr[size_t(i)]});
    return out;
}

struct CiOut {   // host destinations by slot (the candidates of the groups, group-major); any may be null
    double* stat = nullptr;
    int64_t* df = nullptr;
    double* p = nullptr;
    std::vector<uint64_t>* counts = nullptr;   // every slot's N[s][b][a] back to back
    std::vector<int64_t>* counts_at = nullptr; // [slots + 1]
};

// edge / rank: per slot, or null (no decision is recorded); d_edge_rank: the per-edge ranks on the device
int run_ci(bn_info_table* t, const std::vector<GroupIn>& groups, const int32_t* edge, const uint32_t* rank, int32_t df_rule, double alpha,
           uint32_t* d_edge_rank, const CiOut& out, double& count_ns, double& stat_ns) {
    GroupPlan plan;   // (read by the uploads: alive until the stream has been synchronised)
    if (int r = plan_groups(t->k.data(), t->n, groups, ci_scratch_cells(), plan)) return r;
    const size_t n_fams = plan.fams.size();
    // input family f (group-major, base first) -> slot, or -1 for a base
    std::vector<int32_t> slot_of(n_fams, -1);
    int32_t n_slots = 0;
    {
        size_t f = 0;
        for (const GroupIn& g : groups) {
            ++f;
            for (int32_t j = 0; j < g.n_cand; ++j) slot_of[f++] = n_slots++;
        }
    }
    if (n_slots == 0) return BN_OK;
    std::vector<int64_t> out_at(size_t(n_slots) + 1, 0);
    for (size_t i = 0; i < n_fams; ++i) {
        const int32_t s = slot_of[size_t(plan.order[i])];
        if (s >= 0) out_at[size_t(s) + 1] = plan.fams[i].entries;
    }
    for (int32_t s = 0; s < n_slots; ++s) out_at[size_t(s) + 1] += out_at[size_t(s)];
    std::vector<CiTest> tests;   // in launch order: by pass
    std::vector<std::pair<int32_t, int32_t>> pass_tests;
    tests.reserve(size_t(n_slots));
    for (const LearnPass& p : plan.passes) {
        const int32_t first = int32_t(tests.size());
        for (int32_t i = p.fam0; i < p.fam0 + p.n_fams; ++i) {
            const int32_t s = slot_of[size_t(plan.order[size_t(i)])];
            if (s < 0) continue;
            const LearnFamily& f = plan.fams[size_t(i)];
            tests.push_back(CiTest{f.count_at, out_at[size_t(s)], f.entries, f.kc, f.ku, s, edge ? edge[s] : -1, rank ? rank[s] : kCiNoRank});
        }
        pass_tests.emplace_back(first, int32_t(tests.size()) - first);
    }

    ON_DEVICE(t);
    hipStream_t s = t->stream;
    DeviceBuf<LearnChunk> d_chunks;
    DeviceBuf<LearnFamily> d_fams;
    DeviceBuf<CiTest> d_tests;
    DeviceBuf<int32_t> d_par_id, d_par_k, d_cand_id, d_cand_k, d_cand_cell;
    DeviceBuf<unsigned long long> d_N, d_out;
    DeviceBuf<double> d_stat, d_p;
    DeviceBuf<long long> d_df;
    EventOwner ev0, ev1, ev2;
    int r;
    if ((r = upload(d_chunks, plan.chunks, s)) || (r = upload(d_fams, plan.fams, s)) || (r = upload(d_tests, tests, s)) ||
        (r = upload(d_par_id, plan.par_id, s)) || (r = upload(d_par_k, plan.par_k, s)) || (r = upload(d_cand_id, plan.cand_id, s)) ||
        (r = upload(d_cand_k, plan.cand_k, s)) || (r = upload(d_cand_cell, plan.cand_cell, s)) ||
        (r = dalloc(d_N, size_t(plan.scratch_cells))) || (r = dalloc(d_stat, size_t(n_slots))) || (r = dalloc(d_p, size_t(n_slots))) ||
        (r = dalloc(d_df, size_t(n_slots))))
        return r;
    if (out.counts && (r = dalloc(d_out, size_t(out_at.back())))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    HIPCHK(hipEventCreate(ev2.put()));
    const LearnArgs la{t->d_T, t->d_w, t->P, t->Ppad, d_chunks, d_par_id, d_par_k, d_cand_id, d_cand_k, d_cand_cell, d_N, d_fams, nullptr, nullptr};
    const CiArgs ca{d_N, d_tests, d_stat, d_df, d_p, out.counts ? d_out.get() : nullptr, d_edge_rank, df_rule, 0, alpha};
    for (size_t pi = 0; pi < plan.passes.size(); ++pi) {
        const LearnPass& p = plan.passes[pi];
        HIPCHK(hipEventRecord(ev0, s));
        HIPCHK(hipMemsetAsync(d_N, 0, size_t(std::max<int64_t>(p.cells, 1)) * 8, s));
        if (int err = learn_launch_count(la, p.chunk0, p.n_chunks, count_splits(t, p.n_chunks), s))
            return fail(BN_ERR_HIP, std::string("test-group count kernel: ") + hipGetErrorString(hipError_t(err)));
        HIPCHK(hipEventRecord(ev1, s));
        if (int err = ci_launch_stat(ca, pass_tests[pi].first, pass_tests[pi].second, s))
            return fail(BN_ERR_HIP, std::string("test statistic kernel: ") + hipGetErrorString(hipError_t(err)));
        HIPCHK(hipEventRecord(ev2, s));
        HIPCHK(hipStreamSynchronize(s));
        t->ci_launches += 1 + (pass_tests[pi].second > 0 ? 1 : 0);
        float ms_count = 0.0f, ms_stat = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms_count, ev0, ev1));
        HIPCHK(hipEventElapsedTime(&ms_stat, ev1, ev2));
        count_ns += double(ms_count) * 1e6;
        stat_ns += double(ms_stat) * 1e6;
    }
    if (out.stat) HIPCHK(hipMemcpyAsync(out.stat, d_stat, size_t(n_slots) * 8, hipMemcpyDeviceToHost, s));
    if (out.df) HIPCHK(hipMemcpyAsync(out.df, d_df, size_t(n_slots) * 8, hipMemcpyDeviceToHost, s));
    if (out.p) HIPCHK(hipMemcpyAsync(out.p, d_p, size_t(n_slots) * 8, hipMemcpyDeviceToHost, s));
    if (out.counts) {
        out.counts->resize(size_t(out_at.back()));
        HIPCHK(hipMemcpyAsync(out.counts->data(), d_out, size_t(out_at.back()) * 8, hipMemcpyDeviceToHost, s));
        *out.counts_at = out_at;
    }
    HIPCHK(hipStreamSynchronize(s));
    return BN_OK;
}

int check_rule_alpha(int32_t df_rule, double alpha) {
    if (df_rule != 0 && df_rule != 1) return fail(BN_ERR_ARG, "df_rule " + std::to_string(df_rule) + " (0 nominal, 1 adjusted)");
    if (!(alpha > 0.0 && alpha < 1.0)) return fail(BN_ERR_ARG, "alpha must be inside (0, 1)");
    return BN_OK;
}

}  // namespace

extern "C" int bn_ci_tests(bn_info_table* t, int32_t n_tests, const int32_t* x, const int32_t* y, const int32_t* s_ptr, const int32_t* s_idx,
                           int32_t df_rule, double alpha, double* stat_out, int64_t* df_out, double* p_out, uint8_t* indep_out,
                           uint64_t* counts_out) {
    if (!t) return fail(BN_ERR_ARG, "null argument");
    t->ci_count_ns = t->ci_stat_ns = 0.0;
    if (n_tests < 0) return fail(BN_ERR_ARG, "n_tests < 0");
    if (n_tests > 0 && (!x || !y || !s_ptr || !stat_out || !df_out || !p_out)) return fail(BN_ERR_ARG, "null argument");
    if (int r = check_rule_alpha(df_rule, alpha)) return r;
    std::vector<CiTestIn> in(static_cast<size_t>(n_tests));
    for (int32_t i = 0; i < n_tests; ++i) {
        const int32_t s0 = s_ptr[i], s1 = s_ptr[i + 1];
        if (s0 < 0 || s1 < s0 || (s1 > s0 && !s_idx)) return fail(BN_ERR_ARG, "test " + std::to_string(i) + ": bad conditioning set");
        in[size_t(i)] = CiTestIn{x[i], y[i], s_idx ? s_idx + s0 : nullptr, s1 - s0};
    }
    CiGroups g;
    std::vector<int32_t> slot;
    if (int r = ci_group_tests(t->k.data(), t->n, in, g, slot)) return r;
    if (n_tests == 0) return BN_OK;
    const size_t slots = size_t(g.tests());
    std::vector<double> stat(slots), p(slots);
    std::vector<int64_t> df(slots), counts_at;
    std::vector<uint64_t> counts;
    CiOut out;
    out.stat = stat.data();
    out.df = df.data();
    out.p = p.data();
    if (counts_out) {
        out.counts = &counts;
        out.counts_at = &counts_at;
    }
    double count_ns = 0.0, stat_ns = 0.0;
    if (int r = run_ci(t, groups_of(g, 0, g.groups()), nullptr, nullptr, df_rule, alpha, nullptr, out, count_ns, stat_ns)) return r;
    t->ci_count_ns = count_ns;
    t->ci_stat_ns = stat_ns;
    int64_t at = 0;
    for (int32_t i = 0; i < n_tests; ++i) {
        const size_t s = size_t(slot[size_t(i)]);
        stat_out[i] = stat[s];
        df_out[i] = df[s];
        p_out[i] = p[s];
        if (indep_out) indep_out[i] = p[s] > alpha ? 1 : 0;
        if (counts_out) {
            const int64_t cells = counts_at[s + 1] - counts_at[s];
            std::copy(counts.begin() + counts_at[s], counts.begin() + counts_at[s + 1], counts_out + at);
            at += cells;
        }
    }
    return BN_OK;
}

extern "C" int bn_ci_chisq_sf(int64_t n, const double* g, const int64_t* df, double* p_out) {
    if (n < 0 || (n > 0 && (!g || !df || !p_out))) return fail(BN_ERR_ARG, "null argument or n < 0");
    for (int64_t i = 0; i < n; ++i) {
        if (!(std::isfinite(g[i]) && g[i] >= 0.0)) return fail(BN_ERR_ARG, "entry " + std::to_string(i) + ": G must be finite and >= 0");
        if (df[i] < 0) return fail(BN_ERR_ARG, "entry " + std::to_string(i) + ": df < 0");
    }
    if (n == 0) return BN_OK;
    DeviceBuf<double> d_g, d_p;
    DeviceBuf<long long> d_df;
    int r;
    if ((r = dalloc(d_g, size_t(n))) || (r = dalloc(d_p, size_t(n))) || (r = dalloc(d_df, size_t(n)))) return r;
    HIPCHK(hipMemcpy(d_g, g, size_t(n) * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_df, df, size_t(n) * 8, hipMemcpyHostToDevice));
    if (int err = ci_launch_sf(n, d_g, d_df, d_p, nullptr))
        return fail(BN_ERR_HIP, std::string("chi-square tail kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(p_out, d_p, size_t(n) * 8, hipMemcpyDeviceToHost));
    return BN_OK;
}

extern "C" int bn_learn_pc(bn_info_table* t, const bn_pc_params* params, const uint8_t* start_adj, uint8_t* skeleton_out, uint8_t* cpdag_out,
                           int32_t* sep_len_out, int32_t* sep_idx_out, bn_pc_level* levels_out, int32_t* n_levels_out,
                           int64_t* tests_skipped_out) {
    if (!t || !params || !skeleton_out || !cpdag_out || !sep_len_out || !levels_out || !n_levels_out)
        return fail(BN_ERR_ARG, "null argument");
    t->ci_count_ns = t->ci_stat_ns = 0.0;
    if (int r = check_rule_alpha(params->df_rule, params->alpha)) return r;
    const int32_t max_cond = params->max_cond, n = t->n;
    if (max_cond < 0 || max_cond > kCiPlanMaxCond)
        return fail(BN_ERR_ARG, "bn_learn_pc: max_cond " + std::to_string(max_cond) + " (0 .. " + std::to_string(kCiPlanMaxCond) + ")");
    if (max_cond > 0 && !sep_idx_out) return fail(BN_ERR_ARG, "null argument");
    if (params->max_tests < 0 || params->max_tests > kPcMaxMaxTests)
        return fail(BN_ERR_ARG, "bn_learn_pc: max_tests must be in 0 .. 2^26 (0: the default, 2^22)");
    const int64_t max_tests = params->max_tests ? params->max_tests : kPcDefaultMaxTests;
    if (n > kPcMaxNodes)
        return fail(BN_ERR_ARG, "bn_learn_pc: " + std::to_string(n) + " columns (at most " + std::to_string(kPcMaxNodes) +
                                    ": the per-edge tables are n x n)");
    const size_t N = size_t(n);
    std::vector<uint8_t> skel(N * N, 0);
    for (size_t a = 0; a < N; ++a)
        for (size_t b = 0; b < N; ++b) {
            if (a == b) continue;
            if (!start_adj) skel[a * N + b] = 1;
            else {
                if ((start_adj[a * N + b] != 0) != (start_adj[b * N + a] != 0))
                    return fail(BN_ERR_ARG, "bn_learn_pc: the start adjacency is not symmetric at (" + std::to_string(a) + ", " + std::to_string(b) + ")");
                skel[a * N + b] = start_adj[a * N + b] ? 1 : 0;
            }
        }
    const int32_t stride = max_cond;
    std::vector<int32_t> sep_len(N * N, -1), sep_idx(N * N * size_t(stride), 0);
    std::vector<bn_pc_level> levels;
    int64_t skipped = 0;
    double total_count_ns = 0.0, total_stat_ns = 0.0;
    std::vector<std::vector<int32_t>> adj(N);
    for (int32_t level = 0; level <= max_cond; ++level) {
        for (size_t a = 0; a < N; ++a) {
            adj[a].clear();
            for (size_t b = 0; b < N; ++b)
                if (skel[a * N + b]) adj[a].push_back(int32_t(b));
        }
        PcLevel lv;
        if (int r = pc_plan_level(t->k.data(), adj, level, max_tests, lv)) return r;
        if (!lv.any) break;
        bn_pc_level rec{lv.tests, 0, 0.0, 0.0};
        skipped += lv.skipped;
        if (lv.tests > 0) {
            const size_t n_edges = lv.edge_a.size();
            std::vector<uint32_t> ranks(n_edges);
            {
                ON_DEVICE(t);
                DeviceBuf<uint32_t> d_rank;
                if (int r = dalloc(d_rank, n_edges)) return r;
                HIPCHK(hipMemsetAsync(d_rank, 0xFF, n_edges * 4, t->stream));
                std::vector<std::pair<int32_t, int32_t>> chunks;
                pc_chunks(lv, ci_scratch_cells(), kPcChunkTests, chunks);
                for (const auto& c : chunks) {
                    const int32_t c0 = lv.g.cand_ptr[size_t(c.first)];
                    if (int r = run_ci(t, groups_of(lv.g, c.first, c.second), lv.edge.data() + c0, lv.rank.data() + c0, params->df_rule,
                                       params->alpha, d_rank, CiOut{}, rec.count_ns, rec.stat_ns))
                        return r;
                }
                HIPCHK(hipMemcpyAsync(ranks.data(), d_rank, n_edges * 4, hipMemcpyDeviceToHost, t->stream));
                HIPCHK(hipStreamSynchronize(t->stream));
            }
            for (size_t e = 0; e < n_edges; ++e) {
                if (ranks[e] == kCiNoRank) continue;
                const size_t a = size_t(lv.edge_a[e]), b = size_t(lv.edge_b[e]);
                const std::vector<int32_t> S = pc_unrank(adj, int32_t(a), int32_t(b), level, ranks[e]);
                skel[a * N + b] = skel[b * N + a] = 0;
                sep_len[a * N + b] = sep_len[b * N + a] = level;
                for (size_t j = 0; j < S.size(); ++j) sep_idx[(a * N + b) * size_t(stride) + j] = sep_idx[(b * N + a) * size_t(stride) + j] = S[j];
                ++rec.removed;
            }
        }
        total_count_ns += rec.count_ns;
        total_stat_ns += rec.stat_ns;
        levels.push_back(rec);
    }
    std::copy(skel.begin(), skel.end(), skeleton_out);
    pc_orient_colliders(n, skel.data(), sep_len.data(), sep_idx.data(), stride, cpdag_out);
    pc_meek(n, cpdag_out);
    std::copy(sep_len.begin(), sep_len.end(), sep_len_out);
    if (sep_idx_out) std::copy(sep_idx.begin(), sep_idx.end(), sep_idx_out);
    std::copy(levels.begin(), levels.end(), levels_out);
    *n_levels_out = int32_t(levels.size());
    if (tests_skipped_out) *tests_skipped_out = skipped;
    t->ci_count_ns = total_count_ns;
    t->ci_stat_ns = total_stat_ns;
    return BN_OK;
}

extern "C" int bn_pdag_to_dag(int32_t n, const uint8_t* pdag, int32_t* in_ptr_out, int32_t* in_idx_out) {
    if (n < 0 || (n > 0 && (!pdag || !in_ptr_out))) return fail(BN_ERR_ARG, "null argument or n < 0");
    std::vector<std::vector<int32_t>> parents;
    if (!pdag_to_dag(n, pdag, parents)) return fail(BN_ERR_STATE, "bn_pdag_to_dag: the PDAG has no consistent DAG extension");
    int32_t at = 0;
    if (in_ptr_out) in_ptr_out[0] = 0;
    for (int32_t v = 0; v < n; ++v) {
        if (!parents[size_t(v)].empty() && !in_idx_out) return fail(BN_ERR_ARG, "null argument");
        for (int32_t u : parents[size_t(v)]) in_idx_out[at++] = u;
        in_ptr_out[v + 1] = at;
    }
    return BN_OK;
}
