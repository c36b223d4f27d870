// bn_learn_batch.cpp -- the device half of a batch of family scores: run_groups uploads a plan of bn_learn_plan.cpp, counts and scores
// pass by pass (bn_learn_kernels.hip, bn_learn_bd.hip) and scatters the terms back into input order; run_subsets counts the top family
// once and sums every subset's family out of it (bn_learn_lattice.hip).  C ABI: bn_learn_score_groups[_spec], bn_learn_score_subsets[_spec].
// The logarithm is the device's fp64 log: a family term is its own stated function of the counts.
#include "bn_learn_internal.hpp"

namespace {

int launch_score(const bn_score_spec& spec, const LearnArgs& a, int32_t fam0, int32_t n_fams, void* stream) {
    return spec.kind == 0 ? learn_launch_score(a, fam0, n_fams, stream) : learn_launch_score_bd(a, fam0, n_fams, spec.kind, spec.ess, stream);
}

int cu_count(const bn_info_table* t) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus <= 0) cus = 256;
    return cus;
}

}  // namespace

// Workgroups the patterns are split over per chunk.  A short batch leaves a long table to a handful of CUs: split the patterns until
// about four workgroups per CU exist, each keeping at least two tiles (bn_score_nodes' rule).  BN_LEARN_SPLITS > 0 fixes the number.
int bn_eng::count_splits(const bn_info_table* t, int32_t n_chunks) {
    int splits = 0;
    if (const char* env = std::getenv("BN_LEARN_SPLITS")) splits = std::atoi(env);
    if (splits <= 0) {
        const int64_t by_chip = (int64_t(4) * cu_count(t) + n_chunks - 1) / std::max(n_chunks, 1);
        const int64_t by_work = (t->P + 2 * kLearnTile - 1) / (2 * kLearnTile);
        splits = int(std::min(by_chip, by_work));
    }
    return std::max(1, std::min(splits, 65535));
}

int bn_eng::run_groups(bn_info_table* t, const bn_score_spec& spec, const std::vector<GroupIn>& groups, double* ll_out, uint64_t* counts_out,
                       LearnTimes* times) {
    GroupPlan plan;   // (read by the uploads: alive until the stream has been synchronised)
    if (int r = plan_groups(t->k.data(), t->n, groups, kLearnMaxScratchCells, plan)) return r;
    const size_t n_fams = plan.fams.size();
    if (n_fams == 0) return BN_OK;

    ON_DEVICE(t);
    hipStream_t s = t->stream;
    DeviceBuf<LearnChunk> d_chunks;
    DeviceBuf<LearnFamily> d_fams;
    DeviceBuf<int32_t> d_par_id, d_par_k, d_cand_id, d_cand_k, d_cand_cell;
    DeviceBuf<unsigned long long> d_N, d_out;
    DeviceBuf<double> d_ll;
    EventOwner ev0, ev1, ev2;
    int r;
    if ((r = upload(d_chunks, plan.chunks, s)) || (r = upload(d_fams, plan.fams, s)) || (r = upload(d_par_id, plan.par_id, s)) ||
        (r = upload(d_par_k, plan.par_k, s)) || (r = upload(d_cand_id, plan.cand_id, s)) || (r = upload(d_cand_k, plan.cand_k, s)) ||
        (r = upload(d_cand_cell, plan.cand_cell, s)) || (r = dalloc(d_N, size_t(plan.scratch_cells))) || (r = dalloc(d_ll, n_fams)))
        return r;
    if (counts_out && (r = dalloc(d_out, size_t(plan.out_cells)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    HIPCHK(hipEventCreate(ev2.put()));
    const LearnArgs a{t->d_T, t->d_w, t->P, t->Ppad, d_chunks, d_par_id, d_par_k, d_cand_id, d_cand_k, d_cand_cell, d_N, d_fams, d_ll,
                      counts_out ? d_out.get() : nullptr};
    double call_count_ns = 0.0, call_score_ns = 0.0;
    for (const LearnPass& p : plan.passes) {
        HIPCHK(hipEventRecord(ev0, s));
        HIPCHK(hipMemsetAsync(d_N, 0, size_t(std::max<int64_t>(p.cells, 1)) * 8, s));
        if (int err = learn_launch_count(a, p.chunk0, p.n_chunks, count_splits(t, p.n_chunks), s))
            return fail(BN_ERR_HIP, std::string("family-group count kernel: ") + hipGetErrorString(hipError_t(err)));
        HIPCHK(hipEventRecord(ev1, s));
        if (int err = launch_score(spec, a, p.fam0, p.n_fams, s))
            return fail(BN_ERR_HIP, std::string("family score kernel: ") + hipGetErrorString(hipError_t(err)));
        HIPCHK(hipEventRecord(ev2, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms_count = 0.0f, ms_score = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms_count, ev0, ev1));
        HIPCHK(hipEventElapsedTime(&ms_score, ev1, ev2));
        call_count_ns += double(ms_count) * 1e6;
        call_score_ns += double(ms_score) * 1e6;
    }
    std::vector<double> ll(n_fams);
    HIPCHK(hipMemcpyAsync(ll.data(), d_ll, n_fams * 8, hipMemcpyDeviceToHost, s));
    if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, d_out, size_t(plan.out_cells) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n_fams; ++i) ll_out[size_t(plan.order[i])] = ll[i];
    t->learn_count_ns = call_count_ns;
    t->learn_lattice_ns = 0.0;
    t->learn_score_ns = call_score_ns;
    if (times) {
        times->count_ns += call_count_ns;
        times->score_ns += call_score_ns;
        times->families += int64_t(n_fams);
        times->passes += 1;
        for (const LearnChunk& c : plan.chunks) times->count_bytes += t->P * int64_t(8 + c.n_base + 1 + c.n_cand);
    }
    return BN_OK;
}

int bn_eng::run_subsets(bn_info_table* t, const bn_score_spec& spec, int32_t child, int32_t n_base, const int32_t* base, int32_t m,
                        const int32_t* cand, double* ll_out, uint64_t* counts_out, LearnTimes* times) {
    SubsetPlan sh;   // (read by the uploads: alive until the stream has been synchronised)
    if (int r = plan_subsets(t->k.data(), t->n, child, n_base, base, m, cand, kLearnMaxScratchCells, sh)) return r;
    const int32_t nv = sh.nv, n_fams = sh.n_fams, full = n_fams - 1;
    const int64_t top_at = sh.fams[size_t(full)].count_at;

    ON_DEVICE(t);
    hipStream_t s = t->stream;
    DeviceBuf<LearnChunk> d_chunks;
    DeviceBuf<LearnFamily> d_fams;
    DeviceBuf<LatticeStep> d_steps;
    DeviceBuf<int32_t> d_par_id, d_par_k;
    DeviceBuf<unsigned long long> d_N, d_out;
    DeviceBuf<double> d_ll;
    EventOwner ev0, ev1, ev2, ev3;
    int r;
    if ((r = upload(d_chunks, sh.chunks, s)) || (r = upload(d_fams, sh.fams, s)) || (r = upload(d_steps, sh.steps, s)) ||
        (r = upload(d_par_id, sh.id, s)) || (r = upload(d_par_k, sh.k, s)) || (r = dalloc(d_N, size_t(sh.all_cells))) ||
        (r = dalloc(d_ll, size_t(n_fams))))
        return r;
    if (counts_out && (r = dalloc(d_out, size_t(sh.all_cells)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    HIPCHK(hipEventCreate(ev2.put()));
    HIPCHK(hipEventCreate(ev3.put()));
    const LearnArgs a{t->d_T, t->d_w, t->P, t->Ppad, d_chunks, d_par_id, d_par_k, nullptr, nullptr, nullptr, d_N, d_fams, d_ll,
                      counts_out ? d_out.get() : nullptr};
    HIPCHK(hipEventRecord(ev0, s));
    HIPCHK(hipMemsetAsync(d_N.get() + top_at, 0, size_t(sh.top_cells) * 8, s));   // (the lattice writes every other cell)
    if (int err = learn_launch_count(a, 0, 1, count_splits(t, 1), s))
        return fail(BN_ERR_HIP, std::string("top-family count kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev1, s));
    if (sh.lds) {
        LatticeLds la{d_N, d_fams, n_fams, nv, int32_t(sh.top_cells), 0, {}, {}};
        for (int32_t p = 0; p < nv; ++p) {
            la.k[p] = sh.k[size_t(p)];
            la.bit[p] = sh.bit[size_t(p)];
        }
        // 56 KiB of LDS per workgroup: two per CU
        if (int err = learn_launch_lattice_lds(la, std::min(full, 2 * cu_count(t)), s))
            return fail(BN_ERR_HIP, std::string("subset lattice kernel: ") + hipGetErrorString(hipError_t(err)));
    } else {
        for (int32_t l = 1; l <= m; ++l)
            if (int err = learn_launch_lattice_level(d_N, d_steps, sh.level_at[size_t(l)], sh.level_at[size_t(l) + 1] - sh.level_at[size_t(l)],
                                                     sh.level_max[size_t(l)], s))
                return fail(BN_ERR_HIP, std::string("subset lattice level kernel: ") + hipGetErrorString(hipError_t(err)));
    }
    HIPCHK(hipEventRecord(ev2, s));
    if (int err = launch_score(spec, a, 0, n_fams, s))
        return fail(BN_ERR_HIP, std::string("family score kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev3, s));
    HIPCHK(hipMemcpyAsync(ll_out, d_ll, size_t(n_fams) * 8, hipMemcpyDeviceToHost, s));
    if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, d_out, size_t(sh.all_cells) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms_count = 0.0f, ms_lattice = 0.0f, ms_score = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms_count, ev0, ev1));
    HIPCHK(hipEventElapsedTime(&ms_lattice, ev1, ev2));
    HIPCHK(hipEventElapsedTime(&ms_score, ev2, ev3));
    t->learn_count_ns = double(ms_count) * 1e6;
    t->learn_lattice_ns = double(ms_lattice) * 1e6;
    t->learn_score_ns = double(ms_score) * 1e6;
    if (times) {
        times->count_ns += t->learn_count_ns;
        times->lattice_ns += t->learn_lattice_ns;
        times->score_ns += t->learn_score_ns;
        times->families += n_fams;
        times->subsets += n_fams;
        times->passes += 1;
        times->count_bytes += t->P * int64_t(8 + nv + 1);
    }
    return BN_OK;
}

extern "C" int bn_learn_score_groups_spec(bn_info_table* t, const bn_score_spec* spec_in, int32_t n_groups, const int32_t* child,
                                          const int32_t* base_ptr, const int32_t* base_idx, const int32_t* cand_ptr, const int32_t* cand_idx,
                                          double* ll_out, uint64_t* counts_out) {
    if (!t || !ll_out) return fail(BN_ERR_ARG, "null argument");
    bn_score_spec spec;
    if (int r = check_spec(spec_in, spec)) return r;
    if (n_groups < 0) return fail(BN_ERR_ARG, "n_groups < 0");
    if (n_groups > 0 && (!child || !base_ptr || !cand_ptr)) return fail(BN_ERR_ARG, "null argument");
    std::vector<GroupIn> groups(static_cast<size_t>(n_groups));
    for (int32_t g = 0; g < n_groups; ++g) {
        const int32_t b0 = base_ptr[g], b1 = base_ptr[g + 1], c0 = cand_ptr[g], c1 = cand_ptr[g + 1];
        if (b0 < 0 || b1 < b0 || c0 < 0 || c1 < c0 || (b1 > b0 && !base_idx) || (c1 > c0 && !cand_idx))
            return fail(BN_ERR_ARG, "group " + std::to_string(g) + ": bad parent or candidate list");
        groups[size_t(g)] = GroupIn{child[g], base_idx ? base_idx + b0 : nullptr, b1 - b0, cand_idx ? cand_idx + c0 : nullptr, c1 - c0};
    }
    return run_groups(t, spec, groups, ll_out, counts_out, nullptr);
}

extern "C" int bn_learn_score_groups(bn_info_table* t, int32_t n_groups, const int32_t* child, const int32_t* base_ptr,
                                     const int32_t* base_idx, const int32_t* cand_ptr, const int32_t* cand_idx, double* ll_out,
                                     uint64_t* counts_out) {
    return bn_learn_score_groups_spec(t, nullptr, n_groups, child, base_ptr, base_idx, cand_ptr, cand_idx, ll_out, counts_out);
}

extern "C" int bn_learn_score_subsets_spec(bn_info_table* t, const bn_score_spec* spec_in, int32_t child, int32_t n_base, const int32_t* base,
                                           int32_t m, const int32_t* cand, double* ll_out, uint64_t* counts_out) {
    if (!t || !ll_out) return fail(BN_ERR_ARG, "null argument");
    bn_score_spec spec;
    if (int r = check_spec(spec_in, spec)) return r;
    return run_subsets(t, spec, child, n_base, base, m, cand, ll_out, counts_out, nullptr);
}

extern "C" int bn_learn_score_subsets(bn_info_table* t, int32_t child, int32_t n_base, const int32_t* base, int32_t m, const int32_t* cand,
                                      double* ll_out, uint64_t* counts_out) {
    return bn_learn_score_subsets_spec(t, nullptr, child, n_base, base, m, cand, ll_out, counts_out);
}
