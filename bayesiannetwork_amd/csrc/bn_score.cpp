// bn_score.cpp -- C ABI of the log-likelihood scores (include/bn_mi355x.h, bn_score_*), reference
// bayesian/evaluation/basic_info_criteria.hpp:44-78 (calc_likelihood over a sampler's table).  Kernels: bn_score_kernels.hip, and
// the counting kernel of the CPT fit (bn_fit_kernels.hip).  The logarithm is taken HERE, on the host, with libm's std::log in
// fp64 -- the device only gathers and adds -- so a result is a function of that table, the patterns and the stated order of additions.
#include <cmath>

#include "bn_engine_internal.hpp"
#include "bn_info_table.hpp"
#include "bn_score.hpp"
#include "../../include/bn_mi355x.h"

namespace {

// L = log(cpt) (log(0) = -inf); with_device: also the device copies of L and of the structure
int ensure_score(bn_engine* e, bool with_device) {
    ScoreState& sc = e->score;
    const Plan& p = e->plan;
    const size_t entries = p.n > 0 ? size_t(p.cpt_off[p.n]) : 0;
    if (p.cpt_flat.size() != entries) return fail(BN_ERR_STATE, "the engine does not hold the flat CPT");
    if (!sc.ready) {
        sc.h_L.resize(entries);
        for (size_t q = 0; q < entries; ++q) sc.h_L[q] = std::log(p.cpt_flat[q]);
        sc.wide = false;
        for (int32_t v = 0; v < p.n; ++v) sc.wide = sc.wide || p.cpt_off[v + 1] - p.cpt_off[v] > int64_t(0xffffffffu);
        sc.d_L.reset();
        sc.ready = true;
    }
    if (!with_device || sc.d_L) return BN_OK;
    int r;
    if ((r = upload(sc.d_k, p.k, e->stream)) || (r = upload(sc.d_in_ptr, p.in_ptr, e->stream)) || (r = upload(sc.d_in_idx, p.in_idx, e->stream)) ||
        (r = upload(sc.d_cpt_off, p.cpt_off, e->stream)))
        return r;
    DeviceBuf<double> d_L;   // (taken over last: a failure on the way leaves the state "not uploaded")
    if ((r = upload(d_L, sc.h_L, e->stream))) return r;
    HIPCHK(hipStreamSynchronize(e->stream));
    sc.d_L = std::move(d_L);
    return BN_OK;
}

ScoreModel model_of(const bn_engine* e) {
    const ScoreState& sc = e->score;
    return ScoreModel{e->plan.n, sc.d_k, sc.d_in_ptr, sc.d_in_idx, sc.d_cpt_off, sc.d_L};
}

// what every scoring call checks before it touches the device; the engine / table agreement is also what keeps every gather
// inside L: the table's states were validated against the same arities (bn_info_create)
int check_pair(const bn_engine* e, const bn_info_table* t) {
    if (!e || !t) return fail(BN_ERR_ARG, "null argument");
    if (e->host_only) return fail(BN_ERR_NO_DEVICE, "host-only engine (BN_DEVICE_HOST_ONLY): scoring runs on the device");
    if (e->plan.nranks > 1) return fail(BN_ERR_STATE, "sharded engine: a shard holds only its own nodes' tables (score on an unsharded engine)");
    if (int rc = refuse_unusable(e, BN_ERR_NO_DEVICE)) return rc;   // (an engine without a device was refused above, in this call's own words)
    if (t->n != e->plan.n)
        return fail(BN_ERR_ARG, "the table has " + std::to_string(t->n) + " columns, the network " + std::to_string(e->plan.n) + " nodes");
    for (int32_t v = 0; v < t->n; ++v)
        if (t->k[size_t(v)] != e->plan.k[size_t(v)])
            return fail(BN_ERR_ARG, "arity of column " + std::to_string(v) + " differs between the table (" + std::to_string(t->k[size_t(v)]) +
                                        ") and the network (" + std::to_string(e->plan.k[size_t(v)]) + ")");
    if (t->device != e->device) return fail(BN_ERR_ARG, "engine and table are on different devices");
    return BN_OK;
}

// the engine's stream takes over after whatever the table's stream still has in flight (no device-wide synchronise)
int order_after_table(bn_engine* e, const bn_info_table* t) {
    EventOwner ev;
    HIPCHK(hipEventCreateWithFlags(ev.put(), hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev, t->stream));
    HIPCHK(hipStreamWaitEvent(e->stream, ev, 0));
    return BN_OK;
}

}  // namespace

extern "C" int bn_score_log_cpt(bn_engine* e, double* out) {
    if (!e || !out) return fail(BN_ERR_ARG, "null argument");
    if (e->plan.nranks > 1) return fail(BN_ERR_STATE, "sharded engine: a shard holds only its own nodes' tables");
    if (int r = ensure_score(e, false)) return r;
    std::copy(e->score.h_L.begin(), e->score.h_L.end(), out);
    return BN_OK;
}

extern "C" int bn_score_rows(bn_engine* e, bn_info_table* t, int32_t n_sel, const int32_t* nodes, double* ll_out) {
    if (!ll_out) return fail(BN_ERR_ARG, "null argument");
    if (int r = check_pair(e, t)) return r;
    const int32_t n = e->plan.n;
    // the selection as a bit per node, and the segments (node id >> 8) that hold a selected node
    std::vector<uint32_t> sel(size_t(n + 31) / 32, 0u);
    if (!nodes) {
        for (int32_t v = 0; v < n; ++v) sel[size_t(v >> 5)] |= 1u << (v & 31);
    } else {
        if (n_sel < 0) return fail(BN_ERR_ARG, "n_sel < 0");
        for (int32_t i = 0; i < n_sel; ++i) {
            const int32_t v = nodes[i];
            if (v < 0 || v >= n) return fail(BN_ERR_ARG, "node id " + std::to_string(v) + " out of range");
            if (sel[size_t(v >> 5)] >> (v & 31) & 1u) return fail(BN_ERR_ARG, "node id " + std::to_string(v) + " listed twice");
            sel[size_t(v >> 5)] |= 1u << (v & 31);
        }
    }
    std::vector<int32_t> segs;
    const int words_per_seg = (1 << kScoreSegShift) / 32;
    for (size_t w = 0; w < sel.size(); ++w)
        if (sel[w] && (segs.empty() || segs.back() != int32_t(w / words_per_seg))) segs.push_back(int32_t(w / words_per_seg));
    if (segs.empty()) {   // nothing selected: the empty sum
        std::fill(ll_out, ll_out + t->P, 0.0);
        return BN_OK;
    }
    ON_DEVICE(e);
    if (int r = ensure_score(e, true)) return r;
    hipStream_t s = e->stream;
    DeviceBuf<uint32_t> d_sel;
    DeviceBuf<int32_t> d_segs;
    DeviceBuf<double> d_part, d_out;
    EventOwner ev0, ev1;
    int r;
    if ((r = upload(d_sel, sel, s)) || (r = upload(d_segs, segs, s)) || (r = dalloc(d_out, size_t(t->Ppad)))) return r;
    const int32_t n_segs = int32_t(segs.size());
    if (!score_rows_loop(n_segs, t->Ppad))
        if ((r = dalloc(d_part, size_t(n_segs) * size_t(t->Ppad)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    if ((r = order_after_table(e, t))) return r;
    const ScoreRowsArgs a{model_of(e), t->d_T, t->P, t->Ppad, d_sel, d_segs, n_segs, d_part, d_out};
    HIPCHK(hipEventRecord(ev0, s));
    if (int err = score_launch_rows(a, e->score.wide, s))
        return fail(BN_ERR_HIP, std::string("row-score kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev1, s));
    HIPCHK(hipMemcpyAsync(ll_out, d_out, size_t(t->P) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipEventElapsedTime(&e->score.last_rows_ms, ev0, ev1));
    return BN_OK;
}

extern "C" int bn_score_nodes(bn_engine* e, bn_info_table* t, double* ll_node_out, uint64_t* family_counts_out) {
    if (!ll_node_out) return fail(BN_ERR_ARG, "null argument");
    if (int r = check_pair(e, t)) return r;
    const Plan& p = e->plan;
    const int32_t n = p.n;
    const size_t entries = size_t(p.cpt_off[n]);
    ON_DEVICE(e);
    if (int r = ensure_score(e, true)) return r;
    hipStream_t s = e->stream;
    DeviceBuf<unsigned long long> d_N;
    DeviceBuf<double> d_ll;
    EventOwner ev0, ev1, ev2;
    int r;
    if ((r = dalloc(d_N, entries)) || (r = dalloc(d_ll, size_t(n)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    HIPCHK(hipEventCreate(ev2.put()));
    if ((r = order_after_table(e, t))) return r;
    // N: the family counts of the CPT fit (integer atomics: exact, whatever the split).  One workgroup per node leaves a small
    // network's long table to a handful of CUs, so the patterns are split until about four workgroups per CU exist, each keeping
    // at least 4096 patterns.
    int splits = e->score.splits;
    if (splits <= 0) {
        const int cus = e->n_cus > 0 ? e->n_cus : 256;
        const int64_t by_chip = (int64_t(4) * cus + n - 1) / n, by_work = (t->P + 4095) / 4096;
        splits = int(std::max<int64_t>(1, std::min<int64_t>(std::min(by_chip, by_work), 65535)));
    }
    const ScoreModel m = model_of(e);
    FitArgs fa{n, m.k, m.in_ptr, m.in_idx, m.cpt_off, t->P, t->d_T, t->d_w, d_N, 0, nullptr, nullptr, nullptr, t->Ppad};
    HIPCHK(hipEventRecord(ev0, s));
    HIPCHK(hipMemsetAsync(d_N, 0, std::max<size_t>(entries, 1) * 8, s));
    if (int err = launch_fit_count(fa, splits, s))
        return fail(BN_ERR_HIP, std::string("family-count kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev1, s));
    if (int err = score_launch_nodes(m, d_N, d_ll, s))
        return fail(BN_ERR_HIP, std::string("node-score kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev2, s));
    HIPCHK(hipMemcpyAsync(ll_node_out, d_ll, size_t(n) * 8, hipMemcpyDeviceToHost, s));
    if (family_counts_out && entries) HIPCHK(hipMemcpyAsync(family_counts_out, d_N, entries * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipEventElapsedTime(&e->score.last_count_ms, ev0, ev1));
    HIPCHK(hipEventElapsedTime(&e->score.last_nodes_ms, ev1, ev2));
    return BN_OK;
}
