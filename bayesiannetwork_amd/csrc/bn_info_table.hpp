// bn_info_table.hpp -- the object behind bn_info_table (include/bn_mi355x.h): a pattern table resident on the device.  Host code
// only; shared by bn_info.cpp (entropies) and bn_score.cpp (log-likelihood under an engine's network).
#pragma once

#include "bn_engine_internal.hpp"
#include "bn_info.hpp"

struct bn_info_table {
    int device = 0;
    int32_t n = 0;
    int64_t P = 0, Ppad = 0;
    int32_t D = 1;
    std::vector<int32_t> k;
    double Nd = 0.0;
    hipStream_t stream = nullptr;
    DeviceBuf<uint8_t> d_T;
    DeviceBuf<unsigned long long> d_w;
    DeviceBuf<uint8_t> d_wd;
    float last_pairs_ms = 0.0f;
    // device time of the kernels of the last bn_learn_score_groups / bn_learn_score_subsets call (bn_info_get "learn_*_ns")
    double learn_count_ns = 0.0, learn_lattice_ns = 0.0, learn_score_ns = 0.0;
    // device time of the counting and statistic kernels of the last bn_ci_tests / bn_learn_pc call (0 when it was refused), and the
    // number of kernels those calls have launched on the table so far (bn_info_get "ci_count_ns", "ci_stat_ns", "ci_launches")
    double ci_count_ns = 0.0, ci_stat_ns = 0.0;
    int64_t ci_launches = 0;
    // device time of the conditional all-pairs kernel of the last bn_info_cond_pair_* / TAN call, and of the spanning-tree kernel of the
    // last bn_learn_tree call (bn_info_get "cond_pairs_ns", "tree_ns")
    double cond_pairs_ns = 0.0, tree_ns = 0.0;

    InfoDev dev() const { return InfoDev{n, P, Ppad, D, d_T, d_w, d_wd}; }
    ~bn_info_table() {   // (the members' own destructors would run after the guard's)
        DeviceGuard g;
        (void)g.enter(device);
        d_T.reset(); d_w.reset(); d_wd.reset();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// bn_info.cpp: the all-pairs mutual information of every column, left on the device (bn_learn_hc's similarity matrix)
int info_pair_mi_device(bn_info_table* t, double* d_mi, std::vector<double>& mi_host);
// ... and the tree learners' weight matrix over `vars`: mi (cond < 0) or cmi given `cond`, on the device and on the host
int info_pair_matrix_device(bn_info_table* t, int32_t cond, int32_t m, const int32_t* vars, double* d_w, std::vector<double>& w_host);
