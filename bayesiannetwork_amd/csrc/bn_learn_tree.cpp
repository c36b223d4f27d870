// bn_learn_tree.cpp -- C ABI of the tree learners (include/bn_mi355x.h: bn_tree_max_spanning, bn_learn_tree): the Chow-Liu tree and
// the tree of tree-augmented naive Bayes as the maximum spanning tree of the all-pairs (conditional) mutual information.  Kernels:
// bn_info_kernels.hip (the weights), bn_tree.hip (the tree).
#include <cmath>

#include "bn_engine_internal.hpp"
#include "bn_info.hpp"
#include "bn_info_table.hpp"
#include "bn_tree.hpp"
#include "../../include/bn_mi355x.h"

namespace {

// the kernel over d_w [m][m] on `stream`; parent / weight [m] to the host (weight may be null); ns_out: the kernel's device time
int run_prim(const double* d_w, int32_t m, int32_t root, hipStream_t stream, int32_t* parent, double* weight, double* ns_out) {
    DeviceBuf<int32_t> d_parent;
    DeviceBuf<double> d_weight;
    EventOwner ev0, ev1;
    int r;
    if ((r = dalloc(d_parent, size_t(m))) || (r = dalloc(d_weight, size_t(m)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    HIPCHK(hipEventRecord(ev0, stream));
    if (int e = tree_launch_prim(d_w, m, root, d_parent, d_weight, stream))
        return fail(BN_ERR_HIP, std::string("spanning-tree kernel: ") + hipGetErrorString(hipError_t(e)));
    HIPCHK(hipEventRecord(ev1, stream));
    HIPCHK(hipMemcpyAsync(parent, d_parent, size_t(m) * 4, hipMemcpyDeviceToHost, stream));
    if (weight) HIPCHK(hipMemcpyAsync(weight, d_weight, size_t(m) * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    if (ns_out) *ns_out = double(ms) * 1e6;
    return BN_OK;
}

}  // namespace

extern "C" int bn_tree_max_spanning(int32_t m, const double* w, int32_t root, int32_t device, int32_t* parent_out) {
    if (!w || !parent_out) return fail(BN_ERR_ARG, "null argument");
    if (m <= 0) return fail(BN_ERR_ARG, "m must be > 0");
    if (m > kTreeMaxNodes) return fail(BN_ERR_ARG, "the spanning-tree kernel holds one workgroup's nodes in LDS: m must be <= 4096");
    if (root < 0 || root >= m) return fail(BN_ERR_ARG, "root out of range");
    // only the upper triangle is read; the device gets the symmetric matrix (the kernel reads rows)
    std::vector<double> sym(size_t(m) * size_t(m), 0.0);
    for (int32_t lo = 0; lo < m; ++lo)
        for (int32_t hi = lo + 1; hi < m; ++hi) {
            const double x = w[size_t(lo) * m + hi];
            if (std::isnan(x)) return fail(BN_ERR_ARG, "NaN weight in the upper triangle");
            sym[size_t(lo) * m + hi] = sym[size_t(hi) * m + lo] = x;
        }
    if (m == 1) {
        parent_out[0] = -1;
        return BN_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(BN_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device >= ndev || device < BN_DEVICE_CURRENT) return fail(BN_ERR_ARG, "device ordinal out of range");
    if (device == BN_DEVICE_CURRENT) HIPCHK(hipGetDevice(&device));
    DeviceGuard guard;
    HIPCHK(guard.enter(device));
    StreamOwner stream;
    HIPCHK(hipStreamCreateWithFlags(stream.put(), hipStreamNonBlocking));
    DeviceBuf<double> d_w;
    if (int r = upload(d_w, sym, stream)) return r;
    return run_prim(d_w, m, root, stream, parent_out, nullptr, nullptr);
}

extern "C" int bn_learn_tree(bn_info_table* t, int32_t cond, int32_t m, const int32_t* vars, int32_t root, int32_t* parent_out,
                             double* weight_out, double* matrix_out) {
    if (!t || !parent_out || !weight_out) return fail(BN_ERR_ARG, "null argument");
    if (cond < -1 || cond >= t->n) return fail(BN_ERR_ARG, "class column out of range (-1: none)");
    std::vector<int32_t> all;
    if (!vars) {
        for (int32_t v = 0; v < t->n; ++v)
            if (v != cond) all.push_back(v);
        if (m != int32_t(all.size())) return fail(BN_ERR_ARG, "vars == NULL selects every column but the class: m must equal their number");
        vars = all.data();
    }
    if (m <= 0) return fail(BN_ERR_ARG, "m must be > 0");
    if (m > kTreeMaxNodes) return fail(BN_ERR_ARG, "the spanning-tree kernel holds one workgroup's nodes in LDS: m must be <= 4096");
    std::vector<uint8_t> seen(size_t(t->n), 0);
    int32_t lowest = -1, root_pos = -1;
    for (int32_t u = 0; u < m; ++u) {
        const int32_t v = vars[u];
        if (v < 0 || v >= t->n) return fail(BN_ERR_ARG, "variable index out of range");
        if (v == cond) return fail(BN_ERR_ARG, "the class column is among vars");
        if (seen[size_t(v)]) return fail(BN_ERR_ARG, "duplicate column in vars");
        seen[size_t(v)] = 1;
        if (lowest < 0 || v < vars[lowest]) lowest = u;
        if (v == root) root_pos = u;
    }
    if (root == -1) root_pos = lowest;
    else if (root_pos < 0) return fail(BN_ERR_ARG, "root is not among vars");
    ON_DEVICE(t);
    t->tree_ns = 0.0;
    DeviceBuf<double> d_w;
    if (int r = dalloc(d_w, size_t(m) * size_t(m))) return r;
    std::vector<double> w_host;
    if (int r = info_pair_matrix_device(t, cond, m, vars, d_w, w_host)) return r;
    if (matrix_out) std::copy(w_host.begin(), w_host.end(), matrix_out);
    if (m == 1) {
        parent_out[0] = -1;
        weight_out[0] = 0.0;
        return BN_OK;
    }
    std::vector<int32_t> pos(static_cast<size_t>(m));
    if (int r = run_prim(d_w, m, root_pos, t->stream, pos.data(), weight_out, &t->tree_ns)) return r;
    for (int32_t u = 0; u < m; ++u) parent_out[u] = pos[size_t(u)] < 0 ? -1 : vars[pos[size_t(u)]];
    return BN_OK;
}
