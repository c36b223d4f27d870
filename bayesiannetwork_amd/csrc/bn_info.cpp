// bn_info.cpp -- C ABI of the entropy / mutual-information table (include/bn_mi355x.h, bn_info_*),
// reference bayesian/evaluation/transinformation.hpp.  Kernels: bn_info_kernels.hip.
#include <cmath>
#include <memory>

#include "bn_engine_internal.hpp"
#include "bn_info.hpp"
#include "bn_info_table.hpp"
#include "../../include/bn_mi355x.h"

namespace {

int slot_width(int32_t k) {
    int w = 2;
    while (w < k) w <<= 1;
    return w;
}

// canonical set: sorted, duplicates dropped, arity-1 columns dropped (their only state adds no key digit)
int make_set(const bn_info_table* t, int32_t nv, const int32_t* vars, InfoSet& s, uint64_t& cells, int& key_bits) {
    if (nv < 0 || (nv > 0 && !vars)) return fail(BN_ERR_ARG, "bad variable list");
    std::vector<int32_t> v(vars, vars + nv);
    for (int32_t x : v)
        if (x < 0 || x >= t->n) return fail(BN_ERR_ARG, "variable index out of range");
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    s.nv = 0;
    unsigned __int128 prod = 1;
    for (int32_t x : v) {
        if (t->k[x] < 2) continue;
        prod *= unsigned(t->k[x]);
        if (prod > (unsigned __int128)1 << 64)
            return fail(BN_ERR_ARG, "the joint key of the set needs more than 64 bits (product of the arities > 2^64)");
        s.col[s.nv] = x;
        s.k[s.nv] = t->k[x];
        ++s.nv;   // (<= 64 columns of arity >= 2 before the product passes 2^64)
    }
    cells = prod == (unsigned __int128)1 << 64 ? 0 : uint64_t(prod);   // 0: the full 64-bit key space
    key_bits = 0;
    while (key_bits < 64 && (cells == 0 || (uint64_t(1) << key_bits) < cells)) ++key_bits;
    return BN_OK;
}

int run_entropy(bn_info_table* t, const InfoSet& s, uint64_t cells, int key_bits, int route, double* h, unsigned long long* cells_out) {
    if (route == 0) route = (cells != 0 && cells <= kInfoDenseMaxCells) ? 1 : 2;
    if (route == 1 && (cells == 0 || cells > kInfoDenseMaxCells))
        return fail(BN_ERR_ARG, "dense route: the set has more than 2^22 cells");
    if (s.nv == 0) {   // every column of arity 1 (or none): one cell holding every sample
        *h = 0.0;
        return BN_OK;
    }
    const int e = info_entropy_run(t->dev(), s, route, cells, key_bits < 1 ? 1 : key_bits, t->Nd, h, cells_out, t->stream);
    if (e) return fail(BN_ERR_HIP, std::string("entropy kernels: ") + hipGetErrorString(hipError_t(e)));
    return BN_OK;
}

}  // namespace

extern "C" int bn_info_create(int64_t n_patterns, int32_t n_vars, const uint8_t* patterns, const uint64_t* counts,
                              const int32_t* k, int32_t device, bn_info_table** out) {
    if (!out) return fail(BN_ERR_ARG, "null argument");
    *out = nullptr;
    if (n_vars <= 0 || n_vars > (1 << 23)) return fail(BN_ERR_ARG, "n_vars must be in 1..2^23");
    if (n_patterns < 0) return fail(BN_ERR_ARG, "bad pattern table (n_patterns < 0)");
    if (!k) return fail(BN_ERR_ARG, "null arity array");
    if (n_patterns > 0 && (!patterns || !counts)) return fail(BN_ERR_ARG, "bad pattern table");
    for (int32_t v = 0; v < n_vars; ++v)
        if (k[v] < 1 || k[v] > 255) return fail(BN_ERR_ARG, "arity must be in 1..255");
    uint64_t total = 0, maxc = 0;
    for (int64_t i = 0; i < n_patterns; ++i) {
        if (counts[i] > ~total) return fail(BN_ERR_ARG, "the total count does not fit in 64 bits");
        total += counts[i];
        maxc = std::max<uint64_t>(maxc, counts[i]);
    }
    if (total == 0) return fail(BN_ERR_ARG, "empty sample table (sampling_size() == 0)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(BN_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device >= ndev || device < BN_DEVICE_CURRENT) return fail(BN_ERR_ARG, "device ordinal out of range");
    if (device == BN_DEVICE_CURRENT) HIPCHK(hipGetDevice(&device));
    DeviceGuard guard;
    HIPCHK(guard.enter(device));

    std::unique_ptr<bn_info_table> t(new (std::nothrow) bn_info_table);
    if (!t) return fail(BN_ERR_ALLOC, "host allocation failed");
    t->device = device;
    t->n = n_vars;
    t->P = n_patterns;
    t->Ppad = std::max<int64_t>((n_patterns + kInfoPatternAlign - 1) / kInfoPatternAlign * kInfoPatternAlign, kInfoPatternAlign);
    t->k.assign(k, k + n_vars);
    t->Nd = double(total);
    int bits = 0;
    while (bits < 64 && (maxc >> bits)) ++bits;
    t->D = std::max(1, (bits + 6) / 7);
    HIPCHK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    DeviceBuf<uint8_t> d_raw;
    DeviceBuf<int32_t> d_k;
    DeviceBuf<unsigned> d_bad;
    unsigned bad = 0;
    const size_t raw_bytes = size_t(n_patterns) * size_t(n_vars);
    if (int r = dalloc(d_raw, raw_bytes)) return r;
    if (int r = dalloc(t->d_T, size_t(n_vars) * size_t(t->Ppad))) return r;
    if (int r = dalloc(t->d_w, size_t(n_patterns))) return r;
    if (int r = dalloc(t->d_wd, size_t(t->D) * size_t(t->Ppad))) return r;
    if (int r = upload(d_k, t->k, t->stream)) return r;
    if (int r = dalloc(d_bad, 1)) return r;
    HIPCHK(hipMemsetAsync(d_bad, 0, 4, t->stream));
    if (raw_bytes) HIPCHK(hipMemcpyAsync(d_raw, patterns, raw_bytes, hipMemcpyHostToDevice, t->stream));
    if (n_patterns) HIPCHK(hipMemcpyAsync(t->d_w, counts, size_t(n_patterns) * 8, hipMemcpyHostToDevice, t->stream));
    int e = info_launch_transpose(d_raw, n_patterns, n_vars, t->Ppad, d_k, t->d_T, d_bad, t->stream);
    if (!e) e = info_launch_digits(t->d_w, n_patterns, t->Ppad, t->D, t->d_wd, t->stream);
    if (e) return fail(BN_ERR_HIP, std::string("table kernels: ") + hipGetErrorString(hipError_t(e)));
    HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    if (bad) return fail(BN_ERR_ARG, "pattern state out of range (a state >= its column's arity)");
    *out = t.release();
    return BN_OK;
}

extern "C" void bn_info_destroy(bn_info_table* t) { delete t; }

extern "C" int bn_info_entropy(bn_info_table* t, int32_t n_set, const int32_t* set, int32_t route, double* h_out) {
    if (!t || !h_out) return fail(BN_ERR_ARG, "null argument");
    if (route < 0 || route > 2) return fail(BN_ERR_ARG, "route: 0 automatic, 1 dense cells, 2 sorted keys");
    InfoSet s{};
    uint64_t cells = 0;
    int key_bits = 0;
    if (int r = make_set(t, n_set, set, s, cells, key_bits)) return r;
    ON_DEVICE(t);
    return run_entropy(t, s, cells, key_bits, route, h_out, nullptr);
}

namespace {

// The all-pairs kernel over the columns `vars` of arity <= 32, the dense route for every pair with a wider
// column.  hxy [m][m] and h [m] on the host; dump_off / dump: the pair blocks pair_counts asks for.
// d_mi (device, may be null): [m][m] mi = h[x] + h[y] - hxy[x][y], made on the device from the kernel's own h and hxy; the rows and
// columns of a wide column, whose entropies are finished on the host, are written from there.
// cond >= 0 (hz = H(cond)): the conditional form -- h is hxz, hxy is hxyz, the blocks are [k_cond][k_x][k_y], a wide pair is the
// single call over {x, y, cond} on its automatic route, and d_mi is cmi = hxz[x] + hxz[y] - hxyz[x][y] - hz.
int all_pairs(bn_info_table* t, int32_t m, const int32_t* vars, double* h, double* hxy, const std::vector<int64_t>* dump_off,
              unsigned long long* dump_host, size_t dump_len, double* d_mi = nullptr, int32_t cond = -1, double hz = 0.0) {
    // slots: widths 32, 16, 8, 4, 2 in that order (stable in the caller's order), so each starts aligned
    std::vector<int32_t> order;
    std::vector<int32_t> wide;
    for (int w = 32; w >= 2; w >>= 1)
        for (int32_t u = 0; u < m; ++u)
            if (t->k[vars[u]] <= 32 && slot_width(t->k[vars[u]]) == w) order.push_back(u);
    for (int32_t u = 0; u < m; ++u)
        if (t->k[vars[u]] > 32) wide.push_back(u);
    std::vector<int32_t> sv_start, sv_k, sv_col, sv_user;
    int64_t K = 0;
    for (int32_t u : order) {
        sv_start.push_back(int32_t(K));
        sv_k.push_back(t->k[vars[u]]);
        sv_col.push_back(vars[u]);
        sv_user.push_back(u);
        K += slot_width(t->k[vars[u]]);
    }
    const int64_t Kpad = (K + kInfoTile - 1) / kInfoTile * kInfoTile;
    if (Kpad > (int64_t(1) << 20)) return fail(BN_ERR_ARG, "more than 2^20 slot columns in one all-pairs call");
    std::vector<int32_t> colinfo(size_t(Kpad), 255), colvar(size_t(Kpad), -1);   // padding: column 0, state 255 (never a state)
    for (size_t v = 0; v < sv_start.size(); ++v)
        for (int32_t st = 0; st < slot_width(sv_k[v]); ++st) {
            const size_t c = size_t(sv_start[v] + st);
            colvar[c] = int32_t(v);
            colinfo[c] = st < sv_k[v] ? (sv_col[v] << 8) | st : 255;
        }
    for (size_t i = 0; i < size_t(m) * size_t(m); ++i) hxy[i] = 0.0;
    t->last_pairs_ms = 0.0f;
    if (cond >= 0) t->cond_pairs_ns = 0.0;
    if (Kpad > 0) {
        EventOwner ev0, ev1;
        DeviceBuf<int32_t> d_ci, d_cv, d_ss, d_sk, d_sc, d_su;
        DeviceBuf<double> d_hxy, d_h;
        DeviceBuf<int64_t> d_off;
        DeviceBuf<unsigned long long> d_dump;
        int r;
        if ((r = upload(d_ci, colinfo, t->stream)) || (r = upload(d_cv, colvar, t->stream)) || (r = upload(d_ss, sv_start, t->stream)) ||
            (r = upload(d_sk, sv_k, t->stream)) || (r = upload(d_sc, sv_col, t->stream)) || (r = upload(d_su, sv_user, t->stream)))
            return r;
        if ((r = dalloc(d_hxy, size_t(m) * size_t(m))) || (r = dalloc(d_h, size_t(m)))) return r;
        HIPCHK(hipMemsetAsync(d_hxy, 0, size_t(m) * size_t(m) * 8, t->stream));
        if (dump_off) {
            if ((r = upload(d_off, *dump_off, t->stream)) || (r = dalloc(d_dump, dump_len))) return r;
            HIPCHK(hipMemsetAsync(d_dump, 0, std::max<size_t>(dump_len, 1) * 8, t->stream));
        }
        HIPCHK(hipEventCreate(ev0.put()));
        HIPCHK(hipEventCreate(ev1.put()));
        PairArgs a{t->d_T, t->Ppad, t->d_wd, t->D, int32_t(Kpad / kInfoTile), d_ci, d_cv, d_ss, d_sk, d_sc, d_su, m, t->Nd,
                   d_hxy, d_h, d_off, d_dump, cond >= 0 ? t->d_T + size_t(cond) * size_t(t->Ppad) : nullptr,
                   cond >= 0 ? t->k[size_t(cond)] : 0};
        const bool flush = t->D > 1 || t->Ppad > kInfoSegment;
        HIPCHK(hipEventRecord(ev0, t->stream));
        if (int e = info_launch_pairs(a, flush, t->stream))
            return fail(BN_ERR_HIP, std::string("all-pairs kernel: ") + hipGetErrorString(hipError_t(e)));
        HIPCHK(hipEventRecord(ev1, t->stream));
        if (d_mi)
            if (int e = cond >= 0 ? info_launch_cmi(d_h, d_hxy, m, hz, d_mi, t->stream) : info_launch_mi(d_h, d_hxy, m, d_mi, t->stream))
                return fail(BN_ERR_HIP, std::string("mutual-information kernel: ") + hipGetErrorString(hipError_t(e)));
        HIPCHK(hipMemcpyAsync(hxy, d_hxy, size_t(m) * size_t(m) * 8, hipMemcpyDeviceToHost, t->stream));
        std::vector<double> hs(static_cast<size_t>(m));
        HIPCHK(hipMemcpyAsync(hs.data(), d_h, size_t(m) * 8, hipMemcpyDeviceToHost, t->stream));
        if (dump_off) HIPCHK(hipMemcpyAsync(dump_host, d_dump, dump_len * 8, hipMemcpyDeviceToHost, t->stream));
        HIPCHK(hipStreamSynchronize(t->stream));
        HIPCHK(hipEventElapsedTime(&t->last_pairs_ms, ev0, ev1));
        if (cond >= 0) t->cond_pairs_ns = double(t->last_pairs_ms) * 1e6;
        for (int32_t u : order) h[u] = hs[size_t(u)];
    }
    // pairs with a column of arity > 32: one dense joint table each (the single call's route, so its bits)
    for (int32_t x : wide)
        for (int32_t y = 0; y < m; ++y) {
            if (t->k[vars[y]] > 32 && y < x) continue;   // (done as (y, x))
            const int32_t set3[3] = {vars[x], vars[y], cond};
            InfoSet s{};
            uint64_t cells = 0;
            int key_bits = 0;
            if (int r = make_set(t, cond >= 0 ? 3 : 2, set3, s, cells, key_bits)) return r;
            std::vector<unsigned long long> c;
            const int64_t o = dump_off ? (*dump_off)[size_t(x) * m + y] : -1, o2 = dump_off ? (*dump_off)[size_t(y) * m + x] : -1;
            if (o >= 0 || o2 >= 0) {
                if (cells == 0 || cells > kInfoDenseMaxCells)
                    return fail(BN_ERR_ARG, "the counts of a pair with a column of arity > 32 come from the dense route: more than 2^22 cells");
                c.assign(size_t(cells), 0);
            }
            double H = 0.0;
            if (int r = run_entropy(t, s, cells, key_bits, cond >= 0 && c.empty() ? 0 : 1, &H, c.empty() ? nullptr : c.data())) return r;
            hxy[size_t(x) * m + y] = hxy[size_t(y) * m + x] = H;
            if (x == y) h[x] = H;
            if (c.empty()) continue;
            // c is in key order: the set's columns increasing, the smallest the most significant digit; a column of arity 1 has none
            const int32_t kx = t->k[vars[x]], ky = t->k[vars[y]], kz = cond >= 0 ? t->k[size_t(cond)] : 1;
            size_t sx = 0, sy = 0, sz = 0, stride = 1;
            for (int32_t i = s.nv - 1; i >= 0; --i) {
                if (s.col[i] == vars[x]) sx = stride;
                if (s.col[i] == vars[y]) sy = stride;
                if (s.col[i] == cond) sz = stride;
                stride *= size_t(s.k[i]);
            }
            for (int32_t z = 0; z < kz; ++z)
                for (int32_t i = 0; i < kx; ++i)
                    for (int32_t j = 0; j < ky; ++j) {
                        unsigned long long v;
                        if (vars[x] == vars[y]) v = i == j ? c[size_t(z) * sz + size_t(i) * sx] : 0;
                        else v = c[size_t(z) * sz + size_t(i) * sx + size_t(j) * sy];
                        const int64_t zo = int64_t(z) * kx * ky;
                        if (o >= 0) dump_host[o + zo + i * ky + j] = v;
                        if (o2 >= 0 && x != y) dump_host[o2 + zo + j * kx + i] = v;
                    }
        }
    if (d_mi && !wide.empty()) {
        std::vector<double> rows(wide.size() * size_t(m));
        for (size_t w = 0; w < wide.size(); ++w) {
            const int32_t x = wide[w];
            double* row = rows.data() + w * size_t(m);
            for (int32_t y = 0; y < m; ++y) {   // (= h[y] + h[x] - hxy[y][x]: the column too)
                row[y] = h[x] + h[y] - hxy[size_t(x) * m + y];
                if (cond >= 0) row[y] = row[y] - hz;
            }
            HIPCHK(hipMemcpyAsync(d_mi + size_t(x) * m, row, size_t(m) * 8, hipMemcpyHostToDevice, t->stream));
            HIPCHK(hipMemcpy2DAsync(d_mi + x, size_t(m) * 8, row, 8, 8, size_t(m), hipMemcpyHostToDevice, t->stream));
        }
        HIPCHK(hipStreamSynchronize(t->stream));
    }
    return BN_OK;
}

}  // namespace

// every column's mutual information with every other, left on the device at d_mi [n][n]; mi_host: the same matrix from the
// entropies the call brings to the host anyway (the same bits).  The caller has entered the table's device.
int info_pair_mi_device(bn_info_table* t, double* d_mi, std::vector<double>& mi_host) {
    const int32_t n = t->n;
    std::vector<int32_t> all(static_cast<size_t>(n));
    for (int32_t v = 0; v < n; ++v) all[size_t(v)] = v;
    std::vector<double> h(static_cast<size_t>(n)), hxy(size_t(n) * size_t(n));
    if (int r = all_pairs(t, n, all.data(), h.data(), hxy.data(), nullptr, nullptr, 0, d_mi)) return r;
    mi_host.resize(hxy.size());
    for (int32_t x = 0; x < n; ++x)
        for (int32_t y = 0; y < n; ++y) mi_host[size_t(x) * n + y] = h[size_t(x)] + h[size_t(y)] - hxy[size_t(x) * n + y];
    return BN_OK;
}

// the weight matrix of the tree learners, left on the device at d_w [m][m]: mi of `vars` (cond < 0) or cmi given `cond`, and the same
// matrix on the host (the same bits).  `vars` are in range and do not hold cond; the caller has entered the table's device.
int info_pair_matrix_device(bn_info_table* t, int32_t cond, int32_t m, const int32_t* vars, double* d_w, std::vector<double>& w_host) {
    std::vector<double> h(static_cast<size_t>(m)), hxy(size_t(m) * size_t(m));
    double hz = 0.0;
    if (cond >= 0) {
        InfoSet s{};
        uint64_t cells = 0;
        int key_bits = 0;
        if (int r = make_set(t, 1, &cond, s, cells, key_bits)) return r;
        if (int r = run_entropy(t, s, cells, key_bits, 0, &hz, nullptr)) return r;
    }
    if (int r = all_pairs(t, m, vars, h.data(), hxy.data(), nullptr, nullptr, 0, d_w, cond, hz)) return r;
    w_host.resize(hxy.size());
    for (int32_t x = 0; x < m; ++x)
        for (int32_t y = 0; y < m; ++y) {
            double w = h[size_t(x)] + h[size_t(y)] - hxy[size_t(x) * m + y];
            if (cond >= 0) w = w - hz;
            w_host[size_t(x) * m + y] = w;
        }
    return BN_OK;
}

extern "C" int bn_info_cond_pair_entropies(bn_info_table* t, int32_t cond, int32_t m, const int32_t* vars, double* hz_out, double* hxz_out,
                                           double* hxyz_out, double* cmi_out) {
    if (!t || !vars || !hz_out || !hxz_out || !hxyz_out) return fail(BN_ERR_ARG, "null argument");
    if (cond < 0 || cond >= t->n) return fail(BN_ERR_ARG, "conditioning column out of range");
    if (m <= 0) return fail(BN_ERR_ARG, "m must be > 0");
    for (int32_t u = 0; u < m; ++u) {
        if (vars[u] < 0 || vars[u] >= t->n) return fail(BN_ERR_ARG, "variable index out of range");
        if (vars[u] == cond) return fail(BN_ERR_ARG, "the conditioning column is among vars");
    }
    ON_DEVICE(t);
    InfoSet s{};
    uint64_t cells = 0;
    int key_bits = 0;
    if (int r = make_set(t, 1, &cond, s, cells, key_bits)) return r;
    if (int r = run_entropy(t, s, cells, key_bits, 0, hz_out, nullptr)) return r;
    DeviceBuf<double> d_cmi;
    if (cmi_out)
        if (int r = dalloc(d_cmi, size_t(m) * size_t(m))) return r;
    if (int r = all_pairs(t, m, vars, hxz_out, hxyz_out, nullptr, nullptr, 0, cmi_out ? d_cmi.get() : nullptr, cond, *hz_out)) return r;
    if (cmi_out) {
        HIPCHK(hipMemcpyAsync(cmi_out, d_cmi, size_t(m) * size_t(m) * 8, hipMemcpyDeviceToHost, t->stream));
        HIPCHK(hipStreamSynchronize(t->stream));
    }
    return BN_OK;
}

extern "C" int bn_info_pair_entropies(bn_info_table* t, int32_t m, const int32_t* vars, double* h_out, double* hxy_out, double* mi_out) {
    if (!t || !h_out || !hxy_out) return fail(BN_ERR_ARG, "null argument");
    std::vector<int32_t> all;
    if (!vars) {
        if (m != t->n) return fail(BN_ERR_ARG, "vars == NULL selects every column: m must equal n_vars");
        all.resize(size_t(m));
        for (int32_t v = 0; v < m; ++v) all[size_t(v)] = v;
        vars = all.data();
    }
    if (m <= 0) return fail(BN_ERR_ARG, "m must be > 0");
    for (int32_t u = 0; u < m; ++u)
        if (vars[u] < 0 || vars[u] >= t->n) return fail(BN_ERR_ARG, "variable index out of range");
    ON_DEVICE(t);
    if (int r = all_pairs(t, m, vars, h_out, hxy_out, nullptr, nullptr, 0)) return r;
    if (mi_out)   // transinformation.hpp:60 / :80: x_ent + y_ent - xy_ent
        for (int32_t x = 0; x < m; ++x)
            for (int32_t y = 0; y < m; ++y) mi_out[size_t(x) * m + y] = h_out[x] + h_out[y] - hxy_out[size_t(x) * m + y];
    return BN_OK;
}

namespace {

// cond < 0: the blocks [k_x][k_y] of bn_info_pair_counts; else the blocks [k_cond][k_x][k_y] of bn_info_cond_pair_counts
int pair_counts(bn_info_table* t, int32_t cond, int32_t n_pairs, const int32_t* pairs, uint64_t* counts_out) {
    if (!t || !counts_out || n_pairs <= 0 || !pairs) return fail(BN_ERR_ARG, "null argument or n_pairs <= 0");
    const size_t kz = cond >= 0 ? size_t(t->k[size_t(cond)]) : 1;
    std::vector<int32_t> uniq;
    for (int32_t i = 0; i < 2 * n_pairs; ++i) {
        if (pairs[i] < 0 || pairs[i] >= t->n) return fail(BN_ERR_ARG, "variable index out of range");
        if (pairs[i] == cond) return fail(BN_ERR_ARG, "the conditioning column is among the pairs");
        uniq.push_back(pairs[i]);
    }
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    const int32_t m = int32_t(uniq.size());
    auto pos = [&](int32_t v) { return int32_t(std::lower_bound(uniq.begin(), uniq.end(), v) - uniq.begin()); };
    std::vector<int64_t> off(size_t(m) * m, -1), where(static_cast<size_t>(n_pairs));
    int64_t len = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {
        const int32_t x = pos(pairs[2 * i]), y = pos(pairs[2 * i + 1]);
        int64_t& o = off[size_t(x) * m + y];
        if (o < 0) { o = len; len += int64_t(kz) * t->k[pairs[2 * i]] * t->k[pairs[2 * i + 1]]; }
        where[size_t(i)] = o;
    }
    std::vector<unsigned long long> dump(size_t(std::max<int64_t>(len, 1)));
    std::vector<double> h(static_cast<size_t>(m)), hxy(size_t(m) * m);
    ON_DEVICE(t);
    if (int r = all_pairs(t, m, uniq.data(), h.data(), hxy.data(), &off, dump.data(), size_t(len), nullptr, cond)) return r;
    uint64_t* o = counts_out;
    for (int32_t i = 0; i < n_pairs; ++i) {
        const size_t cells = kz * size_t(t->k[pairs[2 * i]]) * size_t(t->k[pairs[2 * i + 1]]);
        std::copy(dump.begin() + where[size_t(i)], dump.begin() + where[size_t(i)] + int64_t(cells), o);
        o += cells;
    }
    return BN_OK;
}

}  // namespace

extern "C" int bn_info_pair_counts(bn_info_table* t, int32_t n_pairs, const int32_t* pairs, uint64_t* counts_out) {
    return pair_counts(t, -1, n_pairs, pairs, counts_out);
}

extern "C" int bn_info_cond_pair_counts(bn_info_table* t, int32_t cond, int32_t n_pairs, const int32_t* pairs, uint64_t* counts_out) {
    if (!t) return fail(BN_ERR_ARG, "null argument or n_pairs <= 0");
    if (cond < 0 || cond >= t->n) return fail(BN_ERR_ARG, "conditioning column out of range");
    return pair_counts(t, cond, n_pairs, pairs, counts_out);
}

extern "C" int bn_info_last_pairs_ms(const bn_info_table* t, double* ms_out) {
    if (!t || !ms_out) return fail(BN_ERR_ARG, "null argument");
    *ms_out = double(t->last_pairs_ms);
    return BN_OK;
}

extern "C" int bn_info_get(const bn_info_table* t, const char* name, int64_t* value_out) {
    if (!t || !name || !value_out) return fail(BN_ERR_ARG, "null argument");
    const std::string s(name);
    if (s == "n_vars") *value_out = t->n;
    else if (s == "n_patterns") *value_out = t->P;
    else if (s == "digit_passes") *value_out = t->D;
    else if (s == "learn_count_ns") *value_out = int64_t(t->learn_count_ns);
    else if (s == "learn_lattice_ns") *value_out = int64_t(t->learn_lattice_ns);
    else if (s == "learn_score_ns") *value_out = int64_t(t->learn_score_ns);
    else if (s == "ci_count_ns") *value_out = int64_t(t->ci_count_ns);
    else if (s == "ci_stat_ns") *value_out = int64_t(t->ci_stat_ns);
    else if (s == "ci_launches") *value_out = t->ci_launches;
    else if (s == "cond_pairs_ns") *value_out = int64_t(t->cond_pairs_ns);
    else if (s == "tree_ns") *value_out = int64_t(t->tree_ns);
    else
        return fail(BN_ERR_ARG, "unknown name (n_vars, n_patterns, digit_passes, learn_count_ns, learn_lattice_ns, learn_score_ns, ci_count_ns, "
                                "ci_stat_ns, ci_launches, cond_pairs_ns, tree_ns)");
    return BN_OK;
}
