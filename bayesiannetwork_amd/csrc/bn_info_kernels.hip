// bn_info_kernels.hip -- entropy of column sets and all-pairs joint entropies of a pattern table
// (reference bayesian/evaluation/transinformation.hpp:14-84).  DESIGN.md "Entropy and mutual information".
//
// Summation order (every route): the non-zero cells of the joint table in increasing mixed-radix key
// (the set's smallest column the most significant digit), in chunks of 4096 consecutive keys; each
// chunk folds `part -= p * log2(p)` from 0.0 in key order, and H = 0.0 + part_0 + part_1 + ... in chunk
// order.  So the result depends on the counts alone, not on the pattern order, and a pair's block
// reduced in the all-pairs kernel's epilogue (<= 32 x 32 cells: one chunk) has the bits of the single
// entropy({x, y}) call.
#include <hip/hip_runtime.h>

#include <cstring>  // (rocPRIM's texture iterator calls the host memset)

#include <rocprim/rocprim.hpp>

#include "bn_info.hpp"

namespace bnmi {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void fold_cell(double& part, unsigned long long c, double Nd) {
    if (c) {
        const double p = double(c) / Nd;
        part -= p * log2(p);
    }
}

// ---- table set-up ---------------------------------------------------------------------------------
// [P][n] -> [n][Ppad] through a 64 x 64 LDS tile; a state >= k sets *bad (checked by the host, no trap)
__global__ __launch_bounds__(256) void info_transpose(const uint8_t* __restrict__ raw, int64_t P, int32_t n, int64_t Ppad,
                                                      const int32_t* __restrict__ k, uint8_t* __restrict__ T, unsigned* bad) {
    __shared__ uint8_t tile[64][65];
    const int64_t p0 = int64_t(blockIdx.x) * 64;
    const int32_t v0 = int32_t(blockIdx.y) * 64;
    unsigned oob = 0;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int pr = i >> 6, vc = i & 63;
        uint8_t s = 0;
        if (p0 + pr < P && v0 + vc < n) {
            s = raw[(p0 + pr) * n + v0 + vc];
            oob |= s >= k[v0 + vc];
        }
        tile[pr][vc] = s;
    }
    if (oob) atomicOr(bad, 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int vr = i >> 6, pc = i & 63;
        if (v0 + vr < n && p0 + pc < Ppad) T[int64_t(v0 + vr) * Ppad + p0 + pc] = tile[pc][vr];
    }
}

__global__ void info_digits(const unsigned long long* __restrict__ w, int64_t P, int64_t Ppad, int32_t D, uint8_t* __restrict__ wd) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < Ppad; i += int64_t(gridDim.x) * blockDim.x) {
        const unsigned long long c = i < P ? w[i] : 0ull;
        for (int d = 0; d < D; ++d) wd[int64_t(d) * Ppad + i] = uint8_t((c >> (7 * d)) & 127u);
    }
}

// ---- one set ----------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long set_key(const uint8_t* __restrict__ T, int64_t Ppad, const InfoSet& s, int64_t p) {
    unsigned long long key = 0;
    for (int i = 0; i < s.nv; ++i) key = key * unsigned(s.k[i]) + T[int64_t(s.col[i]) * Ppad + p];
    return key;
}

__global__ void info_hist(InfoDev t, InfoSet s, unsigned long long* __restrict__ cells) {
    for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < t.P; p += int64_t(gridDim.x) * blockDim.x) {
        const unsigned long long c = t.w[p];
        if (c) atomicAdd(&cells[set_key(t.T, t.Ppad, s, p)], c);
    }
}

__global__ void info_keys(InfoDev t, InfoSet s, unsigned long long* __restrict__ keys) {
    for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < t.P; p += int64_t(gridDim.x) * blockDim.x)
        keys[p] = set_key(t.T, t.Ppad, s, p);
}

// one thread per chunk of 4096 cells
__global__ void info_fold_dense(const unsigned long long* __restrict__ cells, uint64_t ncells, double Nd, double* __restrict__ partial) {
    const uint64_t chunk = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t b = chunk << kInfoChunkShift;
    if (b >= ncells) return;
    const uint64_t e = b + (uint64_t(1) << kInfoChunkShift) < ncells ? b + (uint64_t(1) << kInfoChunkShift) : ncells;
    double part = 0.0;
    for (uint64_t i = b; i < e; ++i) fold_cell(part, cells[i], Nd);
    partial[chunk] = part;
}

// one thread per distinct key; the first key of a chunk folds the chunk, the others leave 0.0
__global__ void info_fold_keys(const unsigned long long* __restrict__ ukeys, const unsigned long long* __restrict__ usums,
                               const unsigned long long* __restrict__ nu, double Nd, double* __restrict__ partial) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t U = *nu;
    if (i >= U) return;
    const unsigned long long chunk = ukeys[i] >> kInfoChunkShift;
    if (i > 0 && (ukeys[i - 1] >> kInfoChunkShift) == chunk) {
        partial[i] = 0.0;
        return;
    }
    double part = 0.0;
    for (uint64_t j = i; j < U && (ukeys[j] >> kInfoChunkShift) == chunk; ++j) fold_cell(part, usums[j], Nd);
    partial[i] = part;
}

// H = 0.0 + partial[0] + partial[1] + ... (adding a 0.0 partial changes no bit of a non-negative sum)
__global__ void info_fold_final(const double* __restrict__ partial, uint64_t n, const unsigned long long* __restrict__ n_dev,
                                double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t cnt = n_dev ? *n_dev : n;
    double h = 0.0;
    for (uint64_t i = 0; i < cnt; ++i) h += partial[i];
    *out = h;
}

// ---- all pairs -------------------------------------------------------------------------------------
// byte-wise (x == s) masks of 4 states: 0x80 in every byte that matches
__device__ __forceinline__ unsigned match80(unsigned x, unsigned srep) {
    const unsigned y = x ^ srep;
    const unsigned t = ((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y;
    return ~t & 0x80808080u;
}

__device__ __forceinline__ v4i onehot_weighted(uint4 x, unsigned srep, uint4 wv) {
    // 0x80 - 0x01 = 0x7f in every matching byte (no borrow crosses a byte), & the <= 127 digit
    unsigned m;
    v4i r;
    m = match80(x.x, srep); r[0] = int((m - (m >> 7)) & wv.x);
    m = match80(x.y, srep); r[1] = int((m - (m >> 7)) & wv.y);
    m = match80(x.z, srep); r[2] = int((m - (m >> 7)) & wv.z);
    m = match80(x.w, srep); r[3] = int((m - (m >> 7)) & wv.w);
    return r;
}

__device__ __forceinline__ v4i onehot(uint4 x, unsigned srep) {
    v4i r;
    r[0] = int(match80(x.x, srep) >> 7);
    r[1] = int(match80(x.y, srep) >> 7);
    r[2] = int(match80(x.z, srep) >> 7);
    r[3] = int(match80(x.w, srep) >> 7);
    return r;
}

// Workgroup: one 128 x 128 tile (ti <= tj) of the slot-column space; wave w the 64 x 64 quarter
// (w >> 1, w & 1) as 2 x 2 MFMA 32x32x32 i8 tiles.  K of the MFMA = 32 patterns: lane (r, h) holds
// the 16 patterns 16h .. 16h+15 of row r for A and of column r for B (the same lane map on both sides,
// so each A byte meets the B byte of the same pattern).  A = one-hot x digit d of the count, B = one-hot.
//
// COND: the conditional form.  For each state s of the column a.zrow (a.kz states, in increasing order) the count digit is also
// masked by T[z][p] == s -- one match80 on the 16 bytes of z, applied to wv, masks A0 and A1 together -- so the accumulators hold
// N(x, y, s); the epilogue folds each pair's block into part_s and adds it to the pair's entry (0.0 + part_0 + part_1 + ...).  Every
// entry has one owner thread, the same for every state, so the sum runs through the output matrix itself.  The table is read
// once per state.
template <bool FLUSH, bool COND>
__global__ __launch_bounds__(256) void info_pairs_mfma(PairArgs a) {
    __shared__ unsigned long long lds[4][32 * 33];
    int ti = 0, b = int(blockIdx.x);
    while (b >= a.ntile - ti) { b -= a.ntile - ti; ++ti; }
    const int tj = ti + b;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wr = w >> 1, wc = w & 1;
    const int row0 = ti * kInfoTile + wr * 64, col0 = tj * kInfoTile + wc * 64;
    const bool active = !(ti == tj && wr > wc);

    const uint8_t* ap[2];
    const uint8_t* bp[2];
    unsigned as[2], bs[2];
    for (int q = 0; q < 2; ++q) {
        const int ia = a.colinfo[row0 + q * 32 + r], ib = a.colinfo[col0 + q * 32 + r];
        ap[q] = a.T + int64_t(ia >> 8) * a.Ppad + 16 * h;
        bp[q] = a.T + int64_t(ib >> 8) * a.Ppad + 16 * h;
        as[q] = unsigned(ia & 255) * 0x01010101u;
        bs[q] = unsigned(ib & 255) * 0x01010101u;
    }

    v16i acc[2][2];
    unsigned long long acc64[2][2][FLUSH ? 16 : 1];
    const int nstates = COND ? a.kz : 1;
    for (int zs = 0; zs < nstates; ++zs) {
        const unsigned zrep = unsigned(zs) * 0x01010101u;
        if (FLUSH)
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j)
                    for (int e = 0; e < 16; ++e) acc64[i][j][FLUSH ? e : 0] = 0;
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) acc[i][j] = v16i{};

        if (active) {
            for (int d = 0; d < a.D; ++d) {
                const uint8_t* wdp = a.wd + int64_t(d) * a.Ppad + 16 * h;
                for (int64_t seg = 0; seg < a.Ppad; seg += kInfoSegment) {
                    const int64_t segend = seg + kInfoSegment < a.Ppad ? seg + kInfoSegment : a.Ppad;
                    for (int i = 0; i < 2; ++i)
                        for (int j = 0; j < 2; ++j) acc[i][j] = v16i{};
                    for (int64_t p = seg; p < segend; p += 32) {
                        uint4 wv = *reinterpret_cast<const uint4*>(wdp + p);
                        if (COND) {
                            const uint4 xz = *reinterpret_cast<const uint4*>(a.zrow + 16 * h + p);
                            unsigned mz;
                            mz = match80(xz.x, zrep); wv.x &= mz - (mz >> 7);
                            mz = match80(xz.y, zrep); wv.y &= mz - (mz >> 7);
                            mz = match80(xz.z, zrep); wv.z &= mz - (mz >> 7);
                            mz = match80(xz.w, zrep); wv.w &= mz - (mz >> 7);
                        }
                        const uint4 xa0 = *reinterpret_cast<const uint4*>(ap[0] + p);
                        const uint4 xa1 = *reinterpret_cast<const uint4*>(ap[1] + p);
                        const uint4 xb0 = *reinterpret_cast<const uint4*>(bp[0] + p);
                        const uint4 xb1 = *reinterpret_cast<const uint4*>(bp[1] + p);
                        const v4i A0 = onehot_weighted(xa0, as[0], wv), A1 = onehot_weighted(xa1, as[1], wv);
                        const v4i B0 = onehot(xb0, bs[0]), B1 = onehot(xb1, bs[1]);
                        acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A0, B0, acc[0][0], 0, 0, 0);
                        acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A0, B1, acc[0][1], 0, 0, 0);
                        acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A1, B0, acc[1][0], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A1, B1, acc[1][1], 0, 0, 0);
                    }
                    if (FLUSH)
                        for (int i = 0; i < 2; ++i)
                            for (int j = 0; j < 2; ++j)
                                for (int e = 0; e < 16; ++e)
                                    acc64[i][j][FLUSH ? e : 0] +=
                                        (unsigned long long)(unsigned)acc[i][j][e] << (7 * d);
                }
            }
        }

        // epilogue: one 32 x 32 quarter at a time through LDS; each aligned k_x x k_y block lies in one quarter
        unsigned long long* L = lds[w];
        for (int q = 0; q < 4; ++q) {
            const int qr = q >> 1, qc = q & 1;
            if (active)
                for (int e = 0; e < 16; ++e) {
                    const int row = (e & 3) + 8 * (e >> 2) + 4 * h;   // C/D map of the 32x32 MFMA: column = lane & 31
                    L[row * 33 + r] = FLUSH ? acc64[qr][qc][FLUSH ? e : 0] : (unsigned long long)(unsigned)acc[qr][qc][e];
                }
            __syncthreads();
            if (active)
                for (int t = lane; t < 32 * 32; t += 64) {
                    const int ra = t >> 5, cb = t & 31;
                    const int R = row0 + qr * 32 + ra, C = col0 + qc * 32 + cb;
                    if (R > C) continue;
                    const int vx = a.colvar[R], vy = a.colvar[C];
                    if (vx < 0 || vy < 0 || a.sv_start[vx] != R || a.sv_start[vy] != C) continue;
                    const int kx = a.sv_k[vx], ky = a.sv_k[vy];
                    const unsigned long long* blk = L + ra * 33 + cb;
                    double part = 0.0;
                    if (a.sv_col[vx] <= a.sv_col[vy]) {   // x the more significant key digit
                        for (int i = 0; i < kx; ++i)
                            for (int j = 0; j < ky; ++j) fold_cell(part, blk[i * 33 + j], a.Nd);
                    } else {
                        for (int j = 0; j < ky; ++j)
                            for (int i = 0; i < kx; ++i) fold_cell(part, blk[i * 33 + j], a.Nd);
                    }
                    const int ux = a.sv_user[vx], uy = a.sv_user[vy];
                    const double H = (COND && zs > 0 ? a.hxy[int64_t(ux) * a.m + uy] : 0.0) + part;
                    a.hxy[int64_t(ux) * a.m + uy] = H;
                    a.hxy[int64_t(uy) * a.m + ux] = H;
                    if (vx == vy) a.h[ux] = H;
                    if (a.dump_off) {
                        int64_t o = a.dump_off[int64_t(ux) * a.m + uy], o2 = a.dump_off[int64_t(uy) * a.m + ux];
                        if (COND) {   // the block of this state: [k_cond][k_x][k_y]
                            if (o >= 0) o += int64_t(zs) * kx * ky;
                            if (o2 >= 0) o2 += int64_t(zs) * kx * ky;
                        }
                        for (int i = 0; i < kx; ++i)
                            for (int j = 0; j < ky; ++j) {
                                const unsigned long long c = blk[i * 33 + j];
                                if (o >= 0) a.dump[o + i * ky + j] = c;
                                if (o2 >= 0 && ux != uy) a.dump[o2 + j * kx + i] = c;
                            }
                    }
                }
            __syncthreads();
        }
    }
}

inline int grid_for(int64_t n, int block) {
    int64_t g = (n + block - 1) / block;
    return int(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace

int info_launch_transpose(const uint8_t* raw, int64_t P, int32_t n, int64_t Ppad, const int32_t* k, uint8_t* T,
                          unsigned* bad, void* stream) {
    dim3 grid(unsigned(Ppad / 64), unsigned((n + 63) / 64));
    hipLaunchKernelGGL(info_transpose, grid, dim3(256), 0, hipStream_t(stream), raw, P, n, Ppad, k, T, bad);
    return int(hipGetLastError());
}

int info_launch_digits(const unsigned long long* w, int64_t P, int64_t Ppad, int32_t D, uint8_t* wd, void* stream) {
    hipLaunchKernelGGL(info_digits, dim3(grid_for(Ppad, 256)), dim3(256), 0, hipStream_t(stream), w, P, Ppad, D, wd);
    return int(hipGetLastError());
}

int info_entropy_run(const InfoDev& t, const InfoSet& s, int route, uint64_t ncells, int key_bits, double Nd,
                     double* h_out, unsigned long long* cells_out, void* stream) {
    hipStream_t st = hipStream_t(stream);
    hipError_t e = hipSuccess;
    void* bufs[8] = {};
    auto alloc = [&](int slot, size_t bytes) -> void* {
        if (e == hipSuccess) e = hipMalloc(&bufs[slot], bytes < 8 ? 8 : bytes);
        return e == hipSuccess ? bufs[slot] : nullptr;
    };
    double* d_h = static_cast<double*>(alloc(0, 8));
    if (route == 1) {
        const uint64_t nchunks = (ncells + (uint64_t(1) << kInfoChunkShift) - 1) >> kInfoChunkShift;
        auto* cells = static_cast<unsigned long long*>(alloc(1, ncells * 8));
        auto* partial = static_cast<double*>(alloc(2, nchunks * 8));
        if (e == hipSuccess) e = hipMemsetAsync(cells, 0, ncells * 8, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(info_hist, dim3(grid_for(t.P, 256)), dim3(256), 0, st, t, s, cells);
            hipLaunchKernelGGL(info_fold_dense, dim3(grid_for(int64_t(nchunks), 64)), dim3(64), 0, st, cells, ncells, Nd, partial);
            hipLaunchKernelGGL(info_fold_final, dim3(1), dim3(64), 0, st, partial, nchunks, nullptr, d_h);
            e = hipGetLastError();
        }
        if (e == hipSuccess && cells_out) e = hipMemcpyAsync(cells_out, cells, ncells * 8, hipMemcpyDeviceToHost, st);
    } else {
        const size_t P = size_t(t.P);
        auto* keys = static_cast<unsigned long long*>(alloc(1, P * 8));
        auto* skeys = static_cast<unsigned long long*>(alloc(2, P * 8));
        auto* svals = static_cast<unsigned long long*>(alloc(3, P * 8));
        auto* ukeys = static_cast<unsigned long long*>(alloc(4, P * 8));
        auto* usums = static_cast<unsigned long long*>(alloc(5, P * 8));
        auto* nu = static_cast<unsigned long long*>(alloc(6, 8));
        size_t sort_bytes = 0, red_bytes = 0;
        if (e == hipSuccess)
            e = rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, skeys, t.w, svals, P, 0, unsigned(key_bits), st);
        if (e == hipSuccess)
            e = rocprim::reduce_by_key(nullptr, red_bytes, skeys, svals, P, ukeys, usums, nu, rocprim::plus<unsigned long long>(),
                                       rocprim::equal_to<unsigned long long>(), st);
        void* tmp = alloc(7, sort_bytes > red_bytes ? sort_bytes : red_bytes);
        double* partial = reinterpret_cast<double*>(keys);   // keys are dead once sorted
        if (e == hipSuccess) {
            hipLaunchKernelGGL(info_keys, dim3(grid_for(t.P, 256)), dim3(256), 0, st, t, s, keys);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            size_t b = sort_bytes;
            e = rocprim::radix_sort_pairs(tmp, b, keys, skeys, t.w, svals, P, 0, unsigned(key_bits), st);
        }
        if (e == hipSuccess) {
            size_t b = red_bytes;
            e = rocprim::reduce_by_key(tmp, b, skeys, svals, P, ukeys, usums, nu, rocprim::plus<unsigned long long>(),
                                       rocprim::equal_to<unsigned long long>(), st);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(info_fold_keys, dim3(unsigned((P + 255) / 256)), dim3(256), 0, st, ukeys, usums, nu, Nd, partial);
            hipLaunchKernelGGL(info_fold_final, dim3(1), dim3(64), 0, st, partial, uint64_t(0), nu, d_h);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_out, d_h, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    else (void)hipStreamSynchronize(st);
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    return int(e);
}

__global__ void info_mi_kernel(const double* __restrict__ h, const double* __restrict__ hxy, int32_t m, double* __restrict__ mi) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= int64_t(m) * m) return;
    const int32_t x = int32_t(i / m), y = int32_t(i % m);
    mi[i] = h[x] + h[y] - hxy[i];
}

int info_launch_mi(const double* h, const double* hxy, int32_t m, double* mi, void* stream) {
    const int64_t cells = int64_t(m) * m;
    hipLaunchKernelGGL(info_mi_kernel, dim3(unsigned((cells + 255) / 256)), dim3(256), 0, hipStream_t(stream), h, hxy, m, mi);
    return int(hipGetLastError());
}

int info_launch_pairs(const PairArgs& a, bool flush, void* stream) {
    const unsigned blocks = unsigned(int64_t(a.ntile) * (a.ntile + 1) / 2);
    if (a.zrow) {
        if (flush)
            hipLaunchKernelGGL((info_pairs_mfma<true, true>), dim3(blocks), dim3(256), 0, hipStream_t(stream), a);
        else
            hipLaunchKernelGGL((info_pairs_mfma<false, true>), dim3(blocks), dim3(256), 0, hipStream_t(stream), a);
    } else if (flush)
        hipLaunchKernelGGL((info_pairs_mfma<true, false>), dim3(blocks), dim3(256), 0, hipStream_t(stream), a);
    else
        hipLaunchKernelGGL((info_pairs_mfma<false, false>), dim3(blocks), dim3(256), 0, hipStream_t(stream), a);
    return int(hipGetLastError());
}

__global__ void info_cmi_kernel(const double* __restrict__ hxz, const double* __restrict__ hxyz, int32_t m, double hz,
                                double* __restrict__ cmi) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= int64_t(m) * m) return;
    const int32_t x = int32_t(i / m), y = int32_t(i % m);
    cmi[i] = hxz[x] + hxz[y] - hxyz[i] - hz;
}

int info_launch_cmi(const double* hxz, const double* hxyz, int32_t m, double hz, double* cmi, void* stream) {
    const int64_t cells = int64_t(m) * m;
    hipLaunchKernelGGL(info_cmi_kernel, dim3(unsigned((cells + 255) / 256)), dim3(256), 0, hipStream_t(stream), hxz, hxyz, m, hz, cmi);
    return int(hipGetLastError());
}

}  // namespace bnmi
