// bn_small_dev.hpp -- device helpers shared by the item kernels: wave-level reductions without LDS traffic (bn_small.hip, bn_mid.hip,
// bn_maxprod.hip), and the pieces of the one-workgroup iteration of sum-product belief propagation -- LDS layout, entry item, run sum,
// normalisation -- which bn_small.hip (bp_small_kernel) and bn_em.hip (em_small_kernel) both run.  The thread's items and the
// iteration's statements themselves are bn_small_items.inc and bn_small_sweep.inc, included by both kernels: one text, the same bits.  The kernels' argument
// structs differ; what the helpers read of them (N, M, T, TT, CL, re, rb, rc and the item tables) has the same names in both, so they
// take the struct as a template parameter.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

#include "bn_small.hpp"
#include "bn_tiles.hpp"

namespace bnmi {

__device__ __forceinline__ void lds_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// max over the wave's lanes with DPP moves (no LDS traffic: __shfl_xor is a ds_bpermute per step, and 64 lanes of one
// LDS atomic on the same word cost ~2.4 us): row_shr 1, 2, 4, 8 leave each row's maximum in its lane 15, row_bcast:15 /
// row_bcast:31 carry it on to lane 63.  ROW = true stops after the rows (the maximum of lanes 0..15 in lane 15).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_umax_step(unsigned x) {
    const unsigned o = unsigned(__builtin_amdgcn_update_dpp(0, int(x), CTRL, ROW_MASK, 0xf, true));
    return o > x ? o : x;
}
template <bool ROW = false>
__device__ __forceinline__ unsigned wave_umax32_dpp(unsigned x) {
    x = dpp_umax_step<0x111, 0xf>(x);
    x = dpp_umax_step<0x112, 0xf>(x);
    x = dpp_umax_step<0x114, 0xf>(x);
    x = dpp_umax_step<0x118, 0xf>(x);
    if (ROW) return unsigned(__builtin_amdgcn_readlane(int(x), 15));
    x = dpp_umax_step<0x142, 0xa>(x);
    x = dpp_umax_step<0x143, 0xc>(x);
    return unsigned(__builtin_amdgcn_readlane(int(x), 63));
}
// ... of 64-bit words: the high halves first, then the low halves of the lanes that hold the largest high half
template <bool ROW = false>
__device__ __forceinline__ unsigned long long wave_umax64_dpp(unsigned long long v) {
    const unsigned hi = unsigned(v >> 32), lo = unsigned(v);
    const unsigned hm = wave_umax32_dpp<ROW>(hi);
    const unsigned lm = wave_umax32_dpp<ROW>(hi == hm ? lo : 0u);
    return (unsigned long long)hm << 32 | lm;
}

__device__ __forceinline__ int wave_imax(int x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(x, off, 64);
        x = o > x ? o : x;
    }
    return __builtin_amdgcn_readfirstlane(x);
}

// ---- the one-workgroup iteration (bn_small.hpp / bn_small_plan.cpp: items and encodings; belief_propagation.hpp:33-158) -------------

struct SmallLds {
    double* pi;     // [2][M]  (buffer c of an array at + c * its length: no pointer tables, they would live in scratch memory)
    double* lam;    // [2][M]
    double* npi;    // [2][N]
    double* nlam;   // [2][N]
    double* stg;
    uint32_t* term;
    uint16_t* clist;
    uint8_t* frz;
    unsigned long long* red;
};

template <class Args>
__device__ __forceinline__ SmallLds small_carve(char* base, const Args& a) {
    SmallLds L;
    double* d = reinterpret_cast<double*>(base);
    L.pi = d; d += 2 * a.M;
    L.lam = d; d += 2 * a.M;
    L.npi = d; d += 2 * a.N;
    L.nlam = d; d += 2 * a.N;
    L.stg = d; d += a.T;
    L.term = reinterpret_cast<uint32_t*>(d);
    char* c = reinterpret_cast<char*>(L.term + (((a.TT > 0 ? a.TT : 1) + 1) & ~1));  // the arrays behind stay 8-byte aligned
    L.clist = reinterpret_cast<uint16_t*>(c);
    c += (size_t(a.CL > 0 ? a.CL : 1) * 2 + 7) & ~size_t(7);
    L.frz = reinterpret_cast<uint8_t*>(c);
    c += (size_t(a.N) + 7) & ~size_t(7);
    L.red = reinterpret_cast<unsigned long long*>(c);
    return L;
}

// One CPT entry: cpt * pi-messages in ascending parent order (:174-200) and, per target parent, (lambda(v)[i] * cpt)
// * the OTHER parents' pi-messages in ascending order (:240-266).  MM = the wave's largest parent count: the loops are
// unrolled to it, a lane with fewer parents multiplies by 1.0 (x * 1.0 == x).
template <int MM, bool REG>
__device__ __forceinline__ void small_entry(const SmallLds& L, const double* pi_cur, const double* nlam_cur, SmallEntry h, double c,
                                            const uint32_t (&treg)[4]) {
    if (((h.y >> 24) & 1u) == 0) return;
    const int m = int((h.y >> 16) & 0xffu), tbase = int(h.y & 0xffffu);
    const double li = nlam_cur[h.x & 0xffffu];
    uint32_t tw[MM > 0 ? MM : 1];
    double pj[MM > 0 ? MM : 1];
#pragma unroll
    for (int j = 0; j < MM; ++j) {
        if (REG && MM <= 4) tw[j] = treg[j < 4 ? j : 0];  // (an entry's parent terms never change: kept in registers when they fit)
        else tw[j] = j < m ? L.term[tbase + j] : 0u;
    }
#pragma unroll
    for (int j = 0; j < MM; ++j) {
        const double x = pi_cur[tw[j] & 0xffffu];
        pj[j] = j < m ? x : 1.0;
    }
    double v = c;
#pragma unroll
    for (int j = 0; j < MM; ++j) v *= pj[j];
    L.stg[h.x >> 16] = v;
    const double lc = li * c;
#pragma unroll
    for (int jt = 0; jt < MM; ++jt) {
        double w = lc;
#pragma unroll
        for (int j = 0; j < MM; ++j)
            if (j != jt) w *= pj[j];
        if (jt < m) L.stg[tw[jt] >> 16] = w;
    }
}

template <bool REG>
__device__ __forceinline__ void small_entry_any(int mm, const SmallLds& L, const double* pi_cur, const double* nlam_cur, SmallEntry h, double c,
                                                const uint32_t (&treg)[4]) {
    switch (mm) {
        case 0: return small_entry<0, REG>(L, pi_cur, nlam_cur, h, c, treg);
        case 1: return small_entry<1, REG>(L, pi_cur, nlam_cur, h, c, treg);
        case 2: return small_entry<2, REG>(L, pi_cur, nlam_cur, h, c, treg);
        case 3: return small_entry<3, REG>(L, pi_cur, nlam_cur, h, c, treg);
        case 4: return small_entry<4, REG>(L, pi_cur, nlam_cur, h, c, treg);
        case 5: case 6: return small_entry<6, REG>(L, pi_cur, nlam_cur, h, c, treg);
        default: return small_entry<8, REG>(L, pi_cur, nlam_cur, h, c, treg);
    }
}

// The run of an accumulator item, added strictly front to back (the reference's order): the chain of dependent additions IS the
// phase's critical path.  Runs are padded with zeros to the wave's common length n4, a multiple of 4 (bn_small_plan.cpp), so a step
// is four loads at immediate offsets -- issued one step ahead -- and four additions, nothing else.
__device__ __forceinline__ double small_run_sum(const double* ptr, int n4) {
    double acc = 0.0;
    double x0 = ptr[0], x1 = ptr[1], x2 = ptr[2], x3 = ptr[3];
    int r0 = 0;
    for (; r0 + 8 <= n4; r0 += 8) {
        const double y0 = ptr[r0 + 4], y1 = ptr[r0 + 5], y2 = ptr[r0 + 6], y3 = ptr[r0 + 7];
        acc += x0; acc += x1; acc += x2; acc += x3;
        x0 = ptr[r0 + 8]; x1 = ptr[r0 + 9]; x2 = ptr[r0 + 10]; x3 = ptr[r0 + 11];
        acc += y0; acc += y1; acc += y2; acc += y3;
    }
    if (r0 < n4) { acc += x0; acc += x1; acc += x2; acc += x3; }  // an odd number of steps: the last four are loaded already
    return acc;
}

// The sum of the vector whose elements sit in adjacent lanes of this wave: the element goes to its place in `buf`, every lane then
// adds the vector's elements front to back (:298-311: plain left-to-right sum).  kmax = the wave's largest arity.  LDS operations of
// one wave execute in order: a caller's later store to the same place comes after every lane's reads.
__device__ __forceinline__ double small_vector_sum(double* buf, bool on, int out_idx, int k, int at, double val, int kmax) {
    if (on) buf[out_idx] = val;
    lds_fence();
    const int vec = on ? out_idx - at : 0;
    double sum = 0.0;
    for (int r0 = 0; r0 < kmax; r0 += 4) {
        double x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = buf[vec + (r0 + q < k ? r0 + q : 0)];
#pragma unroll
        for (int q = 0; q < 4; ++q) sum += r0 + q < k ? x[q] : 0.0;  // + 0.0 past the end: a sum started from +0.0 is never -0.0
    }
    lds_fence();
    return sum;
}
// ... and the normalisation (:298-311, no zero guard)
__device__ __forceinline__ double small_normalize(double* buf, bool on, int out_idx, int k, int at, double val, int kmax) {
    return val / small_vector_sum(buf, on, out_idx, k, at, val, kmax);
}

}  // namespace bnmi
