// bn_small_dev.hpp -- the device pieces the five item kernels share (bp_small_kernel, em_small_kernel, bp_mid_kernel, mpe_small_kernel,
// mpe_mid_kernel: bn_small.hip, bn_em.hip, bn_mid.hip, bn_maxprod.hip):
//   all five             wave-level reductions without LDS traffic; the entry item (item_entry: the ONE routine, told how a state word
//                        is loaded and whether a bare table entry is canonicalised); the thread's items (bn_small_items.inc, as
//                        text; mpe_small_kernel alone keeps its own)
//   one workgroup        LDS layout (SmallLds), run sum, normalisation in place; the iteration's statements of bp_small_kernel and
//                        em_small_kernel are bn_small_sweep.inc, as text (the same bits); the evidence prologue of
//                        bp_small_kernel and mpe_small_kernel is bn_small_evidence.inc, as text
//   several workgroups   LDS layout (MidLds), normalisation through a scratch line, agent-scope state accesses; bp_mid_kernel and
//                        mpe_mid_kernel keep sweeps of their own (a grid barrier inside one launch against one launch per sweep)
// The kernels' argument structs differ; what the helpers read of them (N, M, T, TT, CL, npi_init, node_off) has the same names in
// all, so they take the struct as a template parameter.
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

// How an entry item reads a word of the state: from LDS or from memory no other workgroup writes during the launch (a plain load), or
// from memory other workgroups of the launch write (agent scope, sc1: through to L2 / memory, coherent across the XCDs).
__device__ __forceinline__ double ld_state(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                            __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_state(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
struct LdPlain { __device__ __forceinline__ double operator()(const double* p) const { return *p; } };
struct LdAgent { __device__ __forceinline__ double operator()(const double* p) const { return ld_state(p); } };

// One CPT entry: cpt * pi-messages in ascending parent order (:174-200) and, per target parent, (lambda(v)[i] * cpt)
// * the OTHER parents' pi-messages in ascending order (:240-266), into their places of the staging array `stg`.  MM = the wave's
// largest parent count: the loops are unrolled to it, a lane with fewer parents multiplies by 1.0 (x * 1.0 == x).  REG: the entry's
// parent terms are in `treg` (they never change: kept in registers when they fit -- one round of items, <= 4 parents), else in
// `term`.  pi_cur / nlam_cur: the old state, read through `ld`.  CANON: a bare table entry (no parents) is staged quiet, like every
// product (max-product: bn_maxprod.hip mpe_max).
template <int MM, bool REG, bool CANON, class Ld>
__device__ __forceinline__ void item_entry(double* stg, const uint32_t* term, const double* pi_cur, const double* nlam_cur, SmallEntry h, double c,
                                           const uint32_t (&treg)[4], Ld ld) {
    if (((h.y >> 24) & 1u) == 0) return;
    const int m = int((h.y >> 16) & 0xffu), tbase = int(h.y & 0xffffu);
    const double li = ld(nlam_cur + (h.x & 0xffffu));
    uint32_t tw[MM > 0 ? MM : 1];
    double pj[MM > 0 ? MM : 1];
#pragma unroll
    for (int j = 0; j < MM; ++j) {
        if (REG && MM <= 4) tw[j] = treg[j < 4 ? j : 0];
        else tw[j] = j < m ? term[tbase + j] : 0u;
    }
#pragma unroll
    for (int j = 0; j < MM; ++j) {
        const double x = ld(pi_cur + (tw[j] & 0xffffu));
        pj[j] = j < m ? x : 1.0;
    }
    double v = (CANON && MM == 0) ? __builtin_canonicalize(c) : c;
#pragma unroll
    for (int j = 0; j < MM; ++j) v *= pj[j];
    stg[h.x >> 16] = v;
    const double lc = li * c;
#pragma unroll
    for (int jt = 0; jt < MM; ++jt) {
        double w = lc;
#pragma unroll
        for (int j = 0; j < MM; ++j)
            if (j != jt) w *= pj[j];
        if (jt < m) stg[tw[jt] >> 16] = w;
    }
}

template <bool REG, bool CANON, class Ld>
__device__ __forceinline__ void item_entry_any(int mm, double* stg, const uint32_t* term, const double* pi_cur, const double* nlam_cur, SmallEntry h,
                                               double c, const uint32_t (&treg)[4], Ld ld) {
    switch (mm) {
        case 0: return item_entry<0, REG, CANON>(stg, term, pi_cur, nlam_cur, h, c, treg, ld);
        case 1: return item_entry<1, REG, CANON>(stg, term, pi_cur, nlam_cur, h, c, treg, ld);
        case 2: return item_entry<2, REG, CANON>(stg, term, pi_cur, nlam_cur, h, c, treg, ld);
        case 3: return item_entry<3, REG, CANON>(stg, term, pi_cur, nlam_cur, h, c, treg, ld);
        case 4: return item_entry<4, REG, CANON>(stg, term, pi_cur, nlam_cur, h, c, treg, ld);
        case 5: case 6: return item_entry<6, REG, CANON>(stg, term, pi_cur, nlam_cur, h, c, treg, ld);
        default: return item_entry<8, REG, CANON>(stg, term, pi_cur, nlam_cur, h, c, treg, ld);
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

// ---- several workgroups (bn_mid.hip, bn_maxprod.hip mpe_mid_kernel): the state is in device memory, a workgroup's LDS holds its own
// part's staged terms, parent terms and child lists.  MidPlan::lds_bytes (bn_small_plan.cpp build_plan_of_range, `part`) is sized
// for this whole layout, `flag` and both halves of `red` included, and bn_engine_mpe.cpp launches mpe_mid_kernel with that figure:
// the max-product kernel uses the same layout and simply never touches `flag`.

struct MidLds {
    double* stg;        // [T] this workgroup's staged terms
    uint32_t* term;     // [TT]
    uint16_t* clist;    // [CL]
    double* scratch;    // [waves][64] normalisation: a line per wave
    unsigned long long* red;  // [2][16] per-wave residuals, [32], [33]: what the last grid barrier collected (mpe_mid_kernel: [16] per-wave
                              // residuals, [16], [17]: the previous sweep's maximum, the stop word)
    unsigned* flag;     // [1] set by the polling thread: the grid wait gave up
};

__device__ __forceinline__ MidLds mid_carve(char* base, const MidPart& pt) {
    MidLds L;
    double* d = reinterpret_cast<double*>(base);
    L.stg = d; d += pt.T;
    L.scratch = d; d += kSmallMaxWaves * kWave;
    L.red = reinterpret_cast<unsigned long long*>(d); d += 2 * 16 + 2;
    L.term = reinterpret_cast<uint32_t*>(d);
    char* c = reinterpret_cast<char*>(L.term + (((pt.TT > 0 ? pt.TT : 1) + 1) & ~1));
    L.clist = reinterpret_cast<uint16_t*>(c);
    c += (size_t(pt.CL > 0 ? pt.CL : 1) * 2 + 7) & ~size_t(7);
    L.flag = reinterpret_cast<unsigned*>(c);
    return L;
}

// normalisation of the vector whose elements sit in adjacent lanes of this wave, through the wave's scratch line (:298-311); the line
// keeps the un-normalised vector afterwards
__device__ __forceinline__ double mid_normalize(double* line, int lane, int k, int at, double val, int kmax) {
    line[lane] = val;
    lds_fence();
    const int first = lane - at;
    double sum = 0.0;
    for (int r0 = 0; r0 < kmax; r0 += 4) {
        double x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = line[first + (r0 + q < k ? r0 + q : 0)];
#pragma unroll
        for (int q = 0; q < 4; ++q) sum += r0 + q < k ? x[q] : 0.0;  // + 0.0 past the end: a sum started from +0.0 is never -0.0
    }
    lds_fence();
    return val / sum;
}

}  // namespace bnmi
