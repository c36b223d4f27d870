// bn_small_sweep.inc -- ONE iteration of the reference's while(true) loop (belief_propagation.hpp:75-148) on the one-workgroup path, as
// TEXT: included inside the sweep loop of bp_small_kernel (bn_small.hip) and of em_small_kernel (bn_em.hip), so that both run the
// same statements and give the same bits.  (A function would do for the bits, but not for the code: with the phases behind a call
// boundary the compiler allocates the one-round kernel's registers differently -- 69 scalar spills instead of 34 -- and the sweep
// of the ALARM-shaped network takes 2.00 us instead of 1.83.  mpe_small_kernel (bn_maxprod.hip) keeps a copy of these statements with
// its own fold: included here, with the fold as a macro, its one-round sweep was 11-14 ns slower -- DESIGN 4.16.)
//   phase 1   entry items: the terms of pi(v) (:174-200) and of the lambda-messages (:240-266) -> staging;  barrier
//   phase 2   accumulator items: each adds its run of staged terms front to back, normalises (:298-311), stores;
//             product items: lambda(v) (:220-238) and the pi-messages (:202-218) from the OLD state, normalised, stored;
//             maximum_difference (:105-131) of the wave -> LDS;  barrier;  every wave reduces the same words.
// In scope where it is included: the items bn_small_items.inc declares (ent, ecpt, bs, cs, treg, e_mm, b_rmax, b_kmax, c_dmax, c_kmax,
// kTermsInRegs); SmallLds L; the kernel's arguments `a` (N, M, re, rb, rc); int s (the iteration's number), lane, wave; the macro
// SMALL_STAMP(k).  It defines `cur`, the pointers to the two halves of the state, and `double rr`: the iteration's maximum_difference, never below
// numeric_limits<double>::min() (:105).
const int cur = s & 1;
const double* pi_cur = L.pi + cur * a.M;
const double* lam_cur = L.lam + cur * a.M;
const double* npi_cur = L.npi + cur * a.N;
const double* nlam_cur = L.nlam + cur * a.N;
double* pi_new = L.pi + (cur ^ 1) * a.M;
double* lam_new = L.lam + (cur ^ 1) * a.M;
double* npi_new = L.npi + (cur ^ 1) * a.N;
double* nlam_new = L.nlam + (cur ^ 1) * a.N;
double wres = 0.0;
SMALL_STAMP(0);
// ---- phase 1: entry items
#pragma unroll
for (int r = 0; r < ROUNDS; ++r)
    if (r < a.re) item_entry_any<kTermsInRegs, false>(e_mm[r], L.stg, L.term, pi_cur, nlam_cur, ent[r], ecpt[r], treg[r], LdPlain{});
SMALL_STAMP(1);
__syncthreads();
SMALL_STAMP(2);
// ---- phase 2a: accumulator items
#pragma unroll
for (int r = 0; r < ROUNDS; ++r) {
    if (r >= a.rb) break;
    const SmallSlot q = bs[r];
    const int kind = int(q.z & 0xffu);
    const bool on = kind != 0;
    const int base = int(q.x & 0xffffu);
    const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
    // what the stores behind the sum need of the old state is requested before it
    const double old = kind == 1 ? npi_cur[out_idx] : lam_cur[out_idx];
    const bool frozen = L.frz[out_idx] != 0;
    const double acc = small_run_sum(L.stg + base, b_rmax[r]);   // (front to back: bn_small_dev.hpp)
    if (r == 0) SMALL_STAMP(6);
    double* buf = kind == 1 ? npi_new : lam_new;
    const double val = small_normalize(buf, on, out_idx, k, at, acc, b_kmax[r]);
    if (kind == 1) npi_new[out_idx] = frozen ? old : val;  // evidence nodes are never updated (:177)
    if (kind == 2) {
        lam_new[out_idx] = val;
        wres = res_acc(wres, fabs(val - old));
    }
}
SMALL_STAMP(7);
// ---- phase 2b: product items.  They read the old state only, so they could run on either side of the barrier: here,
// because the plan gives the waves with the longest runs the cheapest products (bn_small_plan.cpp).
#pragma unroll
for (int r = 0; r < ROUNDS; ++r) {
    if (r >= a.rc) break;
    const SmallSlot q = cs[r];
    const int kind = int(q.z & 0xffu), skip = int((q.z >> 8) & 0xffffu);
    const bool on = kind != 0;
    const int cl = int(q.x & 0xffffu), deg = int(q.x >> 16);
    const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
    const double old = kind == 4 ? pi_cur[out_idx] : nlam_cur[out_idx];
    const bool frozen = L.frz[out_idx] != 0;
    // lambda(v): from 1.0 (:220-238); pi-message: from pi(v)[i] (:202-218); children in ascending order
    double val = kind == 4 ? npi_cur[q.w & 0xffffu] : 1.0;
    for (int x0 = 0; x0 < c_dmax[r]; x0 += 4) {
        double f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool has = x0 + u < deg;
            const int cb = L.clist[has ? cl + x0 + u : 0];
            f[u] = lam_cur[has ? cb + at : 0];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) val *= (x0 + u < deg && x0 + u != skip) ? f[u] : 1.0;  // x * 1.0 == x
    }
    double* buf = kind == 4 ? pi_new : nlam_new;
    val = small_normalize(buf, on, out_idx, k, at, val, c_kmax[r]);
    if (kind == 3) nlam_new[out_idx] = frozen ? old : val;  // evidence nodes are never updated (:177)
    if (kind == 4) {
        pi_new[out_idx] = val;
        wres = res_acc(wres, fabs(val - old));
    }
}
SMALL_STAMP(3);
// maximum_difference (:105-131): the wave's maximum (bit patterns of non-negative doubles order like the values)
// -> the wave's LDS word; after the barrier every wave reduces the same 16 words
const unsigned long long bits = wave_umax64_dpp((unsigned long long)__double_as_longlong(wres));
if (lane == 0) L.red[cur * 16 + wave] = bits;
SMALL_STAMP(4);
__syncthreads();
const unsigned long long mx = wave_umax64_dpp<true>(L.red[cur * 16 + (lane & 15)]);
double rr = __longlong_as_double((long long)mx);
rr = rr < DBL_MIN ? DBL_MIN : rr;
SMALL_STAMP(5);
