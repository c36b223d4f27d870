// bn_maxprod.hip -- max-product belief propagation (most probable explanation) over the item tables of the sum-product item
// kernels (bn_small.hpp / bn_small_plan.cpp: entry, accumulator and product items).  The algorithm, the fold's NaN rule, the
// state's tie rule and the cap: bn_maxprod.hpp.  Reference for everything but the fold: belief_propagation.hpp:33-158.
//
//   mpe_small_kernel   one workgroup runs the whole run with the state in LDS (the shape of bn_small.hip's kernel, over the same
//                      pieces of bn_small_dev.hpp and the same evidence prologue, bn_small_evidence.inc): phase 1 entry items ->
//                      staged terms; barrier; phase 2 accumulator items (running MAXIMUM of the run, eight independent partial
//                      maxima), product items, residual; barrier; stop decision by every wave.  The items and the iteration are
//                      written out here, NOT bn_small_items.inc / bn_small_sweep.inc: on those texts the one-round kernel runs
//                      the same instructions under other register names and its sweep of the ALARM-shaped network takes 11-14 ns
//                      longer (measured), against a spread of 1-2 ns between processes.
//   mpe_mid_*          one workgroup per MidPart, state in device memory, ONE LAUNCH PER SWEEP.  Nothing waits inside a kernel:
//                      a sweep's launch reads buffer s & 1 and writes the other, leaves its workgroup's maximum_difference in a
//                      word of its own, and the NEXT launch's workgroups reduce those words and decide.  Items, entry item, LDS
//                      layout and normalisation are the ones bp_mid_kernel uses (bn_small_dev.hpp); the sweep's statements are
//                      its own (plain loads: nothing it reads is written during its launch).
#include "bn_maxprod.hpp"
#include "bn_tiles.hpp"
#include "bn_small_dev.hpp"
#include "bn_item_launch.hpp"

namespace bnmi {

namespace {

// The running maximum of bn_maxprod.hpp, acc = (acc < x) ? x : acc, as ONE instruction.  v_max_f64 returns the other operand where one
// is a quiet NaN and +0.0 for (+0.0, -0.0): with acc never NaN and never -0.0 (it starts at +0.0 and is only ever replaced by a larger
// term) that is the rule exactly -- for every x that is not a SIGNALLING NaN, which the hardware would quiet and return.  A staged term
// never is one: it is the result of a multiplication, or canonicalised where it is a bare table entry (item_entry's CANON).  (The rule spelt
// out in C++ compiles to a compare and two selects per term: three times the issue slots, and slower than the sum's chain of adds.)
__device__ __forceinline__ double mpe_max(double acc, double x) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(acc), "v"(x));
    return r;
}

// The largest of the n4 (a multiple of 4, the same for every lane of the wave) staged terms from `ptr` on, from +0.0.  max is
// associative and commutative and acc is never NaN, so the terms go into W (8 or 4) independent partial maxima -- no chain of n4
// dependent operations as in the sum -- combined at the end.  The loads run ahead of the maxima: by two steps of W terms (TWO; what a
// kernel with one round of items has the registers for) or by one.  What is loaded past the run's end is never used, and lies inside
// the staging array: at most 16 words past, and the plan leaves 16 words behind the last run (bn_small_plan.cpp).
template <int W, bool TWO>
__device__ __forceinline__ double mpe_fold(const double* ptr, int n4) {
    static_assert(W == 4 || W == 8, "n4 is a multiple of 4");
    double m[W], a[W], b[TWO ? W : 1];
#pragma unroll
    for (int q = 0; q < W; ++q) { m[q] = 0.0; a[q] = ptr[q]; }
    int r0 = 0;
    if (TWO) {
#pragma unroll
        for (int q = 0; q < W; ++q) b[TWO ? q : 0] = ptr[W + q];
        for (; r0 + 2 * W <= n4; r0 += 2 * W) {
#pragma unroll
            for (int q = 0; q < W; ++q) { m[q] = mpe_max(m[q], a[q]); a[q] = ptr[r0 + 2 * W + q]; }
#pragma unroll
            for (int q = 0; q < W; ++q) { m[q] = mpe_max(m[q], b[TWO ? q : 0]); b[TWO ? q : 0] = ptr[r0 + 3 * W + q]; }
        }
    }
    // a holds [r0, r0 + W) (and b [r0 + W, r0 + 2 W))
    for (; r0 + W <= n4; r0 += W) {
#pragma unroll
        for (int q = 0; q < W; ++q) { m[q] = mpe_max(m[q], a[q]); a[q] = TWO ? b[TWO ? q : 0] : ptr[r0 + W + q]; }
    }
    if (W == 8 && r0 < n4) {   // four terms are left
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] = mpe_max(m[q], a[q]);
    }
#pragma unroll
    for (int w = W / 2; w >= 1; w /= 2)
#pragma unroll
        for (int q = 0; q < w; ++q) m[q] = mpe_max(m[q], m[q + w]);
    return m[0];
}

// the state of the vector vec[0 .. k): the lowest index that holds the largest element (strict >); all NaN: 0
__device__ __forceinline__ int mpe_decode(const double* vec, int k) {
    int idx = 0;
    double best = vec[0];
    for (int i = 1; i < k; ++i) {
        const double x = vec[i];
        if (x > best) { best = x; idx = i; }
    }
    return idx;
}

// this thread's items of one round and what the wave needs to know of its lanes' items
struct MpeItems {
    SmallEntry ent;
    double ecpt;
    uint32_t treg[4];   // the entry's parent terms (one round of items only)
    SmallSlot bs, cs;
    int e_mm, b_rmax, b_kmax, c_dmax, c_kmax;
};
template <bool REG>
__device__ __forceinline__ void mpe_items_finish(MpeItems& it, const uint32_t* term) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        it.treg[j] = 0u;
        if (REG && ((it.ent.y >> 24) & 1u) && j < int((it.ent.y >> 16) & 0xffu)) it.treg[j] = term[(it.ent.y & 0xffffu) + j];
    }
    it.e_mm = wave_imax(((it.ent.y >> 24) & 1u) ? int((it.ent.y >> 16) & 0xffu) : 0);
    it.b_rmax = wave_imax(int(it.bs.x >> 16));
    it.b_kmax = wave_imax(it.bs.z != 0 ? int((it.bs.y >> 16) & 0xffu) : 0);
    it.c_dmax = wave_imax(int(it.cs.x >> 16));
    it.c_kmax = wave_imax((it.cs.z & 0xffu) != 0 ? int((it.cs.y >> 16) & 0xffu) : 0);
}

}  // namespace

// ROUNDS = items of one kind per thread (1, 2 or kSmallMaxRounds)
template <int ROUNDS>
__global__ __launch_bounds__(kSmallMaxWaves * kWave) void mpe_small_kernel(MpeSmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) char mpe_lds[];
    const int set = blockIdx.x;
    double* state = a.state + int64_t(set) * (2 * int64_t(a.M) + 2 * int64_t(a.N));
    double* res_hist = a.res_hist + int64_t(set) * a.res_cap;
    const SmallLds L = small_carve(mpe_lds, a);   // (the layout SmallPlan::lds_bytes is sized for: bn_small_plan.cpp)
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long t_first = wall_clock64();

    // ---- this thread's items, kept in registers for the whole run
    constexpr bool kTermsInRegs = ROUNDS == 1;
    MpeItems it[ROUNDS];
    int node_of[ROUNDS];   // the node whose state this lane decodes at the end (-1: none): the first element of a lambda(v) item's vector
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        it[r].ent = SmallEntry{0u, 0u}; it[r].ecpt = 0.0;
        it[r].bs = SmallSlot{0u, 0u, 0u, 0u}; it[r].cs = SmallSlot{0u, 0u, 0u, 0u};
        if (r < a.re) { it[r].ent = a.ent[r * nt + tid]; it[r].ecpt = a.ent_cpt[r * nt + tid]; }
        if (r < a.rb) it[r].bs = a.bslot[r * nt + tid];
        if (r < a.rc) it[r].cs = a.cslot[r * nt + tid];
        mpe_items_finish<kTermsInRegs>(it[r], a.term);
        node_of[r] = -1;
        if ((it[r].cs.z & 0xffu) == 3 && lane == int(it[r].cs.y >> 24)) node_of[r] = a.elem_node[it[r].cs.y & 0xffffu];
    }
    // ---- tables and initial state (:33-73) into LDS
    for (int t = tid; t < a.TT; t += nt) L.term[t] = a.term[t];
    for (int t = tid; t < a.CL; t += nt) L.clist[t] = a.clist[t];
    for (int t = tid; t < a.T; t += nt) L.stg[t] = 0.0;  // the padding of the runs stays zero for the whole run
    int s = a.sweep_begin;
    {
        const int c0 = s & 1;
        // the evidence arrays themselves (mapped host memory)
        const int32_t* meta = a.ev_meta + 8 * set;
        const int ne = meta[0], nval = meta[4];
        const int32_t* ev_node = a.ev_node + meta[1];
        const int32_t* ev_off = a.ev_off + meta[2];
        const double* ev_val = a.ev_val + meta[3];
#include "bn_small_evidence.inc"
        for (int x = tid; x < a.M; x += nt) {
            L.pi[c0 * a.M + x] = s == 0 ? 1.0 : state[x];
            L.lam[c0 * a.M + x] = s == 0 ? 1.0 : state[a.M + x];
        }
        if (tid < 32) L.red[tid] = 0ull;
    }
    __syncthreads();

    int done = 0;
    double r_last = 0.0;
    for (;;) {
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
        // ---- phase 1: entry items
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
            if (r < a.re) item_entry_any<kTermsInRegs, true>(it[r].e_mm, L.stg, L.term, pi_cur, nlam_cur, it[r].ent, it[r].ecpt, it[r].treg, LdPlain{});
        __syncthreads();
        // ---- phase 2a: accumulator items: the LARGEST term of the run (the one line that differs from sum-product)
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            if (r >= a.rb) break;
            const SmallSlot q = it[r].bs;
            const int kind = int(q.z & 0xffu);
            const bool on = kind != 0;
            const int base = int(q.x & 0xffffu);
            const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
            const double old = kind == 1 ? npi_cur[out_idx] : lam_cur[out_idx];
            const bool frozen = L.frz[out_idx] != 0;
            const double acc = mpe_fold<(ROUNDS <= 2 ? 8 : 4), ROUNDS == 1>(L.stg + base, it[r].b_rmax);
            double* buf = kind == 1 ? npi_new : lam_new;
            const double val = small_normalize(buf, on, out_idx, k, at, acc, it[r].b_kmax);
            if (kind == 1) npi_new[out_idx] = frozen ? old : val;  // evidence nodes are never updated (:177)
            if (kind == 2) {
                lam_new[out_idx] = val;
                wres = res_acc(wres, fabs(val - old));
            }
        }
        // ---- phase 2b: product items (old state only)
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            if (r >= a.rc) break;
            const SmallSlot q = it[r].cs;
            const int kind = int(q.z & 0xffu), skip = int((q.z >> 8) & 0xffffu);
            const bool on = kind != 0;
            const int cl = int(q.x & 0xffffu), deg = int(q.x >> 16);
            const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
            const double old = kind == 4 ? pi_cur[out_idx] : nlam_cur[out_idx];
            const bool frozen = L.frz[out_idx] != 0;
            // lambda(v): from 1.0 (:220-238); pi-message: from pi(v)[i] (:202-218); children in ascending order
            double val = kind == 4 ? npi_cur[q.w & 0xffffu] : 1.0;
            for (int x0 = 0; x0 < it[r].c_dmax; x0 += 4) {
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
            val = small_normalize(buf, on, out_idx, k, at, val, it[r].c_kmax);
            if (kind == 3) nlam_new[out_idx] = frozen ? old : val;  // evidence nodes are never updated (:177)
            if (kind == 4) {
                pi_new[out_idx] = val;
                wres = res_acc(wres, fabs(val - old));
            }
        }
        // maximum_difference (:105-131): wave -> LDS word; after the barrier every wave reduces the same 16 words
        const unsigned long long bits = wave_umax64_dpp((unsigned long long)__double_as_longlong(wres));
        if (lane == 0) L.red[cur * 16 + wave] = bits;
        __syncthreads();
        const unsigned long long mx = wave_umax64_dpp<true>(L.red[cur * 16 + (lane & 15)]);
        double rr = __longlong_as_double((long long)mx);
        rr = rr < DBL_MIN ? DBL_MIN : rr;
        r_last = rr;
        if (tid == 0 && s < a.res_cap) res_hist[s] = rr;
        ++s;
        if (rr < a.eps) { done = 1; break; }                 // strict < (:147)
        if (s >= a.max_sweeps) { done = 2; break; }          // the cap (always set: bn_maxprod.hpp)
        if (s - a.sweep_begin >= a.budget) break;            // the host continues in another launch
    }

    // ---- the state the run stopped in -> memory; max-marginal = normalize(pi % lambda) (:151-158); the node's state
    const int fin = s & 1;
    for (int x = tid; x < a.M; x += nt) { state[x] = L.pi[fin * a.M + x]; state[a.M + x] = L.lam[fin * a.M + x]; }
    for (int y = tid; y < a.N; y += nt) { state[2 * a.M + y] = L.npi[fin * a.N + y]; state[2 * a.M + a.N + y] = L.nlam[fin * a.N + y]; }
    double* out_mm = a.max_marginals + int64_t(set) * a.N;
    int32_t* out_st = a.states + int64_t(set) * a.n;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (r >= a.rc) break;
        const SmallSlot q = it[r].cs;
        const bool on = (q.z & 0xffu) == 3;  // the lambda(v) items: one per node-vector element
        const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
        const double val = on ? L.npi[fin * a.N + out_idx] * L.nlam[fin * a.N + out_idx] : 0.0;
        const double bel = small_normalize(L.stg, on, out_idx, on ? k : 0, at, val, it[r].c_kmax);
        if (on) { out_mm[out_idx] = bel; L.stg[out_idx] = bel; }
        lds_fence();
        if (node_of[r] >= 0) out_st[node_of[r]] = mpe_decode(L.stg + out_idx, k);
    }
    if (tid == 0) {
        MpeCtl* h = a.host_ctl + set;
        h->last_res = r_last; h->n_sweeps = s; h->t_first = t_first; h->t_last = wall_clock64();
        h->run_id = a.run_id; h->done = done;
    }
}

constexpr auto mpe_small_of = [](auto R) { return mpe_small_kernel<decltype(R)::value>; };

int prepare_mpe_small() { return prepare_item_kernels(mpe_small_of); }

int launch_mpe_small(const MpeSmallArgs& a, int waves, size_t lds_bytes, int n_sets, void* stream) {
    return launch_item_kernel(item_rounds(a.re, a.rb, a.rc), mpe_small_of, dim3(n_sets > 1 ? n_sets : 1), dim3(waves * kWave), lds_bytes, stream, a);
}

// ================================================================================================================================
// several workgroups, one launch per sweep

// Initial state (:33-64) of buffer 0, no evidence marks, the run goes on.  A flat grid over the elements.
__global__ __launch_bounds__(256) void mpe_mid_init_kernel(MpeMidArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x < a.N) {
        a.npi[x] = a.npi_init[x];
        a.nlam[x] = 1.0;
        a.frz[x] = 0;
    }
    if (x < a.M) { a.pi[x] = 1.0; a.lam[x] = 1.0; }
    if (x == 0) { a.sync->stop_sweeps = -1; a.sync->t_first = wall_clock64(); }
}
// Evidence (:68-73): both pi(v) and lambda(v) take the vector; the node is marked.  One thread per finding.
__global__ __launch_bounds__(256) void mpe_mid_evidence_kernel(MpeMidArgs a) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.ev_ne) return;
    const int v = a.ev_node[j], o = a.ev_off[j];
    const int lo = a.node_off[v], hi = a.node_off[v + 1];
    for (int i = 0; i < hi - lo; ++i) {
        const double x = a.ev_val[o + i];
        a.frz[lo + i] = 1;
        a.npi[lo + i] = x;
        a.nlam[lo + i] = x;
    }
}

// Launch number s of a run (FINISH: the launch behind a group of sweeps).  Every workgroup first learns whether the run is over:
// from the stop word an earlier launch left, else by reducing the words of sweep s - 1 -- all workgroups read the same words and
// decide alike, workgroup 0 records the decision.  A run that is over: a sweep launch returns without touching anything, the
// finishing launch writes max-marginals and states.  Else the sweep: old state = buffer s & 1, new state = the other.
template <int ROUNDS, bool FINISH>
__global__ __launch_bounds__(kSmallMaxWaves * kWave) void mpe_mid_kernel(MpeMidArgs a, int32_t s) {
    extern __shared__ __attribute__((aligned(16))) char mpe_lds[];
    const MidPart pt = a.parts[blockIdx.x];
    const MidLds L = mid_carve(mpe_lds, pt);   // (the layout MidPlan::lds_bytes is sized for; `flag` is never touched here)
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* line = L.scratch + wave * kWave;

    // ONE thread reads the stop word (workgroup 0 of this very launch may be writing it: every thread of a workgroup must see the
    // same value, they meet at barriers below -- either value leads to the same decision)
    if (tid == 0) L.red[17] = (unsigned long long)(long long)__hip_atomic_load(&a.sync->stop_sweeps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    int stopped = int((long long)L.red[17]);
    if (stopped < 0 && s > 0) {
        if (tid < kWave) {
            static_assert(kMidMaxParts <= 4 * kWave, "lane l reads the words of workgroups l, l + 64, l + 128, l + 192");
            const unsigned long long* w = a.sync->words[(s - 1) & 1];
            unsigned long long mx = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = tid + u * kWave;
                const unsigned long long x = p < a.nparts ? w[p] : 0ull;
                mx = x > mx ? x : mx;
            }
            mx = wave_umax64_dpp(mx);
            if (tid == 0) L.red[16] = mx;
        }
        __syncthreads();
        double rr = __longlong_as_double((long long)L.red[16]);
        rr = rr < DBL_MIN ? DBL_MIN : rr;
        const int verdict = rr < a.eps ? 1 : (s >= a.max_sweeps ? 2 : 0);   // strict < (:147); the cap
        if (blockIdx.x == 0 && tid == 0) {
            if (s - 1 < a.res_cap) a.res_hist[s - 1] = rr;
            if (verdict != 0) {
                MpeCtl* h = a.host_ctl;
                h->last_res = rr; h->n_sweeps = s; h->t_first = a.sync->t_first; h->t_last = wall_clock64();
                h->run_id = a.run_id; h->done = verdict;
                __hip_atomic_store(&a.sync->stop_sweeps, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (verdict != 0) stopped = s;
    }
    if (!FINISH && stopped >= 0) return;   // a launch queued behind the stopping sweep
    if (FINISH && stopped < 0) return;     // the host reads done == 0 and queues the next group

    // ---- this thread's items (the finishing launch: its product items only)
    const SmallEntry* const it_ent = a.ent + pt.ent_off; const double* const it_cpt = a.ent_cpt + pt.ent_off; const uint32_t* const it_term = a.term + pt.term_off;
    const SmallSlot* const it_bslot = a.bslot + pt.bslot_off; const SmallSlot* const it_cslot = a.cslot + pt.cslot_off;
    const int it_nt = pt.nt, it_re = FINISH ? 0 : pt.re, it_rb = FINISH ? 0 : pt.rb, it_rc = pt.rc;
    const bool it_mine = tid < pt.nt;   // (the launch is as wide as the widest part)
#include "bn_small_items.inc"

    if (FINISH) {
        // ---- max-marginal = normalize(pi % lambda) (:151-158) of this workgroup's nodes from the state the run stopped in; the state
        const int fin = stopped & 1;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            if (r >= pt.rc) break;
            const SmallSlot q = cs[r];
            const bool on = (q.z & 0xffu) == 3;  // the lambda(v) items: one per node-vector element
            const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
            const double val = on ? a.npi[fin * a.N + out_idx] * a.nlam[fin * a.N + out_idx] : 0.0;
            lds_fence();   // (the line is still being read: by mpe_decode of the round before)
            const double bel = mid_normalize(line, lane, on ? k : 0, on ? at : 0, val, c_kmax[r]);
            if (on) a.max_marginals[out_idx] = bel;
            line[lane] = bel;
            lds_fence();
            if (on && at == 0) a.states[a.elem_node[out_idx]] = mpe_decode(line + lane, k);
        }
        return;
    }

    for (int t = tid; t < pt.TT; t += nt) L.term[t] = a.term[pt.term_off + t];
    for (int t = tid; t < pt.CL; t += nt) L.clist[t] = a.clist[pt.clist_off + t];
    for (int t = tid; t < pt.T; t += nt) L.stg[t] = 0.0;  // the padding of the runs
    __syncthreads();

    const int cur = s & 1;
    const double* pi_cur = a.pi + cur * a.M;
    const double* lam_cur = a.lam + cur * a.M;
    const double* npi_cur = a.npi + cur * a.N;
    const double* nlam_cur = a.nlam + cur * a.N;
    double* pi_new = a.pi + (cur ^ 1) * a.M;
    double* lam_new = a.lam + (cur ^ 1) * a.M;
    double* npi_new = a.npi + (cur ^ 1) * a.N;
    double* nlam_new = a.nlam + (cur ^ 1) * a.N;
    double wres = 0.0;
    // ---- phase 1: entry items (gathers from memory, terms into LDS)
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
        if (r < pt.re) item_entry_any<kTermsInRegs, true>(e_mm[r], L.stg, L.term, pi_cur, nlam_cur, ent[r], ecpt[r], treg[r], LdPlain{});
    __syncthreads();
    // ---- phase 2a: accumulator items: the largest term of the run
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (r >= pt.rb) break;
        const SmallSlot q = bs[r];
        const int kind = int(q.z & 0xffu);
        const int base = int(q.x & 0xffffu);
        const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
        double old = 0.0;
        bool frozen = false;
        if (kind == 1) { old = npi_cur[out_idx]; frozen = a.frz[out_idx] != 0; }
        if (kind == 2) old = lam_cur[out_idx];
        const double acc = mpe_fold<(ROUNDS <= 2 ? 8 : 4), ROUNDS == 1>(L.stg + base, b_rmax[r]);
        lds_fence();   // (the line still holds the vector of the item before: its reads come first)
        const double val = mid_normalize(line, lane, kind != 0 ? k : 0, kind != 0 ? at : 0, acc, b_kmax[r]);
        if (kind == 1) npi_new[out_idx] = frozen ? old : val;  // evidence nodes are never updated (:177)
        if (kind == 2) {
            lam_new[out_idx] = val;
            wres = res_acc(wres, fabs(val - old));
        }
    }
    // ---- phase 2b: product items (old state only)
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (r >= pt.rc) break;
        const SmallSlot q = cs[r];
        const int kind = int(q.z & 0xffu), skip = int((q.z >> 8) & 0xffffu);
        const int cl = int(q.x & 0xffffu), deg = int(q.x >> 16);
        const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
        double old = 0.0;
        bool frozen = false;
        if (kind == 4) old = pi_cur[out_idx];
        if (kind == 3) { old = nlam_cur[out_idx]; frozen = a.frz[out_idx] != 0; }
        // lambda(v): from 1.0 (:220-238); pi-message: from pi(v)[i] (:202-218); children in ascending order
        double val = kind == 4 ? npi_cur[q.w & 0xffffu] : 1.0;
        for (int c0 = 0; c0 < c_dmax[r]; c0 += 4) {
            double f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool has = kind != 0 && c0 + u < deg;
                const int cb = L.clist[has ? cl + c0 + u : 0];
                f[u] = has ? lam_cur[cb + at] : 1.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) val *= (c0 + u < deg && c0 + u != skip) ? f[u] : 1.0;  // x * 1.0 == x
        }
        lds_fence();   // (as above)
        val = mid_normalize(line, lane, kind != 0 ? k : 0, kind != 0 ? at : 0, val, c_kmax[r]);
        if (kind == 3) nlam_new[out_idx] = frozen ? old : val;
        if (kind == 4) {
            pi_new[out_idx] = val;
            wres = res_acc(wres, fabs(val - old));
        }
    }
    // maximum_difference (:105-131): wave -> workgroup (LDS) -> the workgroup's word of this sweep's slot
    const unsigned long long bits = wave_umax64_dpp((unsigned long long)__double_as_longlong(wres));
    if (lane == 0) L.red[wave] = bits;
    __syncthreads();
    if (tid < kWave) {
        const int nw = nt >> 6;
        const unsigned long long mx = wave_umax64_dpp((tid < nw) ? L.red[tid] : 0ull);
        if (tid == 0) a.sync->words[s & 1][blockIdx.x] = mx;
    }
}

constexpr auto mpe_mid_sweep_of = [](auto R) { return mpe_mid_kernel<decltype(R)::value, false>; };
constexpr auto mpe_mid_finish_of = [](auto R) { return mpe_mid_kernel<decltype(R)::value, true>; };

int prepare_mpe_mid() { return prepare_item_kernels(mpe_mid_sweep_of, mpe_mid_finish_of); }

int launch_mpe_mid_init(const MpeMidArgs& a, void* stream) {
    (void)hipGetLastError();
    const int count = a.N > a.M ? a.N : a.M;
    hipLaunchKernelGGL(mpe_mid_init_kernel, dim3((count + 255) / 256 > 0 ? (count + 255) / 256 : 1), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}
int launch_mpe_mid_evidence(const MpeMidArgs& a, void* stream) {
    if (a.ev_ne <= 0) return 0;
    (void)hipGetLastError();
    hipLaunchKernelGGL(mpe_mid_evidence_kernel, dim3((a.ev_ne + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}
int launch_mpe_mid_sweep(const MpeMidArgs& a, int32_t s, bool finish, int waves, int rounds, size_t lds_bytes, void* stream) {
    const dim3 grid(a.nparts), block(waves * kWave);
    return finish ? launch_item_kernel(rounds, mpe_mid_finish_of, grid, block, lds_bytes, stream, a, s)
                  : launch_item_kernel(rounds, mpe_mid_sweep_of, grid, block, lds_bytes, stream, a, s);
}

}  // namespace bnmi
