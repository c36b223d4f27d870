// bn_small.hip -- the whole belief-propagation run of a SMALL network in ONE workgroup, state in LDS.
// Work items, encodings and the reasoning: bn_small.hpp / bn_small_plan.cpp.  Reference: belief_propagation.hpp:33-158.
//
// One iteration of the reference's while(true) loop (:75-148) =
//   phase 1   entry items: the terms of pi(v) (:174-200) and of the lambda-messages (:240-266) -> staging;
//   barrier
//   phase 2   accumulator items: each adds its run of staged terms front to back, normalises (:298-311), stores;
//             product items: lambda(v) (:220-238) and the pi-messages (:202-218) from the OLD state, normalised, stored;
//             maximum_difference (:105-131) of the wave -> LDS;
//   barrier   every wave reads the same words and takes the same stop decision (:147, strict <).
// Old and new state are the two halves of double buffers (the reference's new_* maps, :135-143).
// The thread's items and the iteration's statements are bn_small_items.inc and bn_small_sweep.inc, shared as text with
// em_small_kernel (bn_em.hip); the pieces below them -- LDS layout, entry item, run sum,
// normalisation -- are bn_small_dev.hpp's.  The evidence prologue is bn_small_evidence.inc, shared as text with mpe_small_kernel.
#include "bn_small.hpp"
#include "bn_tiles.hpp"
#include "bn_small_dev.hpp"
#include "bn_item_launch.hpp"

namespace bnmi {

// diagnostic builds (make EXTRA=-DBN_TILE_CLOCK): lane 0 of every wave records the 100 MHz clock at the phase
// boundaries of iteration 3 (scripts/experiments/small_clock.py prints them)
#ifdef BN_TILE_CLOCK
__device__ unsigned long long g_small_clock[kSmallMaxWaves][8];
#define SMALL_STAMP(k) do { if (lane == 0 && s == a.sweep_begin + 3) g_small_clock[wave][k] = wall_clock64(); } while (0)
#else
#define SMALL_STAMP(k) do { } while (0)
#endif

// ROUNDS = items of one kind per thread (1, 2 or kSmallMaxRounds): a network that fits one round keeps a third of the registers
template <int ROUNDS>
__global__ __launch_bounds__(kSmallMaxWaves * kWave) void bp_small_kernel(SmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) char small_lds[];
    const int set = blockIdx.x;
    BpBuffers b = a.b;
    shift_to_set(b, a.sets, set);
    double* state = a.state + int64_t(set) * a.state_stride;
    const SmallLds L = small_carve(small_lds, a);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & (kWave - 1);
    [[maybe_unused]] const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long t_first = wall_clock64();

    // ---- this thread's items, kept in registers for the whole run
    const SmallEntry* const it_ent = a.ent; const double* const it_cpt = a.ent_cpt; const uint32_t* const it_term = a.term;
    const SmallSlot* const it_bslot = a.bslot; const SmallSlot* const it_cslot = a.cslot;
    const int it_nt = nt, it_re = a.re, it_rb = a.rb, it_rc = a.rc;
    constexpr bool it_mine = true;
#include "bn_small_items.inc"
    // ---- tables and initial state (:33-73) into LDS
    for (int t = tid; t < a.TT; t += nt) L.term[t] = a.term[t];
    for (int t = tid; t < a.CL; t += nt) L.clist[t] = a.clist[t];
    for (int t = tid; t < a.T; t += nt) L.stg[t] = 0.0;  // the padding of the runs stays zero for the whole run
    int s = a.sweep_begin;
    {
        const int c0 = s & 1;
        if (a.ev_mode == 0) {
            for (int y = tid; y < a.N; y += nt) {
                const bool frozen = b.frozen[a.nv_slot[y]] == b.frozen_mark;  // preconditional_node_ (:69)
                L.frz[y] = frozen ? 1 : 0;
                if (s == 0) {
                    const double ev = b.node0[a.nv_idx[y]];  // where bp_evidence_kernel left the evidence vector
                    L.npi[c0 * a.N + y] = frozen ? ev : a.npi_init[y];
                    L.nlam[c0 * a.N + y] = frozen ? ev : 1.0;
                } else {
                    L.npi[c0 * a.N + y] = state[2 * a.M + y];
                    L.nlam[c0 * a.N + y] = state[2 * a.M + a.N + y];
                }
            }
        } else {
            // the evidence arrays themselves (mapped host memory)
            const int32_t* meta = a.ev_meta ? a.ev_meta + 8 * set : nullptr;
            const int ne = meta ? meta[0] : a.ev_ne, nval = meta ? meta[4] : a.ev_nval;
            const int32_t* ev_node = a.ev_node + (meta ? meta[1] : 0);
            const int32_t* ev_off = a.ev_off + (meta ? meta[2] : 0);
            const double* ev_val = a.ev_val + (meta ? meta[3] : 0);
#include "bn_small_evidence.inc"
        }
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
#include "bn_small_sweep.inc"
        r_last = rr;
        if (tid == 0 && s < b.res_cap) b.res_hist[s] = rr;
        ++s;
        if (rr < a.eps) { done = 1; break; }                                 // strict < (:147)
        if (a.max_sweeps > 0 && s >= a.max_sweeps) { done = 2; break; }
        if (s - a.sweep_begin >= a.budget) break;                            // the host continues in another launch
    }

    // ---- the state the run stopped in -> memory; belief = normalize(pi % lambda) (:151-158)
    const int fin = s & 1;
    for (int x = tid; x < a.M; x += nt) { state[x] = L.pi[fin * a.M + x]; state[a.M + x] = L.lam[fin * a.M + x]; }
    for (int y = tid; y < a.N; y += nt) { state[2 * a.M + y] = L.npi[fin * a.N + y]; state[2 * a.M + a.N + y] = L.nlam[fin * a.N + y]; }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (r >= a.rc) break;
        const SmallSlot q = cs[r];
        const bool on = (q.z & 0xffu) == 3;  // the lambda(v) items: one per node-vector element
        const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
        const double val = on ? L.npi[fin * a.N + out_idx] * L.nlam[fin * a.N + out_idx] : 0.0;
        const double bel = small_normalize(L.stg, on, out_idx, on ? k : 0, at, val, c_kmax[r]);
        if (on) b.beliefs[out_idx] = bel;
    }
    if (tid == 0) {
        Ctl* h = a.host_ctl + set;
        h->last_res = r_last; h->n_sweeps = s; h->t_first = t_first; h->t_last = wall_clock64();
        h->run_id = a.run_id; h->done = done;
    }
}

constexpr auto bp_small_of = [](auto R) { return bp_small_kernel<decltype(R)::value>; };

int prepare_bp_small() { return prepare_item_kernels(bp_small_of); }

int launch_bp_small(const SmallArgs& a, int waves, size_t lds_bytes, int n_sets, void* stream) {
    return launch_item_kernel(item_rounds(a.re, a.rb, a.rc), bp_small_of, dim3(n_sets > 1 ? n_sets : 1), dim3(waves * kWave), lds_bytes, stream, a);
}

}  // namespace bnmi

#ifdef BN_TILE_CLOCK
extern "C" int bn_debug_small_clock(unsigned long long* out) {
    return int(hipMemcpyFromSymbol(out, HIP_SYMBOL(bnmi::g_small_clock), sizeof(unsigned long long) * bnmi::kSmallMaxWaves * 8));
}
#endif
